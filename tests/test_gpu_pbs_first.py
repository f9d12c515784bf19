"""The bootstrap-first order of the 64-bit engine on the GPU (HELM_SI_CREATE_PBS_KS, SiServerKey(order="pbs_ks")): wire rows of
n + 1 words under the small key, a look-up is ONE bootstrap launch that reads its rows straight from the wire table and writes
big rows into the stage buffer, then ONE keyswitch from stage rows to table rows.

Everything is word for word against tests/pbs_first.py (keyswitch(bootstrap(row)) of the CPU oracle, pinned on the CPU by
tests/test_pbs_first_client.py), on toy sets:
  every bootstrap kernel class reads table rows in place, at batch widths 1, 63, 64, 65, 160 and one above round_capacity(),
  with permuted, non-contiguous in / out rows in a table larger than the batch (untouched rows unchanged), on both keyswitch
  paths (HELM_HIP_KS_MFMA unset and 0); the hazards (a job writing its own or another job's input, a two-level chain with an
  in-place latch); many-LUT with skipped outputs and set_level_many_lut on full-adder pairs; sharded calls (world 1 with a
  callback, two ranks over the in-process transport: the unsharded table, n + 1-word rows through the exchange); one key in
  both orders in one process against the primitives the suite already trusts; the host library's evaluators; the refusals; the
  counting build; and one round of 256 look-ups at the full-size set shortint_m2c2_pbs_ks (decrypt level: an approximate set).
The reference rows are computed once per key and shared."""
import contextlib
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import helm_amd
import oracle
from helm_amd import ArithCircuit, Circuit, EvalCircuit, LutCircuit, PtxtType, verilog_parser

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import many_lut as ML  # noqa: E402
import pbs_first as PF  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET = os.path.join(ROOT, "tests", "netlists")

# (id, key: a named set or (k, N, l, logB, g), generic mode, kernel class): one case per bootstrap kernel build
CASES = [
    ("si_toy_512", "si_toy_512", None, "tuned"),                            # k_pbs64
    ("si_toy_1024", "si_toy_1024", None, "tuned"),                          # k_pbs64s
    ("si_toy_2048_l2", "si_toy_2048_l2", None, "tuned"),                    # k_pbs64s, two levels
    ("si_toy_512_k3", "si_toy_512_k3", None, "tuned"),                      # k_pbs64k
    ("si_toy_1024_k2", "si_toy_1024_k2", None, "tuned"),                    # k_pbs64k at N = 1024
    ("si_toy_1024_mb2", "si_toy_1024_mb2", None, "tuned"),                  # k_pbs64s, multi-bit
    ("generic-k2_N512_l2_B12", (2, 512, 2, 12, 0), "allow", "generic"),     # k_pbs64_generic
    ("si_toy_4096", "si_toy_4096", "large", "large"),                       # k_pbs64_large
]
IDS = [c[0] for c in CASES]
T_IN = 16        # input rows of a key's shared reference: the values 0 .. 15


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        os.environ.update(kv)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_keys, _refs = {}, {}


def _client_key(key):
    if key not in _keys:
        if isinstance(key, str):
            _keys[key] = helm_amd.SiClientKey.generate(key, seed=3)
        else:
            k, N, l, logB, g = key
            p, _, _ = helm_amd.si_named_params("si_toy_512")
            p.n, p.k, p.N, p.pbs_l, p.pbs_logB, p.ks_l, p.ks_logB = 12, k, N, l, logB, 4, 4
            p.message_modulus, p.carry_modulus, p.grouping_factor = 4, 4, g
            _keys[key] = helm_amd.SiClientKey(p, 1e-9, 1e-15, seed=7)
    return _keys[key]


def _funcs(t):
    return [lambda v: (5 * v + 3) % t, lambda v: (t - 1 - v) % t]


def _reference(key):
    """Computed once per key, shared, never modified.  -> dict(ck, ref, rows [T_IN, n+1], luts [2, N],
    want {(v, l): keyswitch(bootstrap(rows[v], luts[l]))})"""
    if key not in _refs:
        ck = _client_key(key)
        orc = oracle.Oracle64(ck.params.as_tuple(), ck.bsk, ck.ksk, use_ntt=True)
        ref = PF.PbsFirst(orc)
        rows = ck.encrypt(np.arange(T_IN, dtype=np.uint64), small=True)
        luts = np.stack([orc.make_lut(f) for f in _funcs(ck.t)])
        want = {(v, l): ref.apply_lut_small(rows[v], luts[l]) for v in range(T_IN) for l in range(2)}
        for (v, l), row in want.items():      # the reference itself decrypts
            assert ck.decrypt_message_and_carry(row, small=True) == _funcs(ck.t)[l](v)
        for a in (rows, luts, *want.values()):
            a.setflags(write=False)
        _refs[key] = dict(ck=ck, ref=ref, rows=rows, luts=luts, want=want)
    return _refs[key]


def _server(key, generic=None, order="pbs_ks"):
    ck = _client_key(key)
    sk = helm_amd.SiServerKey(ck, generic=generic, order=order)
    assert (sk.pbs_order(), sk.wire_words()) == ((0, ck.params.n + 1) if order == "pbs_ks" else (1, ck.dim + 1))
    return sk


def _table(sk, n_rows, rows, seed=17):
    """A table of n_rows random rows whose first len(rows) rows are `rows`.  -> (SiWires, its expected contents)"""
    sentinel = np.random.default_rng(seed).integers(0, 2**64, size=(n_rows, sk.wire_words()), dtype=np.uint64)
    sentinel[:len(rows)] = rows
    w = sk.wires(n_rows)
    w.upload(np.arange(n_rows), sentinel)
    return w, sentinel


# ------------------------------------------------------------------------------------------------------------------------
# every bootstrap kernel class, every batch width, both keyswitch paths
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,key,generic,klass", CASES, ids=IDS)
def test_look_ups_word_for_word_on_every_kernel_class(name, key, generic, klass):
    R = _reference(key)
    tables = {}
    for mfma in (None, "0"):
        with _env(**({} if mfma is None else {"HELM_HIP_KS_MFMA": mfma})):
            sk = _server(key, generic)
        assert sk.kernel_class() == klass
        cap = sk.round_capacity()
        assert cap >= 160
        rng = np.random.default_rng(23)
        for W in (1, 63, 64, 65, 160, cap + 1):
            w, expect = _table(sk, T_IN + 2 * W + 3, R["rows"])
            in_idx = rng.integers(0, T_IN, size=W).astype(np.int32)
            lut_idx = rng.integers(0, 2, size=W).astype(np.int32)
            out_idx = (T_IN + 1 + 2 * rng.permutation(W)).astype(np.int32)      # every other row, permuted
            w.apply_luts(in_idx, R["luts"], out_idx, lut_idx)
            got = w.download()
            for g in range(W):
                expect[out_idx[g]] = R["want"][(int(in_idx[g]), int(lut_idx[g]))]
            bad = np.nonzero((got != expect).any(axis=1))[0]
            assert bad.size == 0, f"{name}, KS_MFMA={mfma}, width {W}: rows {bad[:8].tolist()} (written rows: {sorted(out_idx.tolist())[:8]} ...)"
            tables[(mfma, W)] = got
            w.free()
        sk.close()
    for (mfma, W), got in tables.items():      # both keyswitch paths write the same table rows
        assert np.array_equal(got, tables[(None, W)]), (mfma, W)


# ------------------------------------------------------------------------------------------------------------------------
# hazards: every input is read before any output is written
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["si_toy_512", "si_toy_512_k3"])
def test_hazards_equal_the_reference_which_reads_all_inputs_first(key):
    R = _reference(key)
    sk = _server(key)
    for label, in_idx, out_idx in (("a job writes its own input", [0, 1, 2], [0, 1, 2]),
                                   ("a job writes another job's input", [0, 1, 2, 3], [1, 2, 3, 0]),
                                   ("both", [4, 5, 5, 6], [5, 4, 9, 6])):
        w, host = _table(sk, 12, R["rows"][:8])
        lut_idx = np.arange(len(in_idx), dtype=np.int32) % 2
        w.apply_luts(in_idx, R["luts"], out_idx, lut_idx)
        want = host.copy()
        R["ref"].apply_luts(want, in_idx, R["luts"], out_idx, lut_idx)
        for g in range(len(in_idx)):          # (the reference read the rows as they were: the shared reference's rows)
            assert np.array_equal(want[out_idx[g]], R["want"][(in_idx[g], int(lut_idx[g]))])
        assert np.array_equal(w.download(), want), label
    sk.close()


def test_a_two_level_chain_with_an_in_place_latch():
    R = _reference("si_toy_512")
    ck, ref = R["ck"], R["ref"]
    sk = _server("si_toy_512")
    bits = [1, 0, 1, 1, 0]
    w, host = _table(sk, 9, ck.encrypt(bits, small=True))
    # level 1: a 3-input gate over its own first input, a bivariate gate; level 2: a gate that reads both results and
    # rewrites one of them in place, a flip-flop that latches the other, a negation
    levels = [([3, 2], [[0, 1, 2], [3, 4, -1]], [0x96, 0x6], [0, 5]),
              ([3, 0, 1], [[5, 0, 1], [0, -1, -1], [2, -1, -1]], [0xE8, 0, 1], [5, 6, 7])]
    for arity, in_idx, table, out in levels:
        w.eval_lut_level(arity, in_idx, table, out)
        ref.eval_lut_level(host, arity, in_idx, table, out)
    got = w.download()
    assert np.array_equal(got, host)
    a, b, c, d, e = bits
    r0, r5 = a ^ b ^ c, d ^ e
    maj = (r5 & r0) | (r5 & b) | (r0 & b)
    assert [int(v) for v in ck.decrypt_message_and_carry(got[[0, 5, 6, 7]], small=True)] == [r0, maj, r0, (ck.t - c) % ck.t]
    sk.close()


# ------------------------------------------------------------------------------------------------------------------------
# many-LUT: n_out keyswitches per rotation, none for a skipped output
# ------------------------------------------------------------------------------------------------------------------------
def _many_case(ck, n_out):
    t = ck.t
    M = ML.chunks(n_out)
    per = t // M
    fs = [lambda v, x=x: (3 * v + 5 * x + 1) % t for x in range(n_out)]
    tv = ML.many_lut_poly([[f(v) for v in range(per)] for f in fs], t, ck.params.N)
    count = 5
    vals = (np.arange(count) % per).astype(np.uint64)
    out_idx = (8 + np.arange(count * n_out, dtype=np.int32)).reshape(count, n_out)
    out_idx[1, n_out - 1] = -1            # skipped outputs
    out_idx[3, 0] = -1
    out_idx[2, 1] = 2                     # one over its own input row
    out_idx[0, 1] = 4                     # ... and one over the last ciphertext's input row
    return fs, tv, vals, out_idx


@pytest.mark.parametrize("n_out", [2, 3, 16])
def test_many_lut_outputs_are_the_keyswitch_of_each_extract(n_out):
    """Row 0 against the exact accumulator of tests/many_lut.py (a second of Python per row), every row against the order-1
    context's primitives on the same key: keyswitch_batch(pbs_many_batch(row))."""
    R = _reference("si_toy_512")
    ck, ref = R["ck"], R["ref"]
    assert n_out <= ck.t
    fs, tv, vals, out_idx = _many_case(ck, n_out)
    rows = ck.encrypt(vals, small=True)
    sk, sk1 = _server("si_toy_512"), _server("si_toy_512", order="ks_pbs")
    assert np.array_equal(sk.make_many_lut(fs), tv)
    big = sk1.pbs_many_batch(rows, tv, n_out)
    prim = sk1.keyswitch_batch(big.reshape(-1, ck.dim + 1)).reshape(len(vals), n_out, -1)
    exact = ref.many_lut_outputs(rows[0], tv, n_out, ck.bsk)
    for x in range(n_out):
        assert np.array_equal(prim[0, x], exact[x]), x
    w, expect = _table(sk, 8 + len(vals) * n_out + 2, rows)
    w.apply_many_luts(np.arange(len(vals)), tv, out_idx)
    got = w.download()
    for g in range(len(vals)):
        for x in range(n_out):
            if out_idx[g, x] >= 0:
                expect[out_idx[g, x]] = prim[g, x]
    bad = np.nonzero((got != expect).any(axis=1))[0]
    assert bad.size == 0, bad.tolist()
    written = out_idx[out_idx >= 0]
    dec = ck.decrypt_message_and_carry(got[written], small=True)
    assert [int(v) for v in dec] == [fs[x](int(vals[g])) for g in range(len(vals)) for x in range(n_out) if out_idx[g, x] >= 0]
    sk.close()
    sk1.close()


@pytest.mark.parametrize("name,key,generic,klass", CASES[1:], ids=IDS[1:])
def test_many_lut_on_the_other_kernel_classes(name, key, generic, klass):
    ck = _client_key(key)
    n_out = 3
    fs, tv, vals, out_idx = _many_case(ck, n_out)
    rows = ck.encrypt(vals, small=True)
    sk, sk1 = _server(key, generic), _server(key, generic, order="ks_pbs")
    prim = sk1.keyswitch_batch(sk1.pbs_many_batch(rows, tv, n_out).reshape(-1, ck.dim + 1)).reshape(len(vals), n_out, -1)
    w, expect = _table(sk, 8 + len(vals) * n_out + 2, rows)
    w.apply_many_luts(np.arange(len(vals)), tv, out_idx)
    for g in range(len(vals)):
        for x in range(n_out):
            if out_idx[g, x] >= 0:
                expect[out_idx[g, x]] = prim[g, x]
    assert np.array_equal(w.download(), expect)
    sk.close()
    sk1.close()


def test_level_many_lut_on_full_adder_pairs():
    R = _reference("si_toy_512")
    ck, ref = R["ck"], R["ref"]
    t, N = ck.t, ck.params.N
    sk = _server("si_toy_512")
    sk.set_level_many_lut(True)
    bits = [1, 1, 0, 0, 1, 0]
    w, host = _table(sk, 12, ck.encrypt(bits, small=True))
    # two full adders (sum 0x96, carry 0xE8 on the same inputs: one rotation each) and a gate without a partner
    arity = [3, 3, 3, 3, 2]
    in_idx = [[0, 1, 2], [0, 1, 2], [3, 4, 5], [3, 4, 5], [0, 5, -1]]
    table = [0x96, 0xE8, 0x96, 0xE8, 0x6]
    out = [6, 7, 8, 9, 10]
    sk.timing_enable(True)
    sk.timing(reset=True)
    w.eval_lut_level(arity, in_idx, table, out)
    got = w.download()
    assert int(sk.timing().pbs_count) == 3
    per = t // 2
    pair = ML.many_lut_poly([[(tb >> (v & 7)) & 1 for v in range(per)] for tb in (0x96, 0xE8)], t, N)
    want = host.copy()
    for base, ins in ((6, [0, 1, 2]), (8, [3, 4, 5])):
        packed = ref.lincomb_row(host, ins, [4, 2, 1])
        want[base], want[base + 1] = ref.many_lut_outputs(packed, pair, 2, ck.bsk)
    want[10] = ref.apply_lut_small(ref.lincomb_row(host, [0, 5], [2, 1]), ref.level_lut(2, 0x6))
    assert np.array_equal(got, want)
    a, b, c, d, e, f = bits
    assert [int(v) for v in ck.decrypt_message_and_carry(got[6:11], small=True)] == \
           [a ^ b ^ c, (a & b) | (a & c) | (b & c), d ^ e ^ f, (d & e) | (d & f) | (e & f), a ^ f]
    sk.close()


# ------------------------------------------------------------------------------------------------------------------------
# sharded calls: the unsharded table, rows of n + 1 words through the exchange
# ------------------------------------------------------------------------------------------------------------------------
def _sharded_cases(ck):
    """name -> (kind, in_idx, out_idx, lut_idx, capacity_rows, per-rank rows of every exchange round for world 1 and 2)"""
    seven = np.arange(7, dtype=np.int32)
    plain_out = np.array([9, 1, 11, 3, 13, 15, 17], dtype=np.int32)       # jobs 1 and 3 in place (a round boundary may lie between
    _, _, _, many_out = _many_case(ck, 2)                                 # two jobs: hazards across jobs belong to many-LUT)
    many_out = np.where(many_out >= 0, many_out + 8, -1).astype(np.int32)  # its input rows are rows 8 .. 12 of the table here
    return {
        "plain, several rounds": ("luts", seven, plain_out, seven % 2, 2, {1: [2, 2, 2, 1], 2: [2, 2]}),
        "plain, an empty last chunk": ("luts", seven[:3], plain_out[:3] + 20, seven[:3] % 2, 1, {1: [1, 1, 1], 2: [1, 1]}),
        "many-LUT, several rounds, an empty last chunk": ("many", seven[:5], many_out, None, 4, {1: [4, 4, 2], 2: [4, 2]}),
    }


def _sharded_run(sk, ck, R, install, remove, world, rank, want_tables):
    """-> (problems, {case: table}) for one rank"""
    problems, tables = [], {}
    _, tv, vals, _ = _many_case(ck, 2)
    rows = np.concatenate([R["rows"][:8], ck_rows_many(ck, vals)])
    for name, (kind, in_idx, out_idx, lut_idx, cap, rounds) in _sharded_cases(ck).items():
        w, _ = _table(sk, 40, rows)
        if kind == "many":
            in_idx = in_idx + 8
        if install is not None:
            install(cap)
        b0, r0 = sk.exchange_stats()
        if kind == "luts":
            w.apply_luts(in_idx, R["luts"], out_idx, lut_idx)
        else:
            w.apply_many_luts(in_idx, tv, out_idx)
        sk.sync()
        b1, r1 = sk.exchange_stats()
        tables[name] = w.download()
        if install is not None:
            remove()
            if not np.array_equal(tables[name], want_tables[name]):
                problems.append((name, rank, "differs from the unsharded table in rows %s" %
                                 np.nonzero((tables[name] != want_tables[name]).any(axis=1))[0].tolist()))
            if (b1 - b0, r1 - r0) != (len(rounds[world]), sum(rounds[world]) * world):
                problems.append((name, rank, "exchange rounds / rows %s, expected %s" %
                                 ((b1 - b0, r1 - r0), (len(rounds[world]), sum(rounds[world]) * world))))
        w.free()
    return problems, tables


_many_rows = {}


def ck_rows_many(ck, vals):
    """the many-LUT cases' input rows: one encryption per key, shared by every rank and the unsharded run"""
    if id(ck) not in _many_rows:
        _many_rows[id(ck)] = ck.encrypt(vals, small=True)
    return _many_rows[id(ck)]


@pytest.fixture(scope="module")
def unsharded():
    R = _reference("si_toy_512")
    sk = _server("si_toy_512")
    problems, tables = _sharded_run(sk, R["ck"], R, None, None, 1, 0, None)
    sk.close()
    # the plain cases against the reference (same-round hazards included: every input is read first)
    for name, (kind, in_idx, out_idx, lut_idx, _, _) in _sharded_cases(R["ck"]).items():
        if kind == "luts":
            for g in range(len(in_idx)):
                assert np.array_equal(tables[name][out_idx[g]], R["want"][(int(in_idx[g]), int(lut_idx[g]))]), (name, g)
    return R, tables


def test_sharded_world_one_with_a_callback(unsharded):
    import torch
    from helm_amd import _native as nv
    R, want = unsharded
    ck = R["ck"]
    torch.cuda.set_device(0)
    sk = _server("si_toy_512")
    words = sk.wire_words()
    assert words == ck.params.n + 1
    seen = []

    def install(cap):
        dev = torch.device("cuda", torch.cuda.current_device())
        sk.set_stream(torch.cuda.current_stream().cuda_stream)
        stage = torch.zeros((cap, words), dtype=torch.int64, device=dev)
        gather = torch.zeros((cap, words), dtype=torch.int64, device=dev)

        def exchange(_user, rows):
            gather[:rows].copy_(stage[:rows])
            seen.append((rows, stage[:rows].numel() * 8))
            return 0

        fn = nv.SI_EXCHANGE_FN(exchange)
        nv.hip_check(nv.hip.helm_si_set_exchange(sk._h, 0, 1, 1, nv.vp(stage.data_ptr()), nv.vp(gather.data_ptr()), cap, fn, None))
        sk._exchange = (fn, stage, gather)

    def remove():
        nv.hip_check(nv.hip.helm_si_set_exchange(sk._h, 0, 1, 1, None, None, 1, nv.SI_EXCHANGE_FN(0), None))
        sk._exchange = None

    problems, _ = _sharded_run(sk, ck, R, install, remove, 1, 0, want)
    assert problems == []
    want_rounds = [r for c in _sharded_cases(ck).values() for r in c[5][1]]
    assert seen == [(r, r * (ck.params.n + 1) * 8) for r in want_rounds]
    sk.close()


def test_sharded_two_ranks_over_the_in_process_transport(unsharded):
    from helm_amd.comm import Comm
    R, want = unsharded
    ck = R["ck"]
    world = 2
    comms = Comm.in_process_group([0] * world, timeout=120.0)
    sks = [_server("si_toy_512") for _ in range(world)]
    results, errors = [None] * world, []

    def rank_main(r):
        try:
            sk = sks[r]
            results[r] = _sharded_run(sk, ck, R, lambda cap: sk.set_exchange_comm(comms[r], min_batch=1, capacity_rows=cap),
                                      lambda: sk.set_exchange_comm(None), world, r, want)
        except BaseException as e:  # noqa: BLE001 - reported below; the group's barrier is broken so nobody waits for ever
            errors.append((r, repr(e)))
            comms[r].abort_group()

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=300)
        assert not th.is_alive(), "a rank thread is stuck"
    assert not errors, errors
    per_rank_rows = sum(r for c in _sharded_cases(ck).values() for r in c[5][world])
    for r in range(world):
        assert results[r][0] == [], results[r][0]
        # what went through the exchange: rows of n + 1 words
        assert comms[r].stats()["bytes_sent"] == per_rank_rows * (ck.params.n + 1) * 8
        sks[r].close()
    for c in comms:
        c.destroy()


# ------------------------------------------------------------------------------------------------------------------------
# one key, both orders, one process
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,key,generic,klass", CASES, ids=IDS)
def test_same_key_both_orders_in_one_process(name, key, generic, klass):
    """The order-0 output equals keyswitch_batch of the order-1 context applied to the bootstrap of the same small rows - and
    the order-1 context, alive beside it, still computes what it computed."""
    R = _reference(key)
    ck = R["ck"]
    sk1, sk0 = _server(key, generic, order="ks_pbs"), _server(key, generic)
    assert (sk1.pbs_order(), sk0.pbs_order()) == (1, 0) and sk1.kernel_class() == sk0.kernel_class() == klass
    assert sk1.round_capacity() == sk0.round_capacity() and sk1.field_bits() == sk0.field_bits()
    lut_idx = (np.arange(T_IN) % 2).astype(np.int32)
    prim = sk1.keyswitch_batch(sk1.pbs_batch(R["rows"], R["luts"], lut_idx))
    w0 = sk0.wires(2 * T_IN)
    w0.upload(np.arange(T_IN), R["rows"])
    w0.apply_luts(np.arange(T_IN), R["luts"], T_IN + np.arange(T_IN), lut_idx)
    got = w0.download(T_IN + np.arange(T_IN))
    assert np.array_equal(got, prim)
    for v in range(T_IN):
        assert np.array_equal(got[v], R["want"][(v, int(lut_idx[v]))])
    # order 1 on the same key: its look-up of a big encryption is bootstrap(keyswitch(.)) of the oracle, as ever
    big = ck.encrypt(np.arange(4, dtype=np.uint64))
    w1 = sk1.wires(8)
    w1.upload(np.arange(4), big)
    w1.apply_luts(np.arange(4), R["luts"], 4 + np.arange(4), lut_idx[:4])
    orc = R["ref"].orc
    assert np.array_equal(w1.download(4 + np.arange(4)), orc.apply_luts(big, R["luts"], lut_idx[:4]))
    # the primitives mean the same on the order-0 context
    assert np.array_equal(sk0.keyswitch_batch(sk0.pbs_batch(R["rows"], R["luts"], lut_idx)), prim)
    # linear steps and trivial rows have the context's width
    w0.set_trivial([0], [5])
    w0.lincomb([[T_IN, 0]], [[3, 1]], [1])
    rows = w0.download([0, 1])
    assert rows.shape == (2, ck.params.n + 1) and not rows[0, :-1].any() and int(rows[0, -1]) == 5 * ck.delta
    assert np.array_equal(rows[1], R["ref"].lincomb_row(np.stack([got[0], rows[0]]), [0, 1], [3, 1]))
    sk0.close()
    sk1.close()


def test_lanes_report_their_primary_and_work_on_its_table():
    R = _reference("si_toy_1024")
    sk = _server("si_toy_1024")
    lane = sk.fork()
    assert (lane.pbs_order(), lane.wire_words()) == (0, R["ck"].params.n + 1)
    w, expect = _table(sk, 8, R["rows"][:4])
    sk.sync()
    w.sk = lane                          # the primary's table, driven through the lane
    w.apply_luts([0, 1], R["luts"], [5, 6], [0, 1])
    lane.sync()
    w.sk = sk
    expect[5], expect[6] = R["want"][(0, 0)], R["want"][(1, 1)]
    assert np.array_equal(w.download(), expect)
    sk.close()


# ------------------------------------------------------------------------------------------------------------------------
# the host library
# ------------------------------------------------------------------------------------------------------------------------
def _circuit(path_or_text, is_arith=False, is_text=False):
    rd = verilog_parser.read_verilog_text if is_text else verilog_parser.read_verilog_file
    gates_set, wire_set, input_wires, output_wires, dffs, _, _ = rd(path_or_text, is_arith)
    c = Circuit(gates_set, input_wires, output_wires, dffs)
    c.sort_circuit()
    c.compute_levels()
    return c, wire_set


class SmallAuditor:
    """fn for SiServerKey.set_audit on an order-0 key: the rows are wire rows of n + 1 words; every look-up batch is
    recomputed as keyswitch(bootstrap(.)) on the oracle from the GPU's own operand rows, every linear step in integers."""

    def __init__(self, ref):
        self.ref, self.bad, self.luts, self.lin = ref, [], 0, 0
        self.lock = threading.Lock()

    def __call__(self, rec):
        n1 = self.ref.n + 1
        bad = []
        if rec["kind"] == "lincomb":
            cnt, terms, width = rec["in_rows"].shape
            assert width == n1 and rec["out_rows"].shape == (cnt, n1)
            acc = np.zeros_like(rec["out_rows"])
            with np.errstate(over="ignore"):
                for t in range(terms):
                    use = rec["in_idx"][:, t] >= 0
                    acc[use] += rec["coef"][use, t].astype(np.uint64)[:, None] * rec["in_rows"][use, t]
                if rec["const_add"] is not None:
                    acc[:, -1] += rec["const_add"].astype(np.uint64) * np.uint64(self.ref.delta)
            bad = [("lincomb", int(g)) for g in np.nonzero(~np.all(acc == rec["out_rows"], axis=1))[0]]
            with self.lock:
                self.lin += cnt
        else:
            assert rec["kind"] == "luts" and rec["in_rows"].shape[1] == n1 and rec["out_rows"].shape[1] == n1
            for g in range(len(rec["lut_idx"])):
                if not np.array_equal(self.ref.apply_lut_small(rec["in_rows"][g], rec["luts"][rec["lut_idx"][g]]), rec["out_rows"][g]):
                    bad.append(("luts", g))
            with self.lock:
                self.luts += len(rec["lut_idx"])
        with self.lock:
            self.bad += bad
        return True


@pytest.fixture(scope="module")
def host_keys():
    ck = helm_amd.SiClientKey.generate("si_toy_2048", seed=1)     # m2c2's shape (k = 1, N = 2048, t = 16) at toy n
    sk = helm_amd.SiServerKey(ck, order="pbs_ks")
    yield ck, sk
    sk.close()


def test_lut_circuit_8_bit_adder_every_wire_audited(host_keys):
    ck, sk = host_keys
    circuit, wire_set = _circuit(f"{NET}/8-bit-adder-lut-3-1.v")
    a, b, cin = 0xB7, 0x6E, 1
    inputs = {f"a[{i}]": PtxtType.Bool((a >> i) & 1) for i in range(8)}
    inputs.update({f"b[{i}]": PtxtType.Bool((b >> i) & 1) for i in range(8)})
    inputs["cin"] = PtxtType.Bool(cin)
    ptxt = circuit.evaluate(circuit.initialize_wire_map(wire_set, inputs, "bool"))
    aud = SmallAuditor(PF.PbsFirst(oracle.Oracle64(ck.params.as_tuple(), ck.bsk, ck.ksk, use_ntt=True)))
    sk.set_audit(aud)
    lc = LutCircuit(ck, sk, circuit)
    enc = EvalCircuit.encrypt_inputs(lc, wire_set, inputs)
    assert enc.row_words == ck.params.n + 1
    enc = EvalCircuit.evaluate_encrypted(lc, enc, 1, "bool")
    sk.set_audit(None)
    assert lc.pbs_per_cycle() == 16 and aud.luts == 16 and aud.lin > 0 and not aud.bad, aud.bad[:5]
    for wire, want in ptxt.items():
        assert ck.decrypt(enc[wire], small=True) == int(bool(want)), wire
    out = EvalCircuit.decrypt_outputs(lc, enc, True)
    assert sum(out[f"sum[{i}]"].value << i for i in range(8)) + (out["cout"].value << 8) == a + b + cin
    # a client buffer of the other order's width is refused, and the message names both widths
    with pytest.raises(helm_amd._host.Panic, match=f"rows of {ck.dim + 1} words.*row\\(s\\) of {ck.params.n + 1} words"):
        enc["cin"] = ck.encrypt(1)
    enc["cin"] = ck.encrypt(1, small=True)
    assert ck.decrypt(enc["cin"], small=True) == 1


def test_arith_circuit_u8_operators_and_u16_known_answers(host_keys):
    ck, sk = host_keys
    text = """input [7:0] A, B;
output [7:0] S, D, P, M;
add g0(A, B, S);
sub g1(A, B, D);
mult g2(A, B, P);
mult g3(A, 27, M);
"""
    circuit, wire_set = _circuit(text, is_arith=True, is_text=True)
    ac = ArithCircuit(ck, sk, circuit)
    a, b = 201, 100
    out = ac.decrypt_outputs(ac.evaluate_encrypted(ac.encrypt_inputs(wire_set, {"A": PtxtType.U8(a), "B": PtxtType.U8(b)}), 1, "u8"), True)
    assert {k: v.value for k, v in out.items()} == {"S": (a + b) % 256, "D": (a - b) % 256, "P": a * b % 256, "M": a * 27 % 256}
    text = """input [15:0] A, B;
output [15:0] S, D, P, Q, R;
add g0(A, B, S);
sub g1(B, A, D);
mult g2(A, B, P);
add g3(A, 7, Q);
sub g4(B, 3, R);
"""                                       # the K-7 operators (reference tests/gates_test.rs:127-310)
    circuit, wire_set = _circuit(text, is_arith=True, is_text=True)
    ac = ArithCircuit(ck, sk, circuit)
    x, y = 20, 30
    out = ac.decrypt_outputs(ac.evaluate_encrypted(ac.encrypt_inputs(wire_set, {"A": PtxtType.U16(x), "B": PtxtType.U16(y)}), 1, "u16"), True)
    assert (out["S"], out["D"], out["P"], out["Q"], out["R"]) == \
           (PtxtType.U16(x + y), PtxtType.U16(y - x), PtxtType.U16(x * y), PtxtType.U16(x + 7), PtxtType.U16(y - 3))


# ------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------
def test_the_wop_path_refuses_an_order_0_pbs_side():
    from helm_amd import wopbs
    ck = _client_key("si_toy_1024")
    sk0, sk1 = _server("si_toy_1024"), _server("si_toy_1024", order="ks_pbs")
    wck = wopbs.WopClientKey.generate(ck, "wop_toy_1024", seed=2)
    with pytest.raises(helm_amd.HelmError, match="HELM_SI_CREATE_PBS_KS.*helm_si_pbs_order 0"):
        wopbs.WopServerKey(sk0, wck)
    wsk = wopbs.WopServerKey(sk1, wck)                  # the order-1 side of the same key is admitted as ever
    circuit, _ = _circuit(f"{NET}/8-bit-adder-lut-3-1.v")
    lc = LutCircuit(ck, sk0, circuit)
    with pytest.raises(Exception, match="HELM_SI_CREATE_PBS_KS.*helm_si_pbs_order 0"):
        lc.set_wide_lut_key(wsk, 1)
    wsk.close()
    sk0.close()
    sk1.close()


# ------------------------------------------------------------------------------------------------------------------------
# the counting build (it admits the order: nothing in it depends on the row width)
# ------------------------------------------------------------------------------------------------------------------------
CHILD = r"""
import json, sys
import numpy as np
sys.path[:0] = [%r, %r]
import helm_amd
import test_gpu_pbs_first as T
res = {}
for name, key, generic, klass in T.CASES:
    if klass != "tuned" or name == "si_toy_1024_k2":   # the counting build runs the tuned kernels only; its k = 2, N = 1024
        continue                                       # build is launched nowhere in the suite, k_pbs64k is covered by k = 3
    ck = T._client_key(key)
    sk = helm_amd.SiServerKey(ck, order="pbs_ks")
    sk.bound_violations(reset=True)
    t = ck.t
    fs = T._funcs(t)
    luts = np.stack([sk.make_lut(f) for f in fs])
    vals = np.arange(16, dtype=np.uint64)
    w = sk.wires(64)
    w.upload(np.arange(16), ck.encrypt(vals, small=True))
    w.apply_luts(np.arange(16), luts, 16 + np.arange(16), np.arange(16) %% 2)
    two = sk.make_many_lut([lambda v: v %% 4, lambda v: v // 4])
    w.apply_many_luts(np.arange(8), two, 32 + np.arange(16).reshape(8, 2))
    dec = [int(v) for v in ck.decrypt_message_and_carry(w.download(16 + np.arange(32)), small=True)]
    want = [fs[v %% 2](v) for v in range(16)] + [x for v in range(8) for x in (v %% 4, v // 4)]
    res[name] = {"ok": dec == want, "order": sk.pbs_order(), "violations": sk.bound_violations()}
    sk.close()
print("RESULT " + json.dumps(res))
"""


def test_counting_build_counts_nothing_in_order_0():
    """One child process on libhelm_hip_check.so: the kernel-class cases the build runs, values right, every counter zero.  It
    is not retried."""
    lib = os.path.join(ROOT, "helm_amd", "csrc", "libhelm_hip_check.so")
    assert os.path.exists(lib), "make -C helm_amd/csrc libhelm_hip_check.so"
    p = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=dict(os.environ, HELM_HIP_LIB=lib),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert sorted(res) == sorted(c[0] for c in CASES if c[3] == "tuned" and c[0] != "si_toy_1024_k2")
    for name, r in res.items():
        assert r == {"ok": True, "order": 0, "violations": [0] * 8}, (name, r)


# ------------------------------------------------------------------------------------------------------------------------
# full size
# ------------------------------------------------------------------------------------------------------------------------
def test_one_round_of_256_look_ups_at_the_full_size_set_decrypts():
    """shortint_m2c2_pbs_ks is an approximate set (helm_client64.cpp): a decrypt-level check - every row of one round of 256
    look-ups on fresh encryptions decrypts to f(v), and so does 4x + 2y + z of three look-up outputs looked up again (the
    operand of a 3-input gate, where the keyswitch noise is amplified 21-fold)."""
    ck = helm_amd.SiClientKey.generate("shortint_m2c2_pbs_ks", seed=1)
    sk = helm_amd.SiServerKey(ck, order="pbs_ks")
    t = ck.t
    assert sk.wire_words() == ck.params.n + 1 == 841 and sk.kernel_class() == "tuned"
    f = lambda v: (5 * v + 3) % t       # noqa: E731
    vals = (np.arange(256) % t).astype(np.uint64)
    w = sk.wires(512 + 86)
    w.upload(np.arange(256), ck.encrypt(vals, small=True))
    w.apply_luts(np.arange(256), sk.make_lut(f), 256 + np.arange(256))
    got = ck.decrypt_message_and_carry(w.download(256 + np.arange(256)), small=True)
    wrong = [int(g) for g in np.nonzero(got != np.array([f(int(v)) for v in vals], dtype=np.uint64))[0]]
    assert wrong == [], f"{len(wrong)} of 256 rows fail: {wrong[:10]}"
    # bits from look-ups, then 4x + 2y + z of three of them through one more look-up
    bit = sk.make_lut(lambda v: v & 1)
    w.apply_luts(np.arange(256), bit, np.arange(256))
    trip = np.arange(255).reshape(85, 3)
    w.lincomb(trip, np.tile([4, 2, 1], (85, 1)), 512 + np.arange(85))
    w.apply_luts(512 + np.arange(85), sk.make_lut(lambda v: (3 * v + 1) % t), 512 + np.arange(85))
    got = ck.decrypt_message_and_carry(w.download(512 + np.arange(85)), small=True)
    bits = vals & np.uint64(1)
    want = [(3 * int(4 * bits[a] + 2 * bits[b] + bits[c]) + 1) % t for a, b, c in trip]
    assert [int(v) for v in got] == want
    sk.close()
