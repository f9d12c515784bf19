"""The N = 8192 blind-rotate kernel of the 64-bit engine (k_pbs64_n8192, helm_amd/csrc/helm_pbs64_n8192.inc over
helm_pbs64_large_core.inc): k = 1, N = 8192, reached through SiServerKey(generic="n8192") = helm_si_ctx_create_ex with HELM_SI_CREATE_N8192.  n stays at 12
(every case is 12 rotation steps) and the batches small.  Every comparison is word for word against
oracle.Oracle64(..., use_ntt=True); tests/many_lut.py, tests/saturation.py and tests/pbs_first.py are imported as they are.

What the cases are for: the accumulator lives in a row of device memory per workgroup and the two columns of the external
product are computed one after the other, so a stale accumulator under column 1, a rotated read that is not ordered against
the step's writes, a column sum recentred at the wrong level, or rows shared between a primary and a lane or between the
chunks of a wide launch would all show as wrong words here."""
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import helm_amd
import oracle
from helm_amd import Circuit, EvalCircuit, LutCircuit, PtxtType, verilog_parser

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import many_lut as ML  # noqa: E402
import pbs_first as PF  # noqa: E402
import saturation as S  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET = os.path.join(ROOT, "tests", "netlists")
N = 8192

_keys, _oracles = {}, {}


def toy_key(l=2, logB=15, ks=(3, 5), seed=7):
    """si_toy_8192 (n = 12, message 8 x carry 8: t = 64) with another PBS or keyswitch decomposition."""
    key = (l, logB, ks, seed)
    if key not in _keys:
        p, lwe_std, glwe_std = helm_amd.si_named_params("si_toy_8192")
        p.pbs_l, p.pbs_logB, p.ks_l, p.ks_logB = l, logB, ks[0], ks[1]
        _keys[key] = helm_amd.SiClientKey(p, lwe_std, glwe_std, seed=seed)
    return _keys[key]


def oracle_of(ck):
    """One oracle per client key, shared."""
    if id(ck) not in _oracles:
        _oracles[id(ck)] = oracle.Oracle64(ck.params.as_tuple(), ck.bsk, ck.ksk, use_ntt=True)
    return _oracles[id(ck)]


def mask_word(a):
    """A word that modulus-switches to a (mod 2N)."""
    return np.uint64(a << (64 - N.bit_length()))


def n8192_key(ck, mode="n8192", **kw):
    sk = helm_amd.SiServerKey(ck, generic=mode, **kw)
    assert sk.kernel_class() == "n8192" and sk.field_bits() == 50
    return sk


@pytest.mark.parametrize("l,logB", [(2, 15), (1, 21), (3, 8)])
def test_bootstraps_word_for_word(l, logB):
    ck = toy_key(l, logB)
    p, t = ck.params, ck.t
    assert t == 64
    with pytest.raises(helm_amd.HelmError, match="unsupported"):
        helm_amd.SiServerKey(ck)                    # the default entry point keeps refusing N = 8192
    with pytest.raises(helm_amd.HelmError, match="N = 8192 are out of scope"):
        helm_amd.SiServerKey(ck, generic="large")   # ... and so does the large-N bit alone, in the words it had
    sk = n8192_key(ck)
    assert sk.round_capacity() > 0
    orc = oracle_of(ck)
    rng = np.random.default_rng(100 * l + logB)
    vals = np.arange(t, dtype=np.uint64)
    honest = np.array([orc.keyswitch(c) for c in ck.encrypt(vals)], dtype=np.uint64)
    zero = rng.integers(0, 2**64, size=(1, p.n + 1), dtype=np.uint64)
    zero[0, :p.n] = 0                               # no step is active
    rand = rng.integers(0, 2**64, size=(6, p.n + 1), dtype=np.uint64)
    # the modulus-switched mask words and body hit 0, 1, N - 1, N, N + 1, 2N - 1: one row per value, all words alike (low
    # bits random, below the rounding), and one row that walks through all of them
    edges = [0, 1, N - 1, N, N + 1, 2 * N - 1]
    craft = np.stack([np.full(p.n + 1, mask_word(a), dtype=np.uint64) for a in edges] +
                     [np.array([mask_word(edges[(i + 1) % 6]) for i in range(p.n + 1)], dtype=np.uint64)])
    craft |= rng.integers(0, 2**48, size=craft.shape, dtype=np.uint64)
    for row, a in zip(craft, edges):
        assert all(S.modswitch(int(w), N, 64) == a for w in row)
    assert [S.modswitch(int(w), N, 64) for w in craft[6]] == [edges[(i + 1) % 6] for i in range(p.n + 1)]
    small = np.concatenate([honest, zero, rand, craft])
    f = [lambda x: (3 * x + 1) % t, lambda x: x * x % t]
    luts = np.stack([sk.make_lut(f[0]), sk.make_lut(f[1])])
    idx = (np.arange(len(small)) % 2).astype(np.int32)
    big = sk.pbs_batch(small, luts, idx)
    for g in range(len(small)):
        assert np.array_equal(big[g], orc.bootstrap(small[g], luts[idx[g]])), g
    assert [int(v) for v in ck.decrypt_message_and_carry(big[:t])] == [f[g % 2](g) for g in range(t)]
    sk.close()


def test_a_launch_wider_than_a_round():
    """round_capacity() + 1 rows: the launch goes out in two chunks that share the context's accumulator rows.  The first
    row, the last row and the rows on both sides of the chunk boundary equal the oracle, and the boundary rows equal the
    same inputs launched alone."""
    ck = toy_key()
    sk = n8192_key(ck)
    cap = sk.round_capacity()
    import torch
    assert cap == torch.cuda.get_device_properties(0).multi_processor_count     # CUs x 1: one workgroup per CU
    orc = oracle_of(ck)
    rng = np.random.default_rng(cap)
    small = rng.integers(0, 2**64, size=(cap + 1, ck.params.n + 1), dtype=np.uint64)
    luts = np.stack([sk.make_lut(lambda x: (7 * x + 2) % ck.t), rng.integers(0, 2**64, size=N, dtype=np.uint64)])
    idx = (np.arange(cap + 1) % 2).astype(np.int32)
    big = sk.pbs_batch(small, luts, idx)
    for g in sorted({0, cap - 1, cap}):
        assert np.array_equal(big[g], orc.bootstrap(small[g], luts[idx[g]])), g
    edge = [cap - 1, cap]
    alone = sk.pbs_batch(small[edge], luts, idx[edge])
    assert np.array_equal(alone, big[edge])
    again = sk.pbs_batch(small, luts, idx)          # the rows hold whatever the last launch left: nothing of it is read
    assert np.array_equal(again, big)
    sk.close()


def test_a_lane_has_rows_of_its_own():
    """fork(): the same batch on the lane and on the primary, both equal to the oracle; then a wide look-up queued on the
    primary's stream right before the lane's launch - the lane's result is still the oracle's, and so is the primary's."""
    ck = toy_key()
    t = ck.t
    sk = n8192_key(ck, "allow+n8192")
    orc = oracle_of(ck)
    f = lambda x: (5 * x + 3) % t
    lut = sk.make_lut(f)[None]
    rng = np.random.default_rng(3)
    small = rng.integers(0, 2**64, size=(9, ck.params.n + 1), dtype=np.uint64)
    idx = np.zeros(9, dtype=np.int32)
    want = np.array([orc.bootstrap(r, lut[0]) for r in small], dtype=np.uint64)
    lane = sk.fork()
    assert lane.kernel_class() == "n8192" and lane.generic == "allow+n8192" and lane.field_bits() == 50
    assert lane.round_capacity() == sk.round_capacity()
    assert np.array_equal(sk.pbs_batch(small, lut, idx), want)
    assert np.array_equal(lane.pbs_batch(small, lut, idx), want)
    cap = sk.round_capacity()
    rows = cap + t
    w = sk.wires(2 * rows)
    vals = np.arange(rows, dtype=np.uint64) % t
    cts = ck.encrypt(vals)
    w.upload(np.arange(rows), cts)
    w.apply_luts(np.arange(rows), lut, np.arange(rows) + rows)     # queued on the primary's stream, not waited for
    got_lane = lane.pbs_batch(small, lut, idx)                       # ... while the lane launches on its own
    assert np.array_equal(got_lane, want)
    out = w.download(np.arange(rows) + rows)
    assert [int(v) for v in ck.decrypt_message_and_carry(out)] == [f(int(v)) for v in vals]
    for g in (0, cap - 1, cap, rows - 1):           # ... word for word on both sides of the primary's chunk boundary
        assert np.array_equal(out[g], orc.bootstrap(orc.keyswitch(cts[g]), lut[0])), g
    sk.close()


@pytest.mark.parametrize("ks", [(3, 5), (8, 3)], ids=["ks3x5", "ks8x3"])
def test_keyswitch_at_in_dim_8192(ks):
    """40 and 156 rows: the vector-ALU kernel, whose digit buffer would be 8192 x ks_l x 4 B unsliced (256 KiB at ks_l = 8);
    at these widths vector_geometry's grid clause slices it 16 ways already (the LDS clause is the next test's); 192 rows:
    the matrix-core kernel."""
    ck = toy_key(ks=ks, seed=11)
    sk = n8192_key(ck)
    orc = oracle_of(ck)
    rng = np.random.default_rng(ks[0])
    for rows in (40, 156, 192):
        src = rng.integers(0, 2**64, size=(rows, ck.dim + 1), dtype=np.uint64)
        src[:8] = ck.encrypt(np.arange(8, dtype=np.uint64))
        got = sk.keyswitch_batch(src)
        for g in range(rows):
            assert np.array_equal(got[g], orc.keyswitch(src[g])), (rows, g)
    sk.close()


def test_wide_vector_alu_keyswitch_is_sliced_for_lds():
    """vector_geometry's LDS clause: with HELM_HIP_KS_MFMA=0 every batch takes the vector-ALU kernel, and at 8 x CUs + 4 rows
    the grid clause asks for ONE slice (2 CUs + 1 workgroups already) - 256 KiB of digits at ks_l = 8, which no workgroup can
    have; the clause makes it two slices of 128 KiB.  Every row equals the matrix-core path's, three equal the oracle."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = 8 * cus + 4
    assert (rows + 3) // 4 >= 2 * cus and N * 8 * 4 > 160 * 1024 >= N // 2 * 8 * 4
    ck = toy_key(ks=(8, 3), seed=11)
    orc = oracle_of(ck)
    src = np.random.default_rng(8).integers(0, 2**64, size=(rows, ck.dim + 1), dtype=np.uint64)
    src[:8] = ck.encrypt(np.arange(8, dtype=np.uint64))
    old = os.environ.get("HELM_HIP_KS_MFMA")
    os.environ["HELM_HIP_KS_MFMA"] = "0"          # read when the context is created
    try:
        sk = n8192_key(ck)
    finally:
        if old is None:
            del os.environ["HELM_HIP_KS_MFMA"]
        else:
            os.environ["HELM_HIP_KS_MFMA"] = old
    got = sk.keyswitch_batch(src)
    sk.close()
    for g in (0, rows // 2, rows - 1):
        assert np.array_equal(got[g], orc.keyswitch(src[g])), g
    sk = n8192_key(ck)
    assert np.array_equal(sk.keyswitch_batch(src), got)
    sk.close()


def test_audit_hook_and_world_one_sharding():
    """The audit hook hands over the rows of a look-up batch (recomputed by the oracle), and helm_si_set_exchange at world 1
    with a callback - stage -> collective -> scatter, in rounds - leaves the table of the unsharded call."""
    import torch
    from helm_amd import _native as nv
    torch.cuda.set_device(0)
    ck = toy_key()
    t = ck.t
    sk = n8192_key(ck)
    orc = oracle_of(ck)
    lut = sk.make_lut(lambda x: (7 * x + 2) % t)[None]
    rows = 20
    cts = ck.encrypt(np.arange(rows, dtype=np.uint64) % t)

    def run():
        w = sk.wires(2 * rows)
        w.upload(np.arange(rows), cts)
        w.apply_luts(np.arange(rows), lut, np.arange(rows) + rows)
        return w.download()

    seen = {"luts": 0, "bad": 0}

    def audit(rec):
        if rec["kind"] == "luts":
            want = orc.apply_luts(rec["in_rows"][:4], rec["luts"], rec["lut_idx"][:4])
            seen["luts"] += 1
            seen["bad"] += int(np.sum(~np.all(want == rec["out_rows"][:4], axis=1)))
        return True

    sk.set_audit(audit)
    plain = run()
    sk.set_audit(None)
    assert seen == {"luts": 1, "bad": 0}, seen
    dev = torch.device("cuda", 0)
    sk.set_stream(torch.cuda.current_stream().cuda_stream)
    cap = 8
    stage = torch.zeros((cap, sk.dim + 1), dtype=torch.int64, device=dev)
    gather = torch.zeros((cap, sk.dim + 1), dtype=torch.int64, device=dev)
    calls = []

    def exchange(_user, n_rows):
        calls.append(int(n_rows))
        gather[:n_rows].copy_(stage[:n_rows])
        return 0

    fn = nv.SI_EXCHANGE_FN(exchange)
    nv.hip_check(nv.hip.helm_si_set_exchange(sk._h, 0, 1, 2, nv.vp(stage.data_ptr()), nv.vp(gather.data_ptr()), cap, fn, None))
    sharded = run()
    nv.hip_check(nv.hip.helm_si_set_exchange(sk._h, 0, 1, 1, None, None, 1, nv.SI_EXCHANGE_FN(0), None))
    assert calls == [8, 8, 4]
    assert np.array_equal(sharded, plain)
    assert [int(v) for v in ck.decrypt_message_and_carry(sharded[rows:])] == [(7 * v + 2) % t for v in range(rows)]
    sk.close()


@pytest.mark.parametrize("n_out", [2, 4])
def test_many_lut_every_output(n_out):
    """pbs_many_batch against tests/many_lut.py, as tests/test_gpu_large_n.py does at N = 4096: the mask words of every output
    from the oracle's coefficient-0 output, the bodies from the exact integer route (one honest row, one row with a single
    active step), the zero-mask closed form, the oracle (output 0) and decryption."""
    ck = toy_key()
    p, t = ck.params, ck.t
    sk = n8192_key(ck)
    orc = oracle_of(ck)
    shape = S.shape_of(p)
    M = ML.chunks(n_out)
    per = t // M
    assert per >= 8
    funcs = [lambda v, x=x: (3 * v + 5 * x + 1) % t for x in range(n_out)]
    tv = ML.many_lut_poly([[fn(v) for v in range(per)] for fn in funcs], t, N)
    assert np.array_equal(sk.make_many_lut(funcs), tv)
    rng = np.random.default_rng(n_out)
    honest = np.array([orc.keyswitch(c) for c in ck.encrypt(np.arange(per, dtype=np.uint64))], dtype=np.uint64)
    rand = np.zeros((1, p.n + 1), dtype=np.uint64)     # one active step, a random body
    rand[0, p.n // 2] = mask_word(N + 3)
    rand[0, p.n] = rng.integers(0, 2**64, dtype=np.uint64)
    bts = [0, 1, N - 1, N, 2 * N - 1]
    zero = np.zeros((len(bts), p.n + 1), dtype=np.uint64)
    for q, bt in enumerate(bts):
        zero[q, p.n] = mask_word(bt)
    small = np.concatenate([honest, rand, zero])
    exact_rows = [per]              # the integer route (seconds per active step at this N): the single-step row
    got = sk.pbs_many_batch(small, tv, n_out)
    assert got.shape == (len(small), n_out, N + 1)
    for r in range(len(small)):
        out0 = orc.bootstrap(small[r], tv)
        acc = ML.accumulator_exact(small[r], tv, ck.bsk, shape, 1) if r in exact_rows else None
        for x in range(n_out):
            h = ML.output_coefficient(x, n_out, N)
            assert h == x * N // M
            assert np.array_equal(got[r, x, :N], ML.masks_from_output0(out0, 1, N, h)), (r, x, "mask words")
            if r > per:
                assert not got[r, x, :N].any()
                assert got[r, x, N] == ML.zero_mask_body(tv, bts[r - per - 1], h), (r, x, "zero-mask body")
            elif acc is not None:
                assert np.array_equal(got[r, x], ML.extract_at(acc, h)), (r, x, "exact route")
            elif x == 0:
                assert got[r, x, N] == out0[N], (r, "body of output 0")
    dec = ck.decrypt_message_and_carry(got[:per].reshape(-1, N + 1)).reshape(per, n_out)
    assert [[int(v) for v in row] for row in dec] == [[fn(v) for fn in funcs] for v in range(per)]
    sk.close()


def test_at_the_exactness_bound_both_signs():
    """tests/saturation.py's construction for (k, N, l, logB) = (1, 8192, 1, 21), all columns, under one key: the positive
    extreme, the negative extreme and the one-column variant.  The largest exact column-sum coefficient of the saturating
    step is 2^20 x 2 x 8192 x (2^63 - 1) (key words 2^63 - 1, all signs aligned) resp. x 2^63 (key words -2^63): 0.547 of
    p0 p1 / 2 for the pair (FpG, FpI), as exact fractions; the shape's ceiling, (k+1) l N B/2 2^63, is the second of them.
    The kernel equals the Python-integer reference word for word, no tolerance."""
    ck = toy_key(1, 21)
    shape = S.shape_of(ck.params)
    assert shape == S.Shape(12, 1, N, 1, 21)
    case = S.launch_case(shape, 64, ck.bsk)
    half = Fraction(S.FPG * S.FPI, 2)
    ceiling = Fraction(S.capacity_bound(shape, 64)) / half
    assert ceiling == Fraction(2**98, S.FPG * S.FPI) and Fraction(546, 1000) < ceiling < Fraction(548, 1000)
    fractions = [Fraction(pk) / half for pk in case["peak"]]
    print("fractions of p0 p1 / 2:", [float(v) for v in fractions])
    assert fractions[0] == Fraction(2**20 * 2 * N * (2**63 - 1)) / half     # positive extreme
    assert fractions[1] == ceiling                                           # negative extreme: words of -2^63
    assert fractions[2] == fractions[0]                                      # one column saturated
    assert all(Fraction(1, 2) <= v <= ceiling for v in fractions)
    orc = oracle.Oracle64(ck.params.as_tuple(), case["bsk"], ck.ksk, use_ntt=True)
    rng = np.random.default_rng(17)
    lwe = np.concatenate([case["lwe"], rng.integers(0, 2**64, size=(3, shape.n + 1), dtype=np.uint64)])
    tvs = np.stack([case["tv"], rng.integers(0, 2**64, size=N, dtype=np.uint64)])
    idx = np.array([0, 0, 0, 1, 0, 1], dtype=np.int32)
    sk = helm_amd.SiServerKey(params=ck.params, bsk=case["bsk"], ksk=ck.ksk, generic="n8192")
    assert sk.kernel_class() == "n8192"
    got = sk.pbs_batch(lwe, tvs, idx)
    assert np.array_equal(got[:3], case["ref"]), "the saturating rows differ from the integer reference"
    for g in range(len(lwe)):  # the oracle agrees on the saturating rows, and holds the honest controls under the same key
        assert np.array_equal(got[g], orc.bootstrap(lwe[g], tvs[idx[g]])), g
    sk.close()


def test_bootstrap_first_order():
    """order="pbs_ks" beside the bit: look-ups read small rows of the wire table in place, against tests/pbs_first.py;
    permuted, non-contiguous output rows in a table larger than the batch, the other rows untouched."""
    ck = toy_key()
    t = ck.t
    sk = n8192_key(ck, order="pbs_ks")
    assert (sk.pbs_order(), sk.wire_words()) == (0, ck.params.n + 1)
    ref = PF.PbsFirst(oracle_of(ck))
    rows = ck.encrypt(np.arange(8, dtype=np.uint64), small=True)
    luts = np.stack([sk.make_lut(lambda v: (5 * v + 3) % t), sk.make_lut(lambda v: (t - 1 - v) % t)])
    W = 11
    rng = np.random.default_rng(23)
    expect = rng.integers(0, 2**64, size=(8 + 2 * W + 3, sk.wire_words()), dtype=np.uint64)
    expect[:8] = rows
    w = sk.wires(len(expect))
    w.upload(np.arange(len(expect)), expect)
    in_idx = rng.integers(0, 8, size=W).astype(np.int32)
    lut_idx = rng.integers(0, 2, size=W).astype(np.int32)
    out_idx = (8 + 1 + 2 * rng.permutation(W)).astype(np.int32)
    w.apply_luts(in_idx, luts, out_idx, lut_idx)
    got = w.download()
    memo = {}
    for g in range(W):
        key = (int(in_idx[g]), int(lut_idx[g]))
        if key not in memo:
            memo[key] = ref.apply_lut_small(rows[key[0]], luts[key[1]])
        expect[out_idx[g]] = memo[key]
    assert np.array_equal(got, expect)
    dec = ck.decrypt_message_and_carry(got[out_idx], small=True)
    fs = [lambda v: (5 * v + 3) % t, lambda v: (t - 1 - v) % t]
    assert [int(v) for v in dec] == [fs[int(lut_idx[g])](int(in_idx[g])) for g in range(W)]
    sk.close()


def _circuit(path):
    gs, ws, ins, outs, d, _, _ = verilog_parser.read_verilog_file(path, False)
    c = Circuit(gs, ins, outs, d)
    c.sort_circuit()
    c.compute_levels()
    return c, ws


@pytest.mark.parametrize("bits", [0b10110110, 0b01001101])
def test_lut_mode_six_input_gates(bits):
    """tests/netlists/lut6-two-levels.v: six 6-input gates and one 3-input gate over two levels.  Every wire equals the
    plaintext evaluator; one blind rotation per gate (2^6 = t), without a wide-LUT key."""
    ck = toy_key()
    sk = n8192_key(ck)
    c, ws = _circuit(os.path.join(NET, "lut6-two-levels.v"))
    inputs = {name: PtxtType.Bool((bits >> i) & 1) for i, name in enumerate("abcdefgh")}
    ptxt = c.evaluate(c.initialize_wire_map(ws, inputs, "bool"))
    lc = LutCircuit(ck, sk, c)
    sk.timing_enable(True)
    sk.timing(reset=True)
    enc = EvalCircuit.evaluate_encrypted(lc, EvalCircuit.encrypt_inputs(lc, ws, inputs), 1, "bool")
    sk.sync()
    assert int(sk.timing().pbs_count) == 7 == lc.pbs_per_cycle()
    for wire, want in ptxt.items():
        assert ck.decrypt(enc[wire]) == int(bool(want)), wire
    sk.close()


def test_wop_refuses_an_n8192_pbs_side():
    from helm_amd import wopbs
    ck = toy_key()
    sk = n8192_key(ck)
    wp, _, _ = wopbs.wop_named_params("wop_toy_512")
    with pytest.raises(helm_amd.HelmError, match="HELM_SI_CREATE_N8192"):
        wopbs.WopServerKey(sk, params=wp)
    sk.close()


CHILD = r"""
import json, sys
sys.path.insert(0, %r)
import helm_amd
res = {}
p, _, _ = helm_amd.si_named_params("si_toy_8192")
for mode in ("n8192", "force+n8192"):
    try:
        helm_amd.SiServerKey(params=p, generic=mode).close()
        res[mode] = "created"
    except helm_amd.HelmError as e:
        res[mode] = str(e)
sk = helm_amd.SiServerKey(params=helm_amd.si_named_params("si_toy_512")[0], generic="n8192")  # the tuned class is unaffected
res["tuned"] = sk.kernel_class()
sk.close()
print("RESULT " + json.dumps(res))
"""


def test_check_build_refuses_n8192_contexts_before_any_launch():
    """The bound-checking build runs the tuned kernels only: context creation refuses class 3 there, by the bit's name, and
    launches nothing."""
    lib = os.path.join(ROOT, "helm_amd", "csrc", "libhelm_hip_check.so")
    assert os.path.exists(lib), "make -C helm_amd/csrc libhelm_hip_check.so"
    env = dict(os.environ, HELM_HIP_LIB=lib)
    p = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    for mode in ("n8192", "force+n8192"):
        assert "bound-checking build" in res[mode] and "HELM_SI_CREATE_N8192" in res[mode], res
    assert res["tuned"] == "tuned"
