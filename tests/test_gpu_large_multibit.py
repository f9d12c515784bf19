"""The multi-bit form of the two large-N blind-rotate kernels of the 64-bit engine (k_pbs64_large<12, g>,
k_pbs64_n8192<g>; helm_amd/csrc/helm_pbs64_large_core.inc, helm_pbs64_large.inc, helm_pbs64_n8192.inc), reached through
SiServerKey(generic="large+multibit" | "n8192+multibit" | "large+n8192+multibit") = helm_si_ctx_create_ex with
HELM_SI_CREATE_LARGE_MULTIBIT.  n stays at 12 (4 or 6 group steps) and the batches small.  Every comparison is word for word
against oracle.Oracle64(..., use_ntt=True); tests/many_lut.py, tests/pbs_first.py and tests/saturation_mb.py are imported as
they are, the last through tests/saturation_mb_large.py, which places its keys by the half of THIS pair of fields.

What the cases are for: a group that is skipped when its rotations are all 0, a subset sum taken without its reduction mod
2N, a lift that is added instead of replacing the accumulator, a wrong exponent of the evaluation point of a spectrum
position, a column 1 that sees column 0's result, or a sum recentred too late would all show as wrong words here."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

import helm_amd
import oracle
from helm_amd import Circuit, EvalCircuit, LutCircuit, PtxtType, verilog_parser
from helm_amd import _native as nv

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import many_lut as ML  # noqa: E402
import pbs_first as PF  # noqa: E402
import saturation as S  # noqa: E402
import saturation_mb_large as MBL  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET = os.path.join(ROOT, "tests", "netlists")
MODE = {4096: "large+multibit", 8192: "n8192+multibit"}
CLASS = {4096: "large", 8192: "n8192"}

# (N, g, l, logB): each instantiation at one level near the loader's limit, at tfhe's 15 x 2 and at three levels
INSTANCES = [(4096, 2, 1, 21), (4096, 3, 1, 20), (4096, 3, 2, 15), (4096, 2, 3, 8),
             (8192, 3, 2, 15), (8192, 2, 2, 15), (8192, 2, 1, 20), (8192, 3, 3, 8)]

_keys, _oracles = {}, {}


def toy_key(N, g, l=None, logB=None, seed=7):
    """si_toy_<N>_mb<g> (n = 12) with another PBS decomposition."""
    key = (N, g, l, logB, seed)
    if key not in _keys:
        p, lwe_std, glwe_std = helm_amd.si_named_params("si_toy_%d_mb%d" % (N, g))
        if l is not None:
            p.pbs_l, p.pbs_logB = l, logB
        _keys[key] = helm_amd.SiClientKey(p, lwe_std, glwe_std, seed=seed)
    return _keys[key]


def oracle_of(ck, use_ntt=True):
    """One oracle per client key of toy_key (kept alive in _keys, so that its id stays its own) and route, shared."""
    assert any(ck is v for v in _keys.values())
    if (id(ck), use_ntt) not in _oracles:
        _oracles[id(ck), use_ntt] = oracle.Oracle64(ck.params.as_tuple(), ck.bsk, ck.ksk, use_ntt=use_ntt)
    return _oracles[id(ck), use_ntt]


def mask_word(a, N):
    """A word that modulus-switches to a (mod 2N)."""
    return np.uint64(a << (64 - N.bit_length()))


def server_key(ck, mode=None, **kw):
    N = ck.params.N
    sk = helm_amd.SiServerKey(ck, generic=mode or MODE[N], **kw)
    assert sk.kernel_class() == CLASS[N] and sk.field_bits() == 50
    return sk


def crafted_rows(N, g, n, rng):
    """Rows that reach the group step's corners: no rotation at all (no group may be skipped: the result still equals the
    oracle's), one member of one group non-zero, members whose subset sums wrap past 2N, and the modulus-switch edges of
    tests/test_gpu_n8192.py (one row per value, all words alike, and one row that walks through them)."""
    zero = rng.integers(0, 2**64, size=(1, n + 1), dtype=np.uint64)
    zero[0, :n] = 0
    one = np.zeros((1, n + 1), dtype=np.uint64)
    one[0, g + 1] = mask_word(N + 3, N)                       # member 1 of group 1
    one[0, n] = rng.integers(0, 2**64, dtype=np.uint64)
    wrap = rng.integers(0, 2**64, size=(1, n + 1), dtype=np.uint64)
    members = [N, 2 * N - 1] if g == 2 else [N, 1, 2 * N - 1]
    wrap[0, :n] = np.resize([mask_word(a, N) for a in members], n)
    edges = [0, 1, N - 1, N, N + 1, 2 * N - 1]
    craft = np.stack([np.full(n + 1, mask_word(a, N), dtype=np.uint64) for a in edges] +
                     [np.array([mask_word(edges[(i + 1) % 6], N) for i in range(n + 1)], dtype=np.uint64)])
    craft |= rng.integers(0, 2**48, size=craft.shape, dtype=np.uint64)
    for row, a in zip(craft, edges):
        assert all(S.modswitch(int(w), N, 64) == a for w in row)
    assert [S.modswitch(int(w), N, 64) for w in wrap[0, :g]] == members
    assert (2 * N - 1) + N >= 2 * N
    return np.concatenate([zero, one, wrap, craft])


@pytest.mark.parametrize("N,g,l,logB", INSTANCES, ids=["N%d_g%d_l%d_B%d" % c for c in INSTANCES])
def test_bootstraps_word_for_word(N, g, l, logB):
    ck = toy_key(N, g, l, logB)
    p, t = ck.params, ck.t
    assert (p.n, p.grouping_factor, t) == (12, g, N // 128)
    with pytest.raises(helm_amd.HelmError, match="out of scope"):
        helm_amd.SiServerKey(ck, generic=CLASS[N])          # without the flag the bit of this N refuses in its old words
    sk = server_key(ck)
    orc = oracle_of(ck)
    rng = np.random.default_rng(1000 * g + 100 * l + logB + N)
    vals = np.arange(t, dtype=np.uint64)
    honest = np.array([orc.keyswitch(c) for c in ck.encrypt(vals)], dtype=np.uint64)
    rand = rng.integers(0, 2**64, size=(6, p.n + 1), dtype=np.uint64)
    small = np.concatenate([honest, rand, crafted_rows(N, g, p.n, rng)])
    f = [lambda x: (3 * x + 1) % t, lambda x: x * x % t]
    luts = np.stack([sk.make_lut(f[0]), sk.make_lut(f[1])])
    idx = (np.arange(len(small)) % 2).astype(np.int32)
    want = np.array([orc.bootstrap(small[r], luts[idx[r]]) for r in range(len(small))], dtype=np.uint64)
    big = sk.pbs_batch(small, luts, idx)
    for r in range(len(small)):
        assert np.array_equal(big[r], want[r]), r
    assert [int(v) for v in ck.decrypt_message_and_carry(big[:t])] == [f[r % 2](r) for r in range(t)]
    # launches of width 1 and 5: every crafted row alone, and the rows from the zero-mask row on in fives
    first = t + 6
    for r in range(first, len(small)):
        assert np.array_equal(sk.pbs_batch(small[r:r + 1], luts, idx[r:r + 1])[0], want[r]), (r, "width 1")
    for r in range(first, len(small) - 4, 5):
        assert np.array_equal(sk.pbs_batch(small[r:r + 5], luts, idx[r:r + 5]), want[r:r + 5]), (r, "width 5")
    if (N, g, l) == (4096, 3, 1):                            # one case against the schoolbook route as well
        plain = oracle_of(ck, use_ntt=False)
        for r in (0, t + 1, first, first + 1, first + 2, len(small) - 1):
            assert np.array_equal(plain.bootstrap(small[r], luts[idx[r]]), want[r]), (r, "schoolbook")
    sk.close()


@pytest.mark.parametrize("g", [2, 3])
def test_a_launch_wider_than_a_round(g):
    """N = 8192, round_capacity() + 1 rows: two chunks that share the context's accumulator rows.  The first row, the last
    row and the rows on both sides of the chunk boundary equal the oracle; the boundary rows equal the same inputs alone."""
    import torch
    ck = toy_key(8192, g)
    sk = server_key(ck)
    cap = sk.round_capacity()
    assert cap == torch.cuda.get_device_properties(0).multi_processor_count
    orc = oracle_of(ck)
    rng = np.random.default_rng(cap + g)
    small = rng.integers(0, 2**64, size=(cap + 1, ck.params.n + 1), dtype=np.uint64)
    small[cap - 1, :ck.params.n] = 0                         # a zero-mask row at the end of the first chunk
    luts = np.stack([sk.make_lut(lambda x: (7 * x + 2) % ck.t), rng.integers(0, 2**64, size=8192, dtype=np.uint64)])
    idx = (np.arange(cap + 1) % 2).astype(np.int32)
    big = sk.pbs_batch(small, luts, idx)
    for r in sorted({0, cap - 1, cap}):
        assert np.array_equal(big[r], orc.bootstrap(small[r], luts[idx[r]])), r
    edge = [cap - 1, cap]
    assert np.array_equal(sk.pbs_batch(small[edge], luts, idx[edge]), big[edge])
    assert np.array_equal(sk.pbs_batch(small, luts, idx), big)
    sk.close()


def _uniform_key_below(p, bits, seed):
    """Uniform key words below 2^bits in magnitude, both signs: a key of the context's size that the loader's rule admits."""
    rng = np.random.default_rng(seed)
    g = p.grouping_factor
    words = (p.n // g << g) * p.pbs_l * 4 * p.N
    v = rng.integers(-(1 << bits), 1 << bits, size=words, dtype=np.int64)
    return v.view(np.uint64)


@pytest.mark.parametrize("N,logB", [(8192, 21), (4096, 22)])
def test_loader_refuses_an_honest_key_beyond_the_group_sum_rule(N, logB):
    """One level of 21 bits at N = 8192 (22 at N = 4096) with grouping factor 2 is admitted at creation - the classical bound,
    a necessary condition - and an honest key is refused at load: its group sums are near 2^98 against a half of 2^97.87.
    HELM_ERR_INVALID, "capacity", the kernel's name and the ratio; the key the context had keeps running."""
    ck = toy_key(N, 2, 1, logB)
    p = ck.params
    with pytest.raises(helm_amd.HelmError, match="capacity"):
        helm_amd.SiServerKey(ck, generic=MODE[N])
    bound = MBL.loader_bound(ck.bsk, MBL.MbShape(1, N, 1, logB, 2))
    assert MBL.over_threshold(bound)
    small_key = _uniform_key_below(p, 61, seed=N)
    sk = helm_amd.SiServerKey(params=p, bsk=small_key, ksk=ck.ksk, generic=MODE[N])
    assert sk.kernel_class() == CLASS[N]
    orc = oracle.Oracle64(p.as_tuple(), small_key, ck.ksk, use_ntt=True)
    rng = np.random.default_rng(logB)
    small = rng.integers(0, 2**64, size=(3, p.n + 1), dtype=np.uint64)
    lut = rng.integers(0, 2**64, size=(1, N), dtype=np.uint64)
    got = sk.pbs_batch(small, lut)
    for r in range(3):
        assert np.array_equal(got[r], orc.bootstrap(small[r], lut[0])), r
    bsk = np.ascontiguousarray(ck.bsk, dtype=np.uint64)
    rc = nv.hip.helm_si_load_bootstrap_key(sk._h, nv.as_u64p(bsk), bsk.size)
    err = nv.hip.helm_hip_last_error()
    assert rc == -1 and b"capacity" in err and (b"N = 8192 multi-bit kernel" if N == 8192 else b"large-N multi-bit kernel") in err
    assert (MBL.printed_ratio(bound) + " of p0 p1 / 2").encode() in err, (err, MBL.printed_ratio(bound))
    assert np.array_equal(sk.pbs_batch(small, lut), got)     # the old key, untouched
    sk.close()


SAT_CASES = [(s, sign) for s in MBL.LARGE for sign in (+1, -1)]


@pytest.mark.parametrize("s,sign", SAT_CASES, ids=["%s%s" % (MBL.shape_id(s), "+" if sg > 0 else "-") for s, sg in SAT_CASES])
def test_at_the_exactness_bound(s, sign):
    """tests/saturation_mb.py's construction (three groups, n = 3 g) with the key at 0.998 of the loader's threshold for the
    pair FpG x FpI: the saturating row (sign -1: masks whose subset sums wrap), the zero-mask row and two controls equal the
    Python-integer reference word for word; the reached fraction of p0 p1 / 2 is asserted from exact integers
    (tests/test_large_multibit_bounds.py pins the reference against both oracle routes on the CPU)."""
    L = MBL.launch(s, sign)
    case = L["case"]
    peak = L["peaks"][0][1]
    bound = MBL.loader_bound(L["bsk"], s)
    assert peak == MBL.expected_peak(case, s) == bound and not MBL.over_threshold(bound)
    frac = Fraction(2 * peak, MBL.HALF2)
    print("reached fraction of p0 p1 / 2:", float(frac))
    unit = (1 << (s.logB - 1)) * (1 << s.g) * s.l * (s.k + 1)
    assert 0 <= MBL.budget_of(MBL.RATIO) - peak < unit
    assert Fraction(MBL.budget_of(MBL.RATIO) - unit, 1) * 2 / MBL.HALF2 < frac <= Fraction(998, 1001)
    assert "%.5f" % frac == "0.99700"
    p, _, _ = helm_amd.si_named_params("si_toy_%d_mb%d" % (s.N, s.g))
    p.n, p.pbs_l, p.pbs_logB, p.ks_l, p.ks_logB = 3 * s.g, s.l, s.logB, 4, 4
    ksk = np.zeros(s.N * 4 * (3 * s.g + 1), dtype=np.uint64)
    sk = helm_amd.SiServerKey(params=p, bsk=L["bsk"], ksk=ksk, generic=MODE[s.N])
    assert sk.kernel_class() == CLASS[s.N] and sk.field_bits() == 50
    try:
        got = sk.pbs_batch(L["lwe"], L["tv"])
        bad = [r for r in range(4) if not np.array_equal(got[r], L["ref"][r])]
        assert not set(bad) & set(MBL.CONTROLS), f"a control row differs (rows differing: {bad}): key layout of the test?"
        assert not bad, f"rows {bad} differ while the control rows are exact: wrong at the bound"
    finally:
        sk.close()


@pytest.mark.parametrize("N", [4096, 8192])
def test_many_lut_every_output(N):
    """pbs_many_batch with n_out = 2 under grouping factor 3: the mask words of every output from the oracle's
    coefficient-0 output, the bodies of one row from the exact integer route (tests/many_lut.py: every group step runs), the
    body of output 0 from the oracle, and decryption of every output."""
    n_out = 2
    ck = toy_key(N, 3)
    p, t = ck.params, ck.t
    sk = server_key(ck)
    orc = oracle_of(ck)
    per = t // ML.chunks(n_out)
    funcs = [lambda v, x=x: (3 * v + 5 * x + 1) % t for x in range(n_out)]
    tv = ML.many_lut_poly([[fn(v) for v in range(per)] for fn in funcs], t, N)
    assert np.array_equal(sk.make_many_lut(funcs), tv)
    rng = np.random.default_rng(N)
    honest = np.array([orc.keyswitch(c) for c in ck.encrypt(np.arange(per, dtype=np.uint64))], dtype=np.uint64)
    rand = rng.integers(0, 2**64, size=(1, p.n + 1), dtype=np.uint64)
    zero = np.zeros((1, p.n + 1), dtype=np.uint64)
    zero[0, p.n] = mask_word(N + 1, N)
    small = np.concatenate([honest, rand, zero])
    got = sk.pbs_many_batch(small, tv, n_out)
    assert got.shape == (len(small), n_out, N + 1)
    acc = ML.accumulator_exact(small[per], tv, ck.bsk, S.shape_of(p), 3)
    for r in range(len(small)):
        out0 = orc.bootstrap(small[r], tv)
        for x in range(n_out):
            h = ML.output_coefficient(x, n_out, N)
            assert np.array_equal(got[r, x, :N], ML.masks_from_output0(out0, 1, N, h)), (r, x, "mask words")
            if r == per:
                assert np.array_equal(got[r, x], ML.extract_at(acc, h)), (r, x, "exact route")
            elif x == 0:
                assert got[r, x, N] == out0[N], (r, "body of output 0")
    dec = ck.decrypt_message_and_carry(got[:per].reshape(-1, N + 1)).reshape(per, n_out)
    assert [[int(v) for v in row] for row in dec] == [[fn(v) for fn in funcs] for v in range(per)]
    sk.close()


@pytest.mark.parametrize("N", [4096, 8192])
def test_bootstrap_first_order(N):
    """order="pbs_ks" beside the flag: look-ups read small rows of the wire table in place, against tests/pbs_first.py."""
    ck = toy_key(N, 2)
    t = ck.t
    sk = server_key(ck, order="pbs_ks")
    assert (sk.pbs_order(), sk.wire_words()) == (0, ck.params.n + 1)
    ref = PF.PbsFirst(oracle_of(ck))
    rows = ck.encrypt(np.arange(8, dtype=np.uint64), small=True)
    fs = [lambda v: (5 * v + 3) % t, lambda v: (t - 1 - v) % t]
    luts = np.stack([sk.make_lut(fs[0]), sk.make_lut(fs[1])])
    W = 7
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
    for q in range(W):
        expect[out_idx[q]] = ref.apply_lut_small(rows[int(in_idx[q])], luts[int(lut_idx[q])])
    assert np.array_equal(got, expect)
    dec = ck.decrypt_message_and_carry(got[out_idx], small=True)
    assert [int(v) for v in dec] == [fs[int(lut_idx[q])](int(in_idx[q])) for q in range(W)]
    sk.close()


def test_a_lane_with_a_primary_launch_queued_before_it():
    """N = 8192: fork() gives the lane accumulator rows of its own.  A look-up wider than a round is queued on the primary's
    stream right before the lane launches on its own; both results are the oracle's."""
    ck = toy_key(8192, 3)
    t = ck.t
    sk = server_key(ck, "large+n8192+multibit")
    orc = oracle_of(ck)
    f = lambda x: (5 * x + 3) % t                           # noqa: E731
    lut = sk.make_lut(f)[None]
    rng = np.random.default_rng(3)
    small = rng.integers(0, 2**64, size=(9, ck.params.n + 1), dtype=np.uint64)
    want = np.array([orc.bootstrap(r, lut[0]) for r in small], dtype=np.uint64)
    lane = sk.fork()
    assert lane.kernel_class() == "n8192" and lane.generic == "large+n8192+multibit" and lane.field_bits() == 50
    assert np.array_equal(lane.pbs_batch(small, lut), want)
    cap = sk.round_capacity()
    rows = cap + 8
    w = sk.wires(2 * rows)
    vals = np.arange(rows, dtype=np.uint64) % t
    cts = ck.encrypt(vals)
    w.upload(np.arange(rows), cts)
    w.apply_luts(np.arange(rows), lut, np.arange(rows) + rows)     # queued on the primary's stream, not waited for
    got_lane = lane.pbs_batch(small, lut)                            # ... while the lane launches on its own
    assert np.array_equal(got_lane, want)
    out = w.download(np.arange(rows) + rows)
    assert [int(v) for v in ck.decrypt_message_and_carry(out)] == [f(int(v)) for v in vals]
    for r in (0, cap - 1, cap, rows - 1):
        assert np.array_equal(out[r], orc.bootstrap(orc.keyswitch(cts[r]), lut[0])), r
    sk.close()


def _circuit(path):
    gs, ws, ins, outs, d, _, _ = verilog_parser.read_verilog_file(path, False)
    c = Circuit(gs, ins, outs, d)
    c.sort_circuit()
    c.compute_levels()
    return c, ws


def test_lut_mode_six_input_gates():
    """tests/netlists/lut6-two-levels.v through LutCircuit under si_toy_8192_mb3: every wire equals the plaintext evaluator,
    one blind rotation per gate."""
    ck = helm_amd.SiClientKey.generate("si_toy_8192_mb3", seed=5)
    sk = server_key(ck)
    c, ws = _circuit(os.path.join(NET, "lut6-two-levels.v"))
    bits = 0b10110110
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


@pytest.mark.parametrize("N", [4096, 8192])
def test_the_flag_changes_no_classical_rows(N):
    """A classical context (grouping factor 0) created with the flag returns the words of one created without it."""
    ck = helm_amd.SiClientKey.generate("si_toy_%d" % N, seed=7)
    assert ck.params.grouping_factor == 0
    rng = np.random.default_rng(N)
    small = rng.integers(0, 2**64, size=(5, ck.params.n + 1), dtype=np.uint64)
    small[4, :ck.params.n] = 0
    luts = rng.integers(0, 2**64, size=(1, N), dtype=np.uint64)
    rows = []
    for mode in (CLASS[N], MODE[N], "large+n8192+multibit"):
        sk = server_key(ck, mode)
        rows.append(sk.pbs_batch(small, luts))
        sk.close()
    assert np.array_equal(rows[0], rows[1]) and np.array_equal(rows[0], rows[2])
    orc = oracle.Oracle64(ck.params.as_tuple(), ck.bsk, ck.ksk, use_ntt=True)    # (this key is not one of toy_key's)
    assert np.array_equal(rows[0][0], orc.bootstrap(small[0], luts[0]))
