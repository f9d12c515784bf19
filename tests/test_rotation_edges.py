"""tests/rotation_edges.py pinned on the CPU: its words against the three modulus switches (the Python one of
tests/saturation.py and both oracles'), its gate formulas against oracle.lincomb, and the oracles against exact integers
(saturation.bootstrap_exact, saturation_mb.bootstrap_mb_exact: Python integers, schoolbook products) on the very row families
tests/test_gpu_rotation_edges.py runs on the kernels - so that a row that differs there is an error of the engine.

The exact route costs 6 - 10 ms per active step up to N = 1024, 90 ms at N = 4096 and 0.6 s at N = 8192 (its digit loop is
Python), so: every amount at N = 512, the edge set at N = 1024 / 2048 / 4096, four amounts at N = 8192, and the rows with
every mask word alike at n = 2 (the same words, fewer steps)."""
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rotation_edges as RE  # noqa: E402
import saturation as S  # noqa: E402
import saturation_mb as M  # noqa: E402


def _orc64_modswitch(x, log2_2n):
    return int(oracle.lib64().orc64_modswitch(int(x), int(log2_2n)))


@pytest.mark.parametrize("N", [256, 512, 1024, 2048, 4096, 8192])
def test_word_for_switches_to_its_amount_in_all_three_restatements(N):
    log2_2n = (2 * N).bit_length() - 1
    for width, switch in ((32, oracle.modswitch), (64, _orc64_modswitch)):
        h = RE.half_step(N, width)
        assert h >= 2 and h * 4 * N == 1 << width
        for a in RE.ALL(N):
            words = [RE.word_for(a, N, width, f) for f in RE.FLAVOURS]      # (asserts S.modswitch(word) == a itself)
            assert [switch(w, log2_2n) for w in words] == [a, a, a], (width, a)
            # the neighbours: one more than "below" is the next amount's tie, one less than "tie" is the amount before
            assert words[1] + 1 == RE.word_for(a + 1, N, width, "tie") or a == 2 * N - 1
            below_tie = (words[2] - 1) % (1 << width)
            assert S.modswitch(below_tie, N, width) == switch(below_tie, log2_2n) == (a - 1) % (2 * N)
        assert RE.word_for(0, N, width, "tie") == (1 << width) - h
    assert set(RE.E(N)) <= set(RE.R(N)) <= set(RE.ALL(N)) and len(RE.E(N)) == 22
    assert {a % 64 for a in RE.R(N)} == set(range(64)) and len(RE.R(N)) <= 86


@pytest.mark.parametrize("n,N", [(24, 512), (16, 1024), (16, 256), (16, 2048)])
def test_gate_formulas_against_the_oracle(n, N):
    assert (RE.AND, RE.MUX, RE.NAND, RE.NOR, RE.OR, RE.XNOR, RE.XOR) == \
        (oracle.AND, oracle.MUX, oracle.NAND, oracle.NOR, oracle.OR, oracle.XNOR, oracle.XOR)
    G = RE.gate_rows(n, N, RE.E(N), np.random.default_rng(N))
    count = len(G["op"])
    assert count == len(RE.E(N)) * 3 * (6 + 2 + 2)               # XOR and XNOR twice: both pre-images
    for q in range(count):
        got = oracle.lincomb(n, G["op"][q], G["which"][q], G["l"][q], G["r"][q], G["c"][q])
        assert np.array_equal(got, G["want"][q]), q
        assert RE.lincomb(G["op"][q], G["which"][q], G["l"][q], G["r"][q], G["c"][q], n) == [int(v) for v in got]
    # what the construction promises: sums past 2^32 under every op, both pre-images of the doubling, odd words replaced
    assert all(G["wraps"][k] >= 10 for k in RE.GATE_OPS)
    for op in (RE.XOR, RE.XNOR):
        assert {p for o, p in zip(G["op"], G["preimage"]) if o == op} == {0, 1}
    # "below" (a 2h + h - 1) is the one odd flavour: (n + 1) words x targets x 2 ops x 2 pre-images
    assert G["replaced"] == (n + 1) * len(RE.E(N)) * 4
    # the other MUX half of a case is an ordinary random row
    mux = [q for q in range(count) if G["op"][q] == RE.MUX]
    other = RE.lincomb(RE.MUX, 1 - G["which"][mux[0]], G["l"][mux[0]], G["r"][mux[0]], G["c"][mux[0]], n)
    assert other != [int(v) for v in G["want"][mux[0]]]


def _random_key(shape, width, seed):
    return S._random_key(shape, width, seed).reshape(-1)


def _oracles(shape, width, bsk):
    if width == 32:
        t7 = (shape.n, shape.k, shape.N, shape.l, shape.logB, 4, 4)
        ksk = np.zeros(1, dtype=np.uint32)
        return [("schoolbook", oracle.Oracle(t7, bsk, ksk, use_ntt=False).bootstrap_noks),
                ("Goldilocks", oracle.Oracle(t7, bsk, ksk, use_ntt=True).bootstrap_noks)]
    t10 = (shape.n, shape.k, shape.N, shape.l, shape.logB, 4, 4, 4, 4, 1)
    ksk = np.zeros(1, dtype=np.uint64)
    return [("schoolbook", oracle.Oracle64(t10, bsk, ksk, use_ntt=False).bootstrap),
            ("split-key Goldilocks", oracle.Oracle64(t10, bsk, ksk, use_ntt=True).bootstrap)]


def _pin(shape, width, lwe, seed):
    """Every row: exact integers == both oracle routes."""
    bsk = _random_key(shape, width, seed)
    tv = np.random.default_rng(seed + 1).integers(0, 1 << width, size=shape.N, dtype=RE.dtype_of(width))
    routes = _oracles(shape, width, bsk)
    for q in range(len(lwe)):
        ref, _ = S.bootstrap_exact(lwe[q], tv, bsk, shape, width)
        for name, boot in routes:
            assert np.array_equal(boot(lwe[q], tv), ref), (name, q, [S.modswitch(int(w), shape.N, width) for w in lwe[q]])


@pytest.mark.parametrize("shape,width", [(S.NAMED32["toy"], 32), (S.NAMED64["si_toy_512"], 64)], ids=["toy", "si_toy_512"])
def test_oracles_equal_exact_integers_at_every_amount(shape, width):
    lwe, flav = RE.mask_sweep(shape, RE.ALL(shape.N), width, np.random.default_rng(1))
    assert len(lwe) == 2 * shape.N and {flav[a] for a in (0, 1, 2)} == set(RE.FLAVOURS)
    _pin(shape, width, lwe, 7)
    # the row that walks through the edges at the set's own n (every step active), and the all-alike rows of N - 1, N, N + 1
    const, amounts = RE.constant_rows(shape, width, np.random.default_rng(11))
    rows = [amounts.index(a) for a in (shape.N - 1, shape.N, shape.N + 1)] + [len(const) - 1]
    walked = [S.modswitch(int(w), shape.N, width) for w in const[-1, :shape.n]]
    assert walked == [RE.E(shape.N)[(i + 1) % 22] for i in range(shape.n)] and len(set(walked)) == min(shape.n, 22)
    _pin(shape, width, const[rows], 12)


EDGE_SHAPES = [(S.NAMED32["toy_1024"], 32), (S.Shape(16, 1, 2048, 3, 5), 32), (S.NAMED64["si_toy_1024"], 64),
               (S.NAMED64["si_toy_2048_l2"], 64), (S.Shape(12, 1, 4096, 1, 22), 64)]


@pytest.mark.parametrize("shape,width", EDGE_SHAPES, ids=["%d-N%d_l%d" % (w, s.N, s.l) for s, w in EDGE_SHAPES])
def test_oracles_equal_exact_integers_at_the_edges(shape, width):
    lwe, _ = RE.mask_sweep(shape, RE.E(shape.N), width, np.random.default_rng(2))
    _pin(shape, width, lwe, 8)
    two = shape._replace(n=2)                                  # every mask word alike: the same words at two steps per row
    lwe, amounts = RE.constant_rows(two, width, np.random.default_rng(3))
    assert len(lwe) == 23 and amounts[:-1] == RE.E(shape.N)
    _pin(two, width, lwe, 9)


def test_oracles_equal_exact_integers_at_n8192():
    shape = S.Shape(12, 1, 8192, 1, 20)
    lwe, _ = RE.mask_sweep(shape, [1, 8191, 8192, 16383], 64, np.random.default_rng(4))
    _pin(shape, 64, lwe[:, :], 10)


@pytest.mark.parametrize("g", [2, 3])
def test_multibit_oracle_equals_the_exact_group_step(g):
    s = M.MbShape(1, 512, 1, 18, g)
    n = 2 * g
    shape = S.Shape(n, s.k, s.N, s.l, s.logB)
    rng = np.random.default_rng(g)
    bsk = rng.integers(0, 1 << 64, size=(n // g << g) * s.l * 4 * s.N, dtype=np.uint64)
    tv = rng.integers(0, 1 << 64, size=s.N, dtype=np.uint64)
    wrap, labels = RE.wrap_groups(shape, g, 64, rng)
    assert len(wrap) == 10 and labels[-3:] == ["N..N", "top", "wrap"]
    sweep, _ = RE.mask_sweep(shape, RE.E(s.N), 64, rng, g=g)
    for a in RE.E(s.N):                                        # the member and the group the docstring names
        assert RE.mask_position(a, n, g) == ((a // g) % 2) * g + a % g
    lwe = np.concatenate([wrap, sweep])
    t10 = (n, s.k, s.N, s.l, s.logB, 4, 4, 4, 4, g)
    routes = [oracle.Oracle64(t10, bsk, np.zeros(1, dtype=np.uint64), use_ntt=u) for u in (False, True)]
    for q in range(len(lwe)):
        ref, _ = M.bootstrap_mb_exact(lwe[q], tv, bsk, s)
        for orc in routes:
            assert np.array_equal(orc.bootstrap(lwe[q], tv), ref), (orc.use_ntt, q)


@pytest.mark.parametrize("shape,width", [(S.NAMED32["toy_1024"], 32), (S.NAMED64["si_toy_2048"], 64)], ids=["32", "64"])
def test_zero_mask_reference_against_the_oracle(shape, width):
    N, k = shape.N, shape.k
    lwe, flav = RE.body_sweep(shape, RE.ALL(N), width)
    bsk = _random_key(shape, width, 5)
    tvs = np.random.default_rng(6).integers(0, 1 << width, size=(2, N), dtype=RE.dtype_of(width))
    idx = np.arange(len(lwe)) % 2
    want = RE.zero_mask_rows(lwe, tvs, idx, k, N, width)
    _, boot = _oracles(shape, width, bsk)[1]
    for q in range(len(lwe)):
        assert np.array_equal(boot(lwe[q], tvs[idx[q]]), want[q]), (q, flav[q])
    # and against the exact integers at the edges, with and without the one fixed step
    stepped, _ = RE.body_sweep(shape, RE.E(N), width, step=(0, N + 1))
    edge_rows = [q for q in RE.E(N)]
    for q, row in zip(edge_rows, stepped):
        assert np.array_equal(S.bootstrap_exact(lwe[q], tvs[0], bsk, shape, width)[0],
                              RE.zero_mask_reference(tvs[0], q, k, N, width))
        assert S.modswitch(int(row[0]), N, width) == N + 1 and S.modswitch(int(row[-1]), N, width) == q
        assert np.array_equal(boot(row, tvs[0]), S.bootstrap_exact(row, tvs[0], bsk, shape, width)[0]), q
