"""tests/many_lut.py - the plain restatement of the many-LUT bootstrap that tests/test_gpu_many_lut.py holds the kernels
to - pinned against the CPU oracle.  No GPU; these pass with or without the feature in the library: that is their job."""
import os
import sys

import numpy as np
import pytest

import helm_amd
import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import many_lut as ML  # noqa: E402
import saturation as S  # noqa: E402

_cache = {}


def _set(name):
    """-> (client key, oracle, a random small-LWE row, a random test polynomial, its exact accumulator)"""
    if name not in _cache:
        ck = helm_amd.SiClientKey.generate(name, seed=3)
        p = ck.params
        orc = oracle.Oracle64(p.as_tuple(), ck.bsk, ck.ksk, use_ntt=True)
        rng = np.random.default_rng(5)
        lwe = rng.integers(0, 2**64, size=p.n + 1, dtype=np.uint64)
        tv = rng.integers(0, 2**64, size=p.N, dtype=np.uint64)
        acc = ML.accumulator_exact(lwe, tv, ck.bsk, S.shape_of(p), max(1, p.grouping_factor))
        _cache[name] = (ck, orc, lwe, tv, acc)
    return _cache[name]


def test_builder_with_one_function_is_the_oracles_make_lut():
    ck, orc, *_ = _set("si_toy_512")
    f = [(5 * v + 3) % ck.t for v in range(ck.t)]
    assert np.array_equal(ML.many_lut_poly([f], ck.t, ck.params.N), orc.make_lut(f))


@pytest.mark.parametrize("t,n_funcs", [(16, 1), (16, 2), (16, 3), (16, 4), (16, 16), (4, 4)])
def test_every_function_value_sits_where_its_output_is_extracted(t, n_funcs):
    """Input v rotates the accumulator by v box + d, d in [-box/2, box/2): output x, extracted at output_coefficient(x),
    must then read f_x(v) delta - the negacyclic coefficient at x N / M + v box + d of the test polynomial."""
    N = 512
    M, box, delta = ML.chunks(n_funcs), N // t, (1 << 63) // t
    per = t // M
    vals = [[(7 * i + 3 * v + 1) % t for v in range(per)] for i in range(n_funcs)]
    tv = ML.many_lut_poly(vals, t, N)
    for v in range(per):
        for d in range(-box // 2, box // 2):
            bt = (v * box + d) % (2 * N)
            acc = ML.zero_mask_acc(tv, bt, 1)
            for x in range(M):
                h = ML.output_coefficient(x, n_funcs, N)
                assert h == x * N // M
                want = vals[x][v] * delta % ML.MOD if x < n_funcs else 0
                assert int(ML.extract_at(acc, h)[-1]) == want, (v, d, x)
                assert ML.zero_mask_body(tv, bt, h) == want


@pytest.mark.parametrize("name", ["si_toy_512", "si_toy_1024_mb2"])
def test_extract_at_zero_is_the_oracles_bootstrap(name):
    ck, orc, lwe, tv, acc = _set(name)
    assert np.array_equal(ML.extract_at(acc, 0), orc.bootstrap(lwe, tv))


@pytest.mark.parametrize("name", ["si_toy_512", "si_toy_1024_mb2"])
def test_mask_words_of_any_extract_follow_from_output_zero(name):
    ck, orc, lwe, tv, acc = _set(name)
    N, k = ck.params.N, ck.params.k
    out0 = orc.bootstrap(lwe, tv)
    for h in (N // 2, N - N // 16):
        got = ML.extract_at(acc, h)
        assert np.array_equal(got[:-1], ML.masks_from_output0(out0, k, N, h)), h
        assert int(got[-1]) == int(acc[k][h])
    assert np.array_equal(ML.masks_from_output0(out0, k, N, 0), out0[:-1])


def test_zero_mask_accumulator_is_the_exact_route_on_a_zero_mask_row():
    ck, orc, lwe, tv, _ = _set("si_toy_512")
    p = ck.params
    row = np.zeros(p.n + 1, dtype=np.uint64)
    for bt in (0, 1, p.N - 1, p.N, 2 * p.N - 1):
        row[p.n] = np.uint64(bt << (64 - p.N.bit_length()))
        assert S.modswitch(row[p.n], p.N, 64) == bt
        assert ML.accumulator_exact(row, tv, ck.bsk, S.shape_of(p)) == ML.zero_mask_acc(tv, bt, p.k)
