"""tests/saturation.py against the CPU oracles, and the extremality of what it builds (no GPU).

The GPU test (tests/test_gpu_saturation.py) compares every kernel with saturation.py's integer reference and with the
schoolbook oracle on inputs aligned to the exactness bound; here the three CPU routes - Python integers, the oracles'
schoolbook loops and their Goldilocks NTT routes - are pinned to one another on those same inputs, which none of them had
seen, and the inputs are shown to reach what the capacity checks bound (asserted from the exact integers, never from a
kernel's output)."""
import ctypes as C
import random

import numpy as np
import pytest

import oracle
import saturation as S

SHAPES = S.all_shapes()
IDS = [s[0].replace(" ", "_") for s in SHAPES]


def _digits_oracle(x, logB, l, width):
    if width == 32:
        return [int(v) for v in oracle.decompose(x, logB, l)]
    d = (C.c_int64 * l)()
    oracle.lib64().orc64_decompose(C.c_uint64(x), logB, l, d)
    return [int(v) for v in d]


@pytest.mark.parametrize("width,logB,l", [(32, 6, 3), (32, 8, 2), (32, 7, 3), (32, 7, 2), (32, 4, 4), (32, 2, 13), (32, 1, 31),
                                          (32, 5, 3), (32, 6, 5), (64, 15, 2), (64, 23, 1), (64, 18, 1), (64, 12, 2),
                                          (64, 8, 3), (64, 5, 6), (64, 2, 15), (64, 24, 1), (64, 14, 2)])
def test_digits_equal_the_oracles(width, logB, l):
    rnd = random.Random(logB * 100 + l)
    rep, B = logB * l, 1 << logB
    xs = [rnd.getrandbits(width) for _ in range(300)] + [0, 1, (1 << width) - 1, 1 << (width - 1), (1 << (width - 1)) - 1]
    # ties: a digit of exactly B/2 at each level, over both values of the next level's top bit and of the rounding bit
    for lev in range(l):
        for above in (0, B // 2 - 1, B // 2, B - 1):
            for rounding in (0, 1):
                st = (B // 2) << (logB * (l - 1 - lev))
                if lev > 0:
                    st |= above << (logB * (l - lev))
                x = (st << (width - rep)) % (1 << width)
                if rep < width:
                    x = (x + rounding * ((1 << (width - rep - 1)) - 1) - (1 - rounding) * (1 << (width - rep - 1))) % (1 << width)
                xs.append(x)
    xs.append(S.extreme_value(logB, l, width)[0])
    for x in xs:
        assert S.digits(x, logB, l, width) == _digits_oracle(x, logB, l, width), hex(x)


@pytest.mark.parametrize("logB,l", [(1, 12), (2, 7), (3, 4), (4, 3), (4, 4), (6, 2), (5, 3), (7, 2), (13, 1)])
def test_the_search_finds_the_largest_digit_sum(logB, l):
    """Brute force over every representable state: the dynamic programme's maximum (and its closed form) is the true one."""
    rep = logB * l
    assert rep <= 16
    best = max(sum(abs(d) for d in S.digits(st << (32 - rep), logB, l, 32)) for st in range(1 << rep))
    seq, tot = S.extreme_digits(logB, l)
    assert tot == best == l * (1 << logB) // 2 - l // 2
    assert sum(abs(d) for d in seq) == tot


def test_limb_convolution_equals_python_integers():
    rnd = random.Random(3)
    for width, N, dmax in ((32, 16, 128), (64, 16, 1 << 23), (64, 64, 1 << 14)):
        for trial in range(4):
            d = [rnd.randint(-dmax, dmax) for _ in range(N)]
            words = [rnd.getrandbits(width) for _ in range(N)]
            if trial == 0:
                words = [1 << (width - 1)] * N                     # -2^(w-1) everywhere
            if trial == 1:
                words = [(1 << (width - 1)) - 1] * N
            signed = [w - (1 << width) if w >> (width - 1) else w for w in words]
            got = S.negacyclic_exact(d, np.array(words, dtype=np.uint64), width)
            assert [int(v) for v in got] == S.negacyclic_plain(d, signed)


def test_named_shapes_are_the_librarys():
    import helm_amd
    for name, s in S.NAMED32.items():
        assert S.shape_of(helm_amd.named_params(name)[0]) == s, name
    for name, s in S.NAMED64.items():
        p = helm_amd.si_named_params(name)[0]
        assert S.shape_of(p) == s and p.grouping_factor <= 1, name


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


def _cases(shape, width, half, ratio):
    budget = None if ratio is None else int(ratio * half)
    yield "+", S.saturating_case(shape, width, +1, budget=budget)
    yield "-", S.saturating_case(shape, width, -1, budget=budget)
    yield "one column", S.saturating_case(shape, width, +1, columns=shape.k // 2, budget=budget)


@pytest.mark.parametrize("label,shape,width,half,ratio", SHAPES, ids=IDS)
def test_saturating_cases_reach_the_bound_and_the_oracles_agree(label, shape, width, half, ratio):
    bound = S.capacity_bound(shape, width)
    top = 1 << (width - 1)
    for what, case in _cases(shape, width, half, ratio):
        # the three CPU routes agree on the aligned input, word for word
        for route, fn in _oracles(shape, width, case["bsk"]):
            assert np.array_equal(fn(case["lwe"], case["tv"]), case["ref"]), (label, what, route)
        # ... and on an honest row under the same key (the GPU test's control)
        rng = np.random.default_rng(5)
        lwe = rng.integers(0, 1 << width, size=shape.n + 1, dtype=case["lwe"].dtype)
        tv = rng.integers(0, 1 << width, size=shape.N, dtype=case["lwe"].dtype)
        if what == "+" and (shape.k + 1) ** 2 * shape.l * shape.N <= 16384:
            ref, _ = S.bootstrap_exact(lwe, tv, case["bsk"], shape, width)
            for route, fn in _oracles(shape, width, case["bsk"]):
                assert np.array_equal(fn(lwe, tv), ref), (label, "control", route)
        peak = case["peak"]
        print(f"\n{label} [{what}]: digits {case['digits'] if shape.l <= 6 else '...'}, peak / bound = {peak / bound:.4f}, "
              f"bound / half = {bound / half:.4f}, peak / half = {peak / half:.4f}")
        assert peak < half, (label, what)
        if ratio is not None:
            # placed under a loader's threshold: B/2 x l1 within 0.1 % of the request, by the loaders' own rule
            kb = S.key_bound(case["bsk"], shape, width)
            assert abs(kb / (ratio * half) - 1) < 1e-3, (label, kb / half)
            # the aligned sum is the key's bound scaled by the digits' sum over its largest conceivable value
            want = kb * case["digit_sum"] / (shape.l << (shape.logB - 1))
            assert abs(peak / want - 1) < 1e-3
            continue
        # extremality: the digit rule's own maximum, every term aligned
        per = (shape.k + 1) * shape.N * case["digit_sum"]
        assert per * (top - 1) <= peak <= per * top, (label, what)
        assert case["digit_sum"] == shape.l * (1 << shape.logB) // 2 - shape.l // 2
        if shape.logB >= 6:
            assert peak >= 0.95 * bound, (label, what, peak / bound)


def test_a_mis_signed_key_polynomial_is_not_extremal():
    """The extremality assertion sees one wrong sign among the (k+1) l polynomials of a column."""
    shape = S.NAMED32["toy_k2"]
    case = S.saturating_case(shape, 32)
    bsk = case["bsk"].reshape(shape.n, shape.l, shape.k + 1, shape.k + 1, shape.N).copy()
    i2 = case["steps"][1]
    for c in range(shape.k + 1):
        bsk[i2, 1, 0, c] = np.where(bsk[i2, 1, 0, c] == 0x80000000, 0x7FFFFFFF, 0x80000000).astype(np.uint32)
    acc = [[((1 << 32) - case["x_star"]) // 2] * shape.N for _ in range(shape.k + 1)]
    _, peak = S.cmux_step_exact(acc, shape.N, bsk[i2], shape, 32)
    assert peak < 0.95 * S.capacity_bound(shape, 32) < case["peak"]
    assert peak < (shape.k + 1) * shape.N * case["digit_sum"] * ((1 << 31) - 1) <= case["peak"]


@pytest.mark.parametrize("name,width,half,ratios", [("toy_1024", 32, S.HALF_FPI, (0.997, 0.999, 1.01)),
                                                    ("si_toy_512_k3", 64, S.HALF_46 / 1.05, (0.95, 1.001))])
def test_near_threshold_keys_land_where_asked(name, width, half, ratios):
    shape = (S.NAMED32 if width == 32 else S.NAMED64)[name]
    for ratio in ratios:
        case = S.near_threshold_key(shape, width, ratio, half)
        kb = S.key_bound(case["bsk"], shape, width)          # both groupings, as the loaders take them
        assert abs(kb / (ratio * half) - 1) < 1e-3, (ratio, kb / half)
        # the untouched steps (uniform words) stay below the crafted one: the crafted column decides the field
        plain = S.key_bound(S._random_key(shape, width, 99), shape, width)
        assert plain < kb
