"""Worst-case magnitudes of the large-N blind-rotate kernel's fp64 arithmetic (k_pbs64_large,
helm_amd/csrc/helm_pbs64_large.inc over the shared helm_pbs64_large_core.inc), with exact fractions, for its pair
L0 = FpG = 5072^4 + 1, L1 = FpI = 5440^4 + 1.

Every value in the kernel is an integer held in a double: exactness needs |v| < 2^53 at every addition and at the inputs of
mulmod and reduce (helm_amd/csrc/ntt_fp64.h).  The kernel recentres every value a transform stage stores, so the bounds do
not depend on N, l or logB beyond the digit size; they are restated here from the structure of a CMUX step:

  reduce(a)                  |r| <= p/2 + 1                                   (rounding of a / p to the nearest integer)
  mulmod(a, w), |w| <= p/2   |r| <= (1/2 + 3/4 |a| 2^-52) p                   (ntt_fp64.h)
  forward butterfly          U +- mulmod(V, w), U and V recentred or digits
  inverse butterfly          U +- V, then recentred, or multiplied and recentred
  column sum                 recentred after at most FOLD = 4 products (k_pbs64_large: after q = 3, 7, ..., and at the end)
  lift                       t = reduce(mulmod(r1 - r0, p0^-1 mod p1)), x' = r0 + p0 t
"""
from fractions import Fraction as Fr

import pytest

FPG, FPG2, FPI = 5072 ** 4 + 1, 5096 ** 4 + 1, 5440 ** 4 + 1
PAIR = (FPG, FPI)
LIMIT = Fr(2 ** 53)
FOLD = 4            # products a column sum takes between two recentrings
MAX_LOGB = 24       # helm_si_ctx_create_ex: pbs_logB <= 24, digits at most 2^23 in magnitude

# (k, N, pbs_l, pbs_logB) of tests/test_gpu_large_n.py: the three decompositions of the bootstrap test; the saturating
# case, the many-LUT test, the n = 1024 test and both named sets run (1, 4096, 1, 22)
GPU_SHAPES = [(1, 4096, 1, 22), (1, 4096, 2, 15), (1, 4096, 3, 8)]


def recentred(p):
    return Fr(p, 2) + 1


def mulmod_bound(a, p):
    assert a < LIMIT, "mulmod input not exact"
    return (Fr(1, 2) + Fr(3, 4) * a / 2 ** 52) * p


@pytest.mark.parametrize("p", PAIR)
def test_the_mulmod_output_bound(p):
    """A product of a recentred value with a table or key word (|w| <= p/2): below 0.58 p in both fields; FpI, the larger
    prime, is the tighter one (0.5 + 0.75 x 2^-3.36 = 0.573)."""
    out = mulmod_bound(recentred(p), p)
    assert out < Fr(58, 100) * p
    if p == FPI:
        assert out > Fr(57, 100) * p
        assert Fr(1028, 100) < LIMIT / p < Fr(1029, 100)      # 2^53 / p = 10.28
    else:
        assert Fr(136, 10) < LIMIT / p < Fr(137, 10)


@pytest.mark.parametrize("p", PAIR)
def test_every_butterfly_stays_exact(p):
    m = recentred(p)
    # forward, first stage: digits (|d| <= 2^23 < p/2); later stages: recentred values
    digit = Fr(2 ** (MAX_LOGB - 1))
    assert digit < Fr(p, 2)
    for u in (digit, m):
        s = u + mulmod_bound(u, p)
        assert s < Fr(108, 100) * p + 1 < LIMIT               # reduce's input
    # inverse: U + V is recentred; U - V is multiplied, then recentred
    assert 2 * m < LIMIT
    assert mulmod_bound(2 * m, p) < Fr(65, 100) * p < LIMIT
    # the key conversion: hi 2^32 + lo with |hi| <= 2^31, lo < 2^32 - mulmod(hi, 2^32 mod p) + lo, then the transform
    assert mulmod_bound(Fr(2 ** 31), p) + 2 ** 32 < LIMIT


@pytest.mark.parametrize("p", PAIR)
def test_the_column_sum_between_two_recentrings(p):
    product = mulmod_bound(recentred(p), p)
    worst = recentred(p) + FOLD * product
    assert worst < Fr(282, 100) * p + 1 < LIMIT               # 0.5 p + 4 x 0.58 p
    assert LIMIT / worst > 3                                   # (a factor 3.6 of slack in the tighter field)


def test_the_lifts_ranges():
    p0, p1 = PAIR
    r0, r1 = recentred(p0), recentred(p1)
    diff = r0 + r1                                             # |r1 - r0|
    assert diff < Fr(2 ** 50) < LIMIT
    assert mulmod_bound(diff, p1) < Fr(63, 100) * p1 < LIMIT   # then recentred: |t| <= p1/2 + 1
    t = recentred(p1)
    assert r0 < 2 ** 51 and t < 2 ** 51                        # to_int64's range (HELM_BOUND slot 4)
    # x' = r0 + p0 t is congruent to x mod p0 p1; |x| <= p0 p1 / 2 / 1.001 (the capacity check) and
    # |x'| <= p0 p1 / 2 + 1.5 p0 + 1, so |x' - x| < p0 p1 and x' = x
    x_max = Fr(p0 * p1, 2) / Fr(1001, 1000)
    xp_max = r0 + p0 * t
    assert xp_max == Fr(p0 * p1, 2) + Fr(3 * p0, 2) + 1
    assert x_max + xp_max < p0 * p1
    inv = pow(p0, -1, p1)
    assert p0 * inv % p1 == 1


@pytest.mark.parametrize("shape", GPU_SHAPES + [(1, 4096, 15, 2)])
def test_the_capacity_ratio_of_the_shapes_the_gpu_tests_run(shape):
    k, N, l, logB = shape
    half = Fr(FPG * FPI, 2)
    assert Fr(2 ** 97) * Fr(182, 100) < half < Fr(2 ** 97) * Fr(184, 100)      # 2^97.87
    bound = Fr((k + 1) * l * N * 2 ** (logB - 1) * 2 ** 63)
    assert bound * Fr(1001, 1000) < half
    if shape == (1, 4096, 1, 22):
        assert Fr(546, 1000) < bound / half < Fr(548, 1000)                    # 0.547
    # one more bit per digit at one level is refused; N = 8192 at the smallest useful base is over the half as well
    assert Fr(2 * 4096 * 2 ** 22 * 2 ** 63) * Fr(1001, 1000) >= half
    assert Fr(2 * 8192 * 2 ** 21 * 2 ** 63) >= half


def test_the_roots_of_unity():
    """FpG and FpI hold a primitive 8192-th root of unity (generator 3 in both), FpG2 does not (2-adicity 2^12)."""
    for p in PAIR:
        assert (p - 1) % 8192 == 0
        psi = pow(3, (p - 1) // 8192, p)
        assert pow(psi, 4096, p) == p - 1                      # psi^N = -1: primitive, and 3 is a non-residue
    assert (FPG - 1) % 2 ** 16 == 0 and (FPG - 1) % 2 ** 17 != 0
    assert (FPI - 1) % 2 ** 24 == 0
    assert (FPG2 - 1) % 2 ** 12 == 0 and (FPG2 - 1) % 2 ** 13 != 0 and (FPG2 - 1) % 8192 != 0


def test_the_source_states_the_interval_and_the_pair():
    """A tripwire on the text of the kernel and of the core it shares with k_pbs64_n8192, nothing more (white space is
    ignored; it asks whoever edits these lines to look at the bounds above): the pair, the recentring interval of the column sums, the recentring when a column is written back
    and the recentred quotient of the lift.  That the kernel computes exactly AT these bounds is pinned on the device, by
    the saturating case of tests/test_gpu_large_n.py."""
    core, src, n8192 = kernel_sources()
    together = core + src + n8192
    # what the shared core (helm_pbs64_large_core.inc) holds stands ONCE in the three files taken together
    for stmt in ("usingL0=FpG;", "usingL1=FpI;", "s0=reduce<L0>(s0);", "s1=reduce<L1>(s1);",
                 "buf[s]=reduce<L0>(sum[0][m]);", "buf[N+s]=reduce<L1>(sum[1][m]);",
                 "returnreduce<L1>(mulmod<L1>(r1-r0,p0inv_mod_p1));",            # l64_quotient's body: the recentred quotient
                 "constdoublet=l64_quotient(r0,r1,p0inv_mod_p1);"):
        assert together.count(stmt) == 1 and stmt in core, stmt
    assert "constboolfold=(q&3)==%d;" % (FOLD - 1) in src      # FOLD = 4
    assert "l64_products<LOGN>(sum[c],buf,key+(((size_t)(r*2+c)*L+lev)*2)*N,q==0,fold);" in src
    assert src.count("l64_column_back<LOGN,false>(acc,c,buf,sum[c],twi0,twi1,p0inv_mod_p1);") == 1


def kernel_sources():
    """The text of the shared core and of the two kernel files, white space removed."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "helm_amd", "csrc")
    return [re.sub(r"\s+", "", open(os.path.join(csrc, name)).read())
            for name in ("helm_pbs64_large_core.inc", "helm_pbs64_large.inc", "helm_pbs64_n8192.inc")]
