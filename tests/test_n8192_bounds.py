"""What changes for the fp64 arithmetic of the N = 8192 blind-rotate kernel (k_pbs64_n8192,
helm_amd/csrc/helm_pbs64_n8192.inc over the shared helm_pbs64_large_core.inc) against the large-N kernel, with exact fractions.  The per-value bounds of
tests/test_large_n_bounds.py (recentred stage outputs, products below 0.58 p, at most FOUR products between two recentrings
of a column sum, the lift's ranges) hold for any N in the same pair L0 = FpG = 5072^4 + 1, L1 = FpI = 5440^4 + 1 and are
imported from there; what depends on N is restated here: the capacity, the roots of unity, the LDS layout."""
import os
import sys
from fractions import Fraction as Fr

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_large_n_bounds as LB  # noqa: E402

FPG, FPI = LB.FPG, LB.FPI
N = 8192
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (k, N, pbs_l, pbs_logB) of tests/test_gpu_n8192.py, and the deepest decomposition the domain test admits
GPU_SHAPES = [(1, N, 2, 15), (1, N, 1, 21), (1, N, 3, 8)]


def test_the_per_value_bounds_do_not_depend_on_n():
    """The column sum between two recentrings and the mulmod bound, for the pair at hand (the functions of the large-N test)."""
    for p in (FPG, FPI):
        product = LB.mulmod_bound(LB.recentred(p), p)
        assert product < Fr(58, 100) * p
        assert LB.recentred(p) + LB.FOLD * product < Fr(282, 100) * p + 1 < LB.LIMIT
        assert Fr(2 ** (LB.MAX_LOGB - 1)) < Fr(p, 2)                  # digits


@pytest.mark.parametrize("shape", GPU_SHAPES + [(1, N, 15, 2)])
def test_the_capacity_ratio(shape):
    k, n_poly, l, logB = shape
    half = Fr(FPG * FPI, 2)
    assert Fr(2 ** 97) * Fr(182, 100) < half < Fr(2 ** 97) * Fr(184, 100)      # 2^97.87
    bound = Fr((k + 1) * l * n_poly * 2 ** (logB - 1) * 2 ** 63)
    assert bound * Fr(1001, 1000) < half
    if shape == (1, N, 1, 21):
        assert bound == 2 ** 97 and Fr(546, 1000) < bound / half < Fr(548, 1000)   # 0.547
    if shape == (1, N, 2, 15):
        assert bound == 2 ** 92                                                     # tfhe's decomposition for the size


def test_one_more_bit_is_over_the_half():
    half = Fr(FPG * FPI, 2)
    assert Fr(2 * N * 2 ** 21 * 2 ** 63) * Fr(1001, 1000) >= half               # (1, 22) is refused
    assert Fr(2 * N * 2 ** 21 * 2 ** 63) > half                                  # ... being over the half itself
    # the lift is exact below the capacity: |x| + |x'| < p0 p1 (tests/test_large_n_bounds.py::test_the_lifts_ranges)
    x_max = half / Fr(1001, 1000)
    assert x_max + half + Fr(3 * FPG, 2) + 1 < FPG * FPI


def test_the_roots_of_unity():
    """3 generates a primitive 16384-th root of unity in FpG and in FpI."""
    for p in (FPG, FPI):
        assert (p - 1) % (2 * N) == 0
        psi = pow(3, (p - 1) // (2 * N), p)
        assert pow(psi, N, p) == p - 1                                 # psi^N = -1: primitive
        assert pow(psi, 2 * N, p) == 1
    assert (FPG - 1) % 2 ** 16 == 0 and (FPG - 1) % 2 ** 17 != 0       # (N = 32768 would be FpG's last size)
    assert (FPI - 1) % 2 ** 24 == 0


def test_the_lds_layout_fits_a_cu():
    """N8192Lds restated: the two-field transform buffer and the modulus-switched input, rounded to 16 B - at n = 1024, the
    largest n a context admits, 133136 B of the CU's 160 KiB.  The accumulator is not in it: 2 N words more would be 256 KiB."""
    def lds(n):
        buf = 8 * 2 * N
        return (buf + 2 * (n + 1) + 15) // 16 * 16
    assert lds(1024) == 133136 <= 160 * 1024
    assert lds(12) == 131104
    assert lds(1024) + 8 * 2 * N > 160 * 1024
    assert 2 * N <= 1 << 16                                            # the switched values fit the u16 `ms` array
    core = LB.kernel_sources()[0]                                      # N8192Lds stands in the shared core
    assert "ms=buf+sizeof(double)*2*((size_t)1<<N8192_LOGN);" in core
    assert "bytes=(ms+sizeof(uint16_t)*((size_t)n+1)+15)/16*16;" in core
    assert "constexprintN8192_LOGN=13;" in core


def test_the_source_states_the_interval_and_the_pair():
    """A tripwire on the kernel's text, as in the large-N test: the pair, the recentring of a sum, the recentring when a
    column is written back and the recentred quotient of the lift (all in helm_pbs64_large_core.inc, which is included
    first: once in the three files taken together), the recentring interval of the column sums in recurrence order, and
    the skip of a zero rotation, uniform over the workgroup."""
    core, large, src = LB.kernel_sources()
    together = core + large + src
    for stmt in ("usingL0=FpG;", "usingL1=FpI;", "s0=reduce<L0>(s0);", "s1=reduce<L1>(s1);",
                 "buf[s]=reduce<L0>(sum[0][m]);", "buf[N+s]=reduce<L1>(sum[1][m]);",
                 "returnreduce<L1>(mulmod<L1>(r1-r0,p0inv_mod_p1));", "constdoublet=l64_quotient(r0,r1,p0inv_mod_p1);"):
        assert together.count(stmt) == 1 and stmt in core, stmt
    assert "constboolfold=(products&3)==%d;" % (LB.FOLD - 1) in src
    assert "for(intlev=L-1;lev>=0;lev--){" in src
    assert "l64_products<LOGN>(sum,buf,key+(((size_t)(r*2+c)*L+lev)*2)*N,false,fold);" in src
    assert src.count("l64_column_back<LOGN,false>(acc,c,buf,sum,twi0,twi1,p0inv_mod_p1);") == 1
    assert "if(a==0)continue;" in src
    main = open(os.path.join(ROOT, "helm_amd", "csrc", "helm_shortint.hip")).read()
    assert (main.index('#include "helm_pbs64_large_core.inc"') < main.index('#include "helm_pbs64_large.inc"')
            < main.index('#include "helm_pbs64_n8192.inc"'))
