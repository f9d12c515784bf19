"""What the multi-bit form adds to the fp64 arithmetic of the two large-N blind-rotate kernels (k_pbs64_large<12, g>,
k_pbs64_n8192<g>; pair L0 = FpG = 5072^4 + 1, L1 = FpI = 5440^4 + 1), with exact fractions and exact modular integers.

  d^ M(e_S)        a recentred transform output times a table entry |M| <= p/2:             below 0.58 p
  (d^ M) K^        that product (NOT recentred) times a key word |K^| <= p/2:               below 0.59 p
  column sum       recentred after every FOUR such products (the subsets in runs of four):  below 2.9 p < 2^53
  lift             the recentred one of tests/test_large_n_bounds.py; the true coefficient is bounded by the loader's rule
                   for the key at hand: B/2 x the largest l1-norm over the polynomials of a GROUP that meet in one column
                   or row, below p0 p1 / 2 / 1.001 with THIS pair's product

and the fact the monomial table rests on: the kernels' forward transform (Cooley-Tukey, twiddle m + i of the bit-reversed
powers of psi) leaves at position s the value at psi^(2 rev(s) + 1), so the spectrum of X^e is psi^((2 rev(s) + 1) e)."""
import math
import os
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest

import helm_amd
import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import saturation_mb_large as MBL  # noqa: E402
import test_large_n_bounds as LB  # noqa: E402

FPG, FPI = LB.FPG, LB.FPI
PAIR = (FPG, FPI)
LIMIT = LB.LIMIT
FOLD = 4


# ------------------------------------------------------------------------------------------------------------------
# the product chain
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PAIR)
def test_the_product_chain(p):
    d_hat = LB.recentred(p)                                    # a forward transform's output
    dm = LB.mulmod_bound(d_hat, p)                             # d^ M(e_S), |M| <= p/2
    assert dm < Fr(58, 100) * p
    prod = LB.mulmod_bound(dm, p)                              # its product with a key word, |K^| <= p/2
    assert prod == (Fr(1, 2) + Fr(3, 4) * dm / 2 ** 52) * p
    assert prod < (Fr(1, 2) + Fr(3, 4) * Fr(58, 100) * p / 2 ** 52) * p < Fr(59, 100) * p
    worst = LB.recentred(p) + FOLD * prod                      # four products on a recentred sum
    assert worst < Fr(1, 2) * p + 1 + 4 * Fr(59, 100) * p < Fr(29, 10) * p < LIMIT
    if p == FPI:                                               # the tighter field: 2^53 = 10.28 p
        assert Fr(1028, 100) * p < LIMIT < Fr(1029, 100) * p
        assert prod > Fr(58, 100) * p                          # (the second product is the larger one: 0.585 p)
    # the subset S = 0 multiplies d^ itself (M(0) = 1): its product is the classical one, below 0.58 p
    assert LB.mulmod_bound(d_hat, p) < prod
    # 2^g subsets in runs of four: a digit polynomial ends recentred at g = 2 (one run) and g = 3 (two runs)
    assert all((1 << g) % FOLD == 0 for g in (2, 3))


def test_the_source_recentres_after_every_fourth_subset():
    """A tripwire on the kernels' text, as tests/test_large_n_bounds.py has one: the subset loop's recentring interval, the
    replacing lift, the group's rotations in scalar registers, the reduced subset sum and the exponent of a position."""
    core, large, n8192 = LB.kernel_sources()
    together = core + large + n8192
    # the subset term and the lift stand in the shared core (helm_pbs64_large_core.inc): ONCE in the three files together
    for stmt in ("constboolfold=(S&3)==%d;" % (FOLD - 1), "eS&=2*N-1;",
                 "constintex=2*(int)(__brev((unsigned)s)>>(32-LOGN))+1;",
                 "returnreduce<L1>(mulmod<L1>(r1-r0,p0inv_mod_p1));", "constdoublet=l64_quotient(r0,r1,p0inv_mod_p1);",
                 "HELM_BOUND(__builtin_fabs(r0)<0x1p51&&__builtin_fabs(t)<0x1p51,4);",
                 "constuint64_tx=(uint64_t)to_int64(r0)+L0::P_U64*(uint64_t)to_int64(t);",
                 "uint64_t&w=acc.own(c,m);w=REPLACE?x:w+x;"):
        assert together.count(stmt) == 1 and stmt in core, stmt
    assert together.count("HELM_BOUND(") == 1 and together.count("l64_quotient(") == 2   # (its definition and its one use)
    # the own word of each kernel's accumulator view, which the lift writes
    assert "returnp[(size_t)r*N+(int)threadIdx.x+m*L64_THREADS];" in core and "return(p+(size_t)r*N)[base+m];" in core
    # per kernel: the replacing lift, the group's rotations in scalar registers, the rolled subset loop
    for src, lift, term in ((large, "l64_column_back<LOGN,true>(acc,c,buf,sum[c],twi0,twi1,p0inv_mod_p1);",
                             "l64_subset_term<LOGN,GG>(sum,buf,kS,(size_t)L*2*N,psi_pow,am,S);"),
                            (n8192, "l64_column_back<LOGN,true>(acc,c,buf,sum[0],twi0,twi1,p0inv_mod_p1);",
                             "l64_subset_term<LOGN,GG>(sum,buf,kq+(size_t)S*step_words,0,psi_pow,am,S);")):
        assert src.count(lift) == 1 and src.count(term) == 1
        assert src.count("am[i]=__builtin_amdgcn_readfirstlane((int)MS[t*GG+i]);") == 1
        assert src.count("#pragmaunroll1for(intS=0;S<SUB;S++)") == 1


# ------------------------------------------------------------------------------------------------------------------
# the loader's rule
# ------------------------------------------------------------------------------------------------------------------
def _toy_bound(N, l, logB, g, n=6):
    """The loader's bound of a generated key of n / g groups (the key's words belong to the client key: it is kept while they
    are read)."""
    p, lwe_std, glwe_std = helm_amd.si_named_params("si_toy_%d_mb%d" % (N, g))
    p.n, p.pbs_l, p.pbs_logB = n, l, logB
    ck = helm_amd.SiClientKey(p, lwe_std, glwe_std, seed=11)
    bound = MBL.loader_bound(np.array(ck.bsk, dtype=np.uint64), MBL.MbShape(1, N, l, logB, g))
    del ck
    return bound


def test_the_half_of_this_pair():
    half = Fr(MBL.HALF2, 2)
    assert MBL.HALF2 == FPG * FPI
    assert 97.86 < math.log2(half) < 97.88
    assert 97.86 < math.log2(half / Fr(1001, 1000)) < 97.88


@pytest.mark.parametrize("N,top", [(4096, 23), (8192, 22)])
@pytest.mark.parametrize("g", [2, 3])
def test_which_one_level_keys_load(N, g, top):
    """A generated key (uniform mask words, mean magnitude 2^62) has group sums near l 2^(logB + g + 62 + log2 N): one
    level loads up to logB + g = 23 at N = 4096 and 22 at N = 8192, one bit more is refused - although creation admits it."""
    logN = N.bit_length() - 1
    for logB, loads in ((top - g, True), (top - g + 1, False)):
        s = MBL.MbShape(1, N, 1, logB, g)
        assert MBL.creation_admits(s)
        bound = _toy_bound(N, 1, logB, g)
        assert abs(math.log2(bound) - (logB + g + 62 + logN)) < 0.05
        assert MBL.over_threshold(bound) == (not loads), (N, g, logB)
        # the rule itself: l 2^(logB + g + 62 + log2 N) against 2^97.87 / 1.001
        assert (Fr(2 ** (logB + g + 62 + logN)) < Fr(MBL.HALF2, 2) / Fr(1001, 1000)) == loads


def test_the_cases_the_issue_names():
    # N = 8192, one level of 21 bits, grouping factor 2: admitted at creation, refused at load; N = 4096 with 22 bits alike
    for N, logB in ((8192, 21), (4096, 22)):
        s = MBL.MbShape(1, N, 1, logB, 2)
        assert MBL.creation_admits(s) and not MBL.creation_admits(s._replace(logB=logB + 1))
        bound = _toy_bound(N, 1, logB, 2)
        assert MBL.over_threshold(bound) and 1.0 < float(Fr(2 * bound, MBL.HALF2)) < 1.2


@pytest.mark.parametrize("N", [4096, 8192])
@pytest.mark.parametrize("g", [2, 3])
def test_two_levels_of_fifteen_bits_load_at_every_grouping(N, g):
    bound = _toy_bound(N, 2, 15, g)
    assert not MBL.over_threshold(bound)
    # the rule of the one-level test with l = 2: 2 x 2^(15 + g + 62 + log2 N) = 2^(90 + g) at N = 4096, 2^(91 + g) at 8192
    assert abs(math.log2(bound) - ((90 if N == 4096 else 91) + g)) < 0.05
    assert Fr(2 ** (92 + g)) < Fr(MBL.HALF2, 2) / Fr(1001, 1000)                # (a bit more would load as well)


def test_the_saturating_shapes():
    """tests/saturation_mb_large.py's four shapes: admitted at creation, a fully saturated group over the loader's threshold
    (2^98 against 2^97.87), one per kernel and grouping."""
    assert sorted((s.N, s.g) for s in MBL.LARGE) == [(N, g) for N in (4096, 8192) for g in (2, 3)]
    for s in MBL.LARGE:
        assert s.k == 1 and s.l == 1 and MBL.creation_admits(s)
        assert MBL.over_threshold(MBL.saturated_group_bound(s))
        assert (1 << s.g) * 2 * s.N * (1 << (s.logB - 1)) * (1 << 63) == 1 << 98
    assert [tuple(s) for s in MBL.LARGE] == [(1, 4096, 1, 21, 2), (1, 4096, 1, 20, 3), (1, 8192, 1, 20, 2), (1, 8192, 1, 19, 3)]


SAT_CASES = [(s, sign) for s in MBL.LARGE for sign in (+1, -1)]


@pytest.mark.parametrize("s,sign", SAT_CASES, ids=["%s%s" % (MBL.shape_id(s), "+" if sg > 0 else "-") for s, sg in SAT_CASES])
def test_reference_equals_both_oracle_routes(s, sign):
    """The saturating row, the zero-mask row and the two controls of every key the GPU file runs: the Python-integer
    reference equals the schoolbook oracle and the NTT oracle word for word; the key sits at 0.998 of this pair's threshold,
    an exact fraction."""
    L = MBL.launch(s, sign)
    ksk = np.zeros(s.N * 4 * (3 * s.g + 1), dtype=np.uint64)
    for use_ntt in (False, True):
        orc = oracle.Oracle64(MBL.params_tuple(s), L["bsk"], ksk, use_ntt=use_ntt)
        for r in range(len(L["lwe"])):
            assert np.array_equal(orc.bootstrap(L["lwe"][r], L["tv"]), L["ref"][r]), (use_ntt, r)
    case = L["case"]
    assert all(v == case["x_star"] for poly in MBL.programmed_accumulator(case, s) for v in poly)
    peak = L["peaks"][0][1]
    bound = MBL.loader_bound(L["bsk"], s)
    assert peak == MBL.expected_peak(case, s) == max(L["peaks"][0]) == bound
    assert not MBL.over_threshold(bound)
    unit = (1 << (s.logB - 1)) * (1 << s.g) * s.l * (s.k + 1)
    assert 0 <= MBL.budget_of(MBL.RATIO) - bound < unit
    assert MBL.budget_of(MBL.RATIO) == (998 * MBL.HALF2) // 2002
    assert "%.5f" % Fr(2 * peak, MBL.HALF2) == "0.99700" and MBL.printed_ratio(bound) == "0.997"
    assert all(max(L["peaks"][r]) < peak for r in MBL.CONTROLS)


# ------------------------------------------------------------------------------------------------------------------
# the spectrum of a monomial
# ------------------------------------------------------------------------------------------------------------------
def _rev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2)


def forward_model(x, psi, p):
    """l64_ntt_forward (helm_pbs64_large_core.inc) in exact integers mod p: natural order in, bit-reversed out; stage s has m = 2^s
    blocks of 2 t = N / m values, block i multiplies its upper half by table entry m + i of the bit-reversed powers of psi
    (power_table: power i stands at index rev(i))."""
    N = len(x)
    logN = N.bit_length() - 1
    tw = [0] * N
    for i in range(N):
        tw[_rev(i, logN)] = pow(psi, i, p)
    x = list(x)
    for s in range(logN):
        t, m = N >> (s + 1), 1 << s
        for i in range(m):
            for k in range(t):
                j = i * 2 * t + k
                u, v = x[j], x[j + t] * tw[m + i] % p
                x[j], x[j + t] = (u + v) % p, (u - v) % p
    return x


@pytest.mark.parametrize("p", PAIR)
@pytest.mark.parametrize("N", [8, 32])
def test_the_spectrum_of_a_monomial(N, p):
    """NTT(X^e)[s] = psi^((2 rev(s) + 1) e) for every e < 2N (X^(N + e) = -X^e): the table lookup of the multi-bit body."""
    logN = N.bit_length() - 1
    psi = pow(3, (p - 1) // (2 * N), p)
    assert pow(psi, N, p) == p - 1
    for e in range(2 * N):
        mono = [0] * N
        mono[e % N] = 1 if e < N else p - 1
        got = forward_model(mono, psi, p)
        assert got == [pow(psi, ((2 * _rev(s, logN) + 1) * e) % (2 * N), p) for s in range(N)], e
    # ... and the transform is the evaluation at those points: a product of spectra is the negacyclic product
    rng = np.random.default_rng(N)
    a = [int(v) for v in rng.integers(0, 1000, size=N)]
    e = 2 * N - 3
    rot = [0] * N                                              # X^e a, negacyclic
    for j, v in enumerate(a):
        q = (j + e) % (2 * N)
        rot[q % N] = (rot[q % N] + (v if q < N else -v)) % p
    fa, fm = forward_model(a, psi, p), [pow(psi, ((2 * _rev(s, logN) + 1) * e) % (2 * N), p) for s in range(N)]
    assert forward_model(rot, psi, p) == [x * y % p for x, y in zip(fa, fm)]
