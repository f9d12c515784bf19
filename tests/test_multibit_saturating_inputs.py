"""tests/saturation_mb.py pinned on the CPU: the construction against both oracle routes, the peak it reaches as an exact
fraction of the loader's bound, the loader's rule and the figure of its refusal text, the list of shapes, and a model of every
CRT lift of the 64-bit engine (and of the boolean engine's k_pbs_crt, which shares the generic kernel's quotient) that says up
to which fraction of the half-modulus the lift is the exact integer.

The lift.  Every 64-bit bootstrap kernel ends a step with x = r0 + p0 t, t = (r1 - r0) p0^-1 mod p1, where r0, r1 are the
residues of the exact integer column coefficient x.  With t* = (x - r0) / p0 the true quotient, |t*| <= (|x| + |r0|) / p0, and
the computed t is congruent to it mod p1, so t = t* whenever |t*| + |t| < p1.  mulmod's contract (ntt_fp64.h) is
|t| <= (0.5 + 0.75 |a| 2^-52) p1 for the operand a = r1 - r0; reduce() brings that to p1 / 2.  Hence the lift is guaranteed for

    |x| < (1 - T) p0 p1 - max |r0|,     T = max |t| / p1,

that is up to the fraction 2 (1 - T) - 2 max |r0| / (p0 p1) of p0 p1 / 2: 0.777 where centred 49-bit residues are multiplied
and the quotient is taken as it comes, 0.9887 in the 46-bit pair (whose lift recentres the difference first), and the whole
half where the quotient is recentred.  test_every_lift_covers_what_is_admitted_to_it reads off the engine's sources which
form each lift site has and compares the guarantee with what the site is fed: the creation bound for the classical shapes,
the loaders' thresholds for multi-bit keys and the 46-bit pair."""
import os
import random
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import saturation as S  # noqa: E402
import saturation_mb as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "helm_amd", "csrc")
ALL = list(dict.fromkeys(M.TUNED + M.GENERIC + M.BELOW))      # every shape the GPU file runs, once
AT_THRESHOLD = list(dict.fromkeys(M.TUNED + M.GENERIC))
CASES = [(s, sign) for s in ALL for sign in (+1, -1)]
CASE_IDS = ["%s%s" % (M.shape_id(s), "+" if sign > 0 else "-") for s, sign in CASES]


# ------------------------------------------------------------------------------------------------------------------
# the construction
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,sign", CASES, ids=CASE_IDS)
def test_reference_equals_both_oracle_routes(s, sign):
    """The saturating row, the all-zero-mask row and the two control rows (uniform LWE words; every mask odd) of every key:
    bootstrap_mb_exact equals the schoolbook oracle and the Goldilocks-NTT oracle word for word."""
    L = M.launch(s, sign, ratio=None if s in M.BELOW else M.RATIO)
    ksk = np.zeros(s.k * s.N * 4 * (3 * s.g + 1), dtype=np.uint64)
    for use_ntt in (False, True):
        orc = oracle.Oracle64(M.params_tuple(s), L["bsk"], ksk, use_ntt=use_ntt)
        for r in range(len(L["lwe"])):
            assert np.array_equal(orc.bootstrap(L["lwe"][r], L["tv"]), L["ref"][r]), (use_ntt, r)


@pytest.mark.parametrize("s,sign", CASES, ids=CASE_IDS)
def test_reached_peak_is_an_exact_fraction_of_the_loaders_bound(s, sign):
    below = s in M.BELOW
    L = M.launch(s, sign, ratio=None if below else M.RATIO)
    case = L["case"]
    # group 0 wrote x* to every coefficient of every polynomial
    assert all(v == case["x_star"] for poly in M.programmed_accumulator(case, s) for v in poly)
    peak = L["peaks"][0][1]
    assert peak == M.expected_peak(case, s) == max(L["peaks"][0])
    bound = M.loader_bound(L["bsk"], s)
    # peak / bound = (sum_j |d_j|) / (l B/2): 1 at one level, (l B/2 - floor(l/2)) / (l B/2) otherwise
    half_b = 1 << (s.logB - 1)
    assert case["digit_sum"] == s.l * half_b - s.l // 2
    assert Fraction(peak, bound) == Fraction(s.l * half_b - s.l // 2, s.l * half_b)
    assert not M.over_threshold(bound)
    frac = Fraction(2 * bound, M.HALF2)                 # of p0 p1 / 2
    if below:
        assert case["full"] == s.N and bound == M.saturated_group_bound(s)
        # the reached fractions DESIGN.md 2 quotes for the two shapes that cannot reach the threshold
        assert "%.5f" % frac == {M.BELOW[0]: "0.00208", M.BELOW[1]: "0.00003"}[s]
    else:
        # within one unit of magnitude per polynomial of 0.998 x the threshold = 0.99700 of p0 p1 / 2
        assert 0 <= Fraction(case["budget"]) - bound < half_b * (1 << s.g) * s.l * (s.k + 1)
        assert "%.5f" % frac == "0.99700" and "%.5f" % Fraction(2 * peak, M.HALF2) == "0.99700"
    # the control rows stay below: the construction, not chance, reaches the bound; every mask of the second is odd
    assert all(max(L["peaks"][r]) < peak for r in M.CONTROLS)
    assert all(S.modswitch(w, s.N, 64) % 2 == 1 for w in L["lwe"][3][:-1])


def test_one_column_variant_saturates_that_column_only():
    s = M.TUNED[0]
    L = M.launch(s, +1, columns=s.k // 2)
    keys = L["bsk"].reshape(3, 1 << s.g, s.l, s.k + 1, s.k + 1, s.N)
    full = M.launch(s, +1)["bsk"].reshape(keys.shape)
    assert np.array_equal(keys[1, :, :, :, s.k // 2], full[1, :, :, :, s.k // 2])
    assert not np.array_equal(keys[1, :, :, :, 1 - s.k // 2], full[1, :, :, :, 1 - s.k // 2])
    assert L["peaks"][0][1] == M.expected_peak(L["case"], s)


def test_negacyclic_halves_equal_the_plain_product():
    """group_step_exact's two-halves product against plain Python loops, on sums of eight words of the largest magnitude."""
    s = M.MbShape(1, 16, 1, 4, 3)
    rng = np.random.default_rng(1)
    keys = rng.integers(0, M.MOD, size=(8, 1, 2, 2, 16), dtype=np.uint64)
    keys[:, :, :, :, :5] = np.uint64(M.BIG)
    acc = [[int(v) for v in rng.integers(0, M.MOD, size=16, dtype=np.uint64)] for _ in range(2)]
    es = [0, 3, 16, 19, 31, 2, 15, 18]
    new, peak = M.group_step_exact(acc, es, keys, s)
    signed = keys.view(np.int64)
    want, top = [], 0
    for c in range(2):
        col = [0] * 16
        for r in range(2):
            d = [S.digits(v, 4, 1, 64)[0] for v in acc[r]]
            for sub, e in enumerate(es):
                rot = S.rotate([int(v) % M.MOD for v in signed[sub, 0, r, c]], e, 64)
                rot = [v - M.MOD if v >= M.MOD // 2 else v for v in rot]
                col = [a + b for a, b in zip(col, S.negacyclic_plain(d, rot))]
        top = max(top, max(abs(v) for v in col))
        want.append([v % M.MOD for v in col])
    assert new == want and peak == top


# ------------------------------------------------------------------------------------------------------------------
# the loader's rule and the list of shapes
# ------------------------------------------------------------------------------------------------------------------
def test_loader_rule_and_the_figure_of_its_refusal():
    """A key at 1.002 of the threshold is over it, one at 0.998 is not; the refusal prints "%.3f" of bound / (p0 p1 / 2):
    1.002 / 1.001 = 1.001 (tests/test_gpu_multibit_saturation.py looks for that figure in the library's text)."""
    for s in (M.TUNED[0], M.GENERIC[3]):
        over = M.saturating_key(s, [0] * s.g, ratio=1.002)
        under = M.saturating_key(s, [0] * s.g, ratio=M.RATIO)
        b_over, b_under = M.loader_bound(over["bsk"], s), M.loader_bound(under["bsk"], s)
        assert M.over_threshold(b_over) and not M.over_threshold(b_under)
        assert M.printed_ratio(b_over) == "1.001" and M.printed_ratio(b_under) == "0.997"
        # both groupings: the transposed key has the same bound, and a key with one heavy ROW is caught by the row sums
        keys = over["bsk"].reshape(3, 1 << s.g, s.l, s.k + 1, s.k + 1, s.N)
        assert M.loader_bound(np.ascontiguousarray(keys.transpose(0, 1, 2, 4, 3, 5)), s) == b_over
        row = M.saturating_key(s, [0] * s.g, ratio=1.002, columns=0)["bsk"].reshape(keys.shape).transpose(0, 1, 2, 4, 3, 5)
        assert M.over_threshold(M.loader_bound(np.ascontiguousarray(row), s))
        # the saturated group alone decides: with it zeroed the uniform groups sit near 0.71 of the half (mean magnitude 2^62)
        keys = keys.copy()
        keys[1] = 0
        assert Fraction(2 * M.loader_bound(keys, s), M.HALF2) < Fraction(73, 100)


def test_shape_list():
    """Every threshold shape is admitted by context creation while its fully saturated group exceeds the loader's threshold
    (2^g (k+1) N 2^(logB-1) 2^63 = 2^98 against a half of 2^97.49); the tuned ones are the tuned multi-bit build's four
    instantiations, the generic ones cover k_pbs64_generic<LOGN, g> for LOGN = 8..11 and g = 2, 3; the two shapes of more
    than one level cannot reach the threshold."""
    for s in AT_THRESHOLD:
        assert s.l == 1 and M.creation_admits(s), s
        assert M.over_threshold(M.saturated_group_bound(s)), s
        assert (1 << s.g) * (s.k + 1) * s.N * (1 << (s.logB - 1)) * (1 << 63) == 1 << 98
        assert (s.k + 1) * s.N <= 4096                         # the generic kernel's domain
    assert 97.48 < np.log2(float(M.HALF2) / 2) < 97.50
    assert sorted((s.N, s.g) for s in M.TUNED) == [(N, g) for N in (1024, 2048) for g in (2, 3)]
    assert all(s.k == 1 for s in M.TUNED)
    assert sorted((s.N, s.g) for s in M.GENERIC) == [(N, g) for N in (256, 512, 1024, 2048) for g in (2, 3)]
    for s in M.BELOW:
        assert s.l >= 2 and M.creation_admits(s) and not M.over_threshold(M.saturated_group_bound(s))


# ------------------------------------------------------------------------------------------------------------------
# the lift model
# ------------------------------------------------------------------------------------------------------------------
def mulmod_model(a, w, p):
    """ntt_fp64.h's mulmod on doubles, every operation restated: products rounded to double, rint, the two fused
    multiply-adds in exact rationals rounded once."""
    a, w = float(a), float(w)
    h = a * w
    lo = float(Fraction(a) * Fraction(w) - Fraction(h))       # fma(a, w, -h)
    q = float(round(h * (1.0 / p)))                           # rint: ties to even, as Python's round
    r = float(Fraction(h) - Fraction(q) * p)                  # fma(-q, P, h)
    return r + lo


def reduce_model(a, p):
    a = float(a)
    q = float(round(a * (1.0 / p)))
    return float(Fraction(a) - Fraction(q) * p)


def mulmod_bound(a, p):
    assert a < 2.0 ** 53
    return (0.5 + 0.75 * a / 2.0 ** 52) * p


def centre(x, p):
    r = x % p
    return r - p if r > p // 2 else r


def lift_model(x, p0, p1, recentred):
    """lift_pairs on the exact integer x: centred residues in, the lifted integer out."""
    w = centre(pow(p0, -1, p1), p1)
    r0, r1 = centre(x, p0), centre(x, p1)
    t = mulmod_model(r1 - r0, w, p1)
    if recentred:
        t = reduce_model(t, p1)
    assert t == int(t)
    return r0 + p0 * int(t)


def guaranteed_fraction(p0, p1, operand, r0_max, recentred):
    """The largest fraction of p0 p1 / 2 up to which x = r0 + p0 t is the exact integer (this file's docstring).
    operand: the bound of |a| in t = mulmod(a, p0^-1 mod p1); r0_max: of the representative r0 that is added."""
    t_max = (p1 / 2 + 1) if recentred else mulmod_bound(operand, p1)
    return (2 * (p1 - t_max) * p0 - 2 * r0_max) / (p0 * p1)


def _function_text(path, head, tail):
    text = open(os.path.join(CSRC, path)).read()
    a = text.index(head)
    return text[a:text.index(tail, a)]


def lift_sites():
    """-> {site: (p0, p1, bound of the multiplied operand, bound of r0, quotient recentred?)}, the forms read off the
    sources: a site whose statement is not found in its function fails here, so the model cannot drift from the code."""
    P0, P1, J0, J1 = S.FPG, S.FPG2, S.FPJ, S.FPJ2
    cent = lambda p: p / 2 + 1                                                     # noqa: E731
    plain = "mulmod<F1>(r1 - r0, p0inv_mod_p1)"
    si = "helm_shortint.hip"
    sites = {}
    body = _function_text(si, "void pbs64_body(", "\n}\n")
    assert body.count(plain) == 1 and "reduce<F1>(mulmod" not in body
    sites["pbs64_body"] = (P0, P1, cent(P0) + cent(P1), cent(P0), False)
    body = _function_text(si, "void pbs64k_body(", "\n}\n")
    assert body.count("mulmod<FB>(WIDE ? reduce<FB>(r1 - r0) : r1 - r0, p0inv_mod_p1)") == 1
    assert "ntt_inverse<F, LOGN, decltype(twi), 0, !WIDE>" in body and "(<= 21 p)" in body
    sites["pbs64k_body, 49-bit pair"] = (P0, P1, cent(P0) + cent(P1), cent(P0), False)
    # WIDE: the residues arrive unreduced (<= 21 p), their difference is recentred before the multiplication
    sites["pbs64k_body, 46-bit pair (WIDE)"] = (J0, J1, cent(J1), 21.0 * J0, False)
    body = _function_text(si, "void lift_pairs(", "\n}\n")
    assert body.count(plain) == 1
    mb = re.search(r"const double t = ADD \? tq : reduce<F1>\(tq\);", body) is not None
    sites["lift_pairs, classical (ADD)"] = (P0, P1, cent(P0) + cent(P1), cent(P0), False)
    sites["lift_pairs, multi-bit"] = (P0, P1, cent(P0) + cent(P1), cent(P0), mb)
    # the two-prime generic kernels of both engines share one quotient (pbs_twoprime.h): the recentred statement once there,
    # and each kernel's lifts go through it
    shared = "mulmod<FpG2>(r1 - r0, p0inv_mod_p1)"
    body = _function_text("pbs_twoprime.h", "double tp_quotient(", "\n}\n")
    assert body.count("reduce<FpG2>(" + shared + ")") == 1 and body.count(shared) == 1 and body.count("mulmod") == 1
    call = "tp_quotient(r0, r1, p0inv_mod_p1)"
    body = _function_text("helm_pbs64_generic.inc", "void k_pbs64_generic(", "\n}\n")
    assert body.count(call) == 2 and "mulmod<F1>(r1" not in body
    sites["k_pbs64_generic, classical"] = (P0, P1, cent(P0) + cent(P1), cent(P0), True)
    sites["k_pbs64_generic, multi-bit"] = (P0, P1, cent(P0) + cent(P1), cent(P0), True)
    body = _function_text("helm_pbs_crt.inc", "uint32_t crt_lift32(", "\n}\n")
    assert body.count(call) == 1 and "mulmod" not in body
    body = _function_text("helm_pbs_crt.inc", "void k_pbs_crt(", "\n}\n")
    assert body.count("crt_lift32(") == 1 and "mulmod<FpG2>(r1" not in body and "tp_quotient" not in body
    sites["k_pbs_crt"] = (P0, P1, cent(P0) + cent(P1), cent(P0), True)
    return sites


def creation_fractions(shapes):
    """The largest capacity bound, as a fraction of p0 p1 / 2, that helm_si_ctx_create_ex admits over (k, N, l) in shapes."""
    best = 0.0
    for k, N, l in shapes:
        for logB in range(2, 25):
            if logB * l > 31:
                continue
            s = S.Shape(1, k, N, l, logB)
            if S.capacity_bound(s, 64) * 1.001 < S.HALF_49 and (1 << (logB - 1)) * 4 < S.FPG2 / 2:
                best = max(best, S.capacity_bound(s, 64) / S.HALF_49)
    return best


def admitted_fractions():
    """What each lift site is fed at the most, as a fraction of its pair's half."""
    k1_shapes = {t for t in S.TUNED64 if t[0] == 1}
    return {
        "pbs64_body": creation_fractions(k1_shapes),
        "pbs64k_body, 49-bit pair": creation_fractions(S.TUNED64 - k1_shapes),
        "pbs64k_body, 46-bit pair (WIDE)": 1 / 1.05,                   # helm_si_load_bootstrap_key: bound x 1.05 < p p' / 2
        "lift_pairs, classical (ADD)": creation_fractions({t for t in k1_shapes if t[1] >= 1024}),
        "lift_pairs, multi-bit": 1 / 1.001,                             # ... bound x 1.001 < p0 p1 / 2, group sums
        "k_pbs64_generic, classical": S.nearest_capacity_shape(64, 12)[1],
        "k_pbs64_generic, multi-bit": 1 / 1.001,
        # the boolean engine's CRT domain has no capacity check: its largest exact product is below 2^78 whatever the
        # shape (test_crt_shape_domain.py::test_the_creation_time_arithmetic, the static_assert beside crt_admitted)
        "k_pbs_crt": 2.0 ** 78 / S.HALF_49,
    }


def test_every_lift_covers_what_is_admitted_to_it():
    sites, admitted = lift_sites(), admitted_fractions()
    assert sites.keys() == admitted.keys()
    for name, (p0, p1, operand, r0_max, recentred) in sites.items():
        assert operand < 2.0 ** 53
        phi = guaranteed_fraction(p0, p1, operand, r0_max, recentred)
        print(f"\n{name}: exact up to {phi:.4f} of the half, fed at most {admitted[name]:.4f}")
        assert admitted[name] < phi, (name, admitted[name], phi)
    # the figures the sources and DESIGN.md quote
    assert abs(guaranteed_fraction(*sites["pbs64_body"]) - 0.777) < 5e-4
    assert abs(guaranteed_fraction(*sites["pbs64k_body, 46-bit pair (WIDE)"]) - 0.9887) < 5e-4
    assert guaranteed_fraction(*sites["k_pbs64_generic, multi-bit"]) > 1 - 2.0 ** -40
    assert abs(admitted["pbs64_body"] - 0.7101) < 1e-4 and abs(admitted["lift_pairs, classical (ADD)"] - 0.7101) < 1e-4
    assert abs(admitted["pbs64k_body, 49-bit pair"] - 0.7101) < 1e-4


def test_the_guarantee_is_what_the_arithmetic_does():
    """The model run on the operations themselves: with the quotient taken as it comes out of mulmod every lift below the
    guaranteed 0.777 of the half is exact and lifts near the half go wrong by p0 p1; with the quotient recentred every lift
    up to the loader's threshold is exact."""
    p0, p1 = S.FPG, S.FPG2
    assert abs(centre(pow(p0, -1, p1), p1) / p1 - 0.463) < 1e-3
    half = p0 * p1 // 2
    phi = guaranteed_fraction(p0, p1, p0 / 2 + p1 / 2 + 2, p0 / 2 + 1, False)
    rnd = random.Random(1)
    wrong = {}
    for frac in (phi, 0.90, 0.998, 1 / 1.001):
        bad_plain = bad_recentred = 0
        for _ in range(2000):
            x = int(frac * half) - rnd.randrange(0, 1 << 60)
            x = -x if rnd.random() < 0.5 else x
            d = lift_model(x, p0, p1, False) - x
            assert d in (0, p0 * p1, -p0 * p1)
            bad_plain += d != 0
            bad_recentred += lift_model(x, p0, p1, True) != x
        assert bad_recentred == 0
        wrong[frac] = bad_plain
    assert wrong[phi] == 0 and wrong[0.998] > 400 and wrong[1 / 1.001] > 400, wrong
