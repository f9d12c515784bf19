"""Multi-bit bootstraps whose one group step is aligned to the kernels' exactness bound, and a plain exact reference.

A multi-bit blind rotation (grouping factor g) takes g mask elements per step: with e_S the sum of the switched elements of
subset S of the group, the step is acc <- (sum_S X^(e_S) K_S) (x) acc.  No group is skipped and the accumulator itself is
decomposed (there is no difference X^a acc - acc), so the construction of tests/saturation.py does not carry over; this one
uses n = 3 g, three groups, one key per case:

  group 0 (programming)  its masks are 0, the accumulator is the trivial one of the constant test vector t = 2^(64 - logB),
                         digits (1, 0, ...) at every coefficient of the body, 0 in the mask rows.  The body row of all 2^g
                         GGSWs of the group is zero except subset 0, level 0, coefficient 0 of every column, which holds
                         x* = extreme_value(logB, l, 64): after the step every coefficient of every polynomial is x*.
  group 1 (saturating)   every polynomial of subset S, level j is X^(-e_S) P_j, where P_j holds words of the largest
                         magnitude, with the sign of digit j of x* times the case's sign, in its leading coefficients: after
                         the kernel's monomial multiplication all 2^g subsets add with one sign, and coefficient N-1 of every
                         column is (sum_j |d_j|) (k+1) 2^g ||P||_1 - the quantity helm_si_load_bootstrap_key bounds for a
                         multi-bit key.  ||P||_1 follows a budget (saturation.near_threshold_key's mechanism), so that the
                         key sits at a chosen ratio of the loader's threshold; a shape whose fully saturated key stays below
                         the budget is saturated fully, and the reached fraction is reported.
  group 2                uniform words: the saturated accumulator passes through one more step.

No GPU and no project code is used here.  bootstrap_mb_exact sums G = sum_S X^(e_S) K_S subset by subset as exact signed
integers, takes the products through saturation.negacyclic_exact and reduces mod 2^64 only where the accumulator is stored;
it returns the peak |exact column coefficient| of every group.  tests/test_multibit_saturating_inputs.py pins this module
against both CPU oracles; tests/test_gpu_multibit_saturation.py runs the cases on both multi-bit kernels."""
from collections import namedtuple

import numpy as np

import saturation as S

W, MOD = 64, 1 << 64
HALF = S.FPG * S.FPG2 / 2                 # p0 p1 / 2 as the loader has it (a float; exact comparisons use HALF2 below)
HALF2 = S.FPG * S.FPG2                    # twice the half, an integer: bound / half = 2 bound / HALF2
MARGIN_NUM, MARGIN_DEN = 1001, 1000       # the loader refuses when bound x 1.001 >= p0 p1 / 2
BIG = (1 << 63) - 1                       # the largest magnitude both signs have

MbShape = namedtuple("MbShape", "k N l logB g")

# (k, N, l, logB, g).  The tuned multi-bit build, k_pbs64s<., true>: k = 1, l = 1, N >= 1024 - all four instantiations,
# each at a pbs_logB that creation admits and at which a FULLY saturated group exceeds the loader's threshold (2^98 against a
# half of 2^97.49), so that a key can be placed anywhere up to it.
TUNED = [MbShape(1, 1024, 1, 23, 2), MbShape(1, 1024, 1, 22, 3), MbShape(1, 2048, 1, 22, 2), MbShape(1, 2048, 1, 21, 3)]
# one per instantiation k_pbs64_generic<LOGN, g>, likewise
GENERIC = [MbShape(3, 256, 1, 24, 2), MbShape(1, 256, 1, 24, 3), MbShape(7, 512, 1, 22, 2), MbShape(3, 512, 1, 22, 3),
           MbShape(3, 1024, 1, 22, 2), MbShape(3, 1024, 1, 21, 3), MbShape(1, 2048, 1, 22, 2), MbShape(1, 2048, 1, 21, 3)]
# two shapes of more than one level, which cannot reach the threshold: run fully saturated, for the digit rule's neighbours
# and ties
BELOW = [MbShape(2, 512, 2, 12, 3), MbShape(1, 256, 3, 7, 3)]
RATIO = 0.998                             # of the threshold (p0 p1 / 2) / 1.001: the convention of saturation.FPI_RATIO


def shape_id(s):
    return "k%d_N%d_l%d_B%d_g%d" % tuple(s)


def params_tuple(s):
    """The 10-tuple oracle.Oracle64 takes (n, k, N, pbs_l, pbs_logB, ks_l, ks_logB, message, carry, grouping_factor)."""
    return (3 * s.g, s.k, s.N, s.l, s.logB, 4, 4, 4, 4, s.g)


def creation_admits(s):
    """helm_si_ctx_create_ex's capacity check, restated: (k+1) l N 2^(logB-1) 2^63 x 1.001 < p0 p1 / 2 - without the
    factor 2^g of a group."""
    bound = (s.k + 1) * s.l * s.N * (1 << (s.logB - 1)) * (1 << 63)
    return 2 * bound * MARGIN_NUM < HALF2 * MARGIN_DEN and (1 << (s.logB - 1)) * 8 < S.FPG2


def saturated_group_bound(s):
    """The loader's bound of a fully saturated group: B/2 x 2^g l (k+1) N (2^63 - 1)."""
    return (1 << (s.logB - 1)) * (1 << s.g) * s.l * (s.k + 1) * s.N * BIG


def over_threshold(bound):
    """The loader's refusal: bound x 1.001 >= p0 p1 / 2 (exact integers)."""
    return 2 * bound * MARGIN_NUM >= HALF2 * MARGIN_DEN


def printed_ratio(bound):
    """The figure of the loader's refusal text: "%.3f" of bound / (p0 p1 / 2)."""
    return "%.3f" % (2 * bound / HALF2)


# ------------------------------------------------------------------------------------------------------------------
# the loader's rule, restated (key_step_bound over a step of 2^g GGSWs, both groupings)
# ------------------------------------------------------------------------------------------------------------------
def _signed(words):
    return np.ascontiguousarray(words, dtype=np.uint64).view(np.int64)


def loader_bound(bsk, s):
    """B/2 x the largest l1-norm over the key polynomials of one GROUP (its 2^g GGSWs, every level) that meet in one output
    column or, transposed, in one row: what helm_si_load_bootstrap_key compares with (p0 p1 / 2) / 1.001 for a multi-bit
    key, as a Python integer."""
    k1 = s.k + 1
    v = _signed(bsk).reshape(-1, (1 << s.g) * s.l, k1, k1, s.N)
    mag = np.where(v < 0, -v, v).view(np.uint64)      # (-2^63 wraps to the word 2^63: its magnitude)
    norms = (mag >> np.uint64(32)).sum(axis=-1, dtype=np.uint64).astype(object) * (1 << 32) + \
        (mag & np.uint64(0xFFFFFFFF)).sum(axis=-1, dtype=np.uint64).astype(object)
    by_col = norms.sum(axis=(1, 2))                   # [group][c]: over subsets, levels and rows
    by_row = norms.sum(axis=(1, 3))                   # [group][r]
    return max(int(by_col.max()), int(by_row.max())) * (1 << (s.logB - 1))


# ------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------
def _rot_signed(v, e):
    """X^e v in Z[X] / (X^N + 1) along the last axis of an int64 array, e in [0, 2N)."""
    N = v.shape[-1]
    if e >= N:
        v, e = -v, e - N
    out = np.roll(v, e, axis=-1)
    out[..., :e] = -out[..., :e]
    return out


def subset_exponents(masks, N):
    """e_S = the sum over the members i of S (bit i of S) of the switched mask elements, mod 2N."""
    g = len(masks)
    return [sum(masks[i] for i in range(g) if (sub >> i) & 1) % (2 * N) for sub in range(1 << g)]


def group_step_exact(acc, es, keys, s):
    """acc <- (sum_S X^(e_S) K_S) (x) acc in exact integers.  acc: (k+1) polynomials of N Python integers mod 2^64; keys: the
    words [2^g][l][k+1][k+1][N] of the group.  -> (new accumulator, the largest |exact column coefficient|).
    G is summed as signed integers in two halves (G = G_hi 2^32 + G_lo: eight words of 2^63 do not fit an int64, eight
    halves do), each half multiplied through saturation.negacyclic_exact and recombined as Python integers."""
    k1, N, l = s.k + 1, s.N, s.l
    v = _signed(keys).reshape(1 << s.g, l, k1, k1, N)
    g_hi, g_lo = np.zeros((l, k1, k1, N), dtype=np.int64), np.zeros((l, k1, k1, N), dtype=np.int64)
    for sub, e in enumerate(es):
        g_hi += _rot_signed(v[sub] >> 32, e)
        g_lo += _rot_signed(v[sub] & 0xFFFFFFFF, e)
    dig = np.zeros((k1, l, N), dtype=np.int64)
    for r in range(k1):
        for t in range(N):
            dig[r, :, t] = S.digits(acc[r][t], s.logB, l, W)
    peak, new = 0, []
    for c in range(k1):
        col = np.zeros(N, dtype=object)
        for r in range(k1):
            for j in range(l):
                if dig[r, j].any():
                    col = col + S.negacyclic_exact(dig[r, j], g_hi[j, r, c].view(np.uint64), W) * (1 << 32) + \
                        S.negacyclic_exact(dig[r, j], g_lo[j, r, c].view(np.uint64), W)
        peak = max(peak, max(abs(int(x)) for x in col))
        new.append([int(x) % MOD for x in col])
    return new, peak


def bootstrap_mb_exact(lwe, tv, bsk, s):
    """The multi-bit blind rotation (no group skipped) and sample extraction.
    -> (k N + 1 words, [the largest |exact column coefficient| of each group])."""
    k, N, g = s.k, s.N, s.g
    n = len(lwe) - 1
    assert n % g == 0
    keys = np.asarray(bsk, dtype=np.uint64).reshape(n // g, 1 << g, s.l, k + 1, k + 1, N)
    bt = S.modswitch(lwe[n], N, W)
    acc = [[0] * N for _ in range(k)] + [S.rotate([int(x) for x in tv], (2 * N - bt) % (2 * N), W)]
    peaks = []
    for t in range(n // g):
        es = subset_exponents([S.modswitch(lwe[t * g + i], N, W) for i in range(g)], N)
        acc, pk = group_step_exact(acc, es, keys[t], s)
        peaks.append(pk)
    out = []
    for r in range(k):
        out.append(acc[r][0])
        out.extend((-acc[r][N - t]) % MOD for t in range(1, N))
    out.append(acc[k][0])
    return np.array(out, dtype=np.uint64), peaks


# ------------------------------------------------------------------------------------------------------------------
# the construction
# ------------------------------------------------------------------------------------------------------------------
def mask_word(a, N):
    """A mask word that modulus-switches to a (mod 2N)."""
    return np.uint64(a << (W - (N.bit_length() - 1) - 1))


def wrap_masks(s):
    """Group-1 masks whose subset sums wrap past 2N: (N, 2N-1) or (N, 1, 2N-1)."""
    return [s.N, 2 * s.N - 1] if s.g == 2 else [s.N, 1, 2 * s.N - 1]


def saturating_key(s, masks, sign=+1, ratio=RATIO, columns="all", seed=5):
    """-> dict(bsk, lwe, tv, budget, full, rest, digits, digit_sum, x_star).

    bsk: uniform words with group 0 programmed and group 1 saturated under the budget ratio x (p0 p1 / 2) / 1.001 (ratio None,
    or a budget a fully saturated key stays below: saturated fully, `full` = N).  masks: the g switched mask elements of
    group 1 the key is aligned to; lwe is the row that has them.  sign = -1 flips every key sign of group 1.  columns: "all",
    or one column index - only that column of group 1 is saturated, the others keep their uniform words."""
    k, N, l, logB, g = s
    k1, sub = k + 1, 1 << g
    assert len(masks) == g
    rng = np.random.default_rng(seed)
    bsk = rng.integers(0, MOD, size=(3, sub, l, k1, k1, N), dtype=np.uint64)
    x_star, seq, tot = S.extreme_value(logB, l, W)
    t = 1 << (W - logB)
    assert S.digits(t, logB, l, W) == [1] + [0] * (l - 1)
    # group 0: digit +1 (level 0, body row k, subset 0) x (one word at X^0) writes x* to every coefficient of every column
    bsk[0, :, :, k, :, :] = 0
    bsk[0, 0, 0, k, :, 0] = x_star
    # group 1
    per_unit = (1 << (logB - 1)) * sub * l * k1        # budget taken by one unit of magnitude in every polynomial
    budget = None if ratio is None else int(ratio * HALF2 * MARGIN_DEN) // (2 * MARGIN_NUM)
    full, rest = N, 0
    if budget is not None:
        full, rest = divmod(budget // per_unit, BIG)
        if full >= N:
            full, rest = N, 0
    es = subset_exponents(masks, N)
    cols = range(k1) if columns == "all" else [int(columns)]
    for j in range(l):
        sg = sign * (1 if seq[j] >= 0 else -1)
        poly = np.zeros(N, dtype=np.int64)
        poly[:full] = sg * BIG
        if full < N:
            poly[full] = sg * rest
        for sb in range(sub):
            rot = _rot_signed(poly, (2 * N - es[sb]) % (2 * N)).view(np.uint64)     # X^(-e_S) P_j
            for c in cols:
                bsk[1, sb, j, :, c, :] = rot
    lwe = np.zeros(3 * g + 1, dtype=np.uint64)
    for i in range(g):
        lwe[g + i] = mask_word(masks[i], N)
    return dict(bsk=bsk.reshape(-1), lwe=lwe, tv=np.full(N, t, dtype=np.uint64), budget=budget, full=full, rest=rest,
                digits=seq, digit_sum=tot, x_star=x_star)


def programmed_accumulator(case, s):
    """The accumulator after group 0 of the case's own row (every coefficient of every polynomial must be x*)."""
    keys = case["bsk"].reshape(3, 1 << s.g, s.l, s.k + 1, s.k + 1, s.N)
    acc = [[0] * s.N for _ in range(s.k)] + [[int(x) for x in case["tv"]]]
    acc, _ = group_step_exact(acc, [0] * (1 << s.g), keys[0], s)
    return acc


def expected_peak(case, s):
    """(sum_j |d_j|) (k+1) 2^g ||P||_1 of a case with every column saturated."""
    return case["digit_sum"] * (s.k + 1) * (1 << s.g) * (case["full"] * BIG + case["rest"])


_launches = {}
CONTROLS = (2, 3)                         # the control rows of a launch


def launch(s, sign, columns="all", ratio=RATIO):
    """One key and the four rows of a launch, with their references, computed once per (shape, sign, columns, ratio).
    sign +1: group-1 masks 0; sign -1: masks whose subset sums wrap (wrap_masks).  Rows: the saturating row; a row with every
    mask 0 (the same row for sign +1, kept so that both keys run the same launch); two controls (CONTROLS) - uniform words,
    and uniform words whose every mask switches to an ODD exponent (the crafted masks 0, N, 1, 2N-1 leave member 0 of every
    group at a multiple of N, and three uniform groups are all even one time in eight).
    -> dict(bsk, lwe [4, n+1], tv, ref [4, k N + 1], peaks [4][3], case)"""
    key = (s, sign, columns, ratio)
    if key not in _launches:
        masks = [0] * s.g if sign > 0 else wrap_masks(s)
        case = saturating_key(s, masks, sign=sign, ratio=ratio, columns=columns)
        n = 3 * s.g
        rng = np.random.default_rng(3)
        uniform = rng.integers(0, MOD, size=n + 1, dtype=np.uint64)
        odd = rng.integers(0, MOD, size=n + 1, dtype=np.uint64)
        for i in range(n):
            odd[i] = mask_word(int(rng.integers(0, s.N)) * 2 + 1, s.N)
        lwe = np.stack([case["lwe"], np.zeros(n + 1, dtype=np.uint64), uniform, odd])
        refs, peaks = zip(*[bootstrap_mb_exact(row, case["tv"], case["bsk"], s) for row in lwe])
        _launches[key] = dict(bsk=case["bsk"], lwe=lwe, tv=case["tv"], ref=np.stack(refs), peaks=list(peaks), case=case)
    return _launches[key]
