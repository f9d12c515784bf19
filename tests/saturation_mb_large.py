"""tests/saturation_mb.py for the multi-bit form of the large-N kernels (k_pbs64_large<12, g>, k_pbs64_n8192<g>), which
compute in the pair FpG x FpI: p0 p1 / 2 = 2^97.87 instead of the 49-bit pair's 2^97.49.

saturation_mb's construction, reference and loader rule do not depend on the pair; what does is the half its budget is a
ratio of (saturation_mb.HALF2, tied to FpG x FpG2).  saturating_key computes  budget = int(ratio x HALF2 x 1000) // 2002
whatever number type `ratio` has, so a ratio r of THIS pair's threshold is handed over as the exact fraction
r x (FpG FpI) / (FpG FpG2): the product is then the exact rational r x FpG FpI x 1000, and the budget the integer it would be
had the module been written for this pair.  Everything else is imported as it is."""
from fractions import Fraction

import saturation as S
import saturation_mb as M

MbShape, shape_id, params_tuple, loader_bound = M.MbShape, M.shape_id, M.params_tuple, M.loader_bound
saturated_group_bound, bootstrap_mb_exact, expected_peak = M.saturated_group_bound, M.bootstrap_mb_exact, M.expected_peak
programmed_accumulator, wrap_masks, mask_word, CONTROLS, BIG = M.programmed_accumulator, M.wrap_masks, M.mask_word, M.CONTROLS, M.BIG
MARGIN_NUM, MARGIN_DEN = M.MARGIN_NUM, M.MARGIN_DEN

HALF2 = S.FPG * S.FPI                     # twice p0 p1 / 2 of the large-N pair, an integer
RATIO = Fraction(998, 1000)               # of the threshold (p0 p1 / 2) / 1.001, as saturation_mb.RATIO

# (k, N, l, logB, g): one shape per kernel and grouping, each admitted at creation while its fully saturated group exceeds
# the loader's threshold (2^g (k+1) N 2^(logB-1) 2^63 = 2^98 against a half of 2^97.87)
LARGE = [MbShape(1, 4096, 1, 21, 2), MbShape(1, 4096, 1, 20, 3), MbShape(1, 8192, 1, 20, 2), MbShape(1, 8192, 1, 19, 3)]


def _scaled(ratio):
    return None if ratio is None else Fraction(ratio) * Fraction(HALF2, M.HALF2)


def creation_admits(s):
    """helm_si_ctx_create_ex's capacity check for a large-N context: (k+1) l N 2^(logB-1) 2^63 x 1.001 < p0 p1 / 2 of this
    pair - without the factor 2^g of a group."""
    bound = (s.k + 1) * s.l * s.N * (1 << (s.logB - 1)) * (1 << 63)
    return 2 * bound * MARGIN_NUM < HALF2 * MARGIN_DEN and (1 << (s.logB - 1)) * 8 < S.FPG2


def over_threshold(bound):
    """The loader's refusal: bound x 1.001 >= p0 p1 / 2 (exact integers)."""
    return 2 * bound * MARGIN_NUM >= HALF2 * MARGIN_DEN


def printed_ratio(bound):
    """The figure of the loader's refusal text: "%.3f" of bound / (p0 p1 / 2)."""
    return "%.3f" % (2 * bound / HALF2)


def budget_of(ratio):
    """The integer budget saturating_key works with for a ratio of this pair's threshold."""
    return int(Fraction(ratio) * HALF2 * MARGIN_DEN) // (2 * MARGIN_NUM)


def saturating_key(s, masks, sign=+1, ratio=RATIO, columns="all", seed=5):
    case = M.saturating_key(s, masks, sign=sign, ratio=_scaled(ratio), columns=columns, seed=seed)
    assert ratio is None or case["budget"] == budget_of(ratio)
    return case


def launch(s, sign, columns="all", ratio=RATIO):
    """saturation_mb.launch (one key, four rows and their integer references, computed once) at a ratio of this pair."""
    L = M.launch(s, sign, columns=columns, ratio=_scaled(ratio))
    assert ratio is None or L["case"]["budget"] == budget_of(ratio)
    return L
