"""tests/vp_edges.py against the CPU oracles, the extremality of what it builds, and the capacity of the decomposition
vertical packing runs under (no GPU).

The GPU test (tests/test_gpu_vertical_packing_edges.py) compares k_pbs64<., 1> and k_pbs64<., 2> with vp_edges' integer
reference and the schoolbook oracle; here the CPU routes are pinned to one another on those same launches, the crafted
gates are shown to reach the digit rule's own maximum (exact integers, never a kernel's output), the reference is shown to
notice three wrong CMUXes, and two things the engine relies on without checking are pinned:

  * helm_wop_ctx_create applies no capacity check to (cbs_l, cbs_logB).  Over everything it admits - N in {512, 1024, 2048},
    cbs_l in {2, 3}, cbs_logB cbs_l <= 31 - the largest (k+1) l N 2^(logB-1) 2^63 is 2^90 (N = 2048, l = 2, logB = 15),
    0.0055 of p0 p1 / 2 = 2^97.5 for the 49-bit pair: no check is missing today, and this test fails when that changes.
  * cbs_logB = 1 is admitted (the PBS side refuses logB < 2): the kernel's one-addition digit rule has B/2 - 1 = 0 there and
    reads bit 1 of the state; it is compared with the plain rule over every state."""
import random

import numpy as np
import pytest

import oracle
import saturation as S
import vp_edges as V

MOD = V.MOD


@pytest.mark.parametrize("name", list(V.CASES))
def test_integer_reference_equals_the_oracles(name):
    L = V.launch(name)
    v, bits = L["v"], L["bits"]
    for g in range(len(L["ref"])):
        stack = L["stacks"][g][::-1]            # the oracle takes the most significant bit first
        routes = [False, True] if v.N == 512 else [False]
        for use_ntt in routes:
            want = oracle.Ggsw(v.N, 1, v.l, v.logB, stack, use_ntt=use_ntt).vertical_packing(bits, L["tables"][g])
            assert np.array_equal(want, L["ref"][g]), (name, g, L["gates"][g]["kind"], "ntt" if use_ntt else "schoolbook")


@pytest.mark.parametrize("v", V.SHAPES + V.DECOMPOSITIONS, ids=V._name)
def test_crafted_gates_reach_the_digit_rules_maximum(v):
    L = V.launch(("shape-" if v in V.SHAPES else "decomposition-") + V._name(v))
    bound, ratio = V.vp_capacity_bound(v), V.reachable_ratio(v)
    _, seq, tot = S.extreme_value(v.logB, v.l, 64)
    assert tot == v.l * (1 << v.logB) // 2 - v.l // 2 and V.Fraction(tot * 2 * v.N * V.TOP, bound) == ratio
    seen = 0
    for gate, peaks in zip(L["gates"], L["peaks"]):
        if gate["sat"] is None:
            continue
        seen += 1
        per_column = [V.saturating_peak(v, gate["sign"], c) for c in gate["columns"]]
        peak = peaks[gate["sat"]]
        total, short = max(per_column)
        print(f"\n{V._name(v)} {gate['kind']} sign {gate['sign']:+d} columns {gate['columns']}: digits {seq}, "
              f"peak / bound = {peak / bound:.6f}, reachable {float(ratio):.6f}")
        assert peak == total                                       # the aligned coefficient, to the last unit
        assert V.Fraction(peak + short, bound) == ratio            # short of the ratio by the positive words' 1 x |digit| only
        assert all(V.Fraction(t + s, bound) == ratio for t, s in per_column)
        assert peak == max(peaks) and peak < V.HALF_49
    assert seen == 5


@pytest.mark.parametrize("v", [V.VShape(512, 2, 8), V.VShape(512, 3, 1)], ids=V._name)
def test_each_column_alone_reaches_it(v):
    """cmux_step_exact reports the larger of the two columns: each column saturated alone, in the tree and in the rotation."""
    for sign in (+1, -1):
        for c in (0, 1):
            for gate in (V.tree_gate(v, sign, columns=(c,)), V.rotation_gate(v, 3, sign, columns=(c,))):
                _, peaks = V.vertical_packing_exact(gate["stack"], gate["table"], v)
                assert peaks[gate["sat"]] == V.saturating_peak(v, sign, c)[0] == max(peaks), (sign, c, gate["kind"])


def test_a_mis_signed_key_word_is_not_extremal():
    v = V.VShape(512, 2, 8)
    gate = V.tree_gate(v, +1, columns=(0,))
    stack = gate["stack"].copy()
    gb = stack[V.log2(v.N) + 1]
    gb[1, 0, 0] = np.where(gb[1, 0, 0] == V.TOP, V.TOP - 1, V.TOP).astype(np.uint64)
    _, peaks = V.vertical_packing_exact(stack, gate["table"], v)
    # (row 0's level-1 digit, 127 of the column's 2 x 255, now pulls the other way: 2 x 127 of 510 lost)
    assert peaks[2] == max(peaks) and 0.49 < peaks[2] / V.saturating_peak(v, +1, 0)[0] < 0.51


def test_admitted_decompositions_stay_under_the_two_prime_capacity():
    worst = max((V.Fraction(V.vp_capacity_bound(V.VShape(N, l, logB)), 1) / V.HALF_49, N, l, logB)
                for N in (512, 1024, 2048) for l, logB in V.admitted_decompositions())
    assert len(V.admitted_decompositions()) == 15 + 10
    for N in (512, 1024, 2048):
        for l, logB in V.admitted_decompositions():
            bound = 2 * l * N * (1 << (logB - 1)) * (1 << 63)
            assert bound == V.vp_capacity_bound(V.VShape(N, l, logB))
            assert V.Fraction(bound * 1001, 1000) < V.HALF_49, (N, l, logB)
    assert worst[1:] == (2048, 2, 15) and V.vp_capacity_bound(V.VShape(2048, 2, 15)) == 1 << 90
    assert abs(float(worst[0]) - 0.0055) < 1e-4
    # one more built level count at the widest digits would still pass; the margin is 7.5 bits, not unbounded
    assert V.Fraction((1 << 90) << 8) > V.HALF_49


@pytest.mark.parametrize("l", range(1, 15))
def test_the_kernels_digit_rule_at_logB_1(l):
    """Every state of l one-bit levels, at both ends and the middle of the interval that rounds to it."""
    rep = l
    rc = 1 << (63 - rep)
    for st in range(1 << rep):
        for off in (-rc, 0, rc - 1):
            x = ((st << (64 - rep)) + off) % MOD
            assert V.kernel_digits(x, 1, l) == S.digits(x, 1, l, 64), (l, hex(x))


@pytest.mark.parametrize("logB,l", [(2, 2), (2, 3), (3, 3), (4, 2), (5, 3), (8, 2)])
def test_the_kernels_digit_rule_every_state(logB, l):
    rep = logB * l
    for st in range(1 << rep):
        x = st << (64 - rep)
        assert V.kernel_digits(x, logB, l) == S.digits(x, logB, l, 64), hex(x)


@pytest.mark.parametrize("l,logB", [(2, 15), (3, 10), (2, 14), (3, 9), (3, 5)])
def test_the_kernels_digit_rule_at_the_widest_decompositions(l, logB):
    rnd = random.Random(l * 100 + logB)
    rep, B = logB * l, 1 << logB
    xs = [rnd.getrandbits(64) for _ in range(2000)] + [0, 1, MOD - 1, 1 << 63, (1 << 63) - 1, S.extreme_value(logB, l, 64)[0]]
    for lev in range(l):                        # ties: a digit of exactly B/2 at each level, every neighbourhood above it
        for above in (0, B // 2 - 1, B // 2, B - 1):
            st = ((B // 2) << (logB * (l - 1 - lev))) | ((above << (logB * (l - lev))) if lev else 0)
            xs += [((st << (64 - rep)) + off) % MOD for off in (-(1 << (63 - rep)), 0, (1 << (63 - rep)) - 1)]
    for x in xs:
        assert V.kernel_digits(x, logB, l) == S.digits(x, logB, l, 64), hex(x)


# ------------------------------------------------------------------------------------------------------------------
# discriminating power: three wrong CMUXes, each expressed as the right CMUX on altered operands
# ------------------------------------------------------------------------------------------------------------------
def _wrong_sign(c0, c1, ggsw, v):           # c0 + GGSW (x) (c0 - c1)
    return V.cmux_exact(c0, [[(2 * a - b) % MOD for a, b in zip(p0, p1)] for p0, p1 in zip(c0, c1)], ggsw, v)


def _level_off_by_one(c0, c1, ggsw, v):     # digit j meets the key polynomials of level j + 1
    return V.cmux_exact(c0, c1, np.roll(ggsw, -1, axis=0), v)


def _no_rounding(c0, c1, ggsw, v):          # the state is the top logB l bits, truncated
    rc = 1 << (63 - v.logB * v.l)
    return V.cmux_exact(c0, [[(b - rc) % MOD for b in p] for p in c1], ggsw, v)


@pytest.mark.parametrize("mutant", [_wrong_sign, _level_off_by_one, _no_rounding], ids=lambda f: f.__name__.strip("_"))
def test_the_reference_notices_a_wrong_cmux(mutant):
    """Every gate of the N = 512 launches must change under each mutant: 14 of 14 rows."""
    failed = total = 0
    for v in V.SHAPES[:2]:
        L = V.launch("shape-" + V._name(v))
        for g, gate in enumerate(L["gates"]):
            row, _ = V.vertical_packing_exact(gate["stack"], gate["table"], v, cmux=mutant)
            total += 1
            failed += not np.array_equal(row, L["ref"][g])
    print(f"\n{mutant.__name__}: {failed} of {total} rows differ")
    assert failed == total == 14
