"""Vertical packing on GGSWs that no circuit bootstrap produces, and a plain exact reference for it.

helm_wop_vertical_packing_batch takes its GGSWs and its tables from the caller in the standard domain and needs no key, so
every word of every GGSW is the test's to choose.  This module builds, for a shape (N, cbs_l, cbs_logB) with k = 1:

  programming CMUX        the tables are trivial GLWEs: at tree level 0 the difference c1 - c0 has a zero mask, only the body
                          row of the GGSW is multiplied.  Two table polynomials that differ by the single word
                          2^(64 - logB (j+1)) at X^0 give the digit +1 at level j and nothing else: the CMUX adds row
                          (k, level j) of the GGSW, both polynomials, to c0 as it stands - one CMUX writes any GLWE.  The two
                          CMUXes of tree level 0 share one GGSW; one pair carries the level-0 word, the other the level-1
                          word, so they write two independent GLWEs c0' and c1'.
  tree-saturating gate    (bits = log2 N + 2: k_pbs64<., 2>)  level 0 writes c0', c1' with every coefficient of c1' - c0', mask
                          and body, decomposing to the digits of x* = extreme_value(logB, l, 64), the largest sum of
                          magnitudes the rule produces: x* itself or either end of the interval that rounds to it
                          (x* - 2^(63 - rep), x* + 2^(63 - rep) - 1), chosen per coefficient.  The level-1 GGSW holds words of the largest magnitude whose signs follow the digits
                          and the negacyclic wrap, so that ONE coefficient of each column sum has every term of one sign:
                          coefficient N-1 of the mask column, coefficient 0 of the body column (sample extraction keeps the
                          whole mask polynomial but only B[0]).  The rotation GGSWs are zero: the blind rotation passes the
                          accumulator through.  Positive, negative (every sign flipped) and one-column (the body column
                          keeps uniform words) variants, as saturation.launch_case.
  rotation-saturating gate (k_pbs64<., 1>)  the tree's first CMUX writes the accumulator, its further levels hold zero GGSWs
                          (they pass c0 on); rotation step s alone holds the saturating GGSW.  Step s multiplies by
                          X^(-r), r = 2^s; with S = sum_{j < N/r} X^(j r), (X^r - 1) S = X^N - 1 = -2, so the accumulator
                          A = S e has X^(-r) A - A = 2 X^(-r) e.  e = (x*/2) X^r (1 + X + ... + X^(N-1)) - that is -x*/2 below
                          coefficient r and +x*/2 from it on (x* is a multiple of 2^33) - makes that difference x* at every
                          coefficient.  (In place of x*: the lower end of its rounding interval for the body polynomial, the
                          upper end less one for the mask polynomial, there with the other root of 2 e = x, e + 2^63.)
  control gate            uniform words in every GGSW and table: every word pattern is a valid input.  They ride in the same
                          launch; a failure of the crafted gates alone is an error at the extreme, a failure of the controls
                          too is a layout error of the test.

What the aligned coefficient reaches.  The creation check's formula for this decomposition would be
capacity_bound = (k+1) l N 2^(logB-1) 2^63.  The digit rule's largest sum of magnitudes is l B/2 - floor(l/2)
(saturation.extreme_digits), so the ratio that can be reached is reachable_ratio = (l B/2 - floor(l/2)) / (l B/2), and it is
reached up to the sign of the largest word: a word is at most 2^63 - 1 but at least -2^63, so every term whose key word has to
be positive falls 1 x |digit| short.  saturating_peak() gives the exact integer (tests/test_vp_edges.py asserts it equal to
the peak cmux_step_exact measures, and peak + shortfall == reachable_ratio x capacity_bound as fractions).  At logB = 1 the
rule forbids two neighbouring non-zero digits: the ratio is 1/2 (l = 2) and 2/3 (l = 3).

No GPU and no project code is used.  The reference (vertical_packing_exact) is the CMUX tree, the blind rotation and the sample
extraction in Python integers over saturation.cmux_step_exact, reduced mod 2^64 at the very end; stacks are indexed as the
engine takes them (index 0 = least significant bit: rotation steps 0 .. log2 N - 1, then the tree from its lowest level).
"""
from collections import namedtuple
from fractions import Fraction

import numpy as np

from saturation import (FPG, FPG2, Shape, capacity_bound, cmux_step_exact, digits, extreme_value, negacyclic_exact,  # noqa: F401
                        rotate)

VShape = namedtuple("VShape", "N l logB")   # k = 1 throughout
W, MOD, TOP = 64, 1 << 64, 1 << 63
U64 = np.uint64
HALF_49 = Fraction(FPG * FPG2, 2)


def sat_shape(v):
    return Shape(0, 1, v.N, v.l, v.logB)


def log2(N):
    return N.bit_length() - 1


def vp_capacity_bound(v):
    """(k+1) l N 2^(logB-1) 2^63 for (cbs_l, cbs_logB): what a creation check of this decomposition would compare."""
    return capacity_bound(sat_shape(v), W)


def reachable_ratio(v):
    half_sum = v.l * (1 << v.logB) // 2
    return Fraction(half_sum - v.l // 2, half_sum)


def admitted_decompositions():
    """(cbs_l, cbs_logB) that helm_wop_ctx_create admits."""
    return [(l, logB) for l in (2, 3) for logB in range(1, 31 // l + 1)]


def kernel_digits(x, logB, l):
    """The digit rule as k_pbs64 computes it (pbs64_body): the rounded state of logB l <= 32 bits, then per level, least
    significant first, ONE addition - the digit is what the state loses when B/2 - 1 + (bit 2 logB - 1 of the state) is added
    and logB bits are shifted out; 32-bit wrap-around as on the device.  First = most significant level."""
    rep = logB * l
    m32 = (1 << 32) - 1
    state = (((int(x) + (1 << (63 - rep))) % MOD) >> (64 - rep)) & m32
    half_m1 = (1 << (logB - 1)) - 1
    out = [0] * l
    for lev in range(l - 1, -1, -1):
        nxt = ((state + half_m1 + ((state >> (2 * logB - 1)) & 1)) & m32) >> logB
        d = (state - ((nxt << logB) & m32)) & m32
        out[lev] = d - (1 << 32) if d >> 31 else d
        state = nxt
    return out


# ------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------
def cmux_exact(c0, c1, ggsw, v):
    """c0 + GGSW (x) (c1 - c0) -> (GLWE as two lists of Python integers, largest exact column-sum coefficient)."""
    return cmux_step_exact(c0, 0, ggsw, sat_shape(v), W, c1=c1)


def vertical_packing_exact(stack, table, v, cmux=cmux_exact):
    """stack [bits][l][2][2][N] (index 0 = least significant bit), table max(2^bits, N) words
    -> (N + 1 words, [peak of every CMUX in the engine's order: tree levels from the leaves, then the rotation steps])."""
    N, logN = v.N, log2(v.N)
    stack = np.asarray(stack, dtype=U64).reshape(-1, v.l, 2, 2, N)
    bits = stack.shape[0]
    nbr, tree = min(bits, logN), max(bits - logN, 0)
    table = [int(t) for t in np.asarray(table).reshape(-1)]
    assert len(table) == max(1 << bits, N)
    cur = [[[0] * N, table[q * N:(q + 1) * N]] for q in range(1 << tree)]
    peaks = []

    def step(c0, c1, g):
        if not stack[g].any():          # a zero GGSW adds nothing, exactly
            peaks.append(0)
            return c0
        out, pk = cmux(c0, c1, stack[g], v)
        peaks.append(pk)
        return out

    for lev in range(tree):
        cur = [step(cur[2 * q], cur[2 * q + 1], nbr + lev) for q in range(len(cur) // 2)]
    acc = cur[0]
    for i in range(nbr):
        acc = step(acc, [rotate(p, 2 * N - (1 << i), W) for p in acc], i)
    row = [acc[0][0]] + [(-acc[0][N - t]) % MOD for t in range(1, N)] + [acc[1][0]]
    return np.array(row, dtype=U64), peaks


# ------------------------------------------------------------------------------------------------------------------
# the constructions
# ------------------------------------------------------------------------------------------------------------------
def _words(rng, *shape):
    return rng.integers(0, MOD, size=shape, dtype=U64)


def _as_words(poly):
    return np.array([int(x) % MOD for x in poly], dtype=U64)


def program_word(v, j):
    """The table difference whose digits are +1 at level j and 0 elsewhere."""
    w = 1 << (W - v.logB * (j + 1))
    assert digits(w, v.logB, v.l, W) == [int(i == j) for i in range(v.l)]
    return w


def _same_digits(v, x_star, seq, even=False):
    """x* and the two ends of the interval that rounds to it: x* - 2^(63 - rep) (one less rounds down: a rounding term that is
    missing shows) and x* + 2^(63 - rep) - 1 (one more rounds up); even=True: the upper end less one, for a value that is
    halved.  All three decompose to the digits of x*."""
    rc = 1 << (63 - v.logB * v.l)
    out = [(x_star - rc) % MOD, x_star, (x_star + rc - (2 if even else 1)) % MOD]
    assert all(digits(x, v.logB, v.l, W) == seq for x in out)
    assert digits(out[0] - 1, v.logB, v.l, W) != seq and digits(out[2] + (2 if even else 1), v.logB, v.l, W) != seq
    return np.array(out, dtype=U64)


TARGET = {0: lambda N: N - 1, 1: lambda N: 0}     # the aligned coefficient of the mask column and of the body column


def _saturate(ggsw, v, seq, sign, columns):
    """Fill the columns of one GGSW [l][2][2][N] with words of the largest magnitude: the term of digit j at coefficient a
    and key coefficient b lands on a + b (sign +) or a + b - N (sign -); for the target coefficient m the key word at b gets
    the sign  sign x sgn(digit j) x (+ for b <= m, - for b > m)."""
    N = v.N
    for c in columns:
        m = TARGET[c](N)
        for j in range(v.l):
            s = sign * (1 if seq[j] >= 0 else -1)
            poly = np.empty(N, dtype=U64)
            poly[:m + 1] = TOP - 1 if s > 0 else TOP
            poly[m + 1:] = TOP if s > 0 else TOP - 1
            ggsw[j, :, c, :] = poly


def saturating_peak(v, sign, c):
    """The exact aligned coefficient of column c -> (|value|, shortfall against digit_sum (k+1) N 2^63)."""
    _, seq, _ = extreme_value(v.logB, v.l, W)
    N, m = v.N, TARGET[c](v.N)
    total = short = 0
    for d in seq:
        s = sign * (1 if d >= 0 else -1)
        n_pos = m + 1 if s > 0 else N - 1 - m             # key words that have to be +(2^63 - 1)
        total += abs(d) * 2 * (n_pos * (TOP - 1) + (N - n_pos) * TOP)
        short += abs(d) * 2 * n_pos
    return total, short


def tree_gate(v, sign=+1, columns=(0, 1), seed=1):
    """bits = log2 N + 2 -> dict(stack, table, sat (index of the saturating CMUX in vertical_packing_exact's peaks), columns)."""
    N, logN = v.N, log2(v.N)
    assert v.l >= 2
    rng = np.random.default_rng(seed)
    x_star, seq, _ = extreme_value(v.logB, v.l, W)
    stack = np.zeros((logN + 2, v.l, 2, 2, N), dtype=U64)
    T0, T2 = _words(rng, N), _words(rng, N)
    T1, T3 = T0.copy(), T2.copy()
    T1[0] = (int(T0[0]) + program_word(v, 0)) % MOD
    T3[0] = (int(T2[0]) + program_word(v, 1)) % MOD
    c0 = _words(rng, 2, N)
    c1 = c0 + rng.choice(_same_digits(v, x_star, seq), size=(2, N))      # c1' - c0': the digits of x* at every coefficient
    ga = stack[logN]
    ga[...] = _words(rng, v.l, 2, 2, N)                   # the mask row meets zero digits only
    ga[0, 1, 0], ga[0, 1, 1] = c0[0], c0[1] - T0
    ga[1, 1, 0], ga[1, 1, 1] = c1[0], c1[1] - T2
    gb = stack[logN + 1]
    gb[...] = _words(rng, v.l, 2, 2, N)
    _saturate(gb, v, seq, sign, columns)
    return dict(stack=stack, table=np.concatenate([T0, T1, T2, T3]), sat=2, columns=tuple(columns), sign=sign, kind="tree")


def rotation_gate(v, s, sign=+1, columns=(0, 1), bits=None, seed=2):
    """Rotation step s saturated; bits = log2 N + 1 (default) or more: the further tree levels hold zero GGSWs."""
    N, logN = v.N, log2(v.N)
    bits = logN + 1 if bits is None else bits
    assert 0 <= s < logN < bits
    rng = np.random.default_rng(seed)
    x_star, seq, _ = extreme_value(v.logB, v.l, W)
    assert x_star % (1 << 33) == 0
    r = 1 << s
    comb = [int(t % r == 0) for t in range(N)]            # S = sum X^(j r)
    acc = []
    lo, _, hi = [int(x) for x in _same_digits(v, x_star, seq, even=True)]
    for x, e_half in ((hi, (hi // 2 + TOP) % MOD), (lo, lo // 2)):      # mask, body; the two roots of 2 e = x
        e = _as_words([(-e_half) % MOD if t < r else e_half for t in range(N)])
        A = [int(a) % MOD for a in negacyclic_exact(comb, e, W)]
        assert all((a - b) % MOD == x for a, b in zip(rotate(A, 2 * N - r, W), A))
        acc.append(_as_words(A))
    stack = np.zeros((bits, v.l, 2, 2, N), dtype=U64)
    table = _words(rng, 1 << bits)
    table[N:2 * N] = table[:N]
    table[N] = (int(table[0]) + program_word(v, 0)) % MOD
    gt = stack[logN]
    gt[...] = _words(rng, v.l, 2, 2, N)
    gt[0, 1, 0], gt[0, 1, 1] = acc[0], acc[1] - table[:N]
    gs = stack[s]
    gs[...] = _words(rng, v.l, 2, 2, N)
    _saturate(gs, v, seq, sign, columns)
    n_tree = (1 << (bits - logN)) - 1
    return dict(stack=stack, table=table, sat=n_tree + s, columns=tuple(columns), sign=sign, kind="rotation %d" % s)


def control_gate(v, bits, seed):
    rng = np.random.default_rng(seed)
    return dict(stack=_words(rng, bits, v.l, 2, 2, v.N), table=_words(rng, max(1 << bits, v.N)), sat=None, columns=(),
                sign=0, kind="control")


def crafted_launch(v):
    """The launch of the per-shape GPU cases, bits = log2 N + 2, seven gates: the three tree-saturating gates (positive,
    negative, mask column only), rotation step 0 (positive) and step log2 N - 1 (negative) saturated, two controls."""
    logN = log2(v.N)
    bits = logN + 2
    gates = [tree_gate(v, +1, seed=11), tree_gate(v, -1, seed=12), tree_gate(v, +1, columns=(0,), seed=13),
             rotation_gate(v, 0, +1, bits=bits, seed=14), rotation_gate(v, logN - 1, -1, bits=bits, seed=15),
             control_gate(v, bits, 16), control_gate(v, bits, 17)]
    return finish(v, gates)


def control_launch(v, bits, count, seed=30):
    return finish(v, [control_gate(v, bits, seed + g) for g in range(count)])


def finish(v, gates):
    """-> dict(v, bits, stacks [G][bits][l][2][2 N], tables [G][words], ref [G][N+1], peaks (per gate: per CMUX), gates)"""
    refs, peaks = zip(*[vertical_packing_exact(g["stack"], g["table"], v) for g in gates])
    bits = gates[0]["stack"].shape[0]
    return dict(v=v, bits=bits, stacks=np.stack([g["stack"] for g in gates]).reshape(len(gates), bits, v.l, 2, 2 * v.N),
                tables=np.stack([g["table"] for g in gates]), ref=np.stack(refs), peaks=list(peaks), gates=gates)


def permuted(launch, order):
    """The same gates in another order (the references are per gate)."""
    order = list(order)
    return dict(launch, stacks=launch["stacks"][order], tables=launch["tables"][order], ref=launch["ref"][order],
                peaks=[launch["peaks"][g] for g in order], gates=[launch["gates"][g] for g in order])


# the cases of tests/test_gpu_vertical_packing_edges.py (tests/test_vp_edges.py pins every one on the CPU)
MIDDLE = {2: 8, 3: 5}
SHAPES = [VShape(N, l, MIDDLE[l]) for N in (512, 1024, 2048) for l in (2, 3)]
# (2,15) and (3,10) are the two admitted pairs with logB l = 30, the largest; (2,14) and (3,9) the next below
DECOMPOSITIONS = [VShape(512, l, logB) for l, logB in ((2, 1), (3, 1), (2, 15), (3, 10), (2, 14), (3, 9))]
DEPTHS = [(VShape(512, l, MIDDLE[l]), bits, count) for l in (2, 3) for bits, count in ((1, 3), (9, 3), (15, 3))]
BATCH_ORDER = [0, 5, 3, 2, 6, 4, 1]      # crafted gates first and last, the controls inside


def _name(v):
    return "N%d_l%d_B%d" % v


CASES = {}
CASES.update({"shape-" + _name(v): (lambda v=v: crafted_launch(v)) for v in SHAPES})
CASES.update({"decomposition-" + _name(v): (lambda v=v: crafted_launch(v)) for v in DECOMPOSITIONS})
CASES.update({"depth-%s-bits%d" % (_name(v), bits): (lambda v=v, bits=bits, count=count: control_launch(v, bits, count))
              for v, bits, count in DEPTHS})
CASES.update({"batch-" + _name(v): (lambda v=v: permuted(launch("shape-" + _name(v)), BATCH_ORDER)) for v in SHAPES[:2]})
_built = {}


def launch(name):
    """The launch of a named case, built once per process."""
    if name not in _built:
        _built[name] = CASES[name]()
    return _built[name]
