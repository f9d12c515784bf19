"""Rows that drive a bootstrap's front - the modulus switch of the input row, the gate's linear combination, the rotated read
of the accumulator - through every rotation amount and onto the rounding tie, and an exact reference for them.

Every bootstrap kernel carries its own copy of that front and its own indexing of the rotated read; random rows meet a given
amount (a = 1, N, 2N - 1, the lane and wave seams at 63 / 64 / 65) only by chance, and a word on the rounding tie of the
modulus switch practically never.  This module constructs them:

  word_for        a torus word that switches to a chosen amount: the exact multiple, the largest word that still rounds down
                  to it, or the word exactly half way, which rounds UP to it (a = 0: 2^w - h rounds to 2N, which wraps to 0)
  ALL, E, R       amount sets: every amount; the edges and the seams; the edges and one amount per lane residue mod 64
  mask_sweep      one row per amount whose only non-zero mask word switches to it: one active step, the body random
  body_sweep      zero mask, the body switches to the amount: no step runs (zero_mask_reference is the whole output);
                  step=(i, a1) adds one fixed active step, so that every coefficient of the rotated test vector is read
  constant_rows   every mask word alike, one row per edge, and one row that walks through the edges
  wrap_groups     multi-bit groups whose subset sums wrap past 2N or cancel to 0
  gate_rows       operand rows of every boolean gate, solved so that the gate's linear combination IS such a row: the word
                  lost by the XOR / XNOR doubling in both of its pre-images, sums that wrap past 2^32, both MUX halves

The flavour of a row's words cycles with the row index, so every amount set meets every flavour.  No GPU and no project
code is used here; the modulus switch, the rotation and the exact bootstrap are tests/saturation.py's, the multi-bit step is
tests/saturation_mb.py's.  tests/test_rotation_edges.py pins this module and the CPU oracles against each other;
tests/test_gpu_rotation_edges.py runs the rows on every kernel."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import saturation as S  # noqa: E402
import saturation_mb as M  # noqa: E402

Shape = S.Shape
FLAVOURS = ("exact", "below", "tie")


def dtype_of(width):
    return np.uint32 if width == 32 else np.uint64


def half_step(N, width):
    """h = 2^(w - log2(2N) - 1): half the distance of two neighbouring multiples."""
    return 1 << (width - ((2 * N).bit_length() - 1) - 1)


def word_for(a, N, width, flavour):
    """A word of Z_2^w that modulus-switches to a (round half up, 2N wraps to 0) - a Python integer."""
    h = half_step(N, width)
    a = int(a) % (2 * N)
    if flavour == "exact":
        word = a * 2 * h
    elif flavour == "below":
        word = a * 2 * h + h - 1
    elif flavour == "tie":
        word = ((a - 1) % (2 * N)) * 2 * h + h
    else:
        raise ValueError(flavour)
    assert 0 <= word < (1 << width) and S.modswitch(word, N, width) == a, (a, N, width, flavour)
    return word


def ALL(N):
    return list(range(2 * N))


def E(N):
    """The edges (0, 1, N - 1, N, N + 1, 2N - 1 and the quarter points) and the lane / wave seams 63 / 64 / 65 on both sides of
    0, N and 2N."""
    return sorted({0, 1, 2, 63, 64, 65, N // 2, N - 65, N - 64, N - 63, N - 1, N, N + 1, N + 63, N + 64, N + 65, 3 * N // 2,
                   2 * N - 65, 2 * N - 64, 2 * N - 63, 2 * N - 2, 2 * N - 1})


def R(N):
    """E(N) and r (2N / 64) + r for r = 0 .. 63: every lane residue mod 64 once, spread over the whole range (below N = 2048,
    where the last ones would pass 2N, they are reduced mod 2N: the residues stay)."""
    spread = {(r * (2 * N // 64) + r) % (2 * N) for r in range(64)}
    assert {a % 64 for a in spread} == set(range(64)) and max(spread) < 2 * N
    return sorted(set(E(N)) | spread)


def _rand(rng, width, size=None):
    return rng.integers(0, 1 << width, size=size, dtype=dtype_of(width))


def mask_position(a, n, g=1):
    """Where the one non-zero mask word of amount a sits: a mod n; under a grouping factor g, member a mod g of group
    (a // g) mod (n / g)."""
    if g <= 1:
        return a % n
    assert n % g == 0
    return ((a // g) % (n // g)) * g + a % g


def mask_sweep(shape, A, width, rng, g=1):
    """-> (lwe [len(A), n + 1], flavours).  Row q: mask word mask_position(A[q]) = word_for(A[q], flavour q mod 3), the other
    mask words 0, the body random."""
    n, N = shape.n, shape.N
    lwe = np.zeros((len(A), n + 1), dtype=dtype_of(width))
    flav = [FLAVOURS[q % 3] for q in range(len(A))]
    for q, a in enumerate(A):
        lwe[q, mask_position(a, n, g)] = word_for(a, N, width, flav[q])
        lwe[q, n] = _rand(rng, width)
        assert [S.modswitch(int(w), N, width) for w in lwe[q, :n]].count(0) >= n - 1
    return lwe, flav


def body_sweep(shape, A, width, step=None):
    """-> (lwe [len(A), n + 1], flavours).  Row q: a zero mask and the body word_for(A[q], flavour q mod 3); step = (i, a1)
    sets mask word i of every row to an amount a1 (its flavour cycles with the row as well, one place ahead).  Every word of
    these rows is chosen, so the family takes no random generator."""
    n, N = shape.n, shape.N
    lwe = np.zeros((len(A), n + 1), dtype=dtype_of(width))
    flav = [FLAVOURS[q % 3] for q in range(len(A))]
    for q, bt in enumerate(A):
        lwe[q, n] = word_for(bt, N, width, flav[q])
        if step is not None:
            lwe[q, step[0]] = word_for(step[1], N, width, FLAVOURS[(q + 1) % 3])
    return lwe, flav


def constant_rows(shape, width, rng):
    """-> (lwe [len(E) + 1, n + 1], amounts).  Row q < len(E): every mask word is word_for(E[q], flavour q mod 3), the body
    random; the last row's mask word i is E[(i + 1) mod len(E)] with flavour i mod 3 (amounts[-1] is None)."""
    n, N = shape.n, shape.N
    edges = E(N)
    lwe = np.zeros((len(edges) + 1, n + 1), dtype=dtype_of(width))
    for q, a in enumerate(edges):
        lwe[q, :n] = word_for(a, N, width, FLAVOURS[q % 3])
        assert all(S.modswitch(int(w), N, width) == a for w in lwe[q, :n])
    for i in range(n):
        lwe[-1, i] = word_for(edges[(i + 1) % len(edges)], N, width, FLAVOURS[i % 3])
    lwe[:, n] = _rand(rng, width, len(lwe))
    return lwe, edges + [None]


def wrap_group_patterns(N, g):
    """-> [(label, the g switched members of a group)], the subset sums checked here:
    cancel   (a, 2N - a) / (a, a', 2N - a - a'): the full subset's exponent is 0 while the partial ones are not
    N..N     (N, .., N): the full sum is g N, 0 or N mod 2N
    top      (2N - 1, .., 2N - 1): every subset of s members has exponent 2N - s, the sums run to 2 g N - g
    wrap     (N, 2N - 1) / (N, 1, 2N - 1): tests/saturation_mb.py's wrapping members"""
    out = []
    for a in (1, 63, 64, N - 1, N, N + 1, 2 * N - 1):
        if g == 2:
            members = [a, (2 * N - a) % (2 * N)]
        else:
            b = (a + 64) % (2 * N)
            members = [a, b, (4 * N - a - b) % (2 * N)]
        es = M.subset_exponents(members, N)
        assert es[-1] == 0 and es[1] == a and sum(members) >= 2 * N
        out.append(("cancel_%d" % a, members))
    members = [N] * g
    assert M.subset_exponents(members, N)[-1] == (g * N) % (2 * N) and sum(members) == g * N
    out.append(("N..N", members))
    members = [2 * N - 1] * g
    es = M.subset_exponents(members, N)
    assert sum(members) == 2 * g * N - g and all(es[s] == (2 * N - bin(s).count("1")) % (2 * N) for s in range(1 << g))
    out.append(("top", members))
    members = [N, 2 * N - 1] if g == 2 else [N, 1, 2 * N - 1]
    es = M.subset_exponents(members, N)
    assert sum(members) >= 2 * N and es[-1] == (sum(members) - 2 * N) and es[-1] < 2 * N
    out.append(("wrap", members))
    return out


def wrap_groups(shape, g, width, rng):
    """-> (lwe [patterns, n + 1], labels), g > 1 only.  Every group of row q holds pattern q (flavour: member index + q mod 3),
    the body is random."""
    assert g > 1 and shape.n % g == 0 and width == 64
    n, N = shape.n, shape.N
    pats = wrap_group_patterns(N, g)
    lwe = np.zeros((len(pats), n + 1), dtype=dtype_of(width))
    for q, (_, members) in enumerate(pats):
        for i in range(n):
            lwe[q, i] = word_for(members[i % g], N, width, FLAVOURS[(i + q) % 3])
        assert [S.modswitch(int(w), N, width) for w in lwe[q, :g]] == members
    lwe[:, n] = _rand(rng, width, len(lwe))
    return lwe, [p[0] for p in pats]


def zero_mask_reference(tv, bt, k, N, width):
    """The output of a bootstrap no step of which is active: k N zero mask words, and as the body coefficient 0 of
    X^(-bt) tv, that is tv[bt] for bt < N and -tv[bt - N] beyond.  Plain integers."""
    bt = int(bt) % (2 * N)
    body = int(tv[bt]) if bt < N else (-int(tv[bt - N])) % (1 << width)
    out = np.zeros(k * N + 1, dtype=dtype_of(width))
    out[k * N] = body
    return out


def zero_mask_rows(lwe, tvs, idx, k, N, width):
    """zero_mask_reference of every row of a body sweep without a step."""
    assert not lwe[:, :-1].any()
    return np.stack([zero_mask_reference(tvs[idx[q]], S.modswitch(int(lwe[q, -1]), N, width), k, N, width)
                     for q in range(len(lwe))])


# ------------------------------------------------------------------------------------------------------------------
# the boolean gates' linear combinations (tfhe's formulas in integers mod 2^32) and operand rows solved for a chosen one
# ------------------------------------------------------------------------------------------------------------------
MOD32 = 1 << 32
PT_TRUE, PT_FALSE = 1 << 29, (-(1 << 29)) % MOD32
# the op-codes of the gate enumeration (oracle.AND ... are the same numbers; tests/test_rotation_edges.py checks)
AND, MUX, NAND, NOR, OR, XNOR, XOR = 0, 3, 4, 5, 7, 8, 9
GATE_OPS = [(AND, 0), (OR, 0), (NAND, 0), (NOR, 0), (XOR, 0), (XNOR, 0), (MUX, 0), (MUX, 1)]     # (op, which)


def lincomb(op, which, l, r, c, n):
    """The row a gate bootstraps, from operand rows of n + 1 Python integers (c: MUX only)."""
    out = []
    for i in range(n + 1):
        T, F = (PT_TRUE, PT_FALSE) if i == n else (0, 0)
        li, ri = int(l[i]), int(r[i])
        if op == AND:
            v = li + ri + F
        elif op == OR:
            v = li + ri + T
        elif op == NAND:
            v = -(li + ri) + T
        elif op == NOR:
            v = -(li + ri) + F
        elif op == XOR:
            v = 2 * (li + ri + T)
        elif op == XNOR:
            v = 2 * (-(li + ri + T))
        elif op == MUX:
            v = int(c[i]) + li + F if which == 0 else -int(c[i]) + ri + F
        else:
            raise ValueError(op)
        out.append(v % MOD32)
    return out


def _even_word(word, a, N):
    """The nearest even word with the same switched value (the doubling of XOR / XNOR reaches even words only)."""
    if word % 2 == 0:
        return word, 0
    for cand in (word - 1, word + 1):
        if S.modswitch(cand % MOD32, N, 32) == a:
            return cand % MOD32, 1
    raise AssertionError((word, a))


def gate_rows(n, N, targets, rng):
    """Operand rows for every op of GATE_OPS x every target t x the three flavours (XOR / XNOR: x both pre-images of the
    doubling).  The prescribed combination of a case has every mask word = word_for(t, flavour) and the body =
    word_for(the next target, flavour); one operand is solved for it, the others are uniform:
        AND OR NAND NOR XOR XNOR   l uniform, r solved (c unused)
        MUX, half 0  (c + l + F)   c uniform, l solved, r uniform (it enters half 1 only)
        MUX, half 1  (-c + r + F)  c uniform, r solved, l uniform
    -> dict(op, which, l, r, c [cases, n + 1] uint32, want [cases, n + 1] uint32 (the prescribed row), target, flavour,
            preimage (0 / 1: the top bit of the sum before the doubling; -1 where there is none), replaced (count of odd
            words moved to the nearest even word of the same switched value), wraps {op: rows in which l + r passes 2^32})"""
    targets = list(targets)
    ops, whichs, ls, rs, cs, wants, tg, fl, pre = [], [], [], [], [], [], [], [], []
    replaced, wraps = 0, {}
    for op, which in GATE_OPS:
        for ti, t in enumerate(targets):
            body_t = targets[(ti + 1) % len(targets)]
            for f in FLAVOURS:
                for top in ((0, 1) if op in (XOR, XNOR) else (-1,)):
                    want = [word_for(t, N, 32, f)] * n + [word_for(body_t, N, 32, f)]
                    if op in (XOR, XNOR):
                        fixed = [_even_word(w, a, N) for w, a in zip(want, [t] * n + [body_t])]
                        want = [w for w, _ in fixed]
                        replaced += sum(c for _, c in fixed)
                    l = [int(v) for v in _rand(rng, 32, n + 1)]
                    r = [int(v) for v in _rand(rng, 32, n + 1)]
                    c = [int(v) for v in _rand(rng, 32, n + 1)]
                    for i in range(n + 1):
                        T, F = (PT_TRUE, PT_FALSE) if i == n else (0, 0)
                        if op == AND:
                            r[i] = want[i] - l[i] - F
                        elif op == OR:
                            r[i] = want[i] - l[i] - T
                        elif op == NAND:
                            r[i] = -(want[i] - T) - l[i]
                        elif op == NOR:
                            r[i] = -(want[i] - F) - l[i]
                        elif op == XOR:            # 2 u = want, u = l + r + T: both u = want / 2 and want / 2 + 2^31
                            r[i] = want[i] // 2 + (top << 31) - T - l[i]
                        elif op == XNOR:           # -2 u = want: u = -(want / 2) mod 2^31, and that + 2^31
                            r[i] = (-(want[i] // 2)) % (1 << 31) + (top << 31) - T - l[i]
                        elif which == 0:
                            l[i] = want[i] - c[i] - F
                        else:
                            r[i] = want[i] + c[i] - F
                        l[i] %= MOD32
                        r[i] %= MOD32
                    assert lincomb(op, which, l, r, c, n) == want, (op, which, t, f)
                    assert [S.modswitch(w, N, 32) for w in want] == [t] * n + [body_t]
                    if op in (XOR, XNOR):
                        assert all(((l[i] + r[i] + (PT_TRUE if i == n else 0)) % MOD32) >> 31 == top for i in range(n + 1))
                    if any(l[i] + r[i] >= MOD32 for i in range(n + 1)):
                        wraps[(op, which)] = wraps.get((op, which), 0) + 1
                    for lst, v in zip((ops, whichs, ls, rs, cs, wants, tg, fl, pre), (op, which, l, r, c, want, t, f, top)):
                        lst.append(v)
    assert all(wraps.get(k, 0) > 0 for k in GATE_OPS), wraps
    u32 = lambda rows: np.array(rows, dtype=np.uint32)          # noqa: E731
    return dict(op=np.array(ops, dtype=np.int32), which=np.array(whichs, dtype=np.int32), l=u32(ls), r=u32(rs), c=u32(cs),
                want=u32(wants), target=tg, flavour=fl, preimage=pre, replaced=replaced, wraps=wraps)
