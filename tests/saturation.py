"""Bootstraps whose one CMUX step is aligned to the kernels' exactness bound, and a plain exact reference for them.

Every bootstrap kernel computes a blind-rotation step's external product in prime fields and lifts the result back to the
integers; that is exact only while the true integer coefficient of every column sum stays inside the field's (or the CRT
pair's) half.  Random inputs stay orders of magnitude below that, so this module builds the input that does not:

  step i1 (programming)   the test vector is a constant t with -2t = 2^(w - logB): under a rotation by X^N = -1 the difference
                          decomposes to the single digit +1 at the first level, constant over the polynomial, and a key
                          polynomial that holds one word at X^0 adds that word to every coefficient: the key of step i1 writes
                          the accumulator, mask polynomials included.
  step i2 (saturating)    the accumulator written is the constant a with -2a = x*, the torus value whose digits have the
                          largest sum of magnitudes the decomposition rule produces (extreme_value).  Every key polynomial of
                          step i2 holds the largest word, with the sign of the digit it multiplies: coefficient N-1 of every
                          column sum is then sum_j |d_j| x (k+1) x N x 2^(w-1), all terms of one sign - the quantity the
                          capacity checks bound - and the other coefficients sweep the signed range in between.

No GPU and no project code is used here: the decomposition, the rotation, the schoolbook negacyclic products and the column
sums are restated in integers (cmux_step_exact), reduced mod 2^w at the very end, with the largest exact column-sum
coefficient reported beside the result.  tests/test_saturating_inputs.py pins this module against both CPU oracles;
tests/test_gpu_saturation.py runs the cases on every kernel.
"""
from collections import namedtuple

import numpy as np

Shape = namedtuple("Shape", "n k N l logB")

# the primes of helm_amd/csrc/ntt_fp64.h
FPG, FPG2, FPH, FPI = 5072 ** 4 + 1, 5096 ** 4 + 1, 6432 ** 4 + 1, 5440 ** 4 + 1
FPJ, FPJ2 = 2736 ** 4 + 1, 2872 ** 4 + 1


def shape_of(params):
    """Shape of a helm_amd Params / SiParams structure."""
    return Shape(int(params.n), int(params.k), int(params.N), int(params.pbs_l), int(params.pbs_logB))


def capacity_bound(shape, width):
    """(k+1) l N 2^(logB-1) 2^(w-1): what helm_hip_ctx_create / helm_si_ctx_create_ex compare with a half-modulus."""
    return (shape.k + 1) * shape.l * shape.N * (1 << (shape.logB - 1)) * (1 << (width - 1))


# ------------------------------------------------------------------------------------------------------------------
# the decomposition rule (closest representable, balanced digits, ties by the next level's top bit)
# ------------------------------------------------------------------------------------------------------------------
def digits(x, logB, l, width):
    """Signed digits of the torus value x (Python integers), first = most significant level."""
    x = int(x) % (1 << width)
    rep = logB * l
    assert 1 <= rep <= width
    state = x if rep == width else ((x + (1 << (width - 1 - rep))) % (1 << width)) >> (width - rep)
    B = 1 << logB
    out = [0] * l
    for lev in range(l - 1, -1, -1):
        d = state % B
        state //= B
        carry = 1 if (d > B // 2 or (d == B // 2 and (state % B) >= B // 2)) else 0
        state += carry
        out[lev] = d - carry * B
    return out


def extreme_digits(logB, l):
    """-> (digit sequence, sum of magnitudes): the largest sum of |digit| the rule can produce, by dynamic programming over
    the levels.  The rule's outputs are the balanced digit strings with d in [-B/2, B/2] in which a digit of +B/2 has a
    next more significant digit in [0, B/2 - 1] and a digit of -B/2 one in [-B/2 + 1, 0] (that is the tie rule, and it makes
    the representation unique).  State of the program: what the level below demands of this one; per level only the ends of
    the permitted ranges can be optimal.  (Closed form: l B/2 - floor(l/2); test_saturating_inputs.py checks both the
    program and the characterisation by brute force over every input at small sizes.)"""
    h = (1 << logB) // 2
    cand = sorted({h, -h, h - 1, 1 - h, 0})
    allowed = {"free": lambda d: True, "nonneg": lambda d: 0 <= d <= h - 1, "nonpos": lambda d: 1 - h <= d <= 0}
    # best[state] = (sum, digits from the least significant level up to here), state = demand on the NEXT (higher) level
    best = {"free": (0, [])}
    for lev in range(l - 1, -1, -1):
        nxt = {}
        for demand, (tot, seq) in best.items():
            for d in cand:
                # (the most significant level has nothing above it to carry into: its tie is always +B/2)
                if not allowed[demand](d) or (lev == 0 and d == -h):
                    continue
                out = "nonneg" if d == h else "nonpos" if d == -h else "free"
                v = (tot + abs(d), seq + [d])
                if out not in nxt or v[0] > nxt[out][0]:
                    nxt[out] = v
        best = nxt
    tot, seq = max(best.values(), key=lambda v: v[0])
    return seq[::-1], tot


def extreme_value(logB, l, width):
    """-> (x*, digits, sum of |digit|): a torus value whose digits reach extreme_digits' maximum (verified through digits())."""
    seq, tot = extreme_digits(logB, l)
    x = sum(d << (width - logB * (j + 1)) for j, d in enumerate(seq)) % (1 << width)
    assert digits(x, logB, l, width) == seq, (seq, digits(x, logB, l, width))
    return x, seq, tot


# ------------------------------------------------------------------------------------------------------------------
# one CMUX step in integers
# ------------------------------------------------------------------------------------------------------------------
def modswitch(x, N, width):
    """Z_2^w -> Z_2N, round half up."""
    log2_2n = (2 * N).bit_length() - 1
    return (((int(x) >> (width - log2_2n - 1)) + 1) >> 1) % (2 * N)


def rotate(poly, a, width):
    """X^a * poly in Z_2^w[X] / (X^N + 1), a in [0, 2N): a list of Python integers."""
    N = len(poly)
    out = [0] * N
    for j in range(N):
        idx = (j - a) % (2 * N)
        out[j] = int(poly[idx]) if idx < N else (-int(poly[idx - N])) % (1 << width)
    return out


def negacyclic_exact(d, key_words, width):
    """The exact integer negacyclic product of a digit polynomial (small signed integers) and a key polynomial (words of
    2^w read as signed): schoolbook sums, no modulus.  The words are cut into 16-bit limbs so that every partial sum
    (|digit| x 2^16 x N) fits an int64 and numpy's integer convolution is exact; the limbs are recombined as Python
    integers.  -> object array of N Python integers."""
    N = len(d)
    d = np.asarray(d, dtype=np.int64)
    assert int(np.abs(d).max(initial=0)) * (1 << 16) * N < (1 << 62)
    v = np.asarray(key_words, dtype=np.uint64)
    if width == 32:
        v = v.astype(np.uint32).view(np.int32).astype(np.int64)
    else:
        v = v.view(np.int64)
    n_limbs = width // 16
    total = np.zeros(N, dtype=object)
    for i in range(n_limbs):
        limb = (v >> (16 * i)) & 0xFFFF if i < n_limbs - 1 else v >> (16 * i)   # the top limb keeps the sign
        full = np.convolve(d, limb)                                           # 2N - 1 exact int64 sums
        nega = full[:N].copy()
        nega[:N - 1] -= full[N:]
        total = total + nega.astype(object) * (1 << (16 * i))
    return total


def negacyclic_plain(d, key_signed):
    """The same product with Python integers only (two loops): what negacyclic_exact is checked against."""
    N = len(d)
    out = [0] * N
    for a in range(N):
        da = int(d[a])
        if da == 0:
            continue
        for b in range(N):
            if a + b < N:
                out[a + b] += da * int(key_signed[b])
            else:
                out[a + b - N] -= da * int(key_signed[b])
    return out


def cmux_step_exact(acc, a_tilde, key_step, shape, width, c1=None):
    """acc: (k+1) polynomials of N Python integers mod 2^w; key_step: the words [l][k+1][k+1][N] of one blind-rotation step.
    c1: None (the step of a blind rotation: the other operand is X^a_tilde acc), or the (k+1) polynomials of a given second
    ciphertext (a CMUX of two ciphertexts, acc + GGSW (x) (c1 - acc); a_tilde is not read).
    -> (new accumulator, the largest |exact column-sum coefficient| before the reduction mod 2^w)."""
    k1, N, l = shape.k + 1, shape.N, shape.l
    key_step = np.asarray(key_step).reshape(l, k1, k1, N)
    mod = 1 << width
    dig = np.zeros((k1, l, N), dtype=np.int64)
    for r in range(k1):
        rot = rotate(acc[r], a_tilde, width) if c1 is None else c1[r]
        for t in range(N):
            dig[r, :, t] = digits((rot[t] - int(acc[r][t])) % mod, shape.logB, l, width)
    peak, new = 0, []
    for c in range(k1):
        col = np.zeros(N, dtype=object)
        for r in range(k1):
            for j in range(l):
                if dig[r, j].any():
                    col = col + negacyclic_exact(dig[r, j], key_step[j, r, c], width)
        peak = max(peak, max(abs(int(v)) for v in col))
        new.append([(int(acc[c][t]) + int(col[t])) % mod for t in range(N)])
    return new, peak


def bootstrap_exact(lwe, tv, bsk, shape, width):
    """Blind rotation over the active steps (a step whose switched mask element is 0 is skipped) and sample extraction.
    -> (k N + 1 words as a numpy array of the torus type, the largest exact column-sum coefficient of any step)."""
    n, k, N = shape.n, shape.k, shape.N
    mod = 1 << width
    bsk = np.asarray(bsk).reshape(n, -1)
    bt = modswitch(lwe[n], N, width)
    acc = [[0] * N for _ in range(k)] + [rotate([int(v) for v in tv], (2 * N - bt) % (2 * N), width)]
    peak = 0
    for i in range(n):
        a = modswitch(lwe[i], N, width)
        if a == 0:
            continue
        acc, pk = cmux_step_exact(acc, a, bsk[i], shape, width)
        peak = max(peak, pk)
    out = []
    for r in range(k):
        out.append(acc[r][0])
        out.extend((-acc[r][N - t]) % mod for t in range(1, N))
    out.append(acc[k][0])
    return np.array(out, dtype=np.uint32 if width == 32 else np.uint64), peak


# ------------------------------------------------------------------------------------------------------------------
# the loaders' key rule, restated
# ------------------------------------------------------------------------------------------------------------------
def key_bound(bsk, shape, width):
    """B/2 x the largest l1-norm over the key polynomials that meet in one output column or, transposed, in one row, of one
    step: the rule of helm_hip_load_bootstrap_key and helm_si_load_bootstrap_key, both groupings.  A Python integer."""
    k1, N, l = shape.k + 1, shape.N, shape.l
    v = np.asarray(bsk).reshape(shape.n, l, k1, k1, N)
    v = v.astype(np.uint32).view(np.int32).astype(np.int64) if width == 32 else v.astype(np.uint64).view(np.int64)
    mag = np.where(v < 0, -v, v).view(np.uint64)      # (-2^63 wraps to the word 2^63: its magnitude)
    # exact sums of up to N magnitudes below 2^64: the two 32-bit halves summed apart
    norms = (mag >> np.uint64(32)).sum(axis=-1, dtype=np.uint64).astype(object) * (1 << 32) + \
        (mag & np.uint64(0xFFFFFFFF)).sum(axis=-1, dtype=np.uint64).astype(object)
    worst = 0
    for i in range(shape.n):
        l1 = norms[i]
        for c in range(k1):
            by_col = sum(l1[j][r][c] for j in range(l) for r in range(k1))
            by_row = sum(l1[j][c][r] for j in range(l) for r in range(k1))
            worst = max(worst, by_col, by_row)
    return worst * (1 << (shape.logB - 1))


# ------------------------------------------------------------------------------------------------------------------
# the construction
# ------------------------------------------------------------------------------------------------------------------
def _random_key(shape, width, seed):
    """Uniform words: what a generated key's mask polynomials are (used where the caller has no generated key at hand)."""
    rng = np.random.default_rng(seed)
    k1 = shape.k + 1
    return rng.integers(0, 1 << width, size=(shape.n, shape.l, k1, k1, shape.N), dtype=np.uint32 if width == 32 else np.uint64)


def saturating_case(shape, width, sign=+1, columns="all", base_key=None, budget=None, steps=None):
    """-> dict(bsk, lwe, tv, peak, ref, x_star, digits, digit_sum).

    bsk: the words of base_key (a generated key; uniform words when None) with step i1 programmed and step i2 saturated.
    sign = -1 flips every key sign of step i2 (the negative extreme at coefficient N-1).  columns: "all", or one column
    index - only that column of step i2 is saturated, the others keep base_key's words.  budget: None saturates all N
    coefficients of each polynomial; an integer caps B/2 x (the column's l1-norm) at it by saturating only the leading
    coefficients (one more holds the remainder), which is how a key is placed just under or over a loader's threshold.
    peak: the largest exact column-sum coefficient of the saturating step, from cmux_step_exact; ref: the bootstrap's
    output by bootstrap_exact."""
    n, k, N, l, logB = shape
    k1, mod = k + 1, 1 << width
    dt = np.uint32 if width == 32 else np.uint64
    i1, i2 = steps if steps is not None else (1, n - 2)
    assert 0 <= i1 < i2 < n
    bsk = (np.array(base_key, dtype=dt) if base_key is not None else _random_key(shape, width, 99)).reshape(n, l, k1, k1, N).copy()
    x_star, seq, tot = extreme_value(logB, l, width)
    assert x_star % 2 == 0
    a = ((mod - x_star) // 2) % mod                   # -2a = x*
    t = (mod - (1 << (width - logB))) // 2            # -2t = 2^(w - logB): digits (1, 0, ..., 0)
    assert digits((-2 * t) % mod, logB, l, width) == [1] + [0] * (l - 1)
    # step i1: digit +1 (level 0, body row k) x (one word at X^0) adds that word to every coefficient of the column
    for c in range(k1):
        bsk[i1, 0, k, c, :] = 0
        bsk[i1, 0, k, c, 0] = (a - (t if c == k else 0)) % mod
    # step i2
    big_pos, big_neg = (1 << (width - 1)) - 1, 1 << (width - 1)     # 2^(w-1) - 1 and the word of -2^(w-1)
    if budget is None:
        full, rest = N, 0
    else:
        per_coeff = k1 * l * (1 << (logB - 1))                       # budget taken by one unit of magnitude in every polynomial
        units = int(budget) // per_coeff                             # magnitude available per polynomial
        full, rest = divmod(units, big_pos)
        assert full < N, "the budget exceeds a fully saturated key"
    cols = range(k1) if columns == "all" else [int(columns)]
    for c in cols:
        for r in range(k1):
            for j in range(l):
                s = sign * (1 if seq[j] >= 0 else -1)
                poly = np.zeros(N, dtype=object)
                poly[:full] = big_pos if s > 0 else big_neg
                if budget is not None:
                    poly[:full] = big_pos if s > 0 else (mod - big_pos)   # equal magnitudes: the l1-norm is what is set
                    poly[full] = rest if s > 0 else (mod - rest) % mod
                bsk[i2, j, r, c, :] = poly.astype(dt)
    lwe = np.zeros(n + 1, dtype=dt)
    lwe[i1] = lwe[i2] = 1 << (width - 1)              # switches to N: X^N = -1
    tv = np.full(N, t, dtype=dt)
    # the reference, step by step, so that the programmed accumulator and the peak of the saturating step are on record
    acc = [[0] * N for _ in range(k)] + [[t] * N]
    acc, _ = cmux_step_exact(acc, N, bsk[i1], shape, width)
    assert all(v == a for poly in acc for v in poly), "step i1 did not write the accumulator"
    _, peak = cmux_step_exact(acc, N, bsk[i2], shape, width)
    ref, _ = bootstrap_exact(lwe, tv, bsk, shape, width)
    return dict(bsk=bsk.reshape(-1), lwe=lwe, tv=tv, peak=peak, ref=ref, x_star=x_star, digits=seq, digit_sum=tot,
                steps=(i1, i2))


def near_threshold_key(shape, width, target_ratio, half, base_key=None, sign=+1):
    """A saturating case whose key has B/2 x (largest column l1-norm) at target_ratio x half (within 0.1 %), every other
    step keeping base_key's words: saturating_case under a budget.  half: the half-modulus the loader compares with."""
    budget = int(target_ratio * half)
    case = saturating_case(shape, width, sign=sign, base_key=base_key, budget=budget)
    case["budget"] = budget
    return case


# ------------------------------------------------------------------------------------------------------------------
# the shapes of the cases (tests/test_saturating_inputs.py pins the named ones to the library's parameter sets)
# ------------------------------------------------------------------------------------------------------------------
NAMED32 = {"toy": Shape(24, 1, 512, 2, 8), "toy_k2": Shape(20, 2, 512, 3, 6),
           "toy_1024": Shape(16, 1, 1024, 3, 7), "toy_1024_l2": Shape(16, 1, 1024, 2, 7)}
NAMED64 = {"si_toy_512": Shape(12, 1, 512, 2, 15), "si_toy_1024": Shape(10, 1, 1024, 1, 23),
           "si_toy_2048": Shape(8, 1, 2048, 1, 23), "si_toy_2048_l2": Shape(6, 1, 2048, 2, 14),
           "si_toy_512_k3": Shape(10, 3, 512, 1, 18), "si_toy_512_k2": Shape(9, 2, 512, 1, 20),
           "si_toy_1024_k2": Shape(10, 2, 1024, 1, 23)}
TUNED32 = {(512, 2, 3), (512, 1, 3), (512, 1, 2), (1024, 1, 3), (1024, 1, 2)}                        # (N, k, l)
TUNED64 = {(1, N, l) for N in (512, 1024, 2048) for l in (1, 2)} | {(2, 512, 1), (3, 512, 1), (2, 1024, 1)}  # (k, N, l)


def nearest_capacity_shape(width, n):
    """The untuned shape a context creation admits whose capacity bound is the largest fraction of the half-modulus it is
    compared with (ties: the smallest key): enumeration over the admitted domain of helm_hip_ctx_create (32) /
    helm_si_ctx_create_ex with the generic kernel allowed (64).  -> (Shape, bound / half)."""
    best = None
    for N in (256, 512, 1024, 2048):
        for k in range(1, (8192 if width == 32 else 4096) // N):
            for logB in range(1 if width == 32 else 2, 25 if width == 64 else 32):
                for l in range(1, 31 // logB + 1):
                    s = Shape(n, k, N, l, logB)
                    if width == 32:
                        if (N, k, l) in TUNED32 or capacity_bound(s, 32) * 1.0001 >= FPH / 2:
                            continue
                        ratio = capacity_bound(s, 32) / (FPH / 2)
                    else:
                        if (k, N, l) in TUNED64 or capacity_bound(s, 64) * 1.001 >= FPG * FPG2 / 2:
                            continue
                        if (1 << (logB - 1)) * 4 >= FPG2 / 2:
                            continue
                        ratio = capacity_bound(s, 64) / (FPG * FPG2 / 2)
                    key = (ratio, -(k + 1) ** 2 * l * N)
                    if best is None or key > best[0]:
                        best = (key, s)
    return best[1], best[0][0]


# (k, N, l, logB) of tests/test_gpu_generic_shapes.py and tests/test_gpu_si_generic_shapes.py, as Shapes with toy n
GENERIC32 = [Shape(16, *s) for s in [(3, 256, 2, 8), (4, 256, 3, 6), (2, 512, 2, 7), (2, 1024, 2, 6), (1, 2048, 3, 5),
                                     (1, 1024, 5, 6), (1, 256, 13, 2), (1, 256, 31, 1)]]
GENERIC64 = [Shape(12, *s) for s in [(2, 512, 2, 12), (2, 1024, 2, 12), (4, 512, 1, 22), (7, 512, 1, 22), (15, 256, 1, 22),
                                     (3, 1024, 1, 21), (1, 2048, 3, 8), (1, 256, 6, 5), (1, 256, 15, 2)]]
HALF_FPG, HALF_FPH, HALF_FPI = FPG / 2, FPH / 2, FPI / 2
HALF_49, HALF_46 = FPG * FPG2 / 2, FPJ * FPJ2 / 2
# the key-following loaders' thresholds: lazy field FpI when bound x 1.002 < p/2, 46-bit pair when bound x 1.05 < p p'/2
FPI_RATIO, PAIR46_RATIO = 0.997, 0.95


def all_shapes():
    """-> [(label, Shape, width, half-modulus of the field the kernels run it in, budget ratio or None)]: every shape the
    GPU test runs, once per field."""
    out = [("toy", NAMED32["toy"], 32, HALF_FPH, None), ("toy_k2", NAMED32["toy_k2"], 32, HALF_FPG, None),
           ("toy_k2 (FpH: variant 10)", NAMED32["toy_k2"], 32, HALF_FPH, None)]
    for name in ("toy_1024", "toy_1024_l2"):
        out.append((name + " (FpI)", NAMED32[name], 32, HALF_FPI, FPI_RATIO))
        out.append((name + " (FpH)", NAMED32[name], 32, HALF_FPH, None))
    out += [("generic k%d N%d l%d B%d" % s[1:], s, 32, HALF_FPH, None) for s in GENERIC32]
    s, _ = nearest_capacity_shape(32, 16)
    out.append(("generic, nearest the capacity bound: k%d N%d l%d B%d" % s[1:], s, 32, HALF_FPH, None))
    out += [(name, s, 64, HALF_49, None) for name, s in NAMED64.items()]
    # (si_toy_512_k2 has 20-bit digits: the loader takes the 46-bit pair up to 18 bits only, so it has no such row)
    out.append(("si_toy_512_k3 (46-bit pair)", NAMED64["si_toy_512_k3"], 64, HALF_46 / 1.05, PAIR46_RATIO))
    out += [("generic64 k%d N%d l%d B%d" % s[1:], s, 64, HALF_49, None) for s in GENERIC64]
    s, _ = nearest_capacity_shape(64, 12)
    out.append(("generic64, nearest the capacity bound: k%d N%d l%d B%d" % s[1:], s, 64, HALF_49, None))
    return out


def launch_case(shape, width, base_key, budget=None):
    """Three saturating rows that share ONE key, so that they run in one launch: step pairs (0, 1), (2, 3), (4, 5) of
    base_key hold the positive extreme, the negative extreme and the one-column variant; a row activates its own pair
    only, so each row's reference does not depend on the other pairs.
    -> dict(bsk, lwe [3, n+1], tv [N], ref [3, k N + 1], peak [3])"""
    assert shape.n >= 6
    a = saturating_case(shape, width, +1, base_key=base_key, budget=budget, steps=(0, 1))
    b = saturating_case(shape, width, -1, base_key=a["bsk"], budget=budget, steps=(2, 3))
    c = saturating_case(shape, width, +1, columns=shape.k // 2, base_key=b["bsk"], budget=budget, steps=(4, 5))
    assert np.array_equal(a["tv"], b["tv"]) and np.array_equal(a["tv"], c["tv"])
    return dict(bsk=c["bsk"], lwe=np.stack([a["lwe"], b["lwe"], c["lwe"]]), tv=a["tv"],
                ref=np.stack([a["ref"], b["ref"], c["ref"]]), peak=[a["peak"], b["peak"], c["peak"]])
