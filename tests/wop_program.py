"""A bootstrapping key that serves as a table of rows: chosen input rows for the WoP packing keyswitch through the
circuit bootstrap, whose ABI takes small LWE rows and keys only.

Any words are a bootstrapping key, and the accumulators of the circuit bootstrap are constants.  Level j (j < cbs_l)
bootstraps with the constant accumulator -alpha_j, alpha_j = 2^(63 - cbs_logB (j+1)), and adds alpha_j to the body.  An
input row with the body -2^62 (0 after the + q/4: no initial rotation) and one non-zero mask word, word i =
2^(64 - (log2 N + 1)) (it switches to the rotation 1), runs exactly one CMUX step, with GGSW i of the key.  The step's
difference X B - B is 2 alpha_j at coefficient 0 and 0 elsewhere (the mask is 0), so its balanced decomposition under
(pbs_l, pbs_logB) has one non-zero digit d = 2^s at one level `lev` - or none, where cbs_logB (j+1) > pbs_l pbs_logB -
and the step adds d K[i][lev][r=1][c] to column c of the accumulator.  With the key laid out [n][pbs_l][k+1][k+1][N]
and A = K[i][lev][1][0], the row the packing keyswitch decomposes is, k = 1,

    mask  d (A[0], -A[N-1], ..., -A[1])        body  d K[i][lev][1][1][0]        (the - alpha_j and + alpha_j cancel)

Where d = 1 - cbs_logB (j+1) == pbs_logB (lev+1) - every word of that row is a free choice, the body included: a
*targeted* level.  The other levels of the same input row are by-products: d times the key row of their own `lev`
(zero where the level has no digit), predicted exactly but not chosen.  The rows r = 0 of the key and the other
coefficients of K[i][lev][1][1] meet a zero polynomial / are not extracted: they may hold any words.

CPU only, Python integers and ks_edges.digits_of; nothing of the library.  tests/test_keyswitch_edges.py pins the
prediction to the CPU oracle's circuit bootstrap; tests/test_gpu_wop_programmed_rows.py runs it on the device."""
import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ks_edges as E  # noqa: E402

MOD = 1 << 64

# the fields of the WoP parameters the construction depends on (k = 1)
Shape = collections.namedtuple("Shape", "n N pbs_l pbs_logB cbs_l cbs_logB")


def shape_of(p):
    """From anything with the parameters as attributes (helm_wop_params through ctypes, for one)."""
    assert getattr(p, "k", 1) == 1
    return Shape(*(int(getattr(p, f)) for f in Shape._fields))


def level_digit(shape, j):
    """The one non-zero digit of 2 alpha_j under (pbs_l, pbs_logB): -> (lev, d), or None where the level has none."""
    assert 0 <= j < shape.cbs_l and shape.cbs_logB * (j + 1) <= 63
    digits = E.digits_of(1 << (64 - shape.cbs_logB * (j + 1)), shape.pbs_logB, shape.pbs_l, 64)
    hit = [(lev, d) for lev, d in enumerate(digits) if d]
    assert len(hit) <= 1, (shape, j, digits)
    return hit[0] if hit else None


def targeted_levels(shape):
    """The levels whose row is a free choice: d == 1."""
    return [j for j in range(shape.cbs_l) if (level_digit(shape, j) or (0, 0))[1] == 1]


def input_rows(shape):
    """-> [n][n + 1]: row i selects step i (one mask word at the rotation 1, the body -2^62)."""
    logN = shape.N.bit_length() - 1
    assert 1 << logN == shape.N
    rows = np.zeros((shape.n, shape.n + 1), dtype=np.uint64)
    for i in range(shape.n):
        rows[i, i] = 1 << (64 - (logN + 1))
        rows[i, shape.n] = MOD - (1 << 62)
    return rows


def program(shape, targets, seed=31):
    """targets: (step, level j, wanted row of N + 1 words).  -> (key [n][pbs_l][2][2][N] of uniform words with the wanted
    rows written in, input_rows(shape)).  Refuses (ValueError) a level without a digit and a key slot asked for twice;
    a target's digit must be 1."""
    n, N = shape.n, shape.N
    key = np.random.default_rng(seed).integers(0, MOD, size=(n, shape.pbs_l, 2, 2, N), dtype=np.uint64)
    taken = {}
    for step, j, row in targets:
        if not 0 <= step < n or len(row) != N + 1:
            raise ValueError("target (step %d, level %d): no such step, or a row that is not N + 1 words" % (step, j))
        hit = level_digit(shape, j)
        if hit is None:
            raise ValueError("level %d has no digit under pbs (%d, %d): cbs_logB (j+1) = %d exceeds %d bits" %
                             (j, shape.pbs_l, shape.pbs_logB, shape.cbs_logB * (j + 1), shape.pbs_l * shape.pbs_logB))
        lev, d = hit
        assert d == 1, "level %d is no target: its digit is %d (a row scaled by it keeps its extreme digits in part only)" % (j, d)
        if (step, lev) in taken:
            raise ValueError("step %d: levels %d and %d share the key row of decomposition level %d" % (step, taken[(step, lev)], j, lev))
        taken[(step, lev)] = j
        a = [int(row[0])] + [(-int(row[N - u])) % MOD for u in range(1, N)]       # row[m] = -A[N - m], m >= 1
        key[step, lev, 1, 0] = np.array(a, dtype=object).astype(np.uint64)
        key[step, lev, 1, 1, 0] = int(row[N])
    return key, input_rows(shape)


def predicted_rows(shape, key, steps):
    """The row the packing keyswitch reads for every (input row, level), from the key's words alone.
    steps: the step of each input row.  -> [len(steps)][cbs_l][N + 1]"""
    N = shape.N
    key = np.asarray(key).reshape(shape.n, shape.pbs_l, 2, 2, N)
    per_step = {}
    for i in sorted(set(int(s) for s in steps)):
        rows = np.zeros((shape.cbs_l, N + 1), dtype=np.uint64)
        for j in range(shape.cbs_l):
            hit = level_digit(shape, j)
            if hit is None:
                continue                                                         # acc unchanged: -alpha + alpha = 0
            lev, d = hit
            a = [int(v) for v in key[i, lev, 1, 0]]
            row = [d * a[0] % MOD] + [(-d * a[N - m]) % MOD for m in range(1, N)] + [d * int(key[i, lev, 1, 1, 0]) % MOD]
            rows[j] = np.array(row, dtype=object).astype(np.uint64)
        per_step[i] = rows
    return np.stack([per_step[int(s)] for s in steps])


def packing_reference(rows, key, l, logB):
    """The integer reference of the packing keyswitch for whole launches (every word of a row is decomposed, no body
    term): ks_edges.keyswitch_exact, in 8-bit limbs where the 16-bit ones would leave float64's exact range (logB 30).
    key: [k N + 1][l][(k+1) N]"""
    limb = 16 if key.shape[0] * l * (1 << (logB - 1)) * (1 << 16) < (1 << 53) else 8
    return E.keyswitch_exact(rows, key, logB, l, 64, body=False, limb=limb)


# ------------------------------------------------------------------------------------------------------------------
# the programmes the tests run
# ------------------------------------------------------------------------------------------------------------------
# (pfks_l, pfks_logB), as tests/test_gpu_keyswitch_edges.py lists them: the named set's; logB 2 at one and four levels; the
# padded level count 3 and the largest one at the widest digit with byte planes; logB 30 and rep 63, which have none
PFKS = [(2, 15), (1, 2), (4, 2), (3, 15), (4, 15), (1, 15), (2, 30), (1, 30), (3, 21)]

# (pbs_l, pbs_logB, cbs_l, cbs_logB) -> targeted levels.  Between them every level index of cbs_l = 2 and of cbs_l = 3 is a
# target: (2, 8 | 2, 8) levels 0 and 1 (lev = j); (2, 5 | 3, 5) levels 0 and 1, level 2 without a digit (15 > 10 bits);
# (2, 15 | 3, 5) level 2, levels 0 and 1 by-products (2^10 and 2^5 times the same key row, lev 0 for all three).
PROGRAMMES = {"l2": (2, 8, 2, 8), "l3_01": (2, 5, 3, 5), "l3_2": (2, 15, 3, 5)}
CONTROLS = 4                                                 # steps whose key rows stay uniform words


def crafted_programme(name, N, pfks_l, pfks_logB, seed=31):
    """n = 8 + CONTROLS steps: step i < 8 carries the crafted rows of ks_edges for (pfks_l, pfks_logB) - crafted row i at the
    first targeted level, crafted row (i + 3) mod 8 with another body at the second, where the programme has two - and the
    last CONTROLS steps uniform rows.  -> (shape, key, input rows, {(step, level): crafted row index})"""
    pbs_l, pbs_logB, cbs_l, cbs_logB = PROGRAMMES[name]
    nc = len(E.CRAFTED)
    shape = Shape(nc + CONTROLS, N, pbs_l, pbs_logB, cbs_l, cbs_logB)
    first = E.crafted_rows(N, pfks_logB, pfks_l, 64)
    second = E.crafted_rows(N, pfks_logB, pfks_l, 64, bodies=[(0xD1B54A32D192ED03 * (r + 1) | 1) % MOD for r in range(nc)])
    targets, where = [], {}
    for q, j in enumerate(targeted_levels(shape)):
        for i in range(nc):
            r = i if q == 0 else (i + 3) % nc
            targets.append((i, j, (first, second)[q][r]))
            where[(i, j)] = r
    key, rows = program(shape, targets, seed)
    return shape, key, rows, where


def steps_for(bits, cbs_l, levels, pinned=(0, 15, 16, 63, 64)):
    """The step of each of `bits` input rows.  The packing keyswitch sees row x = bit * cbs_l + level.  Two of every three
    bits take a crafted step (0..7, in turn), the third a control step; a bit that holds one of the `pinned` positions at
    a targeted level, or the first such position of the last 16-row tile, always takes a crafted step.
    -> (steps, the positions x that hold a crafted row)"""
    X = bits * cbs_l
    last_tile = [x for x in range((X - 1) // 16 * 16, X) if x % cbs_l in levels]
    want = {x for x in tuple(pinned) + tuple(last_tile[:1]) if x < X and x % cbs_l in levels}
    forced = {x // cbs_l for x in want}
    nc = len(E.CRAFTED)
    steps, a, b = [], 0, 0
    for t in range(bits):
        if t in forced or t % 3 != 2:
            steps.append(a % nc)
            a += 1
        else:
            steps.append(nc + b % CONTROLS)
            b += 1
    crafted = [t * cbs_l + j for t in range(bits) if steps[t] < nc for j in levels]
    assert want <= set(crafted)
    return np.array(steps), crafted


# ------------------------------------------------------------------------------------------------------------------
# the launch rules, restated (tests/test_keyswitch_edges.py pins them to the text of helm_wopbs.inc)
# ------------------------------------------------------------------------------------------------------------------
def pfpks_route(X, pfks_logB, N, mfma_env):
    """The kernels that serve the packing keyswitch of X bootstrap outputs (pfpks_on_matrix_cores): the matrix cores where
    the loader built byte planes (pfks_logB <= 15, (k+1) N a multiple of 16), HELM_HIP_KS_MFMA is not 0 and X >= 64."""
    return "mfma" if mfma_env != "0" and pfks_logB <= 15 and (2 * N) % 16 == 0 and X >= 64 else "valu"


def pfpks_slices(X, N, n_cus):
    """Slices of the input words of a k_pfpks64 launch (launch_pfpks, circuit_bootstrap_device): doubled while the grid
    ceil(X / 4) x ceil((k+1) N / 256) x slices is below two workgroups per compute unit, a slice keeps 64 words and there
    are fewer than 16.  1: the plain store; more: zeroed rows and atomic adds."""
    gx, gy, in_words = (X + 3) // 4, (2 * N + 255) // 256, N + 1
    slices = 1
    while slices < 16 and gx * gy * slices < 2 * n_cus and in_words // (slices * 2) >= 64:
        slices *= 2
    return slices


def gate_chunk(bits):
    """Gates per pass of helm_wop_eval_luts (the GGSW scratch of a pass is reused by the next)."""
    return max(1, 16384 // bits)
