"""Keyswitch inputs at the edges of the digit rule, of the key bytes and of the int32 plane accumulators, and a plain exact
reference for them.

The keyswitch is   out[c] = body [c == n] - sum_t sum_j d_j(in[t]) K[t][j][c]   mod 2^w.   It is linear in the key, so any
words are a valid key; the matrix-core kernels (k_ks_mfma, k_ks64_mfma, and the packing keyswitch on k_ks64_mfma) compute
it as   sum d K = sum_b 2^(8b) sum d (K_b - 128) + 0x80..80 sum d   with one int32 accumulator per byte plane b.  Random keys and
honest ciphertexts keep sum d near zero, the recentred bytes K_b - 128 uniform and the accumulators near their square-root
size; this module builds the rows and keys that do not:

  rows   every mask word the value whose digits have the largest sum (dsum_max), the smallest sum (dsum_min) and the
         largest sum of magnitudes (abs_max) the decomposition rule can produce - a digit of +-B/2 forces a smaller one
         above it, the constraint saturation.extreme_digits states - then rows of 0, 2^w - 1, 2^(w-1), 2^(w-1) - 1 and a row
         that walks every tie of the rule (each level's digit at B/2 with the level above below / at its own tie, the rounding
         tie of the cut-off bits, each one word either side).
  keys   every byte 0x00, 0xFF, 0x80, 0x7F (recentred: -128, +127, 0, -1), a key whose bytes follow the sign of the digit
         they multiply under the abs_max row (every plane accumulator of every column reaches sum |d| x 127..128, all terms of
         one sign) and uniform words.

No GPU and no project code: digits_of is tfhe's closest-representable balanced decomposition restated on Python integers
(NOT the kernels' one-addition recurrence; rep == w, where nothing is cut off, included), keyswitch_plain the double loop on
Python integers, keyswitch_exact the same sums in int64 limbs for whole launches (pinned to keyswitch_plain by
tests/test_keyswitch_edges.py).  The shape enumerators restate the admission rules of helm_hip_ctx_create,
helm_si_ctx_create_ex and helm_wop_ctx_create; vector_geometry restates the launch geometry of the vector-ALU form
(helm_ks::vector_geometry), and wide_cases lists the launches of tests/test_gpu_keyswitch_wide.py by the LDS band they are in.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import saturation as S  # noqa: E402


# ------------------------------------------------------------------------------------------------------------------
# the decomposition, restated
# ------------------------------------------------------------------------------------------------------------------
def closest_representable(x, logB, l, width):
    """x in Z_2^w -> the integer in [0, 2^rep) that names the closest multiple of 2^(w - rep), halves rounding up, wrapping
    at the top; rep == w: x itself (nothing is cut off, no rounding)."""
    rep = logB * l
    assert 1 <= rep <= width
    x = int(x) % (1 << width)
    if rep == width:
        return x
    q = 1 << (width - rep)
    return ((2 * x + q) // (2 * q)) % (1 << rep)


def digits_of(x, logB, l, width):
    """Signed digits of x, first = most significant level: the closest representable value, cut into base-B digits from the
    least significant one; a digit above B/2, or equal to B/2 when the digit above it (as it stands, before any carry into
    it) is at least B/2, becomes digit - B and carries one into the level above; the carry out of the top level is dropped."""
    B, h = 1 << logB, 1 << (logB - 1)
    state = closest_representable(x, logB, l, width)
    out = [0] * l
    for lev in range(l - 1, -1, -1):
        d, state = state % B, state // B
        if d > h or (d == h and state % B >= h):
            d -= B
            state += 1
        out[lev] = d
    return out


def digits_rows(words, logB, l, width):
    """digits_of over an array of words -> int64 [..., l] (pinned to digits_of by tests/test_keyswitch_edges.py).  The
    rounding is (x >> cut) + (bit cut-1 of x), which cannot overflow at any rep."""
    x = np.asarray(words).astype(np.uint64)
    rep = logB * l
    B, h = np.uint64(1 << logB), np.uint64(1 << (logB - 1))
    if rep == width:
        state = x.copy()
    else:
        cut = np.uint64(width - rep)
        state = ((x >> cut) + ((x >> (cut - np.uint64(1))) & np.uint64(1))) & np.uint64((1 << rep) - 1)
    out = np.zeros(x.shape + (l,), dtype=np.int64)
    for lev in range(l - 1, -1, -1):
        d = state & (B - np.uint64(1))
        state = state >> np.uint64(logB)
        carry = (d > h) | ((d == h) & ((state & (B - np.uint64(1))) >= h))
        out[..., lev] = d.astype(np.int64) - (carry.astype(np.int64) << logB)
        state = state + carry.astype(np.uint64)
    return out


def extreme_digits_by(logB, l, score):
    """The digit string the rule can produce with the largest sum of score(d): dynamic programming over the levels under the
    constraint saturation.extreme_digits states (a digit of +B/2 has a next more significant digit in [0, B/2 - 1], a digit
    of -B/2 one in [-B/2 + 1, 0], the top level is never -B/2).  -> (digits, most significant first; the score reached)."""
    h = (1 << logB) // 2
    cand = sorted({h, -h, h - 1, 1 - h, 0})
    ok = {"free": lambda d: True, "nonneg": lambda d: 0 <= d <= h - 1, "nonpos": lambda d: 1 - h <= d <= 0}
    best = {"free": (0, [])}
    for lev in range(l - 1, -1, -1):
        nxt = {}
        for demand, (tot, seq) in best.items():
            for d in cand:
                if not ok[demand](d) or (lev == 0 and d == -h):
                    continue
                out = "nonneg" if d == h else "nonpos" if d == -h else "free"
                v = (tot + score(d), seq + [d])
                if out not in nxt or v[0] > nxt[out][0]:
                    nxt[out] = v
        best = nxt
    tot, seq = max(best.values(), key=lambda v: v[0])
    return seq[::-1], tot


def word_of(seq, logB, width):
    """The torus word whose digits are seq (checked through digits_of)."""
    x = sum(d << (width - logB * (j + 1)) for j, d in enumerate(seq)) % (1 << width)
    assert digits_of(x, logB, len(seq), width) == list(seq), (seq, digits_of(x, logB, len(seq), width))
    return x


def extreme_words(logB, l, width):
    """-> dict name -> (word, digits): dsum_max, dsum_min, abs_max (the last one is saturation.extreme_value's)."""
    hi, _ = extreme_digits_by(logB, l, lambda d: d)
    lo, _ = extreme_digits_by(logB, l, lambda d: -d)
    x, seq, tot = S.extreme_value(logB, l, width)
    assert digits_of(x, logB, l, width) == seq and sum(abs(d) for d in seq) == tot
    return {"dsum_max": (word_of(hi, logB, width), hi), "dsum_min": (word_of(lo, logB, width), lo), "abs_max": (x, seq)}


def tie_words(logB, l, width):
    """Words at and one either side of every tie of the rule: per level, the digit at B/2 with the level above just below
    and at its own tie; the rounding tie of the cut-off bits; the wrap at the top; for digits wider than a byte, the values
    whose low byte is -128 / +127 under the largest high byte of either sign."""
    mod, rep, h = 1 << width, logB * l, 1 << (logB - 1)
    unit = 1 << (width - rep)                                # weight of the least significant level
    out = set()
    for lev in range(l):
        w = 1 << (width - logB * (lev + 1))                  # weight of level lev
        for above in (0, h - 1, h):                          # the digit above: clear, just below the tie bit, at it
            base = h * w + (above * w << logB if lev > 0 else 0)
            for delta in (-unit, -1, 0, 1, unit):
                out.add((base + delta) % mod)
        if logB >= 9:                                        # the packing keyswitch's byte split d = 256 hi + lo at its ends:
            for d in (h - 128, 127 - h, 127, -128, 128):     # (hi, lo) = (+max, -128), (-max, +127), (0, 127), (0, -128), (1, -128)
                out.add(d * w % mod)
    if rep < width:
        half = unit >> 1                                     # the cut-off bits at exactly one half
        for k in (0, 1, h, (1 << rep) - 1):
            for delta in (-1, 0, 1):
                out.add((k * unit + half + delta) % mod)
    for delta in range(-2, 3):
        out.add(delta % mod)
        out.add(((mod >> 1) + delta) % mod)
    return sorted(out)


CRAFTED = ("dsum_max", "dsum_min", "abs_max", "zero", "ones", "half", "half_m1", "ties")


def dtype_of(width):
    return np.uint32 if width == 32 else np.uint64


def crafted_rows(in_dim, logB, l, width, bodies=None):
    """-> [len(CRAFTED), in_dim + 1] words: the mask words as the module docstring lists them, the body word of row r an odd
    constant (so that a dropped or doubled body shows)."""
    ext = extreme_words(logB, l, width)
    mod = 1 << width
    ties = tie_words(logB, l, width)
    fill = {"dsum_max": ext["dsum_max"][0], "dsum_min": ext["dsum_min"][0], "abs_max": ext["abs_max"][0], "zero": 0,
            "ones": mod - 1, "half": mod >> 1, "half_m1": (mod >> 1) - 1}
    rows = np.zeros((len(CRAFTED), in_dim + 1), dtype=dtype_of(width))
    for r, name in enumerate(CRAFTED):
        if name == "ties":
            rows[r, :in_dim] = np.array([ties[t % len(ties)] for t in range(in_dim)], dtype=object).astype(dtype_of(width))
        else:
            rows[r, :in_dim] = fill[name]
        rows[r, in_dim] = (0x9E3779B97F4A7C15 * (r + 1) | 1) % mod if bodies is None else bodies[r]
    return rows


def launch_rows(in_dim, logB, l, width, count, seed=5):
    """count rows: the crafted rows first (repeated with the bodies changed while count allows, so that wide launches hold
    them in every 64-row tile position), uniform control rows at the positions in the returned list.
    -> (rows [count, in_dim + 1], indices of the control rows)"""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 1 << width, size=(count, in_dim + 1), dtype=dtype_of(width))
    c = crafted_rows(in_dim, logB, l, width)
    nc = len(c)
    controls = []
    for g in range(count):
        # of every 12 rows, 8 crafted and 4 controls; a launch narrower than that keeps what fits, crafted first
        if g % 12 < nc:
            rows[g, :in_dim] = c[g % 12, :in_dim]
            rows[g, in_dim] = (int(c[g % 12, in_dim]) + 2 * (g // 12)) % (1 << width)
        else:
            controls.append(g)
    return rows, controls


# ------------------------------------------------------------------------------------------------------------------
# keys
# ------------------------------------------------------------------------------------------------------------------
KEYS = ("00", "ff", "80", "7f", "follow", "random")


def make_key(kind, in_dim, out_words, logB, l, width, seed=23):
    """[in_dim][l][out_words] words.  "follow": every byte 0xFF where the digit of the abs_max row at that level is positive
    and 0x00 where it is negative or zero - the recentred bytes +127 / -128 then have the digit's sign in every plane."""
    dt = dtype_of(width)
    ones = (1 << width) - 1
    if kind in ("00", "ff", "80", "7f"):
        byte = int(kind, 16)
        return np.full((in_dim, l, out_words), sum(byte << (8 * b) for b in range(width // 8)), dtype=dt)
    if kind == "follow":
        _, seq = extreme_words(logB, l, width)["abs_max"]
        key = np.zeros((in_dim, l, out_words), dtype=dt)
        for j, d in enumerate(seq):
            key[:, j, :] = ones if d > 0 else 0
        return key
    assert kind == "random"
    return np.random.default_rng(seed).integers(0, 1 << width, size=(in_dim, l, out_words), dtype=dt)


# ------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------
def keyswitch_plain(row, key, logB, l, width, body=True):
    """One row, Python integers only.  body=True: the keyswitch (in_dim mask words + a body that lands in the last
    column); body=False: the packing keyswitch (every word of the row is decomposed, no body term).  -> list of words"""
    key = np.asarray(key)
    in_dim, _, out_words = key.shape
    mod = 1 << width
    acc = [0] * out_words
    for t in range(in_dim):
        for j, d in enumerate(digits_of(row[t], logB, l, width)):
            if d:
                kr = key[t, j]
                for c in range(out_words):
                    acc[c] += d * int(kr[c])
    out = [(-a) % mod for a in acc]
    if body:
        out[out_words - 1] = (int(row[in_dim]) - acc[out_words - 1]) % mod
    return out


def keyswitch_exact(rows, key, logB, l, width, body=True, limb=16):
    """Whole launches: the same sums with the key cut into 16-bit limbs, so that every partial sum (|digit| <= 2^(logB-1),
    limb < 2^16, in_dim x l terms) stays below 2^53 and is exact as a float64 matrix product; the limbs are recombined
    mod 2^w in unsigned wrapping arithmetic.  limb=8: narrower limbs, for the packing keyswitch's digits of up to 30 bits.
    -> [rows, out_words] words"""
    key = np.asarray(key)
    in_dim = key.shape[0]
    rows = np.asarray(rows)
    D = digits_rows(rows[:, :in_dim], logB, l, width).reshape(len(rows), in_dim * l).astype(np.float64)
    return _exact_from_digits(D, rows, key, logB, l, width, body, limb)


def _exact_from_digits(D, rows, key, logB, l, width, body, limb):
    """keyswitch_exact's sums from the float64 digit matrix D [rows, in_dim * l]."""
    in_dim, _, out_words = key.shape
    assert limb in (8, 16) and in_dim * l * (1 << (logB - 1)) * (1 << limb) < (1 << 53)
    K = key.reshape(in_dim * l, out_words).astype(np.uint64)
    total = np.zeros((len(rows), out_words), dtype=np.uint64)
    for i in range(width // limb):
        piece = ((K >> np.uint64(limb * i)) & np.uint64((1 << limb) - 1)).astype(np.float64)
        part = (D @ piece).astype(np.int64)                                                  # exact: see the assert
        total += part.astype(np.uint64) << np.uint64(limb * i)                               # two's complement, wrapping
    out = np.uint64(0) - total
    if body:
        out[:, out_words - 1] += rows[:, in_dim].astype(np.uint64)
    if width == 32:
        return (out & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return out


def keyswitch_exact_wide(rows, keys, logB, l, width, chunk=256):
    """keyswitch_exact of a wide launch under several keys: the digit matrix is rows x in_dim x l float64 (0.5 MiB a row at
    in_dim 8192, l = 8), so the rows go through in chunks of at most `chunk`, each decomposed once for all keys.
    keys: dict name -> key.  -> dict name -> [rows, out_words] words"""
    assert 1 <= chunk <= 256
    rows = np.asarray(rows)
    keys = {name: np.asarray(key) for name, key in keys.items()}
    in_dim = next(iter(keys.values())).shape[0]
    parts = {name: [] for name in keys}
    for a in range(0, len(rows), chunk):
        part = rows[a:a + chunk]
        D = digits_rows(part[:, :in_dim], logB, l, width).reshape(len(part), in_dim * l).astype(np.float64)
        for name, key in keys.items():
            parts[name].append(_exact_from_digits(D, part, key, logB, l, width, True, 16))
    return {name: np.concatenate(p) for name, p in parts.items()}


def plane_accumulators(row, key, logB, l, width, split_bytes=False):
    """The exact int32-plane sums the matrix-core kernels form for one row: acc[b][c] = sum_r d_r (K_b[r][c] - 128) over the
    rows r = (t, level) of the key, and dsum = sum_r d_r.  split_bytes: the packing keyswitch's virtual rows - the digit
    d = 256 hi + lo (lo in [-128, 127]) against the key words K << 8 (for hi) and K (for lo).
    -> (acc [w/8, out_words] of Python-exact int64, dsum, sum |d| over the virtual rows)"""
    key = np.asarray(key)
    in_dim, _, out_words = key.shape
    D = digits_rows(np.asarray(row)[:in_dim], logB, l, width).reshape(in_dim * l)
    K = key.reshape(in_dim * l, out_words).astype(np.uint64)
    if split_bytes:
        lo = ((D + 128) & 255) - 128
        hi = (D - lo) >> 8
        assert np.abs(hi).max(initial=0) <= 64 and np.array_equal(256 * hi + lo, D)
        D = np.stack([hi, lo], axis=1).reshape(-1)
        K = np.stack([K << np.uint64(8), K], axis=1).reshape(2 * in_dim * l, out_words)
    acc = np.stack([D @ (((K >> np.uint64(8 * b)) & np.uint64(255)).astype(np.int64) - 128) for b in range(width // 8)])
    return acc, int(D.sum()), int(np.abs(D).sum())


def recombine_planes(acc, dsum, width):
    """What the kernels do with the plane sums: sum_b acc_b 2^(8b) + 0x80..80 dsum mod 2^w (= sum d K)."""
    mod = 1 << width
    corr = sum(0x80 << (8 * b) for b in range(width // 8))
    return [(sum(int(acc[b][c]) << (8 * b) for b in range(len(acc))) + corr * dsum) % mod for c in range(acc.shape[1])]


# ------------------------------------------------------------------------------------------------------------------
# admitted shapes (restated from the ctx_create functions; tests/test_keyswitch_edges.py pins the messages' numbers)
# ------------------------------------------------------------------------------------------------------------------
def ks_shapes(width):
    """Every admitted (ks_l, ks_logB): helm_hip_ctx_create asks ks_logB in 1..7, ks_l in {1..6, 8}, ks_l ks_logB <= 32;
    helm_si_ctx_create_ex ks_logB in 1..7, ks_l in 1..8, ks_l ks_logB <= 63."""
    ls = (1, 2, 3, 4, 5, 6, 8) if width == 32 else range(1, 9)
    return [(l, b) for l in ls for b in range(1, 8) if l * b <= (32 if width == 32 else 63)]


def pfks_shapes(matrix_cores=None):
    """Every admitted (pfks_l, pfks_logB) of helm_wop_ctx_create: pfks_l in 1..4, pfks_logB in 2..30, product <= 63.
    matrix_cores=True: those the loader builds byte planes for (pfks_logB <= 15: the high byte of a digit fits [-64, 64])."""
    out = [(l, b) for l in range(1, 5) for b in range(2, 31) if l * b <= 63]
    if matrix_cores is None:
        return out
    return [s for s in out if (s[1] <= 15) == matrix_cores]


def max_in_dim(width, large=False, n8192=False):
    """The largest k N a context admits.  32-bit: (k+1) N <= 8192 (pbs_admitted), N >= 256: 7936.  64-bit: (k+1) N <= 4096
    (si_generic_domain): 3840; with the large-N bit k = 1, N = 4096 as well (si_large_domain): 4096; with the N = 8192 bit
    k = 1, N = 8192 (si_n8192_domain): 8192."""
    if width == 32:
        return 8192 - 256
    return 8192 if n8192 else 4096 if large else 4096 - 256


def in_dims(width):
    """Every k N some admitted context has, as far as the keyswitch geometry can tell them apart: multiples of 256 up to
    max_in_dim, and on the 64-bit engine the two sizes the large-N and the N = 8192 bit add."""
    if width == 32:
        return list(range(256, max_in_dim(32) + 1, 256))
    return list(range(256, max_in_dim(64) + 1, 256)) + [LARGE_IN_DIM, N8192_IN_DIM]


MIN_IN_DIM = 256
LARGE_IN_DIM = 4096                                          # k = 1, N = 4096: SiServerKey(generic="large")
N8192_IN_DIM = 8192                                          # k = 1, N = 8192: SiServerKey(generic="n8192")
MAX_N = 1024                                                 # n must be in [1, 1024], both engines
WOP_MAX_IN_WORDS = 2048 + 1                                  # k = 1, N <= 2048, body word included


# ------------------------------------------------------------------------------------------------------------------
# the launch geometry of the vector-ALU form (helm_ks::vector_geometry, restated; tests/test_ks_geometry.py pins the
# three deciding lines of the source)
# ------------------------------------------------------------------------------------------------------------------
LDS_DEFAULT = 64 * 1024                                      # dynamic LDS a kernel may ask for without an attribute
LDS_LIMIT = 160 * 1024                                       # LDS of a gfx950 workgroup; the attribute the engines set
BANDS = ("default", "raised", "limit", "clause")


def grid_slices(count, n, kN, n_cus):
    """The grid clause alone: double the slices while fewer than two workgroups per CU exist, up to 16, each slice at
    least 64 input words.  -> (gx, gy, slices)"""
    gx, gy = (count + 3) // 4, (n + 1 + 255) // 256
    slices = 1
    while slices < 16 and gx * gy * slices < 2 * n_cus and kN // (slices * 2) >= 64:
        slices *= 2
    return gx, gy, slices


def vector_geometry(count, n, kN, ks_l, n_cus):
    """helm_ks::vector_geometry: the grid clause, then the LDS clause (double the slices while one slice's digits,
    ceil(kN / slices) x ks_l x 4 B, exceed 160 KiB).  -> (gx, gy, slices, t_chunk, lds)"""
    gx, gy, slices = grid_slices(count, n, kN, n_cus)
    while (kN + slices - 1) // slices * ks_l * 4 > LDS_LIMIT:
        slices *= 2
    t_chunk = (kN + slices - 1) // slices
    return gx, gy, slices, t_chunk, t_chunk * ks_l * 4


def lds_band(count, n, kN, ks_l, n_cus):
    """Where a launch stands against the two LDS limits, and which clause decided its slices.
    -> (band, clause): band "default" (lds <= 64 KiB: launches without an attribute), "raised" (64 KiB < lds < 160 KiB),
    "limit" (lds == 160 KiB exactly), each with clause "grid"; or "clause" (the grid clause alone would ask for more than
    160 KiB: the LDS clause slices further), with clause "lds"."""
    _, _, s_grid = grid_slices(count, n, kN, n_cus)
    _, _, slices, _, lds = vector_geometry(count, n, kN, ks_l, n_cus)
    if slices != s_grid:
        return "clause", "lds"
    return ("default" if lds <= LDS_DEFAULT else "raised" if lds < LDS_LIMIT else "limit"), "grid"


def width_for_slices(slices, n, kN, n_cus):
    """A batch width at which the grid clause gives `slices` in {16, 4, 2, 1} - 40 rows, 2 CUs + 4, 4 CUs + 4, 8 CUs + 4 at
    gy = 1, and as many workgroups at gy > 1 (16 slices: fewer than 40 rows where 40 have a quarter of a workgroup per CU
    already) - checked against grid_slices."""
    gy = (n + 1 + 255) // 256
    count = {16: min(40, 4 * ((2 * n_cus - 1) // (8 * gy))), 4: (2 * n_cus) // gy + 4, 2: (4 * n_cus) // gy + 4, 1: (8 * n_cus + gy - 1) // gy + 4}[slices]
    assert grid_slices(count, n, kN, n_cus)[2] == slices, (count, n, kN, n_cus, slices)
    return count


SWEEP = 165                                                  # tests/test_gpu_keyswitch_edges.py's width: 16 slices, mfma on the 64-bit engine


class WideCase:
    """One case of tests/test_gpu_keyswitch_wide.py: a context shape, the slice counts its launches are built for (the
    batch widths follow from the CU count), and per launch what the vector-ALU form is expected to be: (band, clause) of
    lds_band.  mfma0_only: the vector-ALU form serves these widths only under HELM_HIP_KS_MFMA=0 (the unset run takes the
    matrix cores; the two are compared all the same)."""

    def __init__(self, width, n, k, N, l, logB, slices, expect, generic=None, kinds=("random", "follow"), mfma0_only=False):
        self.width, self.n, self.k, self.N, self.l, self.logB = width, n, k, N, l, logB
        self.slices, self.expect, self.generic, self.kinds, self.mfma0_only = slices, expect, generic, kinds, mfma0_only
        self.kN = k * N

    def counts(self, n_cus):
        return [SWEEP if s == "sweep" else width_for_slices(s, self.n, self.kN, n_cus) for s in self.slices]

    def geometry(self, n_cus):
        return [vector_geometry(c, self.n, self.kN, self.l, n_cus) for c in self.counts(n_cus)]

    def bands(self, n_cus):
        return [lds_band(c, self.n, self.kN, self.l, n_cus) for c in self.counts(n_cus)]

    @property
    def id(self):
        return "w%d-n%d-k%dN%d-l%dB%d-s%s" % (self.width, self.n, self.k, self.N, self.l, self.logB,
                                               "x".join(str(s) for s in self.slices))


G, L = "grid", "lds"


def wide_cases():
    """The cases of tests/test_gpu_keyswitch_wide.py.  The uniform key goes first: under the sign-following key an even
    level count can leave all-zero rows behind, which would hide a sliced launch whose rows were not cleared."""
    k32 = dict(width=32, n=46, k=31, N=256)                   # k N = 7936, the largest of the 32-bit engine
    cases = [
        # 32-bit, ks_l = 3 (vector-ALU form only): 95,232 B unsliced
        WideCase(l=3, logB=7, slices=(16, 2, 1), expect=[("default", G), ("default", G), ("raised", G)], **k32),
        # ks_l = 8 on the vector-ALU form: 253,952 B unsliced - the LDS clause makes it 2 x 126,976 B; 4 slices: 63,488 B
        WideCase(l=8, logB=4, slices=(4, 1), expect=[("default", G), ("clause", L)], mfma0_only=True, **k32),
        # ks_l = 5: 158,720 B unsliced, 5 KiB under the limit
        WideCase(l=5, logB=6, slices=(1,), expect=[("raised", G)], **k32),
        # a second column chunk (gy = 2) under a raised launch
        WideCase(32, 300, 31, 256, 3, 7, slices=(1,), expect=[("raised", G)]),
        # k N = 5120, ks_l = 8: exactly 160 KiB on the 32-bit engine
        WideCase(32, 46, 20, 256, 8, 4, slices=(1,), expect=[("limit", G)], mfma0_only=True),
    ]
    # 64-bit: the ends of the decomposition at the two new sizes, all six keys, the crafted construction at SWEEP rows
    for N, generic in ((LARGE_IN_DIM, "large"), (N8192_IN_DIM, "n8192")):
        for l in (1, 8):
            for logB in (1, 7):
                cases.append(WideCase(64, 46, 1, N, l, logB, slices=("sweep",), expect=[("default", G)], generic=generic,
                                      kinds=KEYS, mfma0_only=True))
    cases += [
        # in_dim 4096, ks_l = 8: 32 KiB, exactly 64 KiB and 128 KiB at 4, 2 and 1 slices
        WideCase(64, 46, 1, LARGE_IN_DIM, 8, 7, slices=(4, 2, 1), expect=[("default", G), ("default", G), ("raised", G)],
                 generic="large", mfma0_only=True),
        # in_dim 8192, ks_l = 5: exactly 163,840 B, unsliced
        WideCase(64, 46, 1, N8192_IN_DIM, 5, 7, slices=(1,), expect=[("limit", G)], generic="n8192", mfma0_only=True),
        # in_dim 8192, ks_l = 6: 196,608 B unsliced - the LDS clause makes it 2 x 98,304 B
        WideCase(64, 46, 1, N8192_IN_DIM, 6, 7, slices=(1,), expect=[("clause", L)], generic="n8192", mfma0_only=True),
    ]
    return cases


# Keyswitch-first gate levels (GateKsRows) in the raised band: (k, N, n, ks_l, ks_logB); k N x ks_l x 4 B = 73,728 and 102,400
GATE_SHAPES = [(6, 1024, 16, 3, 7), (5, 1024, 16, 5, 4)]


def padded_levels(l):
    """The 64-bit matrix-core path pads the level count to 1, 2, 4 or 8 bytes per input word."""
    return 1 if l <= 1 else 2 if l <= 2 else 4 if l <= 4 else 8


def plane_bound(in_dim, l, logB):
    """rows x 2^(logB-1) x 128: what no int32 plane accumulator of the keyswitch can exceed in magnitude."""
    return in_dim * l * (1 << (logB - 1)) * 128


def pfks_plane_bound(in_words, l, logB):
    """The packing keyswitch's two-byte split d = 256 hi + lo: per (word, level) a high byte of magnitude <= 2^(logB-9)
    (1 at logB = 8 and 9: the digit +128 is 256 - 128; none below) and a low byte of magnitude <= min(2^(logB-1), 128),
    two virtual key rows, each against a recentred byte of magnitude <= 128."""
    hi = 0 if logB < 8 else max(1, (1 << (logB - 1)) >> 8)
    lo = min(1 << (logB - 1), 128)
    return in_words * l * (hi + lo) * 128


def reach_fraction(l, logB):
    """The fraction of plane_bound the abs_max row under the "follow" key reaches, from the closed forms: sum |d| per word is
    l B/2 - floor(l/2) (saturation.extreme_digits), and the recentred byte is +127 under the positive digits, -128 under
    the others.  A lower bound (all bytes taken as 127); the least over the admitted shapes is logB = 1, l = 2: 0.496."""
    h = 1 << (logB - 1)
    return (l * h - l // 2) * 127 / (l * h * 128)
