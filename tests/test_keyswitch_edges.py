"""tests/ks_edges.py pinned on the CPU: its decomposition against an independent statement and against brute force, its
reference against the double loop and against the three oracles (ks_l * ks_logB == 32 and == 63 included), the byte-plane
identity of the matrix-core kernels from exact integers, and the int32 bound of every plane accumulator for every shape a
context admits, with the fraction of it the crafted rows reach.

Reach, from exact integers: under the "follow" key the abs_max row drives every plane accumulator of every column to
sum |d| x 127..128 with sum |d| = in_dim (l B/2 - floor(l/2)): at least  (l B/2 - floor(l/2)) 127 / (l B/2 128)  of
rows x B/2 x 128 - 0.984 at logB = 7, 0.93 at logB = 4 with l = 8, and 0.496 at its least (logB = 1, l = 2, where the tie rule
allows one of two neighbouring digits to be non-zero).  The dsum extremes reach in_dim (l B/2 - floor(l/2)) and its
negative less at most one unit per word."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ks_edges as E  # noqa: E402
import saturation as S  # noqa: E402
import wop_program as W  # noqa: E402

ALL_SHAPES = [(32, l, b) for l, b in E.ks_shapes(32)] + [(64, l, b) for l, b in E.ks_shapes(64)]


def test_the_shape_enumerators_are_the_admission_rules_of_the_sources():
    """The numbers of ks_shapes / pfks_shapes / max_in_dim, read back from the checks in the three ctx_create functions.
    A tripwire on the source text, nothing more: it asks whoever edits an admission check to look at ks_edges' enumerators
    (a reformatted condition trips it too - update the strings).  The behaviour at the boundaries is pinned on the device,
    by the refusal tests of tests/test_gpu_keyswitch_edges.py."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hip = open(os.path.join(root, "helm_amd", "csrc", "helm_hip.hip")).read()
    si = open(os.path.join(root, "helm_amd", "csrc", "helm_shortint.hip")).read()
    wop = open(os.path.join(root, "helm_amd", "csrc", "helm_wopbs.inc")).read()
    assert "P.ks_logB < 1 || P.ks_logB > 7 || P.ks_logB * P.ks_l > 32 ||" in hip
    assert "!(P.ks_l >= 1 && (P.ks_l <= 6 || P.ks_l == 8))" in hip
    assert "P.ks_logB < 1 || P.ks_logB > 7 || P.ks_l < 1 || P.ks_l > 8 || P.ks_logB * P.ks_l > 63" in si
    assert "P.pfks_l < 1 || P.pfks_l > 4 || P.pfks_logB < 2 || P.pfks_logB > 30 || P.pfks_logB * P.pfks_l > 63" in wop
    assert "if (P.pfks_logB <= 15 && glwe_words % 16 == 0)" in wop          # the loader's byte planes: hi fits [-64, 64]
    assert hip.count("if (P.n < 1 || P.n > 1024)") == 1 and si.count("if (P.n < 1 || P.n > 1024)") == 1
    assert "(k+1) N <= 8192" in hip and "(k+1) N <= 4096" in si
    assert "pbs_side->P.k != 1 || P.k != 1" in wop
    s32, s64 = E.ks_shapes(32), E.ks_shapes(64)
    assert (8, 4) in s32 and (8, 5) not in s32 and (7, 1) not in s32 and (6, 5) in s32 and (6, 6) not in s32
    assert max(l * b for l, b in s32) == 32 and max(l * b for l, b in s64) == 56 and len(s64) == 56
    assert (3, 21) in E.pfks_shapes() and (4, 15) in E.pfks_shapes(True) and (4, 16) not in E.pfks_shapes()
    assert (2, 30) in E.pfks_shapes(False) and (2, 31) not in E.pfks_shapes()


@pytest.mark.parametrize("width,l,logB", ALL_SHAPES + [(64, l, b) for l, b in E.pfks_shapes()[::7]] + [(64, 9, 7), (64, 3, 21), (64, 1, 63)])
def test_digits_three_statements_agree(width, l, logB):
    """digits_of (round, cut, balance), digits_rows (its array form) and saturation.digits (the oracle's recurrence on
    Python integers) on the crafted words, the ties and random words; the digits recompose to the closest representable
    value and stay within [-B/2, B/2]."""
    rng = np.random.default_rng(width + 10 * l + logB)
    ext = E.extreme_words(logB, l, width)
    words = [w for w, _ in ext.values()] + E.tie_words(logB, l, width) + \
        [0, (1 << width) - 1, 1 << (width - 1), (1 << (width - 1)) - 1] + \
        [int(v) for v in rng.integers(0, 1 << width, size=300, dtype=np.uint64 if width == 64 else np.uint32)]
    arr = E.digits_rows(np.array(words, dtype=object).astype(E.dtype_of(width)), logB, l, width)
    rep, h = logB * l, 1 << (logB - 1)
    for i, x in enumerate(words):
        d = E.digits_of(x, logB, l, width)
        assert d == S.digits(x, logB, l, width) == [int(v) for v in arr[i]], (hex(x), d)
        assert max(abs(v) for v in d) <= h
        value = sum(v << (width - logB * (j + 1)) for j, v in enumerate(d)) % (1 << width)
        assert value == (E.closest_representable(x, logB, l, width) << (width - rep)) % (1 << width)
        if rep == width:
            assert value == x


@pytest.mark.parametrize("l,logB", [(1, 1), (2, 1), (3, 1), (8, 1), (1, 3), (2, 3), (3, 3), (4, 3), (2, 4), (3, 4), (2, 6), (1, 7)])
def test_the_extreme_rows_are_extreme_by_brute_force(l, logB):
    """Every word of a torus exactly as wide as the representable part (rep == w) and of one with cut-off bits: the
    largest and smallest digit sums and the largest sum of magnitudes are what the dynamic programme builds."""
    rep = l * logB
    for width in (rep, rep + 2):
        sums = [E.digits_of(x, logB, l, width) for x in range(1 << width)]
        hi, hi_v = E.extreme_digits_by(logB, l, lambda d: d)
        lo, lo_v = E.extreme_digits_by(logB, l, lambda d: -d)
        _, ab_v = S.extreme_digits(logB, l)
        assert max(sum(d) for d in sums) == hi_v == sum(hi)
        assert min(sum(d) for d in sums) == -lo_v == sum(lo)
        assert max(sum(abs(v) for v in d) for d in sums) == ab_v == l * (1 << (logB - 1)) - l // 2


@pytest.mark.parametrize("width,l,logB", ALL_SHAPES)
def test_the_peaks_the_construction_reaches(width, l, logB):
    """Pinned from exact integers, per admitted shape: sum |d|, dsum at both ends, and every int32 plane accumulator of the
    abs_max row under the "follow" key - against rows x B/2 x 128, the bound nothing can exceed, and the fraction of it that
    reach_fraction states (module docstring)."""
    in_dim, out_words, h = 64, 3, 1 << (logB - 1)
    rows = E.crafted_rows(in_dim, logB, l, width)
    peak = l * h - l // 2
    d = E.digits_rows(rows[:, :in_dim], logB, l, width)
    by_name = {name: d[r] for r, name in enumerate(E.CRAFTED)}
    assert int(np.abs(by_name["abs_max"]).sum()) == in_dim * peak
    assert int(by_name["dsum_max"].sum()) == in_dim * peak                       # all digits >= 0: the same peak
    assert -in_dim * peak <= int(by_name["dsum_min"].sum()) <= -in_dim * (peak - 1)   # the top level cannot be -B/2
    assert int(by_name["zero"].sum()) == 0 and not by_name["zero"].any()
    if logB == 7:
        assert d.max() == 64 and d.min() == (-64 if l >= 2 else -63)                # the int8 extremes (the top level is never -B/2)
    bound = E.plane_bound(in_dim, l, logB)
    key = E.make_key("follow", in_dim, out_words, logB, l, width)
    acc, dsum, dabs = E.plane_accumulators(rows[E.CRAFTED.index("abs_max")], key, logB, l, width)
    assert dabs == in_dim * peak and np.abs(acc).max() <= bound
    assert np.abs(acc).min() >= E.reach_fraction(l, logB) * bound               # EVERY plane of every column
    assert E.reach_fraction(l, logB) >= 0.496 and (logB < 7 or E.reach_fraction(l, logB) >= 0.984)
    # the whole-byte keys: -128 x dsum at its two ends, +127 x dsum, 0 and -dsum
    for kind, byte in (("00", -128), ("ff", 127), ("80", 0), ("7f", -1)):
        k = E.make_key(kind, in_dim, out_words, logB, l, width)
        for name in ("dsum_max", "dsum_min"):
            acc, dsum, _ = E.plane_accumulators(rows[E.CRAFTED.index(name)], k, logB, l, width)
            assert (acc == byte * dsum).all() and abs(dsum) >= in_dim * (peak - 1)


def test_every_admitted_shape_keeps_the_plane_accumulators_inside_int32():
    """rows x 2^(logB-1) x 128 < 2^31 at the largest k N either engine admits, for every admitted decomposition (the 64-bit
    kernel widens and shifts these sums: a wrap there would not cancel mod 2^64); the packing keyswitch with its two
    virtual rows per level at the largest input (k = 1, N = 2048, the body word included)."""
    worst = {}
    for width in (32, 64):
        for l, b in E.ks_shapes(width):
            if width == 32 and l not in (1, 2, 4, 8):
                continue                                                         # no byte planes: vector kernel only
            bound = E.plane_bound(E.max_in_dim(width), l, b)
            assert bound < 1 << 31, (width, l, b, bound)
            worst[width] = max(worst.get(width, 0), bound)
    assert worst[32] == 7936 * 4 * 64 * 128 and worst[64] == 3840 * 8 * 64 * 128   # 0.121 and 0.117 of 2^31
    pf = 0
    for l, b in E.pfks_shapes(True):
        bound = E.pfks_plane_bound(E.WOP_MAX_IN_WORDS, l, b)
        assert bound < 1 << 31, (l, b, bound)
        pf = max(pf, bound)
    assert pf == 2049 * 4 * (64 + 128) * 128                                     # (4, 15): 0.094 of 2^31


@pytest.mark.parametrize("l,logB", [(2, 15), (4, 15), (1, 15), (3, 9), (4, 8), (4, 2)])
def test_the_packing_keyswitch_split_reaches_its_bytes(l, logB):
    """d = 256 hi + lo on the crafted rows: hi reaches +-2^(logB-9) (64 at logB = 15), lo -128 and +127, the plane sums of the
    virtual rows stay inside pfks_plane_bound and recombine to sum d K."""
    in_words, out_words = 161, 3
    rows = E.crafted_rows(in_words - 1, logB, l, 64)
    key = E.make_key("random", in_words, out_words, logB, l, 64)
    D = E.digits_rows(rows, logB, l, 64)
    lo = ((D + 128) & 255) - 128
    hi = (D - lo) >> 8
    if logB >= 9:
        assert hi.max() == 1 << (logB - 9) and hi.min() == -(1 << (logB - 9)) and lo.min() == -128 and lo.max() == 127
    # reach, of the two-byte bound in_words x l x (|hi|max + 128) x 128: a digit of +-B/2 is all high byte (lo = 0), so the
    # largest-magnitude rows reach the high byte's share alone - 64 x 127 / (192 x 128) = 0.33 at logB = 15, less the digit
    # rule's floor(l/2) - and the whole bound where the digit is one byte (logB <= 8: 0.98 at (4, 8), 0.75 at (4, 2))
    reach = {(2, 15): 0.32, (4, 15): 0.32, (1, 15): 0.32, (3, 9): 0.01, (4, 8): 0.98, (4, 2): 0.74}[(l, logB)]
    top = 0
    for kind in ("follow", "00", "ff"):
        key = E.make_key(kind, in_words, out_words, logB, l, 64)
        for r in range(len(rows)):
            acc, _, _ = E.plane_accumulators(rows[r], key, logB, l, 64, split_bytes=True)
            top = max(top, int(np.abs(acc).max()))
    assert top >= reach * E.pfks_plane_bound(in_words, l, logB), top / E.pfks_plane_bound(in_words, l, logB)
    for kind in ("follow", "00", "ff", "random"):
        key = E.make_key(kind, in_words, out_words, logB, l, 64)
        for r in range(len(rows)):
            acc, dsum, _ = E.plane_accumulators(rows[r], key, logB, l, 64, split_bytes=True)
            assert np.abs(acc).max() <= E.pfks_plane_bound(in_words, l, logB)
            want = E.keyswitch_plain(rows[r], key, logB, l, 64, body=False)
            assert [(-v) % (1 << 64) for v in E.recombine_planes(acc, dsum, 64)] == want


@pytest.mark.parametrize("width,l,logB", [(32, 8, 4), (32, 4, 7), (32, 1, 1), (32, 5, 6), (64, 8, 7), (64, 7, 1), (64, 6, 7), (64, 3, 21)])
def test_reference_routes_and_the_byte_plane_identity(width, l, logB):
    """keyswitch_exact (int64 limbs) == keyswitch_plain (Python integers), and the kernels' identity
    sum d K = sum_b 2^(8b) sum d (K_b - 128) + 0x80..80 sum d from exact plane sums, on every crafted row under every key."""
    in_dim, out_words = 40, 5
    rows, _ = E.launch_rows(in_dim, logB, l, width, 12)
    for kind in E.KEYS:
        key = E.make_key(kind, in_dim, out_words, logB, l, width)
        fast = E.keyswitch_exact(rows, key, logB, l, width)
        for r in range(len(rows)):
            plain = E.keyswitch_plain(rows[r], key, logB, l, width)
            assert [int(v) for v in fast[r]] == plain, (kind, r)
            acc, dsum, _ = E.plane_accumulators(rows[r], key, logB, l, width)
            sdk = E.recombine_planes(acc, dsum, width)
            body = [0] * (out_words - 1) + [int(rows[r, in_dim])]
            assert [(b - s) % (1 << width) for b, s in zip(body, sdk)] == plain, (kind, r)


ORACLE32 = [(8, 4), (4, 7), (1, 7), (3, 7), (5, 6), (6, 5), (8, 1), (2, 16), (4, 8), (4, 3)]      # rep == 32: (8,4) (2,16) (4,8)
ORACLE64 = [(8, 7), (9, 7), (7, 9), (3, 21), (1, 63), (7, 1), (6, 7), (5, 3), (1, 1)]              # rep == 63: (9,7) (7,9) (3,21) (1,63)


@pytest.mark.parametrize("l,logB", ORACLE32)
def test_oracle32_keyswitch_is_the_integer_reference(l, logB):
    n, k, N = 9, 1, 16
    rows, _ = E.launch_rows(k * N, logB, l, 32, 14)
    for kind in E.KEYS:
        key = E.make_key(kind, k * N, n + 1, logB, l, 32)
        orc = oracle.Oracle((n, k, N, 1, 4, l, logB), np.zeros(n * 4 * N, np.uint32), key.reshape(-1), use_ntt=False)
        for r in range(len(rows)):
            assert [int(v) for v in orc.keyswitch(rows[r])] == E.keyswitch_plain(rows[r], key, logB, l, 32), (kind, r)


@pytest.mark.parametrize("l,logB", ORACLE64)
def test_oracle64_and_wop_keyswitch_are_the_integer_reference(l, logB):
    n, k, N = 9, 1, 16
    rows, _ = E.launch_rows(k * N, logB, l, 64, 14)
    for kind in E.KEYS:
        key = E.make_key(kind, k * N, n + 1, logB, l, 64)
        orc = oracle.Oracle64((n, k, N, 1, 4, l, logB, 2, 2, 0), np.zeros(n * 4 * N, np.uint64), key.reshape(-1))
        flat = np.ascontiguousarray(key.reshape(-1))
        for r in range(len(rows)):
            want = E.keyswitch_plain(rows[r], key, logB, l, 64)
            assert [int(v) for v in orc.keyswitch(rows[r])] == want, (kind, r)
            out = np.zeros(n + 1, dtype=np.uint64)
            row = np.ascontiguousarray(rows[r])
            u64p = C.POINTER(C.c_uint64)
            oracle.libw().orcw_keyswitch(k * N, n, l, logB, flat.ctypes.data_as(u64p), row.ctypes.data_as(u64p),
                                         out.ctypes.data_as(u64p))
            assert [int(v) for v in out] == want, (kind, r)


@pytest.mark.parametrize("l,logB", [(2, 15), (4, 15), (1, 2), (3, 21), (2, 30), (1, 30), (4, 2)])
def test_wop_packing_keyswitch_oracle_is_the_integer_reference(l, logB):
    """orcw_pfpks: every word of the row, the body included, is decomposed; no body term."""
    in_dim, glwe = 16, 8
    rows = E.crafted_rows(in_dim, logB, l, 64)
    u64p = C.POINTER(C.c_uint64)
    for kind in E.KEYS:
        key = E.make_key(kind, in_dim + 1, glwe, logB, l, 64)
        flat = np.ascontiguousarray(key.reshape(-1))
        for r in range(len(rows)):
            out = np.zeros(glwe, dtype=np.uint64)
            row = np.ascontiguousarray(rows[r])
            oracle.libw().orcw_pfpks(in_dim, glwe, l, logB, flat.ctypes.data_as(u64p), row.ctypes.data_as(u64p),
                                     out.ctypes.data_as(u64p))
            assert [int(v) for v in out] == E.keyswitch_plain(rows[r], key, logB, l, 64, body=False), (kind, r)


# ------------------------------------------------------------------------------------------------------------------
# chosen rows for the packing keyswitch through a programmed bootstrapping key (tests/wop_program.py)
# ------------------------------------------------------------------------------------------------------------------
def test_the_programme_digits_and_refusals():
    """Between the three programmes every level of cbs_l = 2 and of cbs_l = 3 is a target (d = 1); the by-products' digits
    are the powers of two the construction states; a level without a digit and a digit other than 1 are refused."""
    shapes = {name: W.Shape(12, 512, *prm) for name, prm in W.PROGRAMMES.items()}
    assert [W.level_digit(shapes["l2"], j) for j in range(2)] == [(0, 1), (1, 1)]
    assert [W.level_digit(shapes["l3_01"], j) for j in range(3)] == [(0, 1), (1, 1), None]
    assert [W.level_digit(shapes["l3_2"], j) for j in range(3)] == [(0, 1 << 10), (0, 1 << 5), (0, 1)]
    assert [W.level_digit(W.Shape(12, 512, 2, 10, 3, 5), j) for j in range(3)] == [(0, 1 << 5), (0, 1), (1, 1 << 5)]
    assert W.targeted_levels(shapes["l2"]) == [0, 1] and W.targeted_levels(shapes["l3_01"]) == [0, 1]
    assert W.targeted_levels(shapes["l3_2"]) == [2]
    row = np.arange(513, dtype=np.uint64)
    with pytest.raises(ValueError, match="has no digit"):
        W.program(shapes["l3_01"], [(0, 2, row)])
    with pytest.raises(AssertionError, match="is no target"):
        W.program(shapes["l3_2"], [(0, 0, row)])
    with pytest.raises(ValueError, match="share the key row"):
        W.program(W.Shape(12, 512, 2, 10, 3, 10), [(0, 0, row), (0, 0, row)])
    with pytest.raises(ValueError, match="no such step"):
        W.program(shapes["l2"], [(12, 0, row)])
    # the input rows: one mask word at the rotation 1, the body 0 after the + q/4
    rows = W.input_rows(shapes["l2"])
    assert rows.shape == (12, 13) and int(rows[3, 3]) == 1 << 54 and (int(rows[3, 12]) + (1 << 62)) % (1 << 64) == 0
    assert np.count_nonzero(rows[:, :12]) == 12


@pytest.mark.parametrize("l,logB", W.PFKS, ids=lambda v: str(v))
def test_the_programmed_key_feeds_the_packing_keyswitch_its_crafted_rows(l, logB):
    """OracleW.circuit_bootstrap under the programmed key == the integer reference on the predicted rows, for every step
    (crafted and control), every level (targets and by-products) and both packing keys r; the targeted rows are
    crafted_rows(k N, logB, l, 64) word for word; under the "follow" key their byte-split plane accumulators reach what
    test_the_packing_keyswitch_split_reaches_its_bytes asserts of the crafted rows."""
    N = 512
    cr = E.crafted_rows(N, logB, l, 64)
    seen = set()
    for name in W.PROGRAMMES:
        shape, bsk, small, where = W.crafted_programme(name, N, l, logB)
        steps = np.arange(shape.n)
        pred = W.predicted_rows(shape, bsk, steps)
        assert sorted({j for _, j in where}) == W.targeted_levels(shape) and len(where) == 8 * len(W.targeted_levels(shape))
        for (i, j), r in where.items():
            assert np.array_equal(pred[i, j, :N], cr[r, :N]) and int(pred[i, j, N]) & 1, (name, i, j)
            seen.add((shape.cbs_l, j, r))
        if name == "l3_01":
            assert not pred[:, 2].any()                                          # the level without a digit: the zero row
        flat = pred.reshape(-1, N + 1)
        for kind in ("random", "ff", "follow"):
            pf = E.make_key(kind, 2 * (N + 1), 2 * N, logB, l, 64).reshape(2, N + 1, l, 2 * N)
            params = (shape.n, 1, N, shape.pbs_l, shape.pbs_logB, 4, 4, l, logB, shape.cbs_l, shape.cbs_logB, 4, 4)
            ow = oracle.OracleW(params, bsk.reshape(-1), np.zeros(1, np.uint64), pf.reshape(-1))
            got = np.stack([ow.circuit_bootstrap(small[i]) for i in steps])      # [step][level][r][2 N]
            cols = [0, 1, 255, 256, N - 1, N, 2 * N - 1]
            for r in range(2):
                want = W.packing_reference(flat, pf[r], l, logB).reshape(shape.n, shape.cbs_l, 2 * N)
                assert np.array_equal(got[:, :, r], want), (name, kind, r)
                if logB == 30:                                                   # keyswitch_exact's 2^53 assertion fails here:
                    for i, j in ((0, 0), (2, shape.cbs_l - 1), (7, 1), (shape.n - 1, 0)):   # Python integers on a column sample
                        plain = E.keyswitch_plain(pred[i, j], pf[r][:, :, cols], logB, l, 64, body=False)
                        assert [int(got[i, j, r, c]) for c in cols] == plain, (name, kind, r, i, j)
        if logB <= 15:
            # the reach of the two-byte split: the mask words' share of the bound - reach_fraction of the digits' magnitudes,
            # of which a digit wider than a byte puts |hi| / (|hi| + 128) into the high byte (a digit of +-B/2 is all high
            # byte) - less what the body word, an odd constant, can take away
            follow = E.make_key("follow", N + 1, 3, logB, l, 64)
            hi = 0 if logB < 8 else max(1, (1 << (logB - 1)) >> 8)
            share = 1.0 if logB < 8 else hi / (hi + 128)
            want = E.reach_fraction(l, logB) * share * E.pfks_plane_bound(N, l, logB) - E.pfks_plane_bound(1, l, logB)
            top = max(int(np.abs(E.plane_accumulators(pred[i, j], follow, logB, l, 64, split_bytes=True)[0]).max())
                      for (i, j) in where)
            assert top >= want > 0, (name, top, want)
            table = {(2, 15): 0.32, (4, 15): 0.32, (1, 15): 0.32, (4, 2): 0.74}     # the figures of the test named above
            if (l, logB) in table:
                assert want >= table[(l, logB)] * E.pfks_plane_bound(N + 1, l, logB)
    # every (cbs_l, level, crafted row) is a target of some programme
    assert seen == {(L, j, r) for L in (2, 3) for j in range(L) for r in range(8)}


def test_the_exact_reference_in_narrow_limbs():
    """keyswitch_exact(limb=8), what the device tests use at logB 30 == keyswitch_plain, whole rows at a small shape."""
    for l, logB in ((2, 30), (1, 30), (3, 21)):
        rows = E.crafted_rows(40, logB, l, 64)
        for kind in E.KEYS:
            key = E.make_key(kind, 41, 5, logB, l, 64)
            fast = E.keyswitch_exact(rows, key, logB, l, 64, body=False, limb=8)
            for r in range(len(rows)):
                assert [int(v) for v in fast[r]] == E.keyswitch_plain(rows[r], key, logB, l, 64, body=False), (kind, r)


def test_the_launch_rules_are_those_of_the_sources():
    """wop_program's restatements of pfpks_on_matrix_cores, of the slicing of k_pfpks64's launches and of the gate chunk of
    helm_wop_eval_luts, read back from helm_wopbs.inc (a tripwire on the text, as the admission rules above), and the
    numbers the device tests build on."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    wop = open(os.path.join(root, "helm_amd", "csrc", "helm_wopbs.inc")).read()
    assert "const int64_t chunk = std::max<int64_t>(1, 16384 / bits);" in wop
    assert "for (int64_t base = 0; base < count; base += chunk)" in wop
    assert "return ctx->d_pf_planes && ctx->wop->keys->ks_mfma && count >= 64;" in wop
    assert wop.count("while (slices < 16 && (int64_t)gx * gy * slices < 2 * (int64_t)W->n_cus && in_words / (slices * 2) >= 64) slices *= 2;") == 2
    assert "const unsigned gx = (unsigned)((count + 3) / 4), gy = (unsigned)((glwe_words + 255) / 256);" in wop
    assert "if (gridDim.z == 1) *dst = 0ull - acc[g];" in wop
    assert (W.gate_chunk(12), W.gate_chunk(1), W.gate_chunk(16385), W.gate_chunk(3)) == (1365, 16384, 1, 5461)
    # N = 512: the grid is X workgroups wide in all, one slice from X = 2 n_cus on (256 compute units: 512)
    assert [W.pfpks_slices(X, 512, 256) for X in (2, 66, 195, 508, 509, 512, 513)] == [8, 8, 4, 2, 1, 1, 1]
    assert W.pfpks_slices(1, 2048, 256) == 16 and W.pfpks_slices(10 ** 6, 2048, 256) == 1
    assert [W.pfpks_route(X, 15, 512, None) for X in (63, 64)] == ["valu", "mfma"]
    assert W.pfpks_route(640, 15, 512, "0") == "valu" and W.pfpks_route(640, 21, 512, None) == "valu"
    # crafted rows at the tile positions the device tests name
    for bits, L, levels in ((32, 2, [0, 1]), (33, 2, [0, 1]), (21, 3, [0, 1]), (22, 3, [2]), (80, 2, [0, 1])):
        steps, crafted = W.steps_for(bits, L, levels)
        X = bits * L
        assert len(steps) == bits and {x for x in (0, 15, 16, 63, 64) if x < X and x % L in levels} <= set(crafted)
        assert any(x >= (X - 1) // 16 * 16 for x in crafted) and (steps >= 8).sum() >= bits // 4
