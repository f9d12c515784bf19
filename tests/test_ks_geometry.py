"""The launch geometry of the vector-ALU keyswitch (helm_ks::vector_geometry, helm_amd/csrc/keyswitch.h) restated in
tests/ks_edges.py and checked on the CPU: the mirror against the source's text, its invariants over every admitted
(k N, ks_l) of both engines, the case table of tests/test_gpu_keyswitch_wide.py against the LDS bands it is built for, and
the accumulator bounds of the matrix-core form at the input dimensions the large-N and the N = 8192 bit admit.

The bands: a launch's dynamic LDS is t_chunk x ks_l x 4 B.  "default": at most 64 KiB, what a kernel may ask for without an
attribute; "raised": above 64 KiB and below 160 KiB, which needs hipFuncAttributeMaxDynamicSharedMemorySize; "limit":
exactly 160 KiB = 163,840 B, all of a gfx950 workgroup's LDS; "clause": the grid clause alone would ask for more than
160 KiB and the LDS clause slices further."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ks_edges as E  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIB = 1024
LEVELS = {32: (1, 2, 3, 4, 5, 6, 8), 64: tuple(range(1, 9))}


def test_the_mirror_is_the_source():
    """A tripwire on the three deciding lines of vector_geometry (and the workgroup counts above them), whitespace-stripped:
    whoever edits them is asked to edit ks_edges.vector_geometry too."""
    src = re.sub(r"\s+", "", open(os.path.join(ROOT, "helm_amd", "csrc", "keyswitch.h")).read())
    assert "constunsignedgx=(unsigned)((count+3)/4),gy=(unsigned)((n+1+255)/256);" in src
    assert "while(slices<16&&(int64_t)gx*gy*slices<2*(int64_t)n_cus&&kN/(slices*2)>=64)slices*=2;" in src       # grid clause
    assert "while((size_t)((kN+slices-1)/slices)*ks_l*sizeof(uint32_t)>(size_t)160*1024)slices*=2;" in src      # LDS clause
    assert "constintt_chunk=(kN+slices-1)/slices;" in src
    assert "(size_t)t_chunk*ks_l*sizeof(uint32_t)}" in src
    # the launcher clears the rows of every sliced launch, whichever clause sliced it
    assert "constGeometrygeo=vector_geometry(count,K.out_dim,K.in_dim,K.l,ctx->n_cus);if(geo.slices>1&&(e=E::zero_rows(" in src
    # the 64-bit engine raises its vector kernels' dynamic-LDS limit to the workgroup's 160 KiB; the boolean engine sets no
    # attribute, and the runtime takes its launches of up to 160 KiB as they are (tests/test_gpu_keyswitch_wide.py runs them)
    eng = re.sub(r"\s+", "", open(os.path.join(ROOT, "helm_amd", "csrc", "helm_shortint.hip")).read())
    assert "hipFuncSetAttribute(kernel,hipFuncAttributeMaxDynamicSharedMemorySize,160*1024);" in eng
    eng = re.sub(r"\s+", "", open(os.path.join(ROOT, "helm_amd", "csrc", "helm_hip.hip")).read())
    assert "template<typename>statichipError_tallow_lds(Ctx*,constvoid*){returnhipSuccess;}" in eng


def test_the_domain_constants():
    assert E.max_in_dim(32) == 7936 and E.max_in_dim(64) == 3840
    assert E.max_in_dim(64, large=True) == 4096 == E.LARGE_IN_DIM and E.max_in_dim(64, n8192=True) == 8192 == E.N8192_IN_DIM
    assert E.in_dims(32) == list(range(256, 7937, 256)) and E.in_dims(64) == list(range(256, 3841, 256)) + [4096, 8192]
    si = open(os.path.join(ROOT, "helm_amd", "csrc", "helm_shortint.hip")).read()
    assert "return P.k == 1 && P.N == 4096 && P.pbs_l >= 1 && P.grouping_factor <= 1;" in si        # si_large_domain
    assert "return P.k == 1 && P.N == 8192 && P.pbs_l >= 1 && P.grouping_factor <= 1;" in si        # si_n8192_domain
    assert (E.LDS_DEFAULT, E.LDS_LIMIT) == (65536, 163840)


def test_a_few_geometries_by_hand():
    # 40 rows of k N = 8192: 10 workgroups, 16 slices of 512 words
    assert E.vector_geometry(40, 46, 8192, 8, 256) == (10, 1, 16, 512, 512 * 8 * 4)
    # 2052 rows: 513 workgroups, one slice by the grid clause; 256 KiB of digits at ks_l = 8: the LDS clause makes it two
    assert E.grid_slices(2052, 46, 8192, 256) == (513, 1, 1)
    assert E.vector_geometry(2052, 46, 8192, 8, 256) == (513, 1, 2, 4096, 131072)
    assert E.vector_geometry(2052, 46, 8192, 5, 256) == (513, 1, 1, 8192, 163840)
    assert E.vector_geometry(2052, 46, 8192, 6, 256) == (513, 1, 2, 4096, 98304)
    assert E.vector_geometry(2052, 46, 7936, 8, 256) == (513, 1, 2, 3968, 126976)
    assert E.vector_geometry(2052, 46, 7936, 3, 256) == (513, 1, 1, 7936, 95232)
    assert E.vector_geometry(2052, 46, 7936, 5, 256) == (513, 1, 1, 7936, 158720)
    assert E.vector_geometry(516, 46, 7936, 8, 256) == (129, 1, 4, 1984, 63488)
    assert E.vector_geometry(1028, 300, 7936, 3, 256) == (257, 2, 1, 7936, 95232)
    # k N = 256: never more than 4 slices (a slice has at least 64 words)
    assert E.vector_geometry(1, 46, 256, 4, 256)[2:4] == (4, 64)
    # an odd k N / slices does not occur (k N is a multiple of 256, slices at most 16 below 160 KiB), but the ceiling is stated
    assert E.vector_geometry(1, 46, 1000, 1, 256)[2:4] == (8, 125)


@pytest.mark.parametrize("n_cus", [64, 256, 304])
def test_the_invariants_over_every_admitted_shape(n_cus):
    """Counts 1 .. 16 n_cus + 8 (as workgroup counts gx = ceil(count / 4): the geometry sees a count through gx alone), n with
    1 to 5 column chunks, every k N and ks_l of both engines.  Beyond (gx, gy) the result depends on (k N, ks_l, the grid
    clause's slices) alone, so the LDS clause and the invariants are evaluated once for each such triple an enumerated
    launch shows."""
    seen = {}
    dims = sorted(set(E.in_dims(32)) | set(E.in_dims(64)))
    for n in (46, 300, 600, 1000, 1024):
        gy = (n + 256) // 256
        for kN in dims:
            widths = [w for w in (32, 64) if kN in E.in_dims(w)]
            for gx in range(1, (16 * n_cus + 8 + 3) // 4 + 1):
                count = 4 * gx
                got = E.grid_slices(count, n, kN, n_cus)
                assert got[:2] == (gx, gy) and E.grid_slices(count - 3, n, kN, n_cus) == got
                s_grid = got[2]
                if (kN, s_grid) in seen:
                    continue
                seen[(kN, s_grid)] = count
                for l in sorted({l for w in widths for l in LEVELS[w]}):
                    ggx, ggy, slices, t_chunk, lds = E.vector_geometry(count, n, kN, l, n_cus)
                    assert (ggx, ggy) == (gx, gy)
                    assert slices & (slices - 1) == 0 and slices >= s_grid                      # a power of two
                    assert slices * t_chunk >= kN and (slices - 1) * t_chunk < kN                # no slice is empty
                    assert lds == t_chunk * l * 4 <= 160 * KIB
                    if kN <= 4096:
                        assert slices == s_grid, (kN, l, count)                                  # the source comment's claim
                    if slices != s_grid:
                        # the LDS clause fired: the grid clause alone was over the limit, and half as many slices still are
                        assert (kN + s_grid - 1) // s_grid * l * 4 > 160 * KIB
                        assert (kN + slices // 2 - 1) // (slices // 2) * l * 4 > 160 * KIB
                        assert kN > 4096 and E.lds_band(count, n, kN, l, n_cus) == ("clause", "lds")
                    else:
                        assert E.lds_band(count, n, kN, l, n_cus)[1] == "grid"
    assert {s for _, s in seen} == {1, 2, 4, 8, 16}
    # the LDS clause fires on the 32-bit engine too: k N > 4096 with ks_l = 6 or 8 (k N x ks_l x 4 B > 160 KiB from k N = 5376)
    assert E.lds_band(8 * n_cus + 4, 46, 5376, 8, n_cus) == ("clause", "lds")
    assert E.lds_band(8 * n_cus + 4, 46, 5120, 8, n_cus) == ("limit", "grid")
    assert E.lds_band(8 * n_cus + 4, 46, 6912, 6, n_cus) == ("clause", "lds")
    assert E.lds_band(8 * n_cus + 4, 46, 6656, 6, n_cus) == ("raised", "grid")


@pytest.mark.parametrize("n_cus", [64, 256, 304])
def test_the_width_pattern(n_cus):
    """40 rows -> 16 slices; 2 CUs + 4 -> 4; 4 CUs + 4 -> 2; 8 CUs + 4 -> 1 at one column chunk; as many workgroups at two."""
    for kN in (4096, 5120, 7936, 8192):
        assert [E.width_for_slices(s, 46, kN, n_cus) for s in (16, 4, 2, 1)] == [40, 2 * n_cus + 4, 4 * n_cus + 4, 8 * n_cus + 4]
        assert [E.width_for_slices(s, 300, kN, n_cus) for s in (16, 4, 2, 1)] == \
            [min(40, 4 * ((2 * n_cus - 1) // 16)), n_cus + 4, 2 * n_cus + 4, 4 * n_cus + 4]
        for s in (4, 2, 1):                       # one workgroup fewer than the pattern's multiple: one more doubling
            count = E.width_for_slices(s, 46, kN, n_cus) - 8
            assert E.grid_slices(count, 46, kN, n_cus)[2] == 2 * s


def reachable_bands(width, n_cus):
    out = set()
    for kN in E.in_dims(width):
        for l in LEVELS[width]:
            for count in (40, 2 * n_cus + 4, 4 * n_cus + 4, 8 * n_cus + 4):
                out.add(E.lds_band(count, 46, kN, l, n_cus)[0])
    return out


def test_the_case_table_covers_every_band_and_slice_count():
    """At 256 compute units (an MI355X), as tests/test_gpu_n8192.py::test_wide_vector_alu_keyswitch_is_sliced_for_lds; the
    device test asserts the same expectations at the device's own count before it launches."""
    n_cus = 256
    cases = E.wide_cases()
    assert len({c.id for c in cases}) == len(cases)
    bands = {32: set(), 64: set()}
    slices = {32: set(), 64: set()}
    by_lds = {}
    for c in cases:
        assert c.kN in E.in_dims(c.width) and c.l in LEVELS[c.width] and (c.l, c.logB) in E.ks_shapes(c.width), c.id
        assert c.generic == {4096: "large", 8192: "n8192"}.get(c.kN if c.width == 64 else 0), c.id
        assert c.bands(n_cus) == c.expect, (c.id, c.bands(n_cus))
        assert c.kinds[0] == "random" or c.kinds == E.KEYS
        for count, (gx, gy, s, t_chunk, lds), (band, clause) in zip(c.counts(n_cus), c.geometry(n_cus), c.expect):
            bands[c.width].add(band)
            slices[c.width].add(s)
            by_lds[(c.width, c.kN, c.l, count) + ((c.n,) if c.n != 46 else ())] = (s, lds, gy)
            if c.width == 64 and count >= 160:
                assert c.mfma0_only                                        # KsEngine64::matrix_path takes such a batch
            if c.width == 32 and c.l in (1, 2, 4, 8):
                assert c.mfma0_only                                        # KsEngine32::matrix_path: byte planes exist
    for w in (32, 64):
        assert bands[w] == reachable_bands(w, n_cus) == set(E.BANDS), (w, bands[w])
        assert slices[w] >= {16, 4, 2, 1}, (w, slices[w])
    # the figures of the table, as DESIGN.md gives them
    assert by_lds[(32, 7936, 3, 2052)] == (1, 95232, 1) and by_lds[(32, 7936, 3, 1028)][:2] == (2, 47616)
    assert by_lds[(32, 7936, 3, 40)][:2] == (16, 5952)
    assert by_lds[(32, 7936, 8, 2052)] == (2, 126976, 1) and by_lds[(32, 7936, 8, 516)] == (4, 63488, 1)
    assert by_lds[(32, 7936, 5, 2052)] == (1, 158720, 1)
    assert by_lds[(32, 7936, 3, 1028, 300)] == (1, 95232, 2)                    # two column chunks
    assert by_lds[(32, 5120, 8, 2052)] == (1, 163840, 1)
    assert by_lds[(64, 4096, 8, 516)] == (4, 32768, 1) and by_lds[(64, 4096, 8, 1028)] == (2, 65536, 1)
    assert by_lds[(64, 4096, 8, 2052)] == (1, 131072, 1)
    assert by_lds[(64, 8192, 5, 2052)] == (1, 163840, 1) and by_lds[(64, 8192, 6, 2052)] == (2, 98304, 1)
    assert by_lds[(64, 8192, 8, E.SWEEP)] == (16, 16384, 1)
    # the keyswitch-first gate shapes: admitted ((k+1) N <= 8192), vector-ALU form only, in the raised band unsliced
    for k, N, n, l, logB in E.GATE_SHAPES:
        assert (k + 1) * N <= 8192 and l in (3, 5, 6) and (l, logB) in E.ks_shapes(32)
        assert E.lds_band(8 * n_cus + 4, n, k * N, l, n_cus) == ("raised", "grid")
        assert E.vector_geometry(40, n, k * N, l, n_cus)[2] == 16


def test_the_accumulators_at_the_new_sizes():
    """Exact integers at in_dim 4096 and 8192, beyond what tests/test_keyswitch_edges.py bounds at 3840 (0.117 of 2^31): every
    int32 plane accumulator within rows x B/2 x 128 = 2^29 at (8, 7) (0.25 of 2^31), the digit sum within 2^22, the 64-row chunk count,
    and what the crafted rows reach of it under the sign-following key."""
    assert E.plane_bound(8192, 8, 7) == 2 ** 29 < 2 ** 31
    assert E.plane_bound(4096, 8, 7) == 2 ** 28
    assert 8192 * 8 * 64 == 2 ** 22 < 2 ** 31                                   # |dsum| fits its int32
    assert 8192 * E.padded_levels(8) // 64 == 1024 and 8192 * E.padded_levels(5) // 64 == 1024   # k-chunks of 64 rows
    for l, b in E.ks_shapes(64):
        assert E.plane_bound(8192, l, b) <= 2 ** 29
    # the fractions beside those test_keyswitch_edges.py pins: a function of (l, logB) alone
    assert [round(E.reach_fraction(l, b), 3) for l, b in ((1, 1), (8, 1), (1, 7), (8, 7))] == [0.992, 0.496, 0.992, 0.984]
    for in_dim in (4096, 8192):
        for l, logB in ((8, 7), (8, 1), (1, 7), (1, 1)):
            h = 1 << (logB - 1)
            peak = l * h - l // 2
            rows = E.crafted_rows(in_dim, logB, l, 64)
            key = E.make_key("follow", in_dim, 2, logB, l, 64)
            acc, dsum, dabs = E.plane_accumulators(rows[E.CRAFTED.index("abs_max")], key, logB, l, 64)
            bound = E.plane_bound(in_dim, l, logB)
            assert dabs == in_dim * peak
            assert E.reach_fraction(l, logB) * bound <= np.abs(acc).min() and np.abs(acc).max() <= bound
            _, dsum, _ = E.plane_accumulators(rows[E.CRAFTED.index("dsum_max")], key, logB, l, 64)
            assert dsum == in_dim * peak <= 2 ** 22
            _, dsum, _ = E.plane_accumulators(rows[E.CRAFTED.index("dsum_min")], key, logB, l, 64)
            assert -in_dim * peak <= dsum <= -in_dim * (peak - 1)
    assert 8192 * (8 * 64 - 4) == 4161536                                       # sum |d| of the abs_max row at (8, 7): 0.992 of 2^22


def test_the_wide_reference_is_the_reference():
    """keyswitch_exact_wide (chunks, digits shared between keys) == keyswitch_exact, across a chunk edge."""
    rows, _ = E.launch_rows(40, 7, 3, 64, 21)
    keys = {kind: E.make_key(kind, 40, 5, 7, 3, 64) for kind in ("random", "follow", "ff")}
    got = E.keyswitch_exact_wide(rows, keys, 7, 3, 64, chunk=8)
    for kind, key in keys.items():
        assert np.array_equal(got[kind], E.keyswitch_exact(rows, key, 7, 3, 64)), kind
    rows, _ = E.launch_rows(24, 4, 8, 32, 13)
    key = E.make_key("random", 24, 3, 4, 8, 32)
    assert np.array_equal(E.keyswitch_exact_wide(rows, {"k": key}, 4, 8, 32, chunk=5)["k"], E.keyswitch_exact(rows, key, 4, 8, 32))
