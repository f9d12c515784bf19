"""Every keyswitch kernel at its digit, key-byte and tile edges (tests/ks_edges.py builds the inputs and the reference).

Contexts are created from parameters and a crafted keyswitching key alone (the keyswitch is linear: any words are a key).
A launch holds the crafted rows - the largest / smallest digit sum, the largest sum of digit magnitudes, 0, 2^w - 1,
2^(w-1), 2^(w-1) - 1, every tie - and uniform control rows; the keys are whole keys of 0x00 / 0xFF / 0x80 / 0x7F bytes, the key
whose bytes follow the digits' signs (every int32 plane accumulator at 0.5 - 0.98 of rows x B/2 x 128, the fraction
tests/test_keyswitch_edges.py pins per shape) and uniform words.  Every output word must equal ks_edges' integer reference;
the control rows the CPU oracle as well; no tolerance.  Controls failing: the key layout of this test; crafted rows failing
alone: a fault at the edge.  The ABI does not report which keyswitch kernel served a launch, so every case runs with
HELM_HIP_KS_MFMA unset and = 0 and the two results are compared word for word; `route` states what the unset run takes by the
launchers' rules (32-bit: byte planes exist for ks_l in {1, 2, 4, 8}; 64-bit: planes and a batch of 160 or more).

ks_l * ks_logB == 32 (admitted, (8, 4)): decompose<L>() shifted by a count of -1 (2^31 added to every mask word where the
hardware masks the count) and lost the carry out of the least significant level; fixed in helm_hip.hip together with this
file, whose (8, 4) cases are its regression test.  DESIGN.md section 2, "Keyswitch at its edges"."""
import contextlib
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helm_amd
import oracle
from helm_amd import _native as nv
from helm_amd import wopbs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ks_edges as E  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _params(width, n, k, N, l, logB):
    if width == 32:
        p, _, _ = helm_amd.named_params("toy")
        p.pbs_l, p.pbs_logB = 1, 4
    else:
        p, _, _ = helm_amd.si_named_params("si_toy_512")
        p.pbs_l, p.pbs_logB = 1, 8
    p.n, p.k, p.N, p.ks_l, p.ks_logB = n, k, N, l, logB
    return p


def _server(width, p, key):
    if width == 32:
        return helm_amd.ServerKey(params=p, ksk=key)
    return helm_amd.SiServerKey(params=p, ksk=key, generic="allow")


def _reload(width, sk, key):
    """Another key of the same shape into the same context (the loaders rebuild the byte planes)."""
    flat = np.ascontiguousarray(key).reshape(-1)
    if width == 32:
        nv.hip_check(nv.hip.helm_hip_load_keyswitch_key(sk._h, nv.as_u32p(flat), flat.size))
    else:
        nv.hip_check(nv.hip.helm_si_load_keyswitch_key(sk._h, nv.as_u64p(flat), flat.size))


def _oracle_rows(width, p, key, rows):
    if width == 32:
        orc = oracle.Oracle((p.n, p.k, p.N, p.pbs_l, p.pbs_logB, p.ks_l, p.ks_logB), np.zeros(1, np.uint32), key.reshape(-1),
                            use_ntt=False)
        return np.stack([orc.keyswitch(r) for r in rows])
    out = np.zeros((len(rows), p.n + 1), dtype=np.uint64)
    u64p = C.POINTER(C.c_uint64)
    flat = np.ascontiguousarray(key.reshape(-1))
    for i, r in enumerate(rows):
        r = np.ascontiguousarray(r)
        oracle.libw().orcw_keyswitch(p.k * p.N, p.n, p.ks_l, p.ks_logB, flat.ctypes.data_as(u64p), r.ctypes.data_as(u64p),
                                     out[i].ctypes.data_as(u64p))
    return out


def route(width, kN, l, count, mfma_env):
    """The kernel pair the launchers' rules give a launch - KsEngine32::matrix_path (helm_hip.hip) and
    KsEngine64::matrix_path (helm_shortint.hip), with the loaders' conditions for byte planes, restated, since the ABI does not
    report the kernel that ran.  The assertion against a case's expected routes therefore checks this model, not the
    device: should the launchers' rules change without it, the unset and the = 0 run of a case could take the same kernel
    unnoticed.  What the device shows is that the two runs, and the integer reference, agree word for word."""
    if mfma_env == "0":
        return "valu"
    if width == 32:
        return "mfma" if l in (1, 2, 4, 8) and (kN * l) % 64 == 0 else "valu"
    return "mfma" if (kN * E.padded_levels(l)) % 64 == 0 and count >= 160 else "valu"


def _first_diff(got, want):
    r, c = np.argwhere(got != want)[0]
    return "row %d word %d: got %#x, want %#x" % (r, c, int(got[r, c]), int(want[r, c]))


def _compare(got, want, controls, label):
    bad = sorted({int(r) for r in np.argwhere(got != want)[:, 0]})
    bad_ctl = [r for r in bad if r in controls]
    assert not bad_ctl, f"{label}: control rows {bad_ctl[:8]} differ ({_first_diff(got, want)}): key layout of the test?"
    assert not bad, f"{label}: crafted rows {bad[:8]} differ while every control row is exact: wrong at the edge; " + \
        _first_diff(got, want)


def run_case(case, kinds=E.KEYS, check_build=False):
    """case: (width, n, k, N, ks_l, ks_logB, batch widths, expected routes of the unset run).  -> the counters of a
    counting build, summed (check_build)."""
    width, n, k, N, l, logB, counts, want_routes = case
    kN = k * N
    p = _params(width, n, k, N, l, logB)
    label = "w%d n%d kN%d l%d B%d" % (width, n, kN, l, logB)
    assert tuple(route(width, kN, l, c, None) for c in counts) == tuple(want_routes), label
    keys = {kind: E.make_key(kind, kN, n + 1, logB, l, width) for kind in kinds}
    launches = {c: E.launch_rows(kN, logB, l, width, c) for c in counts}
    want = {(kind, c): E.keyswitch_exact(launches[c][0], keys[kind], logB, l, width) for kind in kinds for c in counts}
    # the reference against the oracle on the control rows (a few of them: the oracle is one row at a time)
    for kind in kinds:
        rows, controls = launches[counts[0]]
        some = controls[:3]
        if some:
            assert np.array_equal(_oracle_rows(width, p, keys[kind], rows[some]), want[(kind, counts[0])][some]), label
    got, violations = {}, None
    for mode in (None, "0"):
        with _env(HELM_HIP_KS_MFMA=mode):
            sk = _server(width, p, keys[kinds[0]])
        try:
            if check_build:
                sk.bound_violations(reset=True)
            for kind in kinds:
                _reload(width, sk, keys[kind])
                for c in counts:
                    rows, controls = launches[c]
                    out = sk.keyswitch_batch(rows)
                    _compare(out, want[(kind, c)], set(controls), "%s key %s batch %d KS_MFMA=%s (%s)" %
                             (label, kind, c, mode, route(width, kN, l, c, mode)))
                    got[(mode, kind, c)] = out
            if check_build:
                v = sk.bound_violations()
                violations = v if violations is None else [a + b for a, b in zip(violations, v)]
        finally:
            sk.close()
    for kind in kinds:
        for c in counts:
            assert np.array_equal(got[(None, kind, c)], got[("0", kind, c)]), (label, kind, c)
    return violations


def _logBs(width, l):
    """ks_logB = 1 and the largest admitted at this level count: min(7, floor(32 / l)) on the 32-bit engine - 7 for l <= 4
    (the int8 extremes), then 6, 5 and 4 (rep 30, 30 and 32) - and 7 at every level count of the 64-bit one, whose rep is
    56 at most."""
    return [1, min(7, (32 if width == 32 else 63) // l)]


SWEEP = 165     # 8 crafted of every 12 rows; wide enough for the 64-bit matrix-core path, not a multiple of 64
DECOMP32 = [(32, 46, 1, 256, l, b, (SWEEP,), ("mfma" if l in (1, 2, 4, 8) else "valu",))
            for l in (1, 2, 3, 4, 5, 6, 8) for b in _logBs(32, l)] + [(32, 46, 1, 256, 8, 3, (SWEEP,), ("mfma",))]
DECOMP64 = [(64, 46, 1, 512, l, b, (SWEEP,), ("mfma",)) for l in range(1, 9) for b in _logBs(64, l)]
# n + 1 = 0, 1, 15, 16, 17 mod 32 (an odd number of 16-column tiles: the 32-bit wave past the last tile), n + 1 > 256 (a
# second column chunk of the vector kernels), the largest n; then the largest k N of either engine
GEOMETRY = [(32, n, 1, 256, 4, 7, (SWEEP,), ("mfma",)) for n in (31, 32, 46, 47, 48, 300, 1024)] + \
           [(32, n, 1, 256, 3, 7, (SWEEP,), ("valu",)) for n in (32, 300)] + \
           [(64, n, 1, 512, 5, 7, (SWEEP,), ("mfma",)) for n in (31, 32, 46, 47, 48, 300, 1024)] + \
           [(32, 46, 31, 256, 2, 7, (SWEEP,), ("mfma",)), (64, 46, 15, 256, 2, 7, (SWEEP,), ("mfma",))]
WIDTHS = (1, 4, 5, 63, 64, 65, 159, 160, 161, 2100)       # 2100 rows: 525 workgroups, more than two per compute unit - one slice
R64 = ("valu",) * 7 + ("mfma",) * 3
BATCH = [(32, 46, 1, 256, 8, 4, WIDTHS, ("mfma",) * 10), (32, 46, 1, 256, 6, 5, WIDTHS, ("valu",) * 10),
         (64, 46, 1, 512, 6, 7, WIDTHS, R64), (64, 46, 1, 512, 8, 7, WIDTHS, R64)]


def _id(case):
    return "w%d-n%d-k%dN%d-l%dB%d-%s" % (case[:6] + ("x".join(str(c) for c in case[6][:3]),))


@pytest.mark.parametrize("case", DECOMP32 + DECOMP64, ids=_id)
def test_decompositions(case):
    """Every admitted level count with logB 1, 7 (digits of +-64: the int8 extremes) and the widest representable part
    (32-bit: rep 32 at (8, 4); 64-bit: 7 bits a level, rep 56 at most - ks_logB <= 7 keeps the admitted rep off 63), the
    padded level counts 3, 5, 6, 7 of the 64-bit matrix-core path included; all six keys."""
    run_case(case)


@pytest.mark.parametrize("case", GEOMETRY, ids=_id)
def test_geometry(case):
    run_case(case, kinds=("follow", "random", "00"))


@pytest.mark.parametrize("case", BATCH, ids=_id)
def test_batch_widths(case):
    """Both sides of 64-row padding, of the 64-bit engine's switch at 160, the sliced (atomic) and the one-slice (plain
    store) launches of the vector kernels."""
    run_case(case, kinds=("follow", "random"))


def test_refused_decompositions():
    for l, b in ((8, 5), (7, 1), (1, 8), (5, 7)):
        with pytest.raises(helm_amd.HelmError, match="bad keyswitch decomposition"):
            helm_amd.ServerKey(params=_params(32, 46, 1, 256, l, b))
    for l, b in ((9, 1), (1, 8), (8, 8)):
        with pytest.raises(helm_amd.HelmError, match="bad keyswitch decomposition"):
            helm_amd.SiServerKey(params=_params(64, 46, 1, 512, l, b), generic="allow")


@pytest.mark.parametrize("l,logB", [(4, 7), (8, 4), (3, 7)])
def test_mux_level_under_extreme_key_bytes(l, logB):
    """One level with MUX gates (the keyswitch reads big0 + big1 and adds the 1/8 body) and plain gates under crafted
    keyswitching keys, on the matrix-core pair and on the vector kernel: the oracle under the same keys, bit for bit."""
    p, a, b = helm_amd.named_params("toy")
    p.ks_l, p.ks_logB = l, logB
    ck = helm_amd.ClientKey(p, a, b, seed=5)
    ct = ck.encrypt([False, True, True])
    ops = [oracle.MUX, oracle.MUX, oracle.AND, oracle.XOR, oracle.MUX]
    i0, i1, i2 = [0, 1, 0, 1, 2], [1, 2, 1, 2, 0], [2, 0, -1, -1, 1]
    out = np.arange(3, 8, dtype=np.int32)
    for kind in ("ff", "00", "follow", "7f"):
        key = E.make_key(kind, p.k * p.N, p.n + 1, logB, l, 32)
        orc = oracle.Oracle(p.as_tuple7(), ck.bsk, key.reshape(-1))
        ref = np.zeros((8, p.n + 1), dtype=np.uint32)
        ref[:3] = ct
        orc.eval_level(ref, ops, i0, i1, i2, out)
        for mode in (None, "0"):
            with _env(HELM_HIP_KS_MFMA=mode):
                sk = helm_amd.ServerKey(params=p, bsk=ck.bsk, ksk=key)
            try:
                w = sk.wires(8)
                w.upload([0, 1, 2], ct)
                w.eval_gate_level(ops, i0, i1, i2, out)
                got = w.download()
                assert np.array_equal(got, ref), (kind, mode, route(32, p.k * p.N, l, 5, mode), _first_diff(got, ref))
            finally:
                sk.close()


# (pfks_l, pfks_logB): the named set's (2, 15); the smallest digit at the smallest and the largest level count; the padded
# level count 3 (LP = 8: zero bytes interleaved) and the largest level count at the widest digit the byte planes are built
# for (hi = +-64; (4, 15) carries the 0.094 accumulator bound); the widest digit, and rep == 63, which have no byte planes
PFKS = [(2, 15), (1, 2), (4, 2), (3, 15), (4, 15), (1, 15), (2, 30), (1, 30), (3, 21)]


@pytest.fixture(scope="module")
def wop_side():
    sp, a, b = helm_amd.si_named_params("si_toy_512")
    ck = helm_amd.SiClientKey(sp, a, b, seed=11)
    sk = helm_amd.SiServerKey(ck)
    yield ck, sk
    sk.close()


@pytest.mark.parametrize("l,logB", PFKS, ids=lambda v: str(v))
def test_wop_packing_keyswitch_under_extreme_key_bytes(wop_side, l, logB):
    """The circuit bootstrap (bootstraps, then the packing keyswitch of their outputs) at the ends of the admitted
    (pfks_l, pfks_logB), under the generated packing key (the control: a failure under it is this test's layout) and under
    packing keys of extreme bytes: a batch of 5 (k_pfpks64<l>) and of 70 (pfks_logB <= 15: k_pfpks_digits<l> + k_ks64_mfma on
    the byte planes k_pfpks_planes built; above 15 the loader builds no planes - the high byte of a digit would not fit
    [-64, 64] - and k_pfpks64<l> serves every width) against the oracle under the same key, and against each other.  The
    rows the packing keyswitch reads here are the bootstrap outputs of an honest key: uniform words.  The crafted rows of
    ks_edges reach it on the device through a programmed bootstrapping key, in tests/test_gpu_wop_programmed_rows.py."""
    ck, sk = wop_side
    wp, c, d = wopbs.wop_named_params("wop_toy_512")
    assert (wp.pfks_l, wp.pfks_logB) == PFKS[0]
    wp.pfks_l, wp.pfks_logB = l, logB
    assert (l, logB) in E.pfks_shapes(matrix_cores=logB <= 15) and ((wp.k + 1) * wp.N) % 16 == 0
    wk = wopbs.WopClientKey(ck, wp, c, d, seed=12)
    wsk = wopbs.WopServerKey(sk, wk)
    try:
        rng = np.random.default_rng(4)
        lwe_sk = wk.lwe_secret.astype(bool)
        small = rng.integers(0, 1 << 64, size=(70, wp.n + 1), dtype=np.uint64)
        bits = rng.integers(0, 2, size=70).astype(np.uint64)
        small[:, -1] = (small[:, :-1] * lwe_sk).sum(axis=1, dtype=np.uint64) + (bits << np.uint64(63))
        shape = (wp.k + 1, wp.k * wp.N + 1, l, (wp.k + 1) * wp.N)
        assert wk.pfpksk.size == int(np.prod(shape))
        for kind in ("generated", "00", "ff", "7f", "random"):
            key = np.array(wk.pfpksk) if kind == "generated" else \
                E.make_key(kind, shape[0] * shape[1], shape[3], logB, l, 64).reshape(-1)
            wsk.load_key(wopbs.KEY_PFPKSK, key)
            ow = oracle.OracleW(wp.as_tuple(), wk.bsk, wk.ksk, key)
            wide = wsk.circuit_bootstrap(small)
            narrow = wsk.circuit_bootstrap(small[:5])
            for r in (0, 1, 2, 3, 4, 15, 16, 63, 64, 69):
                want = ow.circuit_bootstrap(small[r])
                assert np.array_equal(wide[r], want), (kind, "batch of 70", r)
                if r < 5:
                    assert np.array_equal(narrow[r], want), (kind, "batch of 5", r)
    finally:
        wsk.close()


def test_refused_packing_decompositions(wop_side):
    _, sk = wop_side
    wp, _, _ = wopbs.wop_named_params("wop_toy_512")
    for l, logB in ((5, 2), (1, 31), (4, 16), (2, 1), (0, 15), (3, 22)):
        q = type(wp).from_buffer_copy(wp)
        q.pfks_l, q.pfks_logB = l, logB
        with pytest.raises(helm_amd.HelmError, match="bad packing-keyswitch decomposition"):
            wopbs.WopServerKey(sk, params=q)


def check_build_cases():
    """Every decomposition and batch-width case, and the geometry cases up to n = 48 (the tile edges).  Left out: n = 300
    and 1024 and the largest k N, for their time in a build without optimisation (the 64-bit engine's largest k N is a
    generic context, which the counting build refuses as well)."""
    cases = DECOMP32 + DECOMP64 + [c for c in GEOMETRY if c[1] <= 48 and c[2] == 1] + BATCH
    return [c for i, c in enumerate(cases) if c not in cases[:i]]      # n = 46 is in both lists


def child_main():
    res = {}
    for case in check_build_cases():
        res[_id(case)] = run_case(case, kinds=("follow", "random"), check_build=True)
        print("CASE " + _id(case), res[_id(case)], flush=True)
    print("RESULT " + json.dumps(res))


def test_counting_build_is_exact_and_counts_nothing():
    """The check build (libhelm_hip_check.so, -O0, every contract of the modular arithmetic counted) on the same launches:
    exact words - its keyswitch kernels are compiled without optimisation, another instruction stream for the same
    arithmetic - and every counter zero.  One child process; it ends at its first failure and is not retried."""
    lib = os.path.join(ROOT, "helm_amd", "csrc", "libhelm_hip_check.so")
    assert os.path.exists(lib), "make -C helm_amd/csrc libhelm_hip_check.so"
    env = dict(os.environ, HELM_HIP_LIB=lib)
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_keyswitch_edges as T; T.child_main()" % (ROOT, os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=900)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert len(res) == len(check_build_cases())
    bad = {k: v for k, v in res.items() if v != [0] * 8}
    assert not bad, bad
