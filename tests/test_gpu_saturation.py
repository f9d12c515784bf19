"""Every blind-rotate kernel on bootstraps whose one CMUX step is aligned to the kernel's exactness bound.

tests/saturation.py builds, for any shape, a key and LWE rows under which exactly two blind-rotation steps are active: the
first writes a chosen accumulator, the second multiplies digits of the largest magnitudes with key polynomials of the largest
words, all signs aligned, so that one coefficient of every column sum reaches 0.98 - 1.00 of what the capacity checks of
helm_hip_ctx_create / helm_si_ctx_create_ex bound (tests/test_saturating_inputs.py asserts that on the CPU, from exact
integers).  Each launch holds the positive extreme, the negative extreme, a one-column variant and honest random rows
under the same key (controls: a failure of the saturating rows alone is an error at the bound, a failure of the controls
too is a key-layout error of this test).  The saturating rows must equal saturation.py's integer reference AND the
schoolbook oracle, the controls the oracle; no tolerance anywhere.  The cases are explicit lists of (shape, forced build,
field); each asserts kernel_class() and field_bits(), so none can silently run on another kernel.

Keys that follow the loaded key (N = 1024 boolean: the lazy field FpI; k_pbs64k at N = 512: the 46-bit CRT pair) are
placed just under and just over the loaders' thresholds.  One child process repeats every case the bound-counting build
(libhelm_hip_check.so) admits and requires all of its counters at zero.

The multi-bit kernels (k_pbs64s<., true>, k_pbs64_generic<LOGN, 2 | 3>), whose group sums need another construction, have
theirs: tests/saturation_mb.py, tests/test_gpu_multibit_saturation.py.  The keyswitch has its own edge construction: tests/ks_edges.py, tests/test_gpu_keyswitch_edges.py.  This
file runs MODE 0 of k_pbs64 only (pbs_l 1 and 2); MODE 1 and MODE 2 - the blind rotation and the CMUX tree of vertical packing,
with Pbs64Cfg<., 3> and cbs_logB - have theirs: tests/vp_edges.py, tests/test_gpu_vertical_packing_edges.py."""
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helm_amd
import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import saturation as S  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEAR32, NEAR32_RATIO = S.nearest_capacity_shape(32, 16)   # k = 2, N = 256, l = 1, logB = 10: 0.9867 of FpH's half
NEAR64, NEAR64_RATIO = S.nearest_capacity_shape(64, 12)   # k = 10, N = 256, l = 1, logB = 24: 0.9764 of p0 p1 / 2
FPI = ("FpI", S.FPI_RATIO * S.HALF_FPI)                   # a budget: the key sits at 0.997 of FpI's half
J46 = ("46", S.PAIR46_RATIO * S.HALF_46 / 1.05)

# (shape name or Shape, HELM_HIP_PBS_VARIANT or None, HELM_HIP_FIELD or None, key budget or None, field_bits, kernel_class)
CASES32 = (
    [("toy_k2", v, None, None, 49, "tuned") for v in (None, 4, 5, 6, 7, 9)] + [("toy_k2", 10, None, None, 51, "tuned")] +
    [("toy", v, None, None, 51, "tuned") for v in (None, 4, 5, 6, 7, 10)] +
    [("toy_1024", v, None, FPI, 50, "tuned") for v in (None, 4, 5, 6, 7, 9, 8)] +
    [("toy_1024", v, "51", None, 51, "tuned") for v in (None, 4, 5, 6, 7, 9, 8, 10)] +
    [("toy_1024_l2", v, None, FPI, 50, "tuned") for v in (None, 4, 5, 6, 9, 8)] +
    [("toy_1024_l2", v, "51", None, 51, "tuned") for v in (None, 4, 5, 6, 9, 8, 10)] +
    [(s, None, None, None, 51, "generic") for s in S.GENERIC32 + [NEAR32]])
# (shape name or Shape, generic mode, HELM_SI_FIELD or None, key budget or None, field_bits, kernel_class)
CASES64 = (
    [(name, None, None, None, 49, "tuned") for name in S.NAMED64] +
    [("si_toy_512_k3", None, None, J46, 46, "tuned"), ("si_toy_512_k3", None, "49", J46, 49, "tuned"),
     ("si_toy_512_k2", None, "49", None, 49, "tuned")] +
    [(name, "force", None, None, 49, "generic") for name in S.NAMED64] +
    [(s, "allow", None, None, 49, "generic") for s in S.GENERIC64 + [NEAR64]])


def _id(case):
    s, build, field, budget = case[:4]
    name = s if isinstance(s, str) else "k%d_N%d_l%d_B%d" % s[1:]
    return "-".join([name] + [f"{k}{v}" for k, v in (("build_", build), ("field_", field)) if v is not None] +
                    ([budget[0] + "_budget"] if budget else []))


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


_keys = {}


def _client_key(s, width):
    """The generated key of the shape (the untouched steps of every crafted key hold its words)."""
    if (s, width) not in _keys:
        if width == 32:
            if isinstance(s, str):
                ck = helm_amd.ClientKey.generate(s, seed=11)
            else:
                p, _, _ = helm_amd.named_params("toy")
                p.n, p.k, p.N, p.pbs_l, p.pbs_logB, p.ks_l, p.ks_logB = s.n, s.k, s.N, s.l, s.logB, 4, 4
                ck = helm_amd.ClientKey(p, 1e-7, 1e-9, seed=7)
        elif isinstance(s, str):
            ck = helm_amd.SiClientKey.generate(s, seed=3)
        else:
            p, _, _ = helm_amd.si_named_params("si_toy_512")
            p.n, p.k, p.N, p.pbs_l, p.pbs_logB, p.ks_l, p.ks_logB = s.n, s.k, s.N, s.l, s.logB, 4, 4
            p.message_modulus, p.carry_modulus = 4, 4
            ck = helm_amd.SiClientKey(p, 1e-9, 1e-16 if s.N == 2048 else 1e-15, seed=7)
        _keys[(s, width)] = ck
    return _keys[(s, width)]


_launches = {}


def _launch(s, width, budget, rows):
    """The crafted key, the rows of one launch and their references: 3 saturating rows, then honest random rows."""
    key = (s, width, budget, rows)
    if key not in _launches:
        ck = _client_key(s, width)
        shape = S.shape_of(ck.params)
        case = S.launch_case(shape, width, ck.bsk, budget=None if budget is None else int(budget[1]))
        dt = np.uint32 if width == 32 else np.uint64
        rng = np.random.default_rng(17)
        lwe = rng.integers(0, 1 << width, size=(rows, shape.n + 1), dtype=dt)
        lwe[:3] = case["lwe"]
        tvs = np.stack([case["tv"], rng.integers(0, 1 << width, size=shape.N, dtype=dt)])
        idx = np.array([0, 0, 0] + [1 - g % 2 for g in range(3, rows)], dtype=np.int32)
        if width == 32:
            args = (ck.params.as_tuple7(), case["bsk"], ck.ksk)
            school, ntt = oracle.Oracle(*args, use_ntt=False).bootstrap_noks, oracle.Oracle(*args, use_ntt=True).bootstrap_noks
        else:
            args = (ck.params.as_tuple(), case["bsk"], ck.ksk)
            school, ntt = oracle.Oracle64(*args, use_ntt=False).bootstrap, oracle.Oracle64(*args, use_ntt=True).bootstrap
        want = np.stack([school(lwe[g], tvs[idx[g]]) if g < 5 else ntt(lwe[g], tvs[idx[g]]) for g in range(rows)])
        # the integer reference and the schoolbook oracle agree on the saturating rows (pinned on the CPU as well)
        assert np.array_equal(want[:3], case["ref"])
        _launches[key] = (ck, case["bsk"], lwe, tvs, idx, want, case["peak"])
    return _launches[key]


def _compare(got, want, label):
    bad_sat = [g for g in range(3) if not np.array_equal(got[g], want[g])]
    bad_ctl = [g for g in range(3, len(want)) if not np.array_equal(got[g], want[g])]
    assert not bad_ctl, f"{label}: control rows {bad_ctl} differ (saturating rows differing: {bad_sat}): key layout of the test?"
    assert not bad_sat, f"{label}: saturating rows {bad_sat} differ while every control row is exact: wrong at the bound"


def run32(case, check_build=False):
    s, build, field, budget, want_field, want_class = case
    rows = 11 if build == 9 else 9    # full workgroups and a partial one in every build (tests/test_gpu_parity.py)
    ck, bsk, lwe, tvs, idx, want, _ = _launch(s, 32, budget, rows)
    with _env(HELM_HIP_PBS_VARIANT=build, HELM_HIP_FIELD=field):
        sk = helm_amd.ServerKey(params=ck.params, bsk=bsk, ksk=ck.ksk)   # a build the shape does not have is refused here
        assert os.environ.get("HELM_HIP_PBS_VARIANT") == (None if build is None else str(build))
    try:
        assert sk.kernel_class() == want_class and sk.field_bits() == want_field, (sk.kernel_class(), sk.field_bits())
        if check_build:
            sk.bound_violations(reset=True)
        got = sk.pbs_batch(lwe, tvs, idx)
        _compare(got, want, _id(case))
        assert sk.field_bits() == want_field
        return sk.bound_violations() if check_build else None
    finally:
        sk.close()


def run64(case, check_build=False):
    s, generic, field, budget, want_field, want_class = case
    ck, bsk, lwe, tvs, idx, want, _ = _launch(s, 64, budget, 9)
    with _env(HELM_SI_FIELD=field):
        sk = helm_amd.SiServerKey(params=ck.params, bsk=bsk, ksk=ck.ksk, generic=generic)
    try:
        assert sk.kernel_class() == want_class and sk.field_bits() == want_field, (sk.kernel_class(), sk.field_bits())
        if check_build:
            sk.bound_violations(reset=True)
        got = sk.pbs_batch(lwe, tvs, idx)
        _compare(got, want, _id(case))
        return sk.bound_violations() if check_build else None
    finally:
        sk.close()


@pytest.mark.parametrize("case", CASES32, ids=[_id(c) for c in CASES32])
def test_boolean_kernels_at_the_bound(case):
    run32(case)


@pytest.mark.parametrize("case", CASES64, ids=[_id(c) for c in CASES64])
def test_shortint_kernels_at_the_bound(case):
    run64(case)


def test_the_nearest_admitted_shapes_are_what_the_docstrings_say():
    assert NEAR32 == S.Shape(16, 2, 256, 1, 10) and abs(NEAR32_RATIO - 0.9867) < 1e-4
    assert NEAR64 == S.Shape(12, 10, 256, 1, 24) and abs(NEAR64_RATIO - 0.9764) < 1e-4
    # one step further is refused by the capacity checks
    p = _client_key(NEAR32, 32).params
    p2 = type(p).from_buffer_copy(p)
    p2.pbs_logB += 1
    with pytest.raises(helm_amd.HelmError, match="single-prime NTT capacity"):
        helm_amd.ServerKey(params=p2)
    q = _client_key(NEAR64, 64).params
    q2 = type(q).from_buffer_copy(q)
    q2.k += 1
    with pytest.raises(helm_amd.HelmError, match="two-prime NTT capacity"):
        helm_amd.SiServerKey(params=q2, generic="allow")


# the key-following fields: a key just under the loader's threshold takes the lazy field and must be exact there at its own
# bound; just over, the safe field
THRESHOLD32 = [(0.997, 50), (0.999, 51), (1.01, 51)]      # x FpI's half; the loader asks bound x 1.002 < p/2
THRESHOLD64 = [(0.95, 46), (1.001, 49)]                   # x (p p'/2) / 1.05; the loader asks bound x 1.05 < p p'/2


@pytest.mark.parametrize("ratio,field", THRESHOLD32)
def test_n1024_field_at_the_threshold(ratio, field):
    run32(("toy_1024", None, None, ("FpI%g" % ratio, ratio * S.HALF_FPI), field, "tuned"))


@pytest.mark.parametrize("ratio,field", THRESHOLD64)
def test_k_pbs64k_crt_pair_at_the_threshold(ratio, field):
    run64(("si_toy_512_k3", None, None, ("J%g" % ratio, ratio * S.HALF_46 / 1.05), field, "tuned"))


def check_build_cases():
    """Every case above except the generic 64-bit contexts, which the counting build refuses (tests/test_gpu_si_generic_shapes.py
    keeps that refusal's test)."""
    c32 = CASES32 + [("toy_1024", None, None, ("FpI%g" % r, r * S.HALF_FPI), f, "tuned") for r, f in THRESHOLD32]
    c64 = [c for c in CASES64 if c[5] == "tuned"] + \
        [("si_toy_512_k3", None, None, ("J%g" % r, r * S.HALF_46 / 1.05), f, "tuned") for r, f in THRESHOLD64]
    return c32, c64


def child_main():
    """Runs in the child process of test_counting_build_counts_nothing_at_the_bound: stops at the first failure."""
    c32, c64 = check_build_cases()
    res = {}
    for run, cases in ((run32, c32), (run64, c64)):
        for case in cases:
            res[_id(case) + ("/64" if run is run64 else "/32")] = run(case, check_build=True)
            print("CASE " + _id(case), res[_id(case) + ("/64" if run is run64 else "/32")], flush=True)
    print("RESULT " + json.dumps(res))


def test_counting_build_counts_nothing_at_the_bound():
    """The check build (libhelm_hip_check.so, -DHELM_CHECK_BOUNDS: mulmod / reduce operands, butterfly sums and lifted values
    counted inside the kernels) on the saturating launches: bit-exact and every counter zero - the first inputs that can
    approach what those counters watch.  One child process; it ends at its first failure and is not retried."""
    lib = os.path.join(ROOT, "helm_amd", "csrc", "libhelm_hip_check.so")
    assert os.path.exists(lib), "make -C helm_amd/csrc libhelm_hip_check.so"
    env = dict(os.environ, HELM_HIP_LIB=lib)
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_saturation as T; T.child_main()" % (ROOT, os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=1500)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    c32, c64 = check_build_cases()
    assert len(res) == len(c32) + len(c64)
    bad = {k: v for k, v in res.items() if v != [0] * 8}
    assert not bad, bad
