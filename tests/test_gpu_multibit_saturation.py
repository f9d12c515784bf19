"""Both multi-bit blind-rotate kernels on bootstraps whose one group step is aligned to their exactness bound.

tests/saturation_mb.py builds, for a multi-bit shape, a key of three groups and the LWE row under which the first group writes a
chosen accumulator and the second multiplies digits of the largest magnitude with key polynomials of the largest words, the
2^g subsets of the group aligned after the kernel's monomial products, so that one coefficient of every column reaches the
bound helm_si_load_bootstrap_key admits a multi-bit key by: 0.998 of its threshold (p0 p1 / 2) / 1.001, that is 0.997 of the
half of the CRT pair (tests/test_multibit_saturating_inputs.py asserts that on the CPU, from exact integers).  Two keys per
shape: the positive extreme with group masks 0, the negative extreme with masks whose subset sums wrap past 2N.  Each launch
holds the saturating row, a row with every mask 0 and two controls (uniform words; every mask odd), and must equal
saturation_mb's integer reference word for word (the reference is pinned against both oracle routes on the CPU).  A failure
of the saturating row alone is an error at the bound; a failure of a control too is an error of the kernel anywhere, or a
key-layout error of this test.

The tuned build k_pbs64s<., true> runs its four instantiations (N = 1024, 2048; g = 2, 3), the generic kernel
k_pbs64_generic<LOGN, g> its eight; each case asserts kernel_class(), so none can silently run on the other kernel.  Two
shapes of more than one level, which cannot reach the threshold, run fully saturated for the digit rule's ties.  The loader's
threshold is probed from both sides on both kernels; one child process repeats the tuned cases under the bound-counting
build (libhelm_hip_check.so; it refuses generic contexts) and requires every counter at zero."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helm_amd
from helm_amd import _native as nv

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import saturation_mb as M  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (shape, SiServerKey's generic mode, kernel_class, budget ratio or None = fully saturated)
TUNED_CASES = [(s, None, "tuned", M.RATIO) for s in M.TUNED]
GENERIC_CASES = [(s, "force+multibit" if s in M.TUNED else "allow+multibit", "generic", M.RATIO) for s in M.GENERIC]
BELOW_CASES = [(s, "allow+multibit", "generic", None) for s in M.BELOW]
CASES = [(c, sign) for c in TUNED_CASES + GENERIC_CASES + BELOW_CASES for sign in (+1, -1)]


def _id(case, sign=None):
    s, mode, cls, ratio = case
    return "%s-%s%s%s" % (M.shape_id(s), cls, "" if ratio is not None else "-full", {None: "", 1: "+", -1: "-"}[sign])


def _params(s):
    p, _, _ = helm_amd.si_named_params("si_toy_512")
    p.n, p.k, p.N, p.pbs_l, p.pbs_logB, p.ks_l, p.ks_logB = 3 * s.g, s.k, s.N, s.l, s.logB, 4, 4
    p.message_modulus, p.carry_modulus, p.grouping_factor = 4, 4, s.g
    return p


def _ksk(s):
    return np.zeros(s.k * s.N * 4 * (3 * s.g + 1), dtype=np.uint64)


def _context(s, mode, cls, bsk=None):
    sk = helm_amd.SiServerKey(params=_params(s), bsk=bsk, ksk=_ksk(s), generic=mode)
    assert sk.kernel_class() == cls and sk.field_bits() == 49, (sk.kernel_class(), sk.field_bits())
    return sk


def _compare(got, want, label):
    bad = [r for r in range(len(want)) if not np.array_equal(got[r], want[r])]
    for r in bad:   # the first differing words of each row, for the record
        at = np.flatnonzero(got[r] != want[r])
        print(f"{label}: row {r} differs in {len(at)} of {len(want[r])} words; first at {at[:3].tolist()}: "
              f"got {[hex(int(v)) for v in got[r][at[:3]]]}, want {[hex(int(v)) for v in want[r][at[:3]]]}")
    assert not set(bad) & set(M.CONTROLS), f"{label}: a control row differs (rows differing: {bad}): key layout of the test?"
    assert not bad, f"{label}: rows {bad} differ while the control rows are exact: wrong at the bound"


def run(case, sign, columns="all", check_build=False):
    s, mode, cls, ratio = case
    L = M.launch(s, sign, columns=columns, ratio=ratio)
    sk = _context(s, mode, cls, L["bsk"])
    try:
        if check_build:
            sk.bound_violations(reset=True)
        got = sk.pbs_batch(L["lwe"], L["tv"])
        _compare(got, L["ref"], _id(case, sign))
        return sk.bound_violations() if check_build else got
    finally:
        sk.close()


@pytest.mark.parametrize("case,sign", CASES, ids=[_id(c, sg) for c, sg in CASES])
def test_multibit_kernels_at_the_bound(case, sign):
    run(case, sign)


@pytest.mark.parametrize("s", [s for s in M.GENERIC if s in M.TUNED], ids=M.shape_id)
def test_tuned_and_forced_generic_agree_on_the_identical_key(s):
    for sign in (+1, -1):
        assert np.array_equal(run((s, None, "tuned", M.RATIO), sign), run((s, "force+multibit", "generic", M.RATIO), sign))


@pytest.mark.parametrize("case", [TUNED_CASES[0], GENERIC_CASES[2]], ids=_id)
def test_one_column_variant(case):
    run(case, +1, columns=case[0].k // 2)


THRESHOLD_SHAPE = M.TUNED[0]


@pytest.mark.parametrize("mode,cls", [(None, "tuned"), ("force+multibit", "generic")])
def test_key_at_the_threshold(mode, cls):
    """A key at 0.998 of the loader's threshold loads and is exact; one at 1.002 is refused with "capacity" and the figure
    test_multibit_saturating_inputs.py derives for it; after the refusal a context that had a key runs with that key, and a
    context that had none gives HELM_ERR_STATE."""
    s = THRESHOLD_SHAPE
    L = M.launch(s, +1)
    over = M.saturating_key(s, [0] * s.g, ratio=1.002)["bsk"]
    assert M.printed_ratio(M.loader_bound(over, s)) == "1.001"
    sk = _context(s, mode, cls, L["bsk"])
    try:
        got = sk.pbs_batch(L["lwe"], L["tv"])
        _compare(got, L["ref"], "0.998 key, " + cls)
        rc = nv.hip.helm_si_load_bootstrap_key(sk._h, nv.as_u64p(over), over.size)
        err = nv.hip.helm_hip_last_error()
        assert rc == -1 and b"capacity" in err and b"1.001 of p0 p1 / 2" in err, (rc, err)
        assert np.array_equal(sk.pbs_batch(L["lwe"], L["tv"]), got)      # the old key, untouched
    finally:
        sk.close()
    sk = _context(s, mode, cls)
    try:
        rc = nv.hip.helm_si_load_bootstrap_key(sk._h, nv.as_u64p(over), over.size)
        assert rc == -1 and b"capacity" in nv.hip.helm_hip_last_error()
        with pytest.raises(helm_amd.HelmError, match="error -4"):        # HELM_ERR_STATE: no key is loaded
            sk.pbs_batch(L["lwe"], L["tv"])
    finally:
        sk.close()


def test_a_lane_of_the_tuned_context_gives_the_same_rows():
    s = M.TUNED[3]
    L = M.launch(s, -1)
    sk = _context(s, None, "tuned", L["bsk"])
    try:
        lane = sk.fork()
        assert lane.kernel_class() == "tuned"
        got = lane.pbs_batch(L["lwe"], L["tv"])
        _compare(got, L["ref"], "lane")
        assert np.array_equal(got, sk.pbs_batch(L["lwe"], L["tv"]))
    finally:
        sk.close()


def child_main():
    """Runs in the child process of test_counting_build_counts_nothing_at_the_bound: stops at the first failure."""
    res = {}
    for case in TUNED_CASES:
        for sign in (+1, -1):
            res[_id(case, sign)] = run(case, sign, check_build=True)
            print("CASE " + _id(case, sign), res[_id(case, sign)], flush=True)
    print("RESULT " + json.dumps(res))


def test_counting_build_counts_nothing_at_the_bound():
    """The check build (libhelm_hip_check.so, -DHELM_CHECK_BOUNDS: mulmod / reduce operands and butterfly sums counted
    inside the kernels) on the tuned cases: bit-exact and every counter zero.  One child process; it ends at its first failure
    and is not retried."""
    lib = os.path.join(ROOT, "helm_amd", "csrc", "libhelm_hip_check.so")
    assert os.path.exists(lib), "make -C helm_amd/csrc libhelm_hip_check.so"
    env = dict(os.environ, HELM_HIP_LIB=lib)
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_multibit_saturation as T; T.child_main()" % (
        ROOT, os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert len(res) == 2 * len(TUNED_CASES)
    bad = {k: v for k, v in res.items() if v != [0] * 8}
    assert not bad, bad
