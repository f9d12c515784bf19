"""Vertical packing (k_pbs64<Pbs64Cfg<LOGN, cbs_l>, 1> and <., 2>, helm_wopbs.inc launch_vp) on every built shape, with GGSWs
no circuit bootstrap produces.

tests/vp_edges.py builds the launches and their exact integer reference (tests/test_vp_edges.py pins it against both CPU
oracle routes and asserts what the crafted gates reach); helm_wop_vertical_packing_batch needs no key, so the contexts here
have none.  Every row must equal the integer reference AND the schoolbook oracle, word for word.

Which gate exercises which kernel.  Every gate of a launch with bits > log2 N passes through both kernels: the CMUX tree is
k_pbs64<., 2> (one launch per tree level), the blind rotation and sample extraction k_pbs64<., 1>.  In the launch of seven
(vp_edges.crafted_launch, bits = log2 N + 2):
  gates 0, 1, 2   tree-saturating (positive, negative, mask column only): the level-1 CMUX of MODE 2 has one coefficient of
                  each column sum at the digit rule's maximum x (k+1) N 2^63; MODE 1 sees zero GGSWs (passes through)
  gates 3, 4      rotation step 0 and step log2 N - 1 saturated the same way: MODE 1 at the extreme; MODE 2 programs the
                  accumulator (level 0) and passes it through a zero GGSW (level 1)
  gates 5, 6      controls, uniform words everywhere: both modes on honest-sized sums
The six (LOGN, cbs_l) pairs come from the six contexts' own parameters - launch_vp has no other route - so the twelve kernels
each run at least three crafted gates and two controls.

Further: the decompositions at the ends of what helm_wop_ctx_create admits (cbs_logB = 1, where the one-addition digit rule
has B/2 - 1 = 0; logB l = 30), the depth edges (one bit; log2 N bits = no tree; log2 N + 6 bits = six ping-pong levels with
three gates), the crafted gates at both ends of a batch of seven (the per-gate key offset), the refusals, and one child
process on the bound-counting build (libhelm_hip_check.so) that repeats the six per-shape launches and requires every
counter at zero.

Out of scope: the sharded form of helm_wop_eval_luts (its chunk boundary: tests/test_gpu_wopbs.py); multi-bit saturation."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helm_amd
import oracle
from helm_amd import wopbs
from helm_amd.shortint import si_named_params

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vp_edges as V  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE_CASES = ["shape-" + V._name(v) for v in V.SHAPES]


def wop_params(v):
    p, _, _ = wopbs.wop_named_params("wop_toy_512")
    p.N, p.cbs_l, p.cbs_logB = v.N, v.l, v.logB
    return p


_contexts = {}


@pytest.fixture(scope="module")
def pbs_side():
    sk = helm_amd.SiServerKey(params=si_named_params("si_toy_512")[0])     # a tuned k = 1 context; no key is needed
    assert sk.kernel_class() == "tuned"
    yield sk
    for w in _contexts.values():
        w.close()
    _contexts.clear()
    sk.close()


def _context(pbs_side, v):
    if v not in _contexts:
        _contexts[v] = wopbs.WopServerKey(pbs_side, params=wop_params(v))
    return _contexts[v]


_wants = {}


def _want(name):
    """The launch and the schoolbook oracle's rows, once per process; the integer reference must agree with them."""
    if name not in _wants:
        L = V.launch(name)
        v = L["v"]
        want = np.stack([oracle.Ggsw(v.N, 1, v.l, v.logB, L["stacks"][g][::-1], use_ntt=False)  # most significant first
                         .vertical_packing(L["bits"], L["tables"][g]) for g in range(len(L["ref"]))])
        assert np.array_equal(want, L["ref"]), name
        _wants[name] = (L, want)
    return _wants[name]


def _compare(got, L, want, label):
    crafted = [g for g, gate in enumerate(L["gates"]) if gate["sat"] is not None]
    bad = [g for g in range(len(want)) if not np.array_equal(got[g], want[g])]
    kinds = {g: L["gates"][g]["kind"] for g in bad}
    bad_ctl = [g for g in bad if g not in crafted]
    assert not bad_ctl, f"{label}: control gates {bad_ctl} differ (all differing: {kinds}): GGSW / table layout of the test?"
    assert not bad, f"{label}: crafted gates {kinds} differ while every control is exact: wrong at the extreme"


def run(wsk, name):
    L, want = _want(name)
    got = wsk.vertical_packing(L["stacks"], L["tables"])
    _compare(got, L, want, name)


@pytest.mark.parametrize("name", SHAPE_CASES)
def test_every_built_shape(pbs_side, name):
    """(LOGN, cbs_l) in {9, 10, 11} x {2, 3}: both modes of the shape's kernel, crafted gates and controls in one launch."""
    run(_context(pbs_side, V.launch(name)["v"]), name)


@pytest.mark.parametrize("name", [n for n in V.CASES if n.startswith("decomposition-")])
def test_decomposition_edges(pbs_side, name):
    run(_context(pbs_side, V.launch(name)["v"]), name)


@pytest.mark.parametrize("name", [n for n in V.CASES if n.startswith("depth-")])
def test_depth_edges(pbs_side, name):
    """bits = 1; bits = log2 N (no tree); bits = log2 N + 6 with three gates (six ping-pong levels).  Controls only."""
    run(_context(pbs_side, V.launch(name)["v"]), name)


@pytest.mark.parametrize("name", [n for n in V.CASES if n.startswith("batch-")])
def test_crafted_gates_at_both_ends_of_a_batch_of_seven(pbs_side, name):
    L = V.launch(name)
    assert len(L["ref"]) == 7 and L["gates"][0]["sat"] is not None and L["gates"][-1]["sat"] is not None
    assert [g["sat"] is None for g in L["gates"]].count(True) == 2 and L["gates"][1]["sat"] is None
    run(_context(pbs_side, L["v"]), name)


def test_refusals(pbs_side):
    v = V.VShape(512, 2, 8)
    wsk = _context(pbs_side, v)
    for bits in (0, 9 + 7):
        stack = np.zeros((1, max(bits, 1), v.l, 2, 2 * v.N), dtype=np.uint64)
        tables = np.zeros((1, wsk.table_words(bits)), dtype=np.uint64)
        with pytest.raises(helm_amd.HelmError, match=r"error -1: vertical_packing: 1\.\.log2\(N\)\+6 bits"):   # HELM_ERR_INVALID
            if bits == 0:    # (the wrapper reads the bit count off the stack's shape)
                from helm_amd import _native as nv
                out = np.zeros((1, v.N + 1), dtype=np.uint64)
                nv.hip_check(nv.hip.helm_wop_vertical_packing_batch(wsk._h, nv.as_u64p(stack), 0, nv.as_u64p(tables),
                                                                    nv.as_u64p(out), 1))
            else:
                wsk.vertical_packing(stack, tables)
    for l, logB in ((1, 8), (4, 5), (2, 16), (3, 0), (2, 0)):
        with pytest.raises(helm_amd.HelmError, match="error -1: WoP-PBS: circuit-bootstrap levels must be 2 or 3"):
            wopbs.WopServerKey(pbs_side, params=wop_params(V.VShape(512, l, logB)))


# ------------------------------------------------------------------------------------------------------------------
# the bound-counting build
# ------------------------------------------------------------------------------------------------------------------
def child_main(path):
    """Runs in the child process of test_counting_build_counts_nothing: the six per-shape launches (read from the parent's
    file with the rows they must give), each exact and with all eight counters zero; stops at the first failure."""
    data = np.load(path)
    sk = helm_amd.SiServerKey(params=si_named_params("si_toy_512")[0])
    res = {}
    for name in SHAPE_CASES:
        v = V.VShape(*[int(x) for x in data[name + "/v"]])
        wsk = wopbs.WopServerKey(sk, params=wop_params(v))
        sk.bound_violations(reset=True)
        got = wsk.vertical_packing(data[name + "/stacks"], data[name + "/tables"])
        want = data[name + "/want"]
        bad = [g for g in range(len(want)) if not np.array_equal(got[g], want[g])]
        assert not bad, f"{name}: gates {bad} differ on the counting build"
        res[name] = sk.bound_violations()
        print("CASE", name, res[name], flush=True)
        wsk.close()
        assert res[name] == [0] * 8, (name, res[name])
    sk.close()
    print("RESULT " + json.dumps(res))


def test_counting_build_counts_nothing(tmp_path):
    """The check build (-O0, -DHELM_CHECK_BOUNDS: mulmod / reduce operands, butterfly sums and lifted values counted inside
    the kernels; one set of counters for the whole unit, read through the PBS-side key) on the six per-shape launches: the
    first inputs on which this kernel's three lazily summed products per column come near their bound.  One child process;
    it ends at its first failure and is not retried."""
    lib = os.path.join(ROOT, "helm_amd", "csrc", "libhelm_hip_check.so")
    assert os.path.exists(lib), "make -C helm_amd/csrc libhelm_hip_check.so"
    arrays = {}
    for name in SHAPE_CASES:
        L, want = _want(name)
        arrays.update({name + "/v": np.array(L["v"]), name + "/stacks": L["stacks"], name + "/tables": L["tables"],
                       name + "/want": want})
    path = str(tmp_path / "launches.npz")
    np.savez(path, **arrays)
    env = dict(os.environ, HELM_HIP_LIB=lib)
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_vertical_packing_edges as T; T.child_main(%r)" % (
        ROOT, os.path.join(ROOT, "tests"), path)
    p = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert sorted(res) == sorted(SHAPE_CASES) and all(v == [0] * 8 for v in res.values()), res
