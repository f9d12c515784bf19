"""The WoP packing keyswitch - k_pfpks64, and k_pfpks_digits + k_ks64_mfma on k_pfpks_planes' bytes - on chosen rows.

helm_wop_circuit_bootstrap_batch takes small LWE rows and keys; the rows its packing keyswitch decomposes are bootstrap
outputs.  tests/wop_program.py turns the bootstrapping key into a table of rows: under the programmed key, input row t runs
one CMUX step whose output IS a key row, word for word, at the targeted levels (and a power of two times it at the others).
So the device's packing keyswitch reads the crafted rows of tests/ks_edges.py - the largest and smallest digit sum, the
largest sum of magnitudes (digits of +-2^14 at logB 15: the two-byte split's hi = +-64), 0, 2^64 - 1, 2^63, 2^63 - 1, every tie
(digits of B/2 at logB 21 and 30, which uniform rows never show) - beside uniform control rows, under packing keys of
0x00 / 0xFF / 0x80 / 0x7F bytes, the sign-following key and uniform words.  Every word of every GGSW must equal the integer
reference (ks_edges.keyswitch_exact on wop_program.predicted_rows: Python integers, nothing of the library); the CPU
oracle's circuit bootstrap agrees on a sample of the steps (on all of them in tests/test_keyswitch_edges.py); the run with
HELM_HIP_KS_MFMA unset and the run with it 0 agree with each other.  Control steps failing: this file's layout; crafted
steps failing alone: a fault at the edge.

Widths are in bootstraps X = bits x cbs_l (cbs_l is 2 or 3, so 1, 5 and 65 do not occur as X: they are run as bit counts, and
the switch to the matrix cores at X >= 64 is bracketed by 62 / 64 / 66 at cbs_l = 2 and 63 / 66 at cbs_l = 3).  Crafted rows sit
at positions 0, 15, 16, 63, 64 and in the last, partly filled 16-row tile wherever that position is a targeted level
(wop_program.steps_for).  The launch rules - which kernel, how many slices - are wop_program's restatements, pinned to the
source text by tests/test_keyswitch_edges.py; the ABI does not report them.  DESIGN.md section 2, "Keyswitch at its edges"."""
import contextlib
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
import ks_edges as E  # noqa: E402
import wop_program as W  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC = len(E.CRAFTED)


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


@pytest.fixture(scope="module")
def n_cus():
    """The device's compute units, read as tests/test_gpu_parity.py reads them (the import of torch is most of this file's
    time when it runs alone)."""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def pbs_side():
    sk = helm_amd.SiServerKey(params=si_named_params("si_toy_512")[0])     # a tuned k = 1 context; no key is needed
    assert sk.kernel_class() == "tuned"
    yield sk
    sk.close()


def wop_params(shape, l, logB):
    p, _, _ = wopbs.wop_named_params("wop_toy_512")
    p.n, p.N, p.pbs_l, p.pbs_logB, p.cbs_l, p.cbs_logB = shape
    p.pfks_l, p.pfks_logB = l, logB
    assert p.k == 1 and W.shape_of(p) == shape
    return p


def packing_key(kind, N, l, logB):
    """[k+1][k N + 1][l][(k+1) N]"""
    return E.make_key(kind, 2 * (N + 1), 2 * N, logB, l, 64).reshape(2, N + 1, l, 2 * N)


_refs = {}


def reference(prog, N, l, logB, kinds):
    """Once per process: the programme, and per packing key the GGSW words of every step -> [n][cbs_l][k+1][(k+1) N]."""
    key = (prog, N, l, logB)
    if key not in _refs:
        shape, bsk, small, where = W.crafted_programme(prog, N, l, logB)
        pred = W.predicted_rows(shape, bsk, np.arange(shape.n))
        cr = E.crafted_rows(N, logB, l, 64)
        for (i, j), r in where.items():                                          # the targeted rows ARE the crafted rows
            assert np.array_equal(pred[i, j, :N], cr[r, :N]), (prog, i, j)
        _refs[key] = (shape, bsk, small, where, pred, {})
    shape, bsk, small, where, pred, want = _refs[key]
    for kind in kinds:
        if kind not in want:
            pf = packing_key(kind, N, l, logB)
            flat = pred.reshape(-1, N + 1)
            want[kind] = np.stack([W.packing_reference(flat, pf[r], l, logB) for r in range(2)], axis=1).reshape(
                shape.n, shape.cbs_l, 2, 2 * N)
    return _refs[key]


def _check(got, want, steps, label):
    if np.array_equal(got, want):
        return
    bad = sorted({int(t) for t in np.argwhere(got != want)[:, 0]})
    t, j, r, c = np.argwhere(got != want)[0]
    first = "bit %d (step %d) level %d key %d word %d: got %#x, want %#x" % (t, steps[t], j, r, c, int(got[t, j, r, c]), int(want[t, j, r, c]))
    bad_ctl = [t for t in bad if steps[t] >= NC]
    assert not bad_ctl, f"{label}: control steps at bits {bad_ctl[:8]} differ ({first}): the layout of this test?"
    assert not bad, f"{label}: crafted steps at bits {bad[:8]} differ while every control step is exact: wrong at the edge; {first}"


def run_case(pbs_side, prog, N, l, logB, bit_counts, kinds=E.KEYS, modes=(None, "0"), oracle_steps=(2, NC)):
    """Every bit count under every packing key with HELM_HIP_KS_MFMA at each of `modes`: all words against the reference,
    the modes against each other, the oracle on `oracle_steps` (abs_max and a control) and one further crafted step per key.
    -> {(mode, bits): X} of what ran"""
    shape, bsk, small, where, pred, want = reference(prog, N, l, logB, kinds)
    p = wop_params(shape, l, logB)
    levels = W.targeted_levels(shape)
    label = "%s N%d pfks (%d, %d)" % (prog, N, l, logB)
    launches = {bits: W.steps_for(bits, shape.cbs_l, levels)[0] for bits in bit_counts}
    for q, kind in enumerate(kinds):
        ow = oracle.OracleW(p.as_tuple(), bsk.reshape(-1), np.zeros(1, np.uint64), packing_key(kind, N, l, logB).reshape(-1))
        for i in tuple(oracle_steps) + ((q + 3) % NC,):
            assert np.array_equal(ow.circuit_bootstrap(small[i]), want[kind][i]), (label, kind, "oracle, step", i)
    got, ran = {}, {}
    for mode in modes:
        with _env(HELM_HIP_KS_MFMA=mode):
            wsk = wopbs.WopServerKey(pbs_side, params=p)
        try:
            wsk.load_key(wopbs.KEY_BSK, bsk)
            wsk.load_key(wopbs.KEY_KSK, np.zeros(N * p.ks_l * (p.n + 1), dtype=np.uint64))   # demanded, not used
            for kind in kinds:
                wsk.load_key(wopbs.KEY_PFPKSK, packing_key(kind, N, l, logB))
                for bits, steps in launches.items():
                    X = bits * shape.cbs_l
                    out = wsk.circuit_bootstrap(small[steps])
                    _check(out, want[kind][steps], steps, "%s key %s, %d bits = %d bootstraps, KS_MFMA=%s (%s)" %
                           (label, kind, bits, X, mode, W.pfpks_route(X, logB, N, mode)))
                    got[(mode, kind, bits)] = out
                    ran[(mode, bits)] = X
        finally:
            wsk.close()
    if len(modes) == 2:
        for kind in kinds:
            for bits in bit_counts:
                assert np.array_equal(got[(modes[0], kind, bits)], got[(modes[1], kind, bits)]), (label, kind, bits)
    return ran


def wide(cbs_l):
    """The narrowest bit count whose bootstraps reach the matrix cores, past a whole 64-row tile: 66 bootstraps."""
    return 33 if cbs_l == 2 else 22


@pytest.mark.parametrize("prog", list(W.PROGRAMMES))
@pytest.mark.parametrize("l,logB", W.PFKS, ids=lambda v: str(v))
def test_decompositions(pbs_side, prog, l, logB):
    """The nine packing decompositions x the six packing keys, N = 512, 5 bits (k_pfpks64, sliced) and 66 bootstraps (the
    matrix cores where the loader builds byte planes, logB <= 15; k_pfpks64 above), each with the matrix cores on and off."""
    cbs_l = W.PROGRAMMES[prog][2]
    ran = run_case(pbs_side, prog, 512, l, logB, (5, wide(cbs_l)))
    assert W.pfpks_route(ran[(None, 5)], logB, 512, None) == "valu"
    assert W.pfpks_route(ran[(None, wide(cbs_l))], logB, 512, None) == ("mfma" if logB <= 15 else "valu")
    assert W.pfpks_route(ran[("0", wide(cbs_l))], logB, 512, "0") == "valu"


# bit counts -> bootstraps: cbs_l = 2: 2, 10, 62, 64, 66, 130, 160; cbs_l = 3: 3, 15, 63, 66, 162, 195
BITS = {2: (1, 5, 31, 32, 33, 65, 80), 3: (1, 5, 21, 22, 54, 65)}


@pytest.mark.parametrize("prog", list(W.PROGRAMMES))
@pytest.mark.parametrize("l,logB", [(2, 15), (3, 15)], ids=lambda v: str(v))
def test_batch_widths(pbs_side, prog, l, logB):
    """Both sides of the switch to the matrix cores (X >= 64, rows padded to a multiple of 64): 62, 63 | 64, 66, one bit, five
    bits, 65 bits and 160 / 162 bootstraps; (3, 15) for the level count padded to 4."""
    cbs_l = W.PROGRAMMES[prog][2]
    ran = run_case(pbs_side, prog, 512, l, logB, BITS[cbs_l], kinds=("follow", "random"))
    routes = {X: W.pfpks_route(X, logB, 512, None) for (mode, _), X in ran.items() if mode is None}
    assert {X for X, r in routes.items() if r == "valu"} == ({2, 10, 62} if cbs_l == 2 else {3, 15, 63})
    assert {64 if cbs_l == 2 else 66, 160 if cbs_l == 2 else 162} <= {X for X, r in routes.items() if r == "mfma"}


@pytest.mark.parametrize("prog", list(W.PROGRAMMES))
@pytest.mark.parametrize("l,logB,modes", [(2, 15, ("0",)), (2, 30, (None,)), (3, 21, (None,))],
                         ids=["(2, 15)-matrix-cores-off", "(2, 30)", "(3, 21)"])
def test_the_unsliced_launch(pbs_side, n_cus, prog, l, logB, modes):
    """k_pfpks64 with gridDim.z == 1 (the plain store *dst = 0 - acc): the grid ceil(X / 4) x (k+1) N / 256 reaches two
    workgroups per compute unit - at N = 512, X >= 2 n_cus - so launch_pfpks takes one slice.  Once below the byte planes'
    limit with the matrix cores off, once each at logB 30 and at rep 63, where no planes exist.  Under each key a sliced
    launch two bits narrower runs first and leaves its words - uniform ones under the uniform key, which goes first - in the
    rows the unsliced launch then has to overwrite: a store that adds shows (with the sign-following key first it did
    not at an even level count, where that key is all zeros)."""
    cbs_l = W.PROGRAMMES[prog][2]
    cus = n_cus
    bits = -(-2 * cus // cbs_l)
    X = bits * cbs_l
    assert X >= 2 * cus and W.pfpks_slices(X, 512, cus) == 1                     # (X + 3) / 4 x 4 >= 2 n_cus
    assert W.pfpks_slices(X - cbs_l - 3, 512, cus) == 2 and W.pfpks_slices(66, 512, cus) > 1
    assert W.pfpks_route(X, logB, 512, modes[0]) == "valu" and W.pfpks_slices((bits - 2) * cbs_l, 512, cus) == 2
    ran = run_case(pbs_side, prog, 512, l, logB, (bits - 2, bits), kinds=("random", "follow"), modes=modes)
    assert ran[(modes[0], bits)] == X


@pytest.mark.parametrize("prog,N,l,logB", [("l2", 1024, 2, 15), ("l3_2", 1024, 3, 15), ("l3_2", 2048, 2, 15)],
                         ids=lambda v: str(v))
def test_larger_rings(pbs_side, prog, N, l, logB):
    """N = 1024: 1025 input words, 65 k-chunks of 64 virtual rows with the last one nearly empty (N = 512: 33); N = 2048 at the
    named sets' (2, 15) under their own pbs (2, 15) / cbs (3, 5)."""
    cbs_l = W.PROGRAMMES[prog][2]
    run_case(pbs_side, prog, N, l, logB, (5, wide(cbs_l)), kinds=("follow", "random"), oracle_steps=(2,))


def test_refused_programmes():
    """What the device tests rely on the helper to refuse (the CPU file has the rest)."""
    with pytest.raises(ValueError, match="has no digit"):
        W.program(W.Shape(12, 512, 2, 5, 3, 5), [(0, 2, np.zeros(513, np.uint64))])


# ------------------------------------------------------------------------------------------------------------------
# the bound-counting build
# ------------------------------------------------------------------------------------------------------------------
CHECK_CASES = [(prog, l, logB) for l, logB in ((2, 15), (4, 15), (3, 21)) for prog in W.PROGRAMMES]


def child_main():
    sk = helm_amd.SiServerKey(params=si_named_params("si_toy_512")[0])
    res = {}
    for prog, l, logB in CHECK_CASES:
        name = "%s-%d-%d" % (prog, l, logB)
        sk.bound_violations(reset=True)
        run_case(sk, prog, 512, l, logB, (5, 65), kinds=("follow", "random"), oracle_steps=())
        res[name] = sk.bound_violations()
        print("CASE", name, res[name], flush=True)
        assert res[name] == [0] * 8, (name, res[name])
    print("RESULT " + json.dumps(res))
    sk.close()


def test_counting_build_is_exact_and_counts_nothing():
    """The check build (libhelm_hip_check.so, -O0: another instruction stream for the same arithmetic, every contract of the
    modular arithmetic counted) on the N = 512 cases at (2, 15), (4, 15) and (3, 21), 5 and 65 bits: exact words, every counter
    zero.  One child process; it ends at its first failure and is not retried."""
    lib = os.path.join(ROOT, "helm_amd", "csrc", "libhelm_hip_check.so")
    assert os.path.exists(lib), "make -C helm_amd/csrc libhelm_hip_check.so"
    env = dict(os.environ, HELM_HIP_LIB=lib)
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_wop_programmed_rows as T; T.child_main()" % (
        ROOT, os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert len(res) == len(CHECK_CASES) and all(v == [0] * 8 for v in res.values()), res
