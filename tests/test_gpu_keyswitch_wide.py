"""The keyswitch at large input dimensions under wide launches: the vector-ALU form's launch geometry
(helm_ks::vector_geometry, helm_amd/csrc/keyswitch.h) in every LDS band - at most 64 KiB of digits, between 64 and 160 KiB,
exactly 160 KiB, and more than 160 KiB unsliced, where the LDS clause slices - at 16, 4, 2 and 1 slices on both engines,
and the crafted rows and keys of tests/ks_edges.py at in_dim 4096 and 8192 of the 64-bit engine.

The cases are ks_edges.wide_cases(); tests/test_ks_geometry.py checks the table on the CPU at 256 compute units, and every
case asserts here, at the device's own count and before it launches, the band and the clause it was built for.  The
conventions are those of tests/test_gpu_keyswitch_edges.py: contexts from parameters and a crafted key alone, every case
with HELM_HIP_KS_MFMA unset and = 0 and the two compared word for word, control rows named apart from crafted rows, EVERY row
of every launch against ks_edges' integer reference (in chunks of 256 rows), no tolerance.  Within a context the uniform key
runs first and a context's launches follow each other on the same buffers, so a sliced launch whose rows were not cleared
adds to what the launch before it left.

Keyswitch-first gate levels (the third row source, GateKsRows) run one level wide enough for one slice on a generic shape
whose digits take 72 and 100 KiB, against the same gates in narrow levels (16 slices) and tests/ks_first.py's reference.

What the runtime answered ("Keyswitch at its edges"): the boolean engine sets no dynamic-LDS attribute
on its vector kernels, and its launches with 95,232, 126,976, 158,720 and exactly 163,840 B of dynamic LDS were taken and
computed every word right; so did the 64-bit engine's at exactly 163,840 B.  No engine code changed with this file."""
import os
import sys

import numpy as np
import pytest

import helm_amd
import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ks_edges as E  # noqa: E402
import ks_first as K  # noqa: E402
import test_gpu_keyswitch_edges as T  # noqa: E402  (its environment switch, loaders, oracle rows and comparison, unchanged)

pytestmark = pytest.mark.gpu
O = oracle
CASES = E.wide_cases()


@pytest.fixture(scope="module")
def n_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _params(case):
    if case.width == 32:
        return T._params(32, case.n, case.k, case.N, case.l, case.logB)
    name = {"large": "si_toy_4096", "n8192": "si_toy_8192"}[case.generic]       # pbs (1, 22) and (2, 15)
    p, _, _ = helm_amd.si_named_params(name)
    assert (p.k, p.N) == (case.k, case.N)
    p.n, p.ks_l, p.ks_logB = case.n, case.l, case.logB
    return p


def _server(case, p, key):
    if case.width == 32:
        return helm_amd.ServerKey(params=p, ksk=key)
    sk = helm_amd.SiServerKey(params=p, ksk=key, generic=case.generic)
    assert sk.kernel_class() == case.generic
    return sk


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_wide_launches(case, n_cus):
    width, n, kN, l, logB = case.width, case.n, case.kN, case.l, case.logB
    counts = case.counts(n_cus)
    geometry = case.geometry(n_cus)
    label = "%s: " % case.id + ", ".join("%d rows -> %d x %d B" % (c, g[2], g[4]) for c, g in zip(counts, geometry))
    print(label)
    assert case.bands(n_cus) == case.expect, label
    assert [g[2] for g in geometry] == [16 if s == "sweep" else 2 if b == "clause" else s
                                        for s, (b, _) in zip(case.slices, case.expect)], label
    for c in counts:
        assert T.route(width, kN, l, c, None) == ("mfma" if case.mfma0_only else "valu"), label
    p = _params(case)
    rows, controls = E.launch_rows(kN, logB, l, width, max(counts))             # a narrower launch is a prefix of it
    keys = {kind: E.make_key(kind, kN, n + 1, logB, l, width) for kind in case.kinds}
    want = E.keyswitch_exact_wide(rows, keys, logB, l, width)
    some = controls[:2]
    for kind in case.kinds[:2]:                                                 # the reference against the oracle, two rows
        assert np.array_equal(T._oracle_rows(width, p, keys[kind], rows[some]), want[kind][some]), label
    got = {}
    for mode in (None, "0"):
        with T._env(HELM_HIP_KS_MFMA=mode):
            sk = _server(case, p, keys[case.kinds[0]])
        try:
            for kind in case.kinds:
                T._reload(width, sk, keys[kind])
                for c in counts:
                    out = sk.keyswitch_batch(rows[:c])
                    T._compare(out, want[kind][:c], {g for g in controls if g < c}, "%s key %s batch %d KS_MFMA=%s (%s)" %
                               (label, kind, c, mode, T.route(width, kN, l, c, mode)))
                    got[(mode, kind, c)] = out
        finally:
            sk.close()
    for kind in case.kinds:
        for c in counts:
            assert np.array_equal(got[(None, kind, c)], got[("0", kind, c)]), (label, kind, c)


# ---------------------------------------------------------------------------------------------------------------------------
# keyswitch-first gate levels
# ---------------------------------------------------------------------------------------------------------------------------
BOOT = [O.AND, O.NAND, O.OR, O.NOR, O.XOR, O.XNOR, O.MUX]
NARROW = 32        # gates of a narrow level: at most 37 jobs, 10 workgroups - 16 slices


@pytest.mark.parametrize("shape", E.GATE_SHAPES, ids=lambda s: "k%dN%d-n%d-l%dB%d" % s)
def test_a_wide_gate_level_on_a_large_shape(shape, n_cus):
    """One level of 8 CUs + 4 gates, every seventh a MUX (two keyswitch jobs each), one of them updating its own row in place:
    one slice, 72 / 100 KiB of digits (ks_l = 3 and 5 have no matrix-core form: HELM_HIP_KS_MFMA changes nothing here).  Every
    row of the table equals the same gates in levels of 32 (16 slices, a few KiB of digits), and six rows - the first, the
    two either side of the first four-job workgroup's edge, a MUX, the in-place MUX, the last - the composed oracle."""
    k, N, n, l, logB = shape
    p, a, b = helm_amd.named_params("toy_1024_ks_pbs")
    p.n, p.k, p.N, p.pbs_l, p.pbs_logB, p.ks_l, p.ks_logB = n, k, N, 1, 5, l, logB
    assert p.pbs_order == 1
    kN = k * N
    ck = helm_amd.ClientKey(p, a, b, seed=5)
    G = 8 * n_cus + 4
    rng = np.random.default_rng(l)
    ops = np.array([BOOT[g % 7] for g in range(G)], dtype=np.int32)
    i0, i1 = rng.integers(0, 8, G).astype(np.int32), rng.integers(0, 8, G).astype(np.int32)
    i2 = np.where(ops == O.MUX, rng.integers(0, 8, G), -1).astype(np.int32)
    out = np.arange(9, 9 + G, dtype=np.int32)
    IN_PLACE = 13                                   # row 8 = row 2 ? row 0 : row 8; no other gate reads row 8
    assert ops[IN_PLACE] == O.MUX
    i0[IN_PLACE], i1[IN_PLACE], i2[IN_PLACE], out[IN_PLACE] = 0, 8, 2, 8
    jobs = G + int((ops == O.MUX).sum())
    geo = E.vector_geometry(jobs, n, kN, l, n_cus)
    print("gate level k N %d ks_l %d: %d gates, %d jobs -> %d x %d B" % (kN, l, G, jobs, geo[2], geo[4]))
    assert E.lds_band(jobs, n, kN, l, n_cus) == ("raised", "grid") and geo[2] == 1 and geo[4] == kN * l * 4
    ct = ck.encrypt(rng.integers(0, 2, 9).astype(bool))
    assert ct.shape == (9, kN + 1)
    sk = helm_amd.ServerKey(ck, device=0)
    try:
        assert sk.kernel_class() == "generic" and sk.wire_words() == kN + 1
        wide = sk.wires(9 + G)
        wide.upload(np.arange(9), ct)
        wide.eval_gate_level(ops, i0, i1, i2, out)
        got = wide.download()
        wide.free()
        narrow = sk.wires(9 + G)
        narrow.upload(np.arange(9), ct)
        for a0 in range(0, G, NARROW):
            s = slice(a0, a0 + NARROW)
            j = len(ops[s]) + int((ops[s] == O.MUX).sum())
            assert E.vector_geometry(j, n, kN, l, n_cus)[2] == 16
            narrow.eval_gate_level(ops[s], i0[s], i1[s], i2[s], out[s])
        ref = narrow.download()
        narrow.free()
    finally:
        sk.close()
    assert np.array_equal(got[:8], ct[:8]) and np.array_equal(ref[:8], ct[:8])
    assert np.array_equal(got, ref), "the one-slice level differs from the 16-slice levels: " + T._first_diff(got, ref)
    comp = K.KsFirst(O.Oracle(p.as_tuple7(), ck.bsk, ck.ksk))
    row = lambda i: np.ascontiguousarray(ct[i]) if i >= 0 else None  # noqa: E731
    for g in (0, 3, 4, 6, IN_PLACE, G - 1):
        want = comp.gate(int(ops[g]), row(i0[g]), row(i1[g]), row(i2[g]))
        assert np.array_equal(got[out[g]], want), ("gate", g, "op", int(ops[g]))
