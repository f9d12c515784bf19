"""Noise of the three-input gates at boolean_default, measured.

2,048 MAJ3 gates and 2,048 XOR3 gates whose operands are OUTPUTS of a first level of two-input gates (the steady state of a
fused circuit; three gate outputs in one operand is the worst operand the new gates form).  All outputs decrypt correctly;
the output variance sits within [0.6, 1.5] of V_br + V_ks (the band and the formulas of tests/test_gpu_noise.py - a gate's
output noise does not depend on its operand while the bootstrap succeeds); and the failure probability implied by
3 v_measured + V_ms at a margin of 1/8 is below 2^-100, that test's sanity bound (the formulas predict about 2^-202)."""
import math
import os
import sys

import numpy as np
import pytest

import helm_amd

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_noise as TN  # noqa: E402

pytestmark = pytest.mark.gpu
NAND, XOR, MAJ3, XOR3 = 4, 9, 20, 21


def test_three_input_gates_on_gate_outputs_sit_inside_the_noise_budget():
    name, B = "boolean_default", 2048
    p, s_lwe, s_glwe = helm_amd.named_params(name)
    ck = helm_amd.ClientKey.generate(name, seed=19)
    sk = helm_amd.ServerKey(ck)
    try:
        rng = np.random.default_rng(5)
        bits = rng.integers(0, 2, size=2 * B).astype(bool)
        w = sk.wires(5 * B)
        w.upload(np.arange(2 * B), ck.encrypt(bits))
        ar = np.arange(B, dtype=np.int32)
        m1 = np.full(B, -1, np.int32)
        lvl1 = 2 * B + ar
        ops1 = np.where(ar % 2 == 0, NAND, XOR).astype(np.int32)
        w.eval_gate_level(ops1, ar, B + ar, m1, lvl1)
        v1 = np.where(ar % 2 == 0, ~(bits[:B] & bits[B:]), bits[:B] ^ bits[B:])
        assert np.array_equal(ck.decrypt(w.download(lvl1)), v1)
        a, b, c = v1, np.roll(v1, 1), np.roll(v1, 2)
        br, ks, ms = TN.predicted(p, s_lwe, s_glwe)
        for op, out, want in ((MAJ3, 3 * B + ar, (a.astype(int) + b + c) >= 2), (XOR3, 4 * B + ar, a ^ b ^ c)):
            w.eval_gate_level(np.full(B, op, np.int32), lvl1, np.roll(lvl1, 1), np.roll(lvl1, 2), out)
            sk.sync()
            ct = w.download(out)
            assert np.array_equal(ck.decrypt(ct), want), op
            err = TN.signed_err(ck.phase(ct), np.where(want, 1 << 29, 7 << 29).astype(np.uint32), 32)
            v_meas = float(np.mean(err ** 2))
            ratio = v_meas / (br + ks)
            lp_maj = TN.log2_pfail(0.125, 3 * v_meas + ms)
            lp_xor = TN.log2_pfail(0.25, 12 * v_meas + ms)
            print(f"\n{name}, op {op} on three gate outputs: measured variance {v_meas:.3e}, predicted {br + ks:.3e} "
                  f"(ratio {ratio:.3f}), max |err| {np.abs(err).max():.2e}; modulus switch {ms:.3e}; implied failure "
                  f"probability MAJ3 2^{lp_maj:.1f}, XOR3 2^{lp_xor:.1f}")
            assert abs(float(np.mean(err))) < 4 * math.sqrt(v_meas / B), "the phase error is biased"
            assert 0.6 < ratio < 1.5, f"measured variance {v_meas:.3e} vs predicted {br + ks:.3e}"
            assert lp_maj < -100
    finally:
        sk.close()
