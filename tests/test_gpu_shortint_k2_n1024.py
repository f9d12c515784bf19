"""The 3-bit shape (k = 2, N = 1024, one level: PARAM_MESSAGE_2_CARRY_1_KS_PBS, reference tests/circuit_test.rs:13, 287) on
the GPU: k_pbs64k<10, 2>, two ciphertexts per CU with the accumulator kept in registers and the transform scratch
(helm_shortint.hip).  The toy twin si_toy_1024_k2 bit for bit against the shortint oracle through every
primitive; the full set shortint_m2c1 on a whole level of 1,024 three-input LUTs (every row against the oracle) and on the
reference's LUT adders, decrypted and audited operation by operation; a lane; and the counting debug build."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import helm_amd
import oracle
from helm_amd import Circuit, EvalCircuit, LutCircuit, verilog_parser

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NET = os.path.join(HERE, "netlists")
INPUTS = os.path.join(HERE, "golden", "8-bit-adder.inputs.csv")


@pytest.fixture(scope="module")
def toy():
    ck = helm_amd.SiClientKey.generate("si_toy_1024_k2", seed=3)
    sk = helm_amd.SiServerKey(ck)
    orc = oracle.Oracle64(ck.params.as_tuple(), ck.bsk, ck.ksk)
    yield ck, sk, orc
    sk.close()


@pytest.fixture(scope="module")
def full():
    ck, sk = helm_amd.gen_keys_shortint("shortint_m2c1", seed=1)
    orc = oracle.Oracle64(ck.params.as_tuple(), ck.bsk, ck.ksk, use_ntt=True)
    yield ck, sk, orc
    sk.close()


def _circuit(path):
    gs, ws, ins, outs, d, _, _ = verilog_parser.read_verilog_file(path, False)
    c = Circuit(gs, ins, outs, d)
    c.sort_circuit()
    c.compute_levels()
    return c, ws


def test_toy_keyswitch_vector_and_matrix_core_bit_exact(toy, monkeypatch):
    """k N = 2,048 as in m2c2: both keyswitch kernels (a batch of 203 takes the matrix cores, HELM_HIP_KS_MFMA=0 and a narrow
    batch the vector ALUs) give the oracle's words."""
    ck, sk, orc = toy
    monkeypatch.setenv("HELM_HIP_KS_MFMA", "0")
    sk_valu = helm_amd.SiServerKey(ck)
    monkeypatch.delenv("HELM_HIP_KS_MFMA")
    rng = np.random.default_rng(4)
    count = 203
    cts = ck.encrypt(rng.integers(0, ck.t, count).astype(np.uint64))
    cts[2] = rng.integers(0, 2**64, size=cts.shape[1], dtype=np.uint64)  # every digit pattern
    got = sk.keyswitch_batch(cts)
    assert np.array_equal(got, sk_valu.keyswitch_batch(cts))
    for g in (0, 1, 2, 63, 64, 159, 160, count - 1):
        assert np.array_equal(got[g], orc.keyswitch(cts[g])), g
    narrow = sk.keyswitch_batch(cts[:7])
    assert np.array_equal(narrow, got[:7])
    for g in range(7):
        assert np.array_equal(narrow[g], orc.keyswitch(cts[g])), g
    sk_valu.close()


def test_toy_pbs_batch_every_value_bit_exact(toy):
    ck, sk, orc = toy
    vals = np.arange(ck.t, dtype=np.uint64)
    small = sk.keyswitch_batch(ck.encrypt(vals))
    luts = np.stack([orc.make_lut(lambda x: (5 * x + 3) % ck.t), orc.make_lut(lambda x: x & 1)])
    assert np.array_equal(luts[0], sk.make_lut(lambda x: (5 * x + 3) % ck.t))
    idx = (np.arange(ck.t) % 2).astype(np.int32)
    got = sk.pbs_batch(small, luts, idx)
    for g in range(ck.t):
        assert np.array_equal(got[g], orc.bootstrap(small[g], luts[idx[g]])), g
    dec = ck.decrypt_message_and_carry(got)
    assert list(dec) == [((5 * v + 3) % ck.t) if i == 0 else (v & 1) for v, i in zip(range(ck.t), idx)]


def test_toy_lut_level_arities_0_to_3_bit_exact(toy):
    ck, sk, orc = toy
    bits = np.array([1, 0, 1, 1], dtype=np.uint64)
    gates = [(3, [0, 1, 2], 0x96), (3, [0, 1, 2], 0xE8), (3, [3, 2, 1], 0x1B), (2, [0, 1], 0x6), (2, [2, 3], 0x8),
             (2, [1, 0], 0xD), (1, [0], 0x0), (1, [2], 0x2), (0, [3], 0x0)]
    n_in, count = len(bits), len(gates)
    arity = np.array([g[0] for g in gates], dtype=np.int32)
    in_idx = np.full((count, 3), -1, dtype=np.int32)
    for g, (_, ins, _) in enumerate(gates):
        in_idx[g, :len(ins)] = ins
    table = np.array([g[2] for g in gates], dtype=np.uint64)
    out_idx = np.arange(n_in, n_in + count, dtype=np.int32)
    host = np.zeros((n_in + count, ck.dim + 1), dtype=np.uint64)
    host[:n_in] = ck.encrypt(bits)
    w = sk.wires(n_in + count)
    w.upload(np.arange(n_in), host[:n_in])
    w.eval_lut_level(arity, in_idx, table, out_idx)
    got = w.download()
    orc.eval_lut_level(host, arity, in_idx, table, out_idx)
    assert np.array_equal(got, host)
    dec = ck.decrypt_message_and_carry(got[n_in:])
    for g, (ar, ins, tb) in enumerate(gates):
        x = [int(bits[i]) for i in ins]
        if ar >= 2:
            want = (tb >> sum(b << (ar - 1 - q) for q, b in enumerate(x))) & 1  # first input = MSB (gates.rs:159-167)
        elif ar == 1:
            want = x[0] if tb == 0 else (-x[0]) % ck.t  # smart_neg (gates.rs:769)
        else:
            want = x[0]
        assert int(dec[g]) == want, g


def test_toy_lincomb_and_apply_luts(toy):
    ck, sk, orc = toy
    w = sk.wires(8)
    w.upload([0, 1, 2], ck.encrypt([1, 2, 3]))
    w.set_trivial([3], [2])
    w.lincomb([[0, 1], [0, 2], [3, -1]], [[2, 1], [1, 1], [-1, 0]], [4, 0, 5], const_add=[3, 0, 1])
    assert list(ck.decrypt_message_and_carry(w.download([4, 0, 5]))) == [7 % ck.t, 4, (-2 + 1) % ck.t]
    lut = sk.make_lut(lambda x: (x * x + 1) % ck.t)
    before = w.download([4, 0])
    w.apply_luts([4, 0], lut, [4, 6])  # row 4 in place
    got = w.download([4, 6])
    for g in range(2):
        assert np.array_equal(got[g], orc.apply_lut(before[g], lut)), g
    assert list(ck.decrypt_message_and_carry(got)) == [(49 + 1) % ck.t, (16 + 1) % ck.t]


def test_toy_lane_uses_the_primarys_key(toy):
    ck, sk, orc = toy
    lane = sk.fork()
    assert lane.field_bits() == sk.field_bits() == 49
    vals = np.arange(ck.t, dtype=np.uint64)
    small = lane.keyswitch_batch(ck.encrypt(vals))
    luts = np.stack([orc.make_lut(lambda x: (3 * x + 1) % ck.t)])
    got = lane.pbs_batch(small, luts, np.zeros(ck.t, np.int32))
    lane.sync()
    for g in range(ck.t):
        assert np.array_equal(got[g], orc.bootstrap(small[g], luts[0])), g
    assert list(ck.decrypt_message_and_carry(got)) == [(3 * v + 1) % ck.t for v in range(ck.t)]
    lane.close()


def test_round_capacity_is_two_ciphertexts_per_cu(toy):
    ck, sk, orc = toy
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert sk.round_capacity() == 2 * cus


def test_full_set_whole_level_every_row_bit_exact(full):
    """1,024 three-input LUTs (majority) as ONE level, the launch shape tools/microbench_luts.py times: decrypted, and every
    output row against the oracle."""
    ck, sk, orc = full
    B, arity, table = 1024, 3, 0xE8
    bits = np.random.default_rng(0).integers(0, 2, size=arity * B).astype(np.uint64)
    host = np.zeros(((arity + 1) * B, ck.dim + 1), dtype=np.uint64)
    host[:arity * B] = ck.encrypt(bits)
    w = sk.wires(len(host))
    w.upload(np.arange(arity * B), host[:arity * B])
    in_idx = np.arange(arity * B, dtype=np.int32).reshape(arity, B).T.copy()
    ar, tb = np.full(B, arity, np.int32), np.full(B, table, np.uint64)
    out = np.arange(arity * B, (arity + 1) * B, dtype=np.int32)
    w.eval_lut_level(ar, in_idx, tb, out)
    sk.sync()
    got = w.download(out)
    b = bits.reshape(arity, B)
    idx = sum(b[q].astype(np.int64) << (arity - 1 - q) for q in range(arity))
    assert np.array_equal(ck.decrypt(got), (table >> idx) & 1)
    want = orc.eval_lut_rows(host, ar, in_idx, tb, np.arange(B, dtype=np.int32))
    bad = [g for g in range(B) if not np.array_equal(got[g], want[g])]
    assert not bad, f"rows {bad[:8]} of the 1,024-LUT level differ from the oracle"


@pytest.mark.parametrize("netlist,luts", [("8-bit-adder-lut-3-1.v", 16), ("8-bit-adder-lut-2-1.v", 40)])
def test_full_set_lut_adder_every_wire(full, netlist, luts):  # reference tests/circuit_test.rs:266-311
    ck, sk, orc = full
    c, ws = _circuit(os.path.join(NET, netlist))
    inputs = verilog_parser.read_input_wires(INPUTS, "bool")
    ptxt = c.evaluate(c.initialize_wire_map(ws, inputs, "bool"))
    lc = LutCircuit(ck, sk, c)
    enc = EvalCircuit.evaluate_encrypted(lc, EvalCircuit.encrypt_inputs(lc, ws, inputs), 1, "bool")
    assert lc.pbs_per_cycle() == luts
    for wire, want in ptxt.items():
        assert ck.decrypt(enc[wire]) == int(bool(want)), wire
    out = EvalCircuit.decrypt_outputs(lc, enc, True)
    a = sum(int(bool(inputs[f"a[{i}]"])) << i for i in range(8))
    b = sum(int(bool(inputs[f"b[{i}]"])) << i for i in range(8))
    assert sum(out[f"sum[{i}]"].value << i for i in range(8)) + (out["cout"].value << 8) == a + b + int(bool(inputs["cin"]))


class _Auditor:
    """SiServerKey.set_audit hook: every linear step and every look-up batch recomputed on the oracle from the GPU's operands."""

    def __init__(self, orc):
        self.orc, self.delta = orc, np.uint64(orc.delta)
        self.lock = threading.Lock()
        self.bad, self.luts, self.lin = [], 0, 0

    def __call__(self, rec):
        if rec["kind"] == "lincomb":
            _, terms, _ = rec["in_rows"].shape
            acc = np.zeros_like(rec["out_rows"])
            with np.errstate(over="ignore"):
                for t in range(terms):
                    use = rec["in_idx"][:, t] >= 0
                    acc[use] += rec["coef"][use, t].astype(np.uint64)[:, None] * rec["in_rows"][use, t]
                if rec["const_add"] is not None:
                    acc[:, -1] += rec["const_add"].astype(np.uint64) * self.delta
            ok = np.all(acc == rec["out_rows"], axis=1)
            with self.lock:
                self.lin += len(ok)
                self.bad += [("lincomb", int(g)) for g in np.nonzero(~ok)[0]]
            return True
        want = self.orc.apply_luts(rec["in_rows"], rec["luts"], rec["lut_idx"])
        ok = np.all(want == rec["out_rows"], axis=1)
        with self.lock:
            self.luts += len(ok)
            self.bad += [("luts", int(g)) for g in np.nonzero(~ok)[0]]
        return True


@pytest.mark.parametrize("netlist,luts", [("8-bit-adder-lut-3-1.v", 16), ("8-bit-adder-lut-2-1.v", 40)])
def test_full_set_lut_adder_every_operation_audited(full, netlist, luts):
    ck, sk, orc = full
    aud = _Auditor(orc)
    sk.set_audit(aud)
    try:
        c, ws = _circuit(os.path.join(NET, netlist))
        inputs = verilog_parser.read_input_wires(INPUTS, "bool")
        ptxt = c.evaluate(c.initialize_wire_map(ws, inputs, "bool"))
        lc = LutCircuit(ck, sk, c)
        enc = EvalCircuit.evaluate_encrypted(lc, EvalCircuit.encrypt_inputs(lc, ws, inputs), 1, "bool")
    finally:
        sk.set_audit(None)
    assert not aud.bad, aud.bad[:5]
    assert aud.luts == lc.pbs_per_cycle() == luts and aud.lin >= luts
    for wire, want in ptxt.items():
        assert ck.decrypt(enc[wire]) == int(bool(want)), wire


CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, %r)
import helm_amd, oracle
from helm_amd import Circuit, EvalCircuit, LutCircuit, verilog_parser
res = {}
# the toy set: keyswitch (both kernels), every value through a bootstrap, a LUT level of arity 0..3
for mfma in ("1", "0"):
    os.environ["HELM_HIP_KS_MFMA"] = mfma
    ck = helm_amd.SiClientKey.generate("si_toy_1024_k2", seed=3)
    sk = helm_amd.SiServerKey(ck)
    orc = oracle.Oracle64(ck.params.as_tuple(), ck.bsk, ck.ksk)
    sk.bound_violations(reset=True)
    cts = ck.encrypt((np.arange(203) %% ck.t).astype(np.uint64))
    small = sk.keyswitch_batch(cts)
    ks_ok = all(np.array_equal(small[g], orc.keyswitch(cts[g])) for g in (0, 100, 202))
    lut = orc.make_lut(lambda x: (5 * x + 3) %% ck.t)
    got = sk.pbs_batch(small[:8], lut[None, :], np.zeros(8, np.int32))
    pbs_ok = all(np.array_equal(got[g], orc.bootstrap(small[g], lut)) for g in range(8))
    bits = np.array([1, 0, 1, 1], dtype=np.uint64)
    ar = np.array([3, 2, 1, 0], np.int32)
    in_idx = np.array([[0, 1, 2], [2, 3, -1], [0, -1, -1], [3, -1, -1]], np.int32)
    tb = np.array([0x96, 0x6, 0x2, 0x0], np.uint64)
    host = np.zeros((8, ck.dim + 1), np.uint64)
    host[:4] = ck.encrypt(bits)
    w = sk.wires(8)
    w.upload(np.arange(4), host[:4])
    w.eval_lut_level(ar, in_idx, tb, np.arange(4, 8, dtype=np.int32))
    lvl = w.download()
    orc.eval_lut_level(host, ar, in_idx, tb, np.arange(4, 8, dtype=np.int32))
    res["si_toy_1024_k2:mfma" + mfma] = {"ok": bool(ks_ok and pbs_ok and np.array_equal(lvl, host)), "violations": sk.bound_violations()}
    sk.close()
os.environ.pop("HELM_HIP_KS_MFMA")
# the full set: a level of 1,024 three-input LUTs, and the LUT-3-1 adder through LutCircuit
ck, sk = helm_amd.gen_keys_shortint("shortint_m2c1", seed=1)
sk.bound_violations(reset=True)
B = 1024
bits = np.random.default_rng(0).integers(0, 2, size=3 * B).astype(np.uint64)
w = sk.wires(4 * B)
w.upload(np.arange(3 * B), ck.encrypt(bits))
in_idx = np.arange(3 * B, dtype=np.int32).reshape(3, B).T.copy()
w.eval_lut_level(np.full(B, 3, np.int32), in_idx, np.full(B, 0xE8, np.uint64), np.arange(3 * B, 4 * B, dtype=np.int32))
b = bits.reshape(3, B).astype(np.int64)
level_ok = bool(np.array_equal(ck.decrypt(w.download(np.arange(3 * B, 4 * B))), (0xE8 >> (4 * b[0] + 2 * b[1] + b[2])) & 1))
gs, ws, ins, outs, d, _, _ = verilog_parser.read_verilog_file(os.path.join(%r, "8-bit-adder-lut-3-1.v"), False)
c = Circuit(gs, ins, outs, d)
c.sort_circuit()
c.compute_levels()
inputs = verilog_parser.read_input_wires(%r, "bool")
ptxt = c.evaluate(c.initialize_wire_map(ws, inputs, "bool"))
lc = LutCircuit(ck, sk, c)
enc = EvalCircuit.evaluate_encrypted(lc, EvalCircuit.encrypt_inputs(lc, ws, inputs), 1, "bool")
adder_ok = all(ck.decrypt(enc[wire]) == int(bool(v)) for wire, v in ptxt.items())
res["shortint_m2c1"] = {"ok": bool(level_ok and adder_ok), "violations": sk.bound_violations()}
sk.close()
print("RESULT " + json.dumps(res))
"""


def test_check_build_counts_no_violation():
    """The counting debug build (libhelm_hip_check.so, loaded through HELM_HIP_LIB as tests/test_gpu_bounds_check.py does)
    over the toy primitives and the full set's level and adder: zero violations of the lazy arithmetic's contracts."""
    lib = os.path.join(ROOT, "helm_amd", "csrc", "libhelm_hip_check.so")
    assert os.path.exists(lib), "make -C helm_amd/csrc libhelm_hip_check.so"
    env = dict(os.environ, HELM_HIP_LIB=lib)
    p = subprocess.run([sys.executable, "-c", CHILD % (ROOT, NET, INPUTS)], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=1200)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert set(res) == {"si_toy_1024_k2:mfma1", "si_toy_1024_k2:mfma0", "shortint_m2c1"}
    for name, r in res.items():
        assert r["ok"], (name, r)
        assert r["violations"] == [0] * 8, (name, r["violations"])
