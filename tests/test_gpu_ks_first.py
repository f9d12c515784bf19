"""Keyswitch-first levels (pbs_order = 1, HELM_HIP_CREATE_KS_PBS) on the GPU, word for word against tests/ks_first.py - the
composition of the oracle's lincomb, keyswitch and bootstrap: every gate type on every kernel class and both keyswitch
paths, the launch edges of k_keyswitch_gate / k_ks_gate_digits / k_big_out, crafted rows, the wire table at width k N + 1,
programs (in place, sharded, through GateCircuit), the counting build, the full-size set, and order 0 under the new flag.

What is compared where no accessor exists: the small rows between the gate keyswitch and the bootstrap stay inside the
context, so the keyswitch stage is checked THROUGH the gate's full output against the composed oracle (a wrong small row
gives another extracted row); the two halves of a MUX likewise through their recombined row.  The composition's own
keyswitch stage is pinned to the Python-integer reference of tests/ks_edges.py by tests/test_ks_first_reference.py."""
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

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ks_edges as E  # noqa: E402
import ks_first as K  # noqa: E402
import test_gpu_eight_ranks as T8  # noqa: E402  (its random netlist and plaintext evaluator, unchanged)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET = os.path.join(ROOT, "tests", "netlists")
O = oracle
BOOT = [O.AND, O.NAND, O.OR, O.NOR, O.XOR, O.XNOR, O.MUX]


def _set(name, **over):
    p, a, b = helm_amd.named_params(name)
    for k, v in over.items():
        setattr(p, k, v)
    return p, a, b


# name -> (params, noise, crt option, takes the matrix-core keyswitch)
SETS = {
    "toy_ks_pbs": (_set("toy_ks_pbs"), None, True),                                   # ks_l 4
    "toy_1024_ks_pbs": (_set("toy_1024_ks_pbs"), None, True),                         # ks_l 8
    "toy_k2_ks_pbs": (_set("toy_k2_ks_pbs"), None, True),
    "generic_2_512_2_7": (_set("toy_k2_ks_pbs", pbs_l=2, pbs_logB=7), None, True),    # no tuned build: k_pbs_generic
    "toy_crt_ks_pbs": (_set("toy_crt", pbs_order=1), "allow", True),                  # flag 17: k_pbs_crt
    "ks_l3": (_set("toy_ks_pbs", ks_l=3, ks_logB=5), None, False),                    # vector-ALU path only
    "ks_l5": (_set("toy_ks_pbs", ks_l=5, ks_logB=4), None, False),
}
CLASS = {"generic_2_512_2_7": "generic", "toy_crt_ks_pbs": "crt"}


class Keys:
    def __init__(self, name, seed=5):
        (p, a, b), self.crt, self.mfma = SETS[name]
        self.name, self.p = name, p
        self.ck = helm_amd.ClientKey(p, a, b, seed=seed)
        self.kN = p.k * p.N
        self.ref = K.KsFirst(O.Oracle(p.as_tuple7(), self.ck.bsk, self.ck.ksk))

    def server(self, ks_mfma=None):
        """A fresh context; ks_mfma=0 sets HELM_HIP_KS_MFMA=0 before it is created."""
        old = os.environ.pop("HELM_HIP_KS_MFMA", None)
        try:
            if ks_mfma is not None:
                os.environ["HELM_HIP_KS_MFMA"] = str(ks_mfma)
            return helm_amd.ServerKey(self.ck, device=0, crt=self.crt)
        finally:
            os.environ.pop("HELM_HIP_KS_MFMA", None)
            if old is not None:
                os.environ["HELM_HIP_KS_MFMA"] = old


_KEYS = {}


def keys(name):
    if name not in _KEYS:
        _KEYS[name] = Keys(name)
    return _KEYS[name]


def _every_gate_level():
    """Rows 0, 1, 2 = inputs; one gate of every type, the binary ones over (0, 1), MUX = row 2 ? row 0 : row 1."""
    ops = BOOT + [O.NOT, O.BUF, O.DFF, O.CONST_ONE, O.CONST_ZERO]
    i0 = [0] * 7 + [1, 0, 1, -1, -1]
    i1 = [1] * 7 + [-1] * 5
    i2 = [-1] * 6 + [2] + [-1] * 5
    out = list(range(3, 3 + len(ops)))
    return [np.array(a, dtype=np.int32) for a in (ops, i0, i1, i2, out)]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. every gate type, every kernel path
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETS))
def test_every_gate_type_word_for_word(name):
    k = keys(name)
    ops, i0, i1, i2, out = _every_gate_level()
    want_rows = {}
    for bits in ([True, False, True], [False, True, False]):
        ct = k.ck.encrypt(bits)
        host = np.zeros((3 + len(ops), k.kN + 1), dtype=np.uint32)
        host[:3] = ct
        k.ref.eval_level(host, ops, i0, i1, i2, out)
        a, b, c = bits
        plain = [K.plain_gate(int(o), a if o not in (O.NOT, O.DFF) else b, b, c) for o in ops]
        assert list(k.ck.decrypt(host[3:])) == plain, (name, bits)
        want_rows[tuple(bits)] = (ct, host)
    for ks_mfma in ([None, 0] if k.mfma else [None]):
        sk = k.server(ks_mfma)
        assert sk.kernel_class() == CLASS.get(name, "tuned") and sk.wire_words() == k.kN + 1
        for bits, (ct, host) in want_rows.items():
            w = sk.wires(len(host))
            w.upload([0, 1, 2], ct)
            w.eval_gate_level(ops, i0, i1, i2, out)
            got = w.download()
            for g in range(len(ops)):
                assert np.array_equal(got[out[g]], host[out[g]]), (name, ks_mfma, bits, "gate", g, "op", int(ops[g]))
            assert np.array_equal(got[:3], ct)
            w.free()
        sk.close()


def test_the_order_does_not_change_class_field_or_quantum():
    for name, base in (("toy_ks_pbs", "toy"), ("toy_1024_ks_pbs", "toy_1024"), ("toy_k2_ks_pbs", "toy_k2")):
        s1 = keys(name).server()
        # the same key material in order 0 (the N = 1024 field is chosen from the loaded key)
        s0 = helm_amd.ServerKey(helm_amd.ClientKey.generate(base, seed=5), device=0)
        assert (s1.kernel_class(), s1.field_bits(), s1.launch_quantum(), s1.digit_batch()) == \
               (s0.kernel_class(), s0.field_bits(), s0.launch_quantum(), s0.digit_batch())
        assert s0.wire_words() == s0.params.n + 1 and s1.wire_words() == s1.params.k * s1.params.N + 1
        s0.close()
        s1.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. launch edges: the four-gate workgroup tail, the 16- and 64-row padding of the A fragments, the row split
# ---------------------------------------------------------------------------------------------------------------------------
POOL = 160
COUNTS = [1, 3, 4, 5, 63, 64, 65, 160]


@pytest.fixture(scope="module")
def pool():
    """160 gates over 8 input rows - a launch of `count` gates is the pool's first `count` - and their reference rows."""
    k = keys("toy_ks_pbs")
    rng = np.random.default_rng(9)
    bits = rng.integers(0, 2, 8).astype(bool)
    ct = k.ck.encrypt(bits)
    ops = np.array([BOOT[g % 7] for g in range(POOL)], dtype=np.int32)
    i0, i1 = rng.integers(0, 8, POOL).astype(np.int32), rng.integers(0, 8, POOL).astype(np.int32)
    i2 = np.where(ops == O.MUX, rng.integers(0, 8, POOL), -1).astype(np.int32)
    out = np.arange(8, 8 + POOL, dtype=np.int32)
    host = np.zeros((8 + POOL, k.kN + 1), dtype=np.uint32)
    host[:8] = ct
    k.ref.eval_level(host, ops, i0, i1, i2, out)
    plain = [K.plain_gate(int(ops[g]), bits[i0[g]], bits[i1[g]], bits[max(i2[g], 0)]) for g in range(POOL)]
    assert list(k.ck.decrypt(host[8:])) == plain
    return k, ct, (ops, i0, i1, i2, out), host


@pytest.mark.parametrize("ks_mfma", [None, 0], ids=["matrix-core", "vector-alu-row-split"])
def test_launch_edges(pool, ks_mfma):
    """HELM_HIP_KS_MFMA=0 at these counts: (count + 3) / 4 workgroups is far below two per CU, so the key rows are split
    (slices > 1): k_ks_zero over the identity job list and the atomic accumulation run."""
    k, ct, (ops, i0, i1, i2, out), host = pool
    sk = k.server(ks_mfma)
    for count in COUNTS:  # ascending: the staging and job-list buffers of the context grow between launches
        w = sk.wires(len(host))
        w.upload(np.arange(8), ct)
        w.eval_gate_level(ops[:count], i0[:count], i1[:count], i2[:count], out[:count])
        got = w.download()
        assert np.array_equal(got[:8 + count], host[:8 + count]), (ks_mfma, count)
        assert not got[8 + count:].any(), (ks_mfma, count, "rows past the launch were written")
        w.free()
    # and a narrower launch after the widest one, on the buffers as they are
    w = sk.wires(len(host))
    w.upload(np.arange(8), ct)
    w.eval_gate_level(ops[:5], i0[:5], i1[:5], i2[:5], out[:5])
    assert np.array_equal(w.download()[:13], host[:13])
    sk.timing_enable(True)
    sk.timing(reset=True)  # (the launch counters run with timing off as well)
    w.eval_gate_level(ops[:65], i0[:65], i1[:65], i2[:65], out[:65])
    sk.sync()
    t = sk.timing(reset=True)
    n_pbs = 65 + int((ops[:65] == O.MUX).sum())
    assert (t.pbs_count, t.ks_count, t.pbs_launches, t.ks_launches) == (n_pbs, n_pbs, 1, 1)
    assert t.ks_ms > 0 and t.pbs_ms > 0
    sk.close()


def test_a_launch_wide_enough_for_one_slice(pool):
    """Vector-ALU keyswitch with (count + 3) / 4 >= two workgroups per CU: slices == 1, plain stores.  A sample of rows word
    for word (first, last, around the 4-gate and 64-gate boundaries), every output decrypted."""
    k, ct, (ops, i0, i1, i2, out), host = pool
    sk = k.server(0)
    count = 8 * sk.launch_quantum() // 4  # 8 gates per CU -> two workgroups of four gates per CU
    assert (count + 3) // 4 >= 2 * (sk.launch_quantum() // 4)
    rng = np.random.default_rng(4)
    bits = k.ck.decrypt(ct)
    wops = np.array([BOOT[g % 6] for g in range(count)], dtype=np.int32)  # binary gates
    w0, w1 = rng.integers(0, 8, count).astype(np.int32), rng.integers(0, 8, count).astype(np.int32)
    wout = np.arange(8, 8 + count, dtype=np.int32)
    w = sk.wires(8 + count)
    w.upload(np.arange(8), ct)
    w.eval_gate_level(wops, w0, w1, np.full(count, -1, np.int32), wout)
    got = w.download()
    plain = np.array([K.plain_gate(int(wops[g]), bits[w0[g]], bits[w1[g]]) for g in range(count)])
    assert np.array_equal(k.ck.decrypt(got[8:]), plain)
    sample = sorted({0, 1, 3, 4, 5, 63, 64, 65, count // 2, count - 5, count - 4, count - 1})
    for g in sample:
        want = k.ref.gate(int(wops[g]), np.ascontiguousarray(ct[w0[g]]), np.ascontiguousarray(ct[w1[g]]))
        assert np.array_equal(got[8 + g], want), g
    sk.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. crafted rows
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks_mfma", [None, 0], ids=["matrix-core", "vector-alu"])
def test_crafted_rows_through_the_gates(ks_mfma):
    """tests/ks_edges.py's rows (largest / smallest digit sums, ties, ...) as wire in0 with in1 an all-zero row: AND passes
    the words through, NAND negates them, XOR doubles them, MUX's second half is -c + e.  Checked through the gate's full
    output against the composed oracle (no accessor exposes the staging)."""
    k = keys("toy_ks_pbs")
    p = k.p
    rows = E.crafted_rows(k.kN, p.ks_logB, p.ks_l, 32)
    R = len(rows)
    host = np.zeros((R + 1 + 4 * R, k.kN + 1), dtype=np.uint32)
    host[:R] = rows                                   # row R stays all zero
    ops, i0, i1, i2 = [], [], [], []
    for r in range(R):
        ops += [O.AND, O.NAND, O.XOR, O.MUX]
        i0 += [r, r, r, R]
        i1 += [R, R, R, R]
        i2 += [-1, -1, -1, r]                         # MUX(sel = crafted row, 0, 0): halves c + 0 and -c + 0
    out = np.arange(R + 1, R + 1 + 4 * R, dtype=np.int32)
    ops, i0, i1, i2 = (np.array(a, dtype=np.int32) for a in (ops, i0, i1, i2))
    want = host.copy()
    k.ref.eval_level(want, ops, i0, i1, i2, out)
    sk = k.server(ks_mfma)
    w = sk.wires(len(host))
    w.upload(np.arange(R + 1), host[:R + 1])
    w.eval_gate_level(ops, i0, i1, i2, out)
    got = w.download()
    for g in range(len(ops)):
        assert np.array_equal(got[out[g]], want[out[g]]), (E.CRAFTED[g // 4], int(ops[g]))
    sk.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the wire table at width k N + 1
# ---------------------------------------------------------------------------------------------------------------------------
def test_wire_table_at_the_big_width():
    k = keys("toy_k2_ks_pbs")
    sk = k.server()
    W = k.kN + 1
    rng = np.random.default_rng(1)
    w = sk.wires(11)
    assert not w.download().any()
    rows = rng.integers(0, 1 << 32, size=(4, W), dtype=np.uint32)
    idx = [10, 0, 7, 3]                                # the last row, non-contiguous, unordered
    w.upload(idx, rows)
    full = w.download()
    assert full.shape == (11, W)
    for r, i in enumerate(idx):
        assert np.array_equal(full[i], rows[r])
    assert not full[[1, 2, 4, 5, 6, 8, 9]].any()
    assert np.array_equal(w.download([3, 10]), rows[[3, 0]])
    w2 = sk.wires(6)
    hip = nv.hip
    src, dst = np.array([10, 3], dtype=np.int32), np.array([5, 0], dtype=np.int32)
    nv.hip_check(hip.helm_hip_wires_copy(sk._h, w._h, nv.as_i32p(src), w2._h, nv.as_i32p(dst), 2))
    c = w2.download()
    assert np.array_equal(c[5], rows[0]) and np.array_equal(c[0], rows[3]) and not c[1:5].any()
    w2.set_trivial([5, 2], [False, True])
    c = w2.download()
    assert not c[[5, 2], :-1].any() and c[5, -1] == K.PT_FALSE and c[2, -1] == K.PT_TRUE
    assert np.array_equal(c[0], rows[3])
    assert list(k.ck.decrypt(c[[5, 2]])) == [False, True]
    sk.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. programs
# ---------------------------------------------------------------------------------------------------------------------------
def _circuit(path_or_text, is_text=False):
    from helm_amd import Circuit, verilog_parser
    rd = verilog_parser.read_verilog_text if is_text else verilog_parser.read_verilog_file
    gates_set, wire_set, input_wires, output_wires, dffs, _, _ = rd(path_or_text, False)
    c = Circuit(gates_set, input_wires, output_wires, dffs)
    c.sort_circuit()
    c.compute_levels()
    return c, wire_set, input_wires, output_wires


def test_two_bit_adder_program_and_gate_circuit():
    from helm_amd import GateCircuit, PtxtType
    from helm_amd.distributed import level_arrays
    k = keys("toy_k2_ks_pbs")
    sk = k.server()
    circuit, wire_set, input_wires, _ = _circuit(f"{NET}/2-bit-adder.v")
    vals = {"a[0]": True, "a[1]": False, "b[0]": True, "b[1]": True, "cin": True}
    ptxt = {x: PtxtType.None_() for x in wire_set}
    ptxt.update({n: PtxtType.Bool(v) for n, v in vals.items()})
    ptxt = circuit.evaluate(ptxt)
    gc = GateCircuit(k.ck, sk, circuit)
    enc_in = gc.encrypt_inputs(wire_set, {n: PtxtType.Bool(v) for n, v in vals.items()})
    enc = gc.evaluate_encrypted(enc_in, 1, "bool")
    names = list(input_wires) + sorted(wire_set)
    index = {n: i for i, n in enumerate(names)}
    arrays = level_arrays(circuit, index)
    host = np.zeros((len(names), k.kN + 1), dtype=np.uint32)
    for n in names:
        host[index[n]] = enc_in[n]
    start = host.copy()
    k.ref.run_program(host, *arrays)
    for n in sorted(ptxt):
        assert np.array_equal(enc[n], host[index[n]]), n                     # GateCircuit, bit for bit
        assert k.ck.decrypt(enc[n]) == bool(ptxt[n].value), n
    w = sk.wires(len(names))
    w.upload(np.arange(len(names)), start)
    prog = helm_amd.Program(sk, *arrays)
    prog.run(w)
    assert np.array_equal(w.download(), host)                                # Program.run, bit for bit
    prog.destroy()
    sk.close()


def _latch_program():
    """Rows 0..3 inputs (a, b, ready, held).  Level 0: x = a ^ b (row 4), nr = !ready (row 5).  Level 1: the READY latch in
    place, held = ready ? x : held (row 3 read and written by one gate), beside a gate that reads row 4.  Level 2: reads the
    latched row."""
    ops = [O.XOR, O.NOT, O.MUX, O.AND, O.OR, O.BUF]
    i0 = [0, 2, 4, 4, 3, 3]
    i1 = [1, -1, 3, 5, 6, -1]
    i2 = [-1, -1, 2, -1, -1, -1]
    out = [4, 5, 3, 6, 7, 8]
    off = [0, 2, 4, 6]
    a32 = lambda a: np.array(a, dtype=np.int32)  # noqa: E731
    return a32(ops), a32(i0), a32(i1), a32(i2), a32(out), np.array(off, dtype=np.int64)


@pytest.mark.parametrize("ready", [False, True])
def test_a_latch_that_updates_its_row_in_place(ready):
    k = keys("toy_ks_pbs")
    sk = k.server()
    bits = [True, False, ready, False]
    ct = k.ck.encrypt(bits)
    arrays = _latch_program()
    host = np.zeros((9, k.kN + 1), dtype=np.uint32)
    host[:4] = ct
    k.ref.run_program(host, *arrays)
    x = bits[0] != bits[1]
    held = x if ready else bits[3]
    x_and_nr = x and not ready
    assert list(k.ck.decrypt(host)) == bits[:3] + [held, x, not ready, x_and_nr, held or x_and_nr, held]
    w = sk.wires(9)
    w.upload(np.arange(4), ct)
    prog = helm_amd.Program(sk, *arrays)
    prog.run(w)
    assert np.array_equal(w.download(), host)
    prog.destroy()
    sk.close()


def test_ready_latch_through_gate_circuit():
    """The sequential netlist of tests/test_gpu_circuits.py under a keyswitch-first key: GateCircuit.evaluate_ready is the
    in-place MUX level."""
    from helm_amd import GateCircuit, PtxtType
    k = keys("toy_k2_ks_pbs")
    sk = k.server()
    text = """input en;
output q0, READY;
dff g0(d0, q0);
dff g1(d1, q1);
xor g2(q0, en, d0);
and g3(q0, en, c0);
xor g4(q1, c0, d1);
buf g5(q1, READY);
"""
    circuit, wire_set, _, _ = _circuit(text, is_text=True)
    gc = GateCircuit(k.ck, sk, circuit)
    enc = gc.encrypt_inputs(wire_set, {"en": PtxtType.Bool(True), "q0": PtxtType.Bool(False), "q1": PtxtType.Bool(False)})
    ready_map = gc.init_ready()
    state = []
    for _ in range(3):
        enc = gc.evaluate_encrypted(enc, 1, "bool")
        gc.evaluate_ready(enc, ready_map)
        assert enc["q0"].shape == (k.kN + 1,)
        state.append((k.ck.decrypt(enc["q0"]), k.ck.decrypt(enc["q1"])))
    assert state == [(True, False), (False, True), (True, True)]
    assert gc.decrypt_outputs(ready_map, True)["READY"] == PtxtType.Bool(True)
    sk.close()


@pytest.fixture(scope="module")
def netlist():
    """The random netlist of tests/test_gpu_eight_ranks.py (every gate type, levels of 1 .. 60 gates) under toy_ks_pbs: the
    unsharded table, equal to the composed oracle on every wire and to the plaintext evaluator after decryption."""
    k = keys("toy_ks_pbs")
    arrays, n_rows, n_in = T8._random_program(7)
    bits = np.random.default_rng(2).integers(0, 2, size=n_in).astype(bool)
    in_rows = np.arange(n_in, dtype=np.int32)
    enc = k.ck.encrypt(bits)
    sk = k.server()
    prog = helm_amd.Program(sk, *arrays)
    w = sk.wires(n_rows)
    w.upload(in_rows, enc)
    prog.run(w)
    want = w.download()
    host = np.zeros((n_rows, k.kN + 1), dtype=np.uint32)
    host[:n_in] = enc
    k.ref.run_program(host, *arrays)
    assert np.array_equal(want, host)
    assert np.array_equal(k.ck.decrypt(want), T8._plain(arrays, bits, n_rows))
    widths = [prog.level_pbs(l) for l in range(prog.n_levels)]
    prog.destroy()
    sk.close()
    return k, arrays, n_rows, in_rows, enc, want, widths


def test_run_sharded_with_a_callback_at_world_1(netlist):
    """helm_hip_program_run_sharded: stage -> the caller's all-gather -> scatter for every launch wider than
    replicate_below, through helm_amd.distributed (its row_words is the context's)."""
    import torch
    from helm_amd.distributed import GpuLevelExecutor, ShardedRunner
    k, arrays, n_rows, in_rows, enc, want, widths = netlist

    class OneRank:  # torch.distributed at world size 1: the gathered buffer is the staged one
        @staticmethod
        def all_gather_into_tensor(out, inp):
            out.copy_(inp)

    sk = k.server()
    prog = helm_amd.Program(sk, *arrays)
    w = sk.wires(n_rows)
    w.upload(in_rows, enc)
    ex = GpuLevelExecutor(prog, w)
    assert ex.row_words == k.kN + 1
    runner = ShardedRunner(ex, rank=0, world=1, dist=OneRank, replicate_below=4, in_library=True, force=True)
    assert runner.in_library and len(runner.sharded_levels) >= 3 and any(x <= 4 for x in widths)
    runner.run()
    torch.cuda.synchronize()
    sk.sync()
    assert np.array_equal(w.download(), want)
    prog.destroy()
    sk.close()


@pytest.mark.parametrize("overlap", [False, True])
def test_two_rank_threads_through_the_in_process_communicator(netlist, overlap):
    k, arrays, n_rows, in_rows, enc, want, widths = netlist
    assert max(widths) > 4 and min(widths) <= 4  # launches on both sides of replicate_below
    tables, stats, sharded = T8._run_world(2, arrays, n_rows, in_rows, enc, k.ck, 4, overlap)
    assert sharded >= 3 and stats[0] == stats[1] == sharded
    for r in range(2):
        assert np.array_equal(tables[r], want), r


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the counting build
# ---------------------------------------------------------------------------------------------------------------------------
CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests"))
import helm_amd, oracle
import ks_first as K
ck = helm_amd.ClientKey.generate("toy_ks_pbs", seed=3)
sk = helm_amd.ServerKey(ck, device=0)
sk.bound_violations(reset=True)
ops = np.array([0, 4, 7, 5, 9, 8, 3, 6, 10, 11, 12] * 3, dtype=np.int32)  # AND NAND OR NOR XOR XNOR MUX NOT BUF ONE ZERO
B = len(ops)
i0 = np.where(ops >= 11, -1, 0).astype(np.int32)
i1 = np.where(np.isin(ops, [6, 10, 11, 12]), -1, 1).astype(np.int32)
i2 = np.where(ops == 3, 2, -1).astype(np.int32)
out = np.arange(3, 3 + B, dtype=np.int32)
ct = ck.encrypt([True, False, True])
w = sk.wires(3 + B)
w.upload([0, 1, 2], ct)
w.eval_gate_level(ops, i0, i1, i2, out)
sk.sync()
got = w.download()
host = np.zeros_like(got)
host[:3] = ct
K.KsFirst(oracle.Oracle(ck.params.as_tuple7(), ck.bsk, ck.ksk)).eval_level(host, ops, i0, i1, i2, out)
print("RESULT " + json.dumps({"equal": bool(np.array_equal(got, host)), "violations": sk.bound_violations(),
                              "words": sk.wire_words()}))
sk.close()
"""


def test_one_level_under_the_counting_build():
    lib = os.path.join(ROOT, "helm_amd", "csrc", "libhelm_hip_check.so")
    assert os.path.exists(lib), "make -C helm_amd/csrc libhelm_hip_check.so"
    env = dict(os.environ, HELM_HIP_LIB=lib)
    env.pop("HELM_HIP_KS_MFMA", None)
    p = subprocess.run([sys.executable, "-c", CHILD % (ROOT, ROOT)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert res["equal"] and res["violations"] == [0] * 8 and res["words"] == 513, res


# ---------------------------------------------------------------------------------------------------------------------------
# 7. full size
# ---------------------------------------------------------------------------------------------------------------------------
def test_full_size_level_of_512_mixed_gates():
    """boolean_default_ks_pbs (recalled values): 512 gates, 64 rows against the composition over the oracle's fp route, every
    output decrypted."""
    ck = helm_amd.ClientKey.generate("boolean_default_ks_pbs", seed=2)
    sk = helm_amd.ServerKey(ck, device=0)
    assert sk.kernel_class() == "tuned" and sk.wire_words() == 1025
    p = ck.params
    kN = p.k * p.N
    B = 512
    rng = np.random.default_rng(6)
    bits = rng.integers(0, 2, 3 * B).astype(bool)
    ct = ck.encrypt(bits)
    ops = np.array([BOOT[g % 7] for g in range(B)], dtype=np.int32)
    i0, i1 = np.arange(B, dtype=np.int32), np.arange(B, 2 * B, dtype=np.int32)
    i2 = np.where(ops == O.MUX, np.arange(2 * B, 3 * B), -1).astype(np.int32)
    out = np.arange(3 * B, 4 * B, dtype=np.int32)
    w = sk.wires(4 * B)
    w.upload(np.arange(3 * B), ct)
    w.eval_gate_level(ops, i0, i1, i2, out)
    got = w.download(out)
    assert got.shape == (B, kN + 1)
    plain = np.array([K.plain_gate(int(ops[g]), bits[g], bits[B + g], bits[2 * B + g]) for g in range(B)])
    assert np.array_equal(ck.decrypt(got), plain)
    ref = K.KsFirst(O.Oracle(p.as_tuple7(), ck.bsk, ck.ksk, use_ntt=False, use_fp=True), fp=True)
    for g in range(0, B, 8):  # 64 rows, every gate type among them (8 and 7 are coprime)
        row = lambda i: np.ascontiguousarray(ct[i]) if i >= 0 else None  # noqa: E731
        assert np.array_equal(got[g], ref.gate(int(ops[g]), row(i0[g]), row(i1[g]), row(i2[g]))), g
    sk.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 8. order 0 under the new flag
# ---------------------------------------------------------------------------------------------------------------------------
def test_an_order_0_context_created_with_the_flag_computes_what_it_computed():
    ck = helm_amd.ClientKey.generate("toy_k2", seed=1)
    ops, i0, i1, i2, out = _every_gate_level()
    ct = ck.encrypt([True, False, True])
    tables = []
    for flags in (None, 16):
        sk = helm_amd.ServerKey.__new__(helm_amd.ServerKey)
        sk.params, sk.device = ck.params, 0
        h = nv.vp()
        if flags is None:
            nv.hip_check(nv.hip.helm_hip_ctx_create(0, C.byref(ck.params), C.byref(h)))
        else:
            nv.hip_check(nv.hip.helm_hip_ctx_create_ex(0, C.byref(ck.params), flags, C.byref(h)))
        sk._h = h
        bsk, ksk = np.ascontiguousarray(ck.bsk), np.ascontiguousarray(ck.ksk)
        nv.hip_check(nv.hip.helm_hip_load_bootstrap_key(h, nv.as_u32p(bsk), bsk.size))
        nv.hip_check(nv.hip.helm_hip_load_keyswitch_key(h, nv.as_u32p(ksk), ksk.size))
        assert sk.wire_words() == ck.params.n + 1
        w = sk.wires(3 + len(ops))
        w.upload([0, 1, 2], ct)
        w.eval_gate_level(ops, i0, i1, i2, out)
        tables.append((w.download(), sk.kernel_class(), sk.field_bits(), sk.launch_quantum()))
        sk.close()
    assert np.array_equal(tables[0][0], tables[1][0]) and tables[0][1:] == tables[1][1:]
    host = np.zeros_like(tables[0][0])
    host[:3] = ct
    O.Oracle(ck.params.as_tuple7(), ck.bsk, ck.ksk).eval_level(host, ops, i0, i1, i2, out)
    assert np.array_equal(tables[0][0], host)
