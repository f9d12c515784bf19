"""LUT levels that share rotations (helm_si_set_level_many_lut / LutCircuit(many_lut=True)): gates of a level on the same
inputs in the same order are the functions of one many-LUT table.  The 8-bit adder of full adders (0x96 and 0xE8 on the same
three inputs) at the 4-bit toy set: every wire right, every dispatch recomputed through the audit hook against
tests/many_lut.py, 8 rotations where the switch off takes 16; one mixed level; a t = 4 set (nothing to group); a forked lane."""
import os
import sys

import numpy as np
import pytest

import helm_amd
import oracle
from helm_amd import Circuit, LutCircuit, PtxtType, verilog_parser

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from many_lut_audit import ManyLutAuditor  # noqa: E402

pytestmark = pytest.mark.gpu
NET = os.path.join(os.path.dirname(os.path.abspath(__file__)), "netlists")
SET = "si_toy_512"   # t = 16


def _adder():
    gs, ws, ins, outs, d, _, _ = verilog_parser.read_verilog_file(os.path.join(NET, "8-bit-adder-lut-3-1.v"), False)
    c = Circuit(gs, ins, outs, d)
    c.sort_circuit()
    c.compute_levels()
    return c, ws


def test_adder_of_full_adders_one_rotation_per_pair():
    ck, sk = helm_amd.gen_keys_shortint(SET, seed=1)
    orc = oracle.Oracle64(ck.params.as_tuple(), ck.bsk, ck.ksk, use_ntt=True)
    c, ws = _adder()
    a, b, cin = 0xB7, 0x6E, 1
    inputs = {f"a[{i}]": PtxtType.Bool((a >> i) & 1) for i in range(8)}
    inputs.update({f"b[{i}]": PtxtType.Bool((b >> i) & 1) for i in range(8)})
    inputs["cin"] = PtxtType.Bool(cin)
    ptxt = c.evaluate(c.initialize_wire_map(ws, inputs, "bool"))
    # the switch off, in the same run: 16 look-ups, kind 0 records only
    off = LutCircuit(ck, sk, c)
    aud0 = ManyLutAuditor(ck, orc)
    sk.set_audit(aud0)
    enc0 = off.evaluate_encrypted(off.encrypt_inputs(ws, inputs), 1, "bool")
    n_off = off.pbs_per_cycle()
    assert not aud0.bad and "many_luts" not in aud0.kinds
    # ... and on
    on = LutCircuit(ck, sk, c, many_lut=True)
    aud = ManyLutAuditor(ck, orc, exact=True)
    sk.set_audit(aud)
    sk.timing_enable(True)
    sk.timing(reset=True)
    enc = on.evaluate_encrypted(on.encrypt_inputs(ws, inputs), 1, "bool")
    sk.sync()
    rotations = int(sk.timing().pbs_count)
    sk.set_audit(None)
    n_on = on.pbs_per_cycle()
    print("rotations per evaluation: off", n_off, "on", n_on, "engine count", rotations)
    assert n_off == 16 and n_on == 8 and rotations == 8
    assert not aud.bad, aud.bad[:5]
    assert aud.many_batches == 8 and aud.many_rows == 8 and aud.many_outputs == 16 and aud.luts_checked == aud.luts_seen == 8
    for wire, want in ptxt.items():
        assert ck.decrypt(enc[wire]) == int(bool(want)) == ck.decrypt(enc0[wire]), wire
    on.set_many_lut(False)
    sk.close()


def _mixed_level(sk, ck, cts, many):
    """One level: a pair (0x96, 0xE8 on rows 0 1 2), a lone arity-3 gate (rows 2 1 0: another order), an arity-2 gate, an
    arity-1 gate (negation) and a flip-flop.  -> (table rows after the level, rotations)"""
    rng = np.random.default_rng(11)
    rows = 12
    w = sk.wires(rows)
    w.upload(np.arange(rows), rng.integers(0, 2**64, size=(rows, ck.dim + 1), dtype=np.uint64))
    w.upload([0, 1, 2, 3], cts)
    arity = [3, 3, 3, 2, 1, 0]
    in_idx = [[0, 1, 2], [0, 1, 2], [2, 1, 0], [1, 3, -1], [3, -1, -1], [0, -1, -1]]
    table = [0x96, 0xE8, 0xCA, 0x6, 1, 0]
    out_idx = [4, 5, 6, 7, 8, 9]
    sk.set_level_many_lut(many)
    sk.timing_enable(True)
    sk.timing(reset=True)
    w.eval_lut_level(arity, in_idx, table, out_idx)
    sk.sync()
    n = int(sk.timing().pbs_count)
    sk.set_level_many_lut(False)
    return w.download(), n


def test_one_mixed_level_ungrouped_gates_word_identical():
    ck, sk = helm_amd.gen_keys_shortint(SET, seed=2)
    orc = oracle.Oracle64(ck.params.as_tuple(), ck.bsk, ck.ksk, use_ntt=True)
    cts = ck.encrypt(np.array([1, 0, 1, 1], dtype=np.uint64))   # the same input ciphertexts both times
    off, n_off = _mixed_level(sk, ck, cts, False)
    aud = ManyLutAuditor(ck, orc, exact=True)
    sk.set_audit(aud)
    on, n_on = _mixed_level(sk, ck, cts, True)
    sk.set_audit(None)
    assert (n_off, n_on) == (4, 3)
    assert not aud.bad and aud.many_batches == 1 and aud.many_outputs == 4
    # the lone arity-3 gate, the arity-2 gate, the negation, the flip-flop and every row the level does not write: word for
    # word.  (The pair's rows come from another test polynomial - 0xE8 in its second half - so their values are compared.)
    untouched = [r for r in range(12) if r not in (4, 5)]
    assert np.array_equal(on[untouched], off[untouched])
    x = [1, 0, 1, 1]
    want = {4: x[0] ^ x[1] ^ x[2], 5: int(x[0] + x[1] + x[2] >= 2), 6: (0xCA >> (x[2] * 4 + x[1] * 2 + x[0])) & 1,
            7: (0x6 >> (x[1] * 2 + x[3])) & 1, 9: x[0]}
    for r, v in want.items():
        assert int(ck.decrypt(on[r])) == v == int(ck.decrypt(off[r])), r
    t = ck.t
    assert int(ck.decrypt_message_and_carry(on[8])) == (t - x[3]) % t     # smart_neg
    sk.close()


def test_read_after_write_inside_a_level_is_still_refused():
    ck, sk = helm_amd.gen_keys_shortint(SET, seed=2)
    sk.set_level_many_lut(True)
    w = sk.wires(8)
    w.upload([0, 1, 2], ck.encrypt(np.array([1, 0, 1], dtype=np.uint64)))
    with pytest.raises(helm_amd.HelmError, match="read-after-write"):
        w.eval_lut_level([3, 3], [[0, 1, 2], [0, 1, 4]], [0x96, 0xE8], [4, 5])
    with pytest.raises(helm_amd.HelmError, match="write-after-write"):
        w.eval_lut_level([3, 3], [[0, 1, 2], [0, 1, 2]], [0x96, 0xE8], [4, 4])
    sk.close()


def test_nothing_to_group_at_t_4():
    p, a, b = helm_amd.si_named_params(SET)
    p.message_modulus = p.carry_modulus = 2
    ck = helm_amd.SiClientKey(p, a, b, seed=4)
    sk = helm_amd.SiServerKey(ck)
    rng = np.random.default_rng(12)
    sentinel = rng.integers(0, 2**64, size=(6, ck.dim + 1), dtype=np.uint64)
    cts = ck.encrypt(np.array([1, 1], dtype=np.uint64))
    res = []
    for many in (False, True):
        w = sk.wires(6)
        w.upload(np.arange(6), sentinel)
        w.upload([0, 1], cts)
        sk.set_level_many_lut(many)                     # accepted
        sk.timing_enable(True)
        sk.timing(reset=True)
        w.eval_lut_level([2, 2], [[0, 1], [0, 1]], [0x6, 0x8], [2, 3])   # a half adder: same inputs, but 2^2 = t
        sk.sync()
        res.append((w.download(), int(sk.timing().pbs_count)))
    assert res[0][1] == res[1][1] == 2
    assert np.array_equal(res[0][0], res[1][0])
    assert [int(v) for v in ck.decrypt(res[1][0][[2, 3]])] == [0, 1]
    sk.close()


def test_a_lane_forked_afterwards_inherits_the_setting():
    ck, sk = helm_amd.gen_keys_shortint(SET, seed=2)
    before = sk.fork()
    sk.set_level_many_lut(True)
    after = sk.fork()
    counts = []
    for ctx in (before, after):
        w = sk.wires(6)
        w.upload([0, 1, 2], ck.encrypt(np.array([1, 1, 0], dtype=np.uint64)))
        sk.sync()
        v = helm_amd.shortint.SiWires.__new__(helm_amd.shortint.SiWires)
        v.sk, v.n_rows, v._h = ctx, w.n_rows, w._h
        ctx.timing_enable(True)
        ctx.timing(reset=True)
        try:
            v.eval_lut_level([3, 3], [[0, 1, 2], [0, 1, 2]], [0x96, 0xE8], [3, 4])
        finally:
            v._h = None
        ctx.sync()
        counts.append(int(ctx.timing().pbs_count))
        assert [int(x) for x in ck.decrypt(w.download([3, 4]))] == [0, 1]
    assert counts == [2, 1]
    sk.close()
