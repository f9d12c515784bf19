"""tests/ks_first.py - the keyswitch-first level composed of the oracle's parts - pinned under toy_ks_pbs: every gate type's
truth table decrypts, the schoolbook and NTT routes of the oracle agree word for word, and the keyswitch stage of the
composition is the plain Python-integer keyswitch of tests/ks_edges.py on crafted rows.  CPU only."""
import itertools
import os
import sys

import numpy as np
import pytest

import helm_amd
import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ks_edges as E  # noqa: E402
import ks_first as K  # noqa: E402


@pytest.fixture(scope="module")
def toy():
    ck = helm_amd.ClientKey.generate("toy_ks_pbs", seed=21)
    orc = oracle.Oracle(ck.params.as_tuple7(), ck.bsk, ck.ksk)
    ct = {False: ck.encrypt(False), True: ck.encrypt(True)}
    return ck, K.KsFirst(orc), ct


@pytest.mark.parametrize("op", [oracle.AND, oracle.NAND, oracle.OR, oracle.NOR, oracle.XOR, oracle.XNOR])
def test_binary_truth_tables_decrypt(toy, op):
    ck, ref, ct = toy
    for a, b in itertools.product((False, True), repeat=2):
        out = ref.gate(op, ct[a], ct[b])
        assert out.shape == (ck.params.k * ck.params.N + 1,)
        assert ck.decrypt(out) == K.plain_gate(op, a, b), (op, a, b)


def test_mux_truth_table_decrypts(toy):
    ck, ref, ct = toy
    for a, b, c in itertools.product((False, True), repeat=3):
        assert ck.decrypt(ref.gate(oracle.MUX, ct[a], ct[b], ct[c])) == (a if c else b), (a, b, c)


def test_linear_gates_decrypt(toy):
    ck, ref, ct = toy
    for a in (False, True):
        assert ck.decrypt(ref.gate(oracle.NOT, ct[a])) == (not a)
        assert np.array_equal(ref.gate(oracle.BUF, ct[a]), ct[a]) and np.array_equal(ref.gate(oracle.DFF, ct[a]), ct[a])
    one, zero = ref.gate(oracle.CONST_ONE), ref.gate(oracle.CONST_ZERO)
    assert ck.decrypt(one) and not ck.decrypt(zero)
    assert not one[:-1].any() and one[-1] == K.PT_TRUE and zero[-1] == K.PT_FALSE


def test_the_schoolbook_and_the_ntt_route_agree_word_for_word(toy):
    ck, ref, ct = toy
    exact = K.KsFirst(oracle.Oracle(ck.params.as_tuple7(), ck.bsk, ck.ksk, use_ntt=False))
    for op in (oracle.AND, oracle.NAND, oracle.OR, oracle.NOR, oracle.XOR, oracle.XNOR):
        assert np.array_equal(exact.gate(op, ct[True], ct[False]), ref.gate(op, ct[True], ct[False])), op
    assert np.array_equal(exact.gate(oracle.MUX, ct[True], ct[False], ct[True]), ref.gate(oracle.MUX, ct[True], ct[False], ct[True]))


def test_a_level_reads_the_table_as_it_was(toy):
    """eval_level: a gate that updates its own row in place, beside one that reads that row."""
    ck, ref, ct = toy
    w = np.stack([ct[True], ct[True], ct[False]])  # (the NOT first would turn the MUX to its other input)
    ref.eval_level(w, [oracle.MUX, oracle.NOT], [0, 0], [2, -1], [1, -1], [2, 1])  # w2 = w1 ? w0 : w2 ; w1 = !w0
    assert list(ck.decrypt(w)) == [True, False, True]


def test_the_keyswitch_stage_on_crafted_rows_is_the_plain_keyswitch(toy):
    """AND passes in0's words through (in1 = 0), NAND negates them, XOR doubles them, the second MUX half is -c + e: the
    small row of the composition is keyswitch_exact of that linear combination (keyswitch_exact itself is pinned to the
    Python-integer double loop by tests/test_keyswitch_edges.py)."""
    ck, ref, ct = toy
    p = ck.params
    kN = p.k * p.N
    rows = E.crafted_rows(kN, p.ks_logB, p.ks_l, 32)
    zero = np.zeros(kN + 1, dtype=np.uint32)
    key = np.ascontiguousarray(ck.ksk).reshape(kN, p.ks_l, p.n + 1)
    for r in range(len(rows)):
        row = np.ascontiguousarray(rows[r])
        cases = [(oracle.AND, 0, row, zero, None), (oracle.NAND, 0, row, zero, None), (oracle.XOR, 0, row, zero, None),
                 (oracle.MUX, 1, zero, zero, row)]
        for op, which, a, b, c in cases:
            lin = ref.lin(op, which, a, b, c)
            want = E.keyswitch_exact(lin[None, :], key, p.ks_logB, p.ks_l, 32)[0]
            assert np.array_equal(ref.small(op, which, a, b, c), want), (E.CRAFTED[r], op)
        assert np.array_equal(ref.lin(oracle.AND, 0, row, zero)[:kN], row[:kN])
        assert np.array_equal(ref.lin(oracle.XOR, 0, row, zero)[:kN], row[:kN] * np.uint32(2))
        assert np.array_equal(ref.lin(oracle.MUX, 1, zero, zero, row)[:kN], np.uint32(0) - row[:kN])
