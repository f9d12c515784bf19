"""Carry propagation on the many-LUT bootstrap (helm_host_radix_level_ex with HELM_RADIX_MANY_LUT, ArithCircuit(many_lut=True)):
round 1 of RadixEngine::propagate issues ONE rotation per block - message in place, weighted carry state beside it - instead of
two look-ups on the same row.  Same values, fewer rotations; merged rounds cut through pair jobs; off stays word-identical."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helm_amd
import oracle
from helm_amd import ArithCircuit, Circuit, PtxtType, SiEncWireMap, verilog_parser
from helm_amd import _host as H

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from many_lut_audit import ManyLutAuditor  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SET = "si_toy_512"   # 2+2-bit blocks at toy size
ADD, DIV, MANY_LUT = 1, 4, 1


class Op(C.Structure):   # helm_radix_op
    _fields_ = [("kind", C.c_int32), ("a", C.c_int32), ("b", C.c_int32), ("out", C.c_int32),
                ("scalar_lo", C.c_uint64), ("scalar_hi", C.c_uint64)]


def _blocks(x, nb):
    return np.array([(x >> (2 * i)) & 3 for i in range(nb)], dtype=np.uint64)


def _value(ck, rows):
    return sum(int(v) << (2 * i) for i, v in enumerate(ck.decrypt(rows)))


def radix_binary(ck, sk, kind, nb, pairs, flags, entry="ex"):
    """One level of `kind` on every pair at once -> (values, pbs_out, rounds_out)."""
    n = len(pairs)
    ops = (Op * n)()
    for i in range(n):
        ops[i] = Op(kind, (3 * i) * nb, (3 * i + 1) * nb, (3 * i + 2) * nb, 0, 0)
    scratch = int(H.host.helm_host_radix_scratch_rows(sk._h, nb, C.cast(ops, C.c_void_p), n))
    assert scratch >= 0
    w = sk.wires(3 * n * nb + scratch)
    for i, (a, b) in enumerate(pairs):
        w.upload(np.arange(3 * i * nb, (3 * i + 1) * nb), ck.encrypt(_blocks(a, nb)))
        w.upload(np.arange((3 * i + 1) * nb, (3 * i + 2) * nb), ck.encrypt(_blocks(b, nb)))
    pbs, rounds = C.c_int64(), C.c_int64()
    if entry == "ex":
        H.check(H.host.helm_host_radix_level_ex(sk._h, w._h, nb, C.cast(ops, C.c_void_p), n, 3 * n * nb, C.byref(pbs),
                                                C.byref(rounds), flags))
    else:
        H.check(H.host.helm_host_radix_level(sk._h, w._h, nb, C.cast(ops, C.c_void_p), n, 3 * n * nb, C.byref(pbs),
                                             C.byref(rounds)))
    sk.sync()
    vals = [_value(ck, w.download(np.arange((3 * i + 2) * nb, (3 * i + 3) * nb))) for i in range(n)]
    return vals, int(pbs.value), int(rounds.value)


# block sums of a + b: 0xFF + 0x01 generates in block 0 and propagates through the rest; 0xAA + 0x55 propagates, 0xFF + 0xFF
# generates, 0x11 + 0x44 absorbs in every block; the last two mix the three
PAIRS8 = [(0xFF, 0x01), (0xAA, 0x55), (0xFF, 0xFF), (0x11, 0x44), (0x3B, 0xC6), (0xE7, 0x1D)]


def test_one_add_on_four_blocks_saves_the_three_state_look_ups():
    ck, sk = helm_amd.gen_keys_shortint(SET, seed=1)
    for a, b in PAIRS8:
        off, pbs_off, rounds_off = radix_binary(ck, sk, ADD, 4, [(a, b)], 0)
        on, pbs_on, rounds_on = radix_binary(ck, sk, ADD, 4, [(a, b)], MANY_LUT)
        print("ADD u8: pbs_out off", pbs_off, "on", pbs_on, "rounds", rounds_off, rounds_on)
        assert off == on == [(a + b) % 256], (hex(a), hex(b), off, on)
        assert pbs_on == pbs_off - 3 and rounds_on == rounds_off     # the three state look-ups of round 1; no round more
    old, pbs_old, _ = radix_binary(ck, sk, ADD, 4, [PAIRS8[0]], 0, entry="plain")   # the old entry is the flag-off call
    assert old == [0] and pbs_old == pbs_off
    with pytest.raises(helm_amd.HelmError, match="unknown flag"):
        radix_binary(ck, sk, ADD, 4, [PAIRS8[0]], 2)                  # an unknown flag bit
    sk.close()


def test_sixteen_blocks_and_the_carry_out_flag_path():
    ck, sk = helm_amd.gen_keys_shortint(SET, seed=2)
    pairs = [(0xFFFFFFFF, 1), (0x89ABCDEF, 0x76543211), (0x12345678, 0x0FEDCBA9)]
    off, pbs_off, _ = radix_binary(ck, sk, ADD, 16, pairs, 0)
    on, pbs_on, _ = radix_binary(ck, sk, ADD, 16, pairs, MANY_LUT)
    assert off == on == [(a + b) % 2**32 for a, b in pairs]
    assert pbs_on == pbs_off - 15 * len(pairs)                       # blocks 0..14 of each integer had a state look-up
    # division propagates with the carry OUT of the top block kept (`flags`): every block has a state look-up there
    dpairs = [(0xB5, 0x0B), (0xFF, 0x01), (0x64, 0x07)]
    off, pbs_off, r_off = radix_binary(ck, sk, DIV, 4, dpairs, 0)
    on, pbs_on, r_on = radix_binary(ck, sk, DIV, 4, dpairs, MANY_LUT)
    print("DIV u8: pbs_out off", pbs_off, "on", pbs_on)
    assert off == on == [a // b for a, b in dpairs]
    assert pbs_on < pbs_off and r_on == r_off and (pbs_off - pbs_on) % len(dpairs) == 0
    sk.close()


def _chi():
    gs, ws, ins, outs, d, _, _ = verilog_parser.read_verilog_file(os.path.join(HERE, "netlists", "chi_squared_arith.v"), True)
    c = Circuit(gs, ins, outs, d)
    c.sort_circuit()
    c.compute_levels()
    return c, ws


CHI_IN = {"N0": PtxtType.U32(2), "N1": PtxtType.U32(7), "N2": PtxtType.U32(9)}
CHI_OUT = {"alpha": 529, "beta1": 242, "beta2": 275, "beta3": 1250}


def test_chi_squared_whole_circuit_audited_and_cut_by_forced_capacities():
    ck, sk = helm_amd.gen_keys_shortint(SET, seed=1)
    orc = oracle.Oracle64(ck.params.as_tuple(), ck.bsk, ck.ksk, use_ntt=True)
    c, ws = _chi()
    off = ArithCircuit(ck, sk, c)
    off.evaluate_encrypted(off.encrypt_inputs(ws, CHI_IN), 1, "u32")
    n_off = off.pbs_per_cycle()
    aud = ManyLutAuditor(ck, orc, batch_every=3, exact=False)          # the sampled default of tests/test_gpu_audit.py
    sk.set_audit(aud)   # before the evaluator forks its lanes
    ac = ArithCircuit(ck, sk, c, many_lut=True)
    enc = ac.encrypt_inputs(ws, CHI_IN)
    out = ac.evaluate_encrypted(enc, 1, "u32")
    sk.set_audit(None)
    assert {k: int(v.value) for k, v in ac.decrypt_outputs(out, True).items()} == CHI_OUT
    assert not aud.bad, aud.bad[:5]
    assert aud.kinds == {"luts", "lincomb", "many_luts"}
    assert aud.many_rows > 0 and aud.many_outputs > aud.many_rows and aud.lin_checked > 0
    n_on = ac.pbs_per_cycle()
    print("chi-squared u32: rotations per evaluation off", n_off, "on", n_on, "rounds", off.pbs_rounds_per_cycle(),
          ac.pbs_rounds_per_cycle())
    assert aud.luts_seen == n_on < n_off
    # merged rounds cut through pair jobs: capacity 1 (every rotation its own launch) and 3
    for cycle, cap in ((2, 1), (3, 3)):
        ac.set_round_capacity(cap)
        out = ac.evaluate_encrypted(enc, cycle, "u32")
        assert {k: int(v.value) for k, v in ac.decrypt_outputs(out, True).items()} == CHI_OUT, cap
        assert ac.pbs_per_cycle() == n_on and ac.pbs_rounds_per_cycle() >= n_on // cap
    sk.close()


def test_off_stays_off_word_for_word():
    ck, sk = helm_amd.gen_keys_shortint(SET, seed=3)
    c, ws = _chi()
    never = ArithCircuit(ck, sk, c)
    toggled = ArithCircuit(ck, sk, c)
    toggled.set_many_lut(True)
    toggled.set_many_lut(False)
    enc = never.encrypt_inputs(ws, CHI_IN)
    saved = {w: np.array(enc[w], copy=True) for w in enc.keys()}
    a = never.evaluate_encrypted(enc, 1, "u32")
    again = SiEncWireMap(sk, blocks=16)
    for w, ct in saved.items():
        again[w] = ct
    b = toggled.evaluate_encrypted(again, 1, "u32")
    assert set(a.keys()) == set(b.keys())
    for w in a.keys():
        assert np.array_equal(a[w], b[w]), w
    assert never.pbs_per_cycle() == toggled.pbs_per_cycle()
    sk.close()


def test_setter_refuses_other_block_shapes():
    p, a, b = helm_amd.si_named_params(SET)
    p.message_modulus = p.carry_modulus = 2
    ck = helm_amd.SiClientKey(p, a, b, seed=4)
    sk = helm_amd.SiServerKey(ck)
    c, _ = _chi()
    ac = ArithCircuit(ck, sk, c)
    with pytest.raises(helm_amd.HelmError, match="2\\+2-bit"):
        ac.set_many_lut(True)
    ac.set_many_lut(False)
    sk.close()


CHILD = r"""
import json, sys
sys.path[:0] = [%r, %r]
import helm_amd
import test_gpu_radix_many_lut as T
ck, sk = helm_amd.gen_keys_shortint(T.SET, seed=1)
sk.bound_violations(reset=True)
vals, pbs, _ = T.radix_binary(ck, sk, T.ADD, 4, T.PAIRS8, T.MANY_LUT)
res = {"ok": vals == [(a + b) %% 256 for a, b in T.PAIRS8], "pbs": pbs, "violations": sk.bound_violations()}
sk.close()
print("RESULT " + json.dumps(res))
"""


def test_counting_build_counts_nothing_in_the_add():
    """One child process on libhelm_hip_check.so: the ADD case on the many-LUT path, values right, every counter zero."""
    lib = os.path.join(ROOT, "helm_amd", "csrc", "libhelm_hip_check.so")
    assert os.path.exists(lib), "make -C helm_amd/csrc libhelm_hip_check.so"
    env = dict(os.environ, HELM_HIP_LIB=lib)
    p = subprocess.run([sys.executable, "-c", CHILD % (ROOT, HERE)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert res["ok"] and res["violations"] == [0] * 8, res
