"""The 3-bit shortint shape (k = 2, N = 1024, one PBS level): PARAM_MESSAGE_2_CARRY_1_KS_PBS, the set of the reference's
LUT-mode test (reference tests/circuit_test.rs:13, 287), as the named set shortint_m2c1, and its toy twin si_toy_1024_k2.
The parameters, the oracle's bootstrap at this shape, and the admission rule of the 64-bit engine (k = 2 is built at
N = 512 and N = 1024 with one level, nothing else).  CPU only: context creation refuses an unsupported shape before it
looks for a device."""
import ctypes as C

import numpy as np
import pytest

import helm_amd
import oracle
from helm_amd import _native as nv


@pytest.mark.parametrize("name", ["shortint_m2c1", "si_toy_1024_k2"])
def test_named_set_has_the_3_bit_shape(name):
    p, s_lwe, s_glwe = helm_amd.si_named_params(name)
    assert (p.k, p.N, p.pbs_l, p.message_modulus, p.carry_modulus, p.grouping_factor) == (2, 1024, 1, 4, 2, 0)
    assert 2 <= p.pbs_logB <= 23  # 3 * 1024 * 2^(logB - 1) * 2^63 below the two-prime CRT range (2^97.5)
    assert s_lwe > 0 and s_glwe > 0


def test_full_set_dimensions_and_capacity():
    p, _, _ = helm_amd.si_named_params("shortint_m2c1")
    assert p.as_tuple() == (742, 2, 1024, 1, 23, 5, 3, 4, 2, 0)
    bound = (p.k + 1) * p.pbs_l * p.N * 2 ** (p.pbs_logB - 1) * 2 ** 63
    assert bound * 1.001 < 2 ** 97.5


def test_client_key_and_encryption_at_t_8():
    ck = helm_amd.SiClientKey.generate("si_toy_1024_k2", seed=4)
    assert ck.t == 8 and ck.dim == 2 * 1024
    vals = np.arange(ck.t, dtype=np.uint64)
    ct = ck.encrypt(vals)
    assert ct.shape == (ck.t, ck.dim + 1)
    assert np.array_equal(ck.decrypt_message_and_carry(ct), vals)
    assert ck.bsk.size == ck.params.n * 9 * ck.params.N  # (k + 1)^2 polynomials per GGSW
    # gen_keys_shortint builds the full set's client key through the same path (the server half needs a device)
    full = helm_amd.SiClientKey.generate("shortint_m2c1", seed=4)
    assert full.t == 8 and np.array_equal(full.decrypt_message_and_carry(full.encrypt(vals)), vals)


def test_oracle_bootstrap_of_every_value_decrypts_to_the_lut():
    ck = helm_amd.SiClientKey.generate("si_toy_1024_k2", seed=5)
    orc = oracle.Oracle64(ck.params.as_tuple(), ck.bsk, ck.ksk)
    f = lambda v: (3 * v + 5) % ck.t
    lut = orc.make_lut(f)
    for v in range(ck.t):
        out = orc.apply_lut(ck.encrypt(v), lut)  # keyswitch, bootstrap, sample extract
        assert ck.decrypt_message_and_carry(out) == f(v), v
        assert orc.decrypt(ck.glwe_secret, out) == f(v)


def test_three_input_lut_packs_into_t_8():
    """gates::lut() packs three bits into 0..7 (reference src/gates.rs:773-778): with t = 8 every combination is a value."""
    ck = helm_amd.SiClientKey.generate("si_toy_1024_k2", seed=6)
    orc = oracle.Oracle64(ck.params.as_tuple(), ck.bsk, ck.ksk)
    combos = [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]
    wires = np.zeros((3 * len(combos) + len(combos), ck.dim + 1), dtype=np.uint64)
    wires[:3 * len(combos)] = ck.encrypt(np.array(combos, dtype=np.uint64).reshape(-1))
    in_idx = np.arange(3 * len(combos), dtype=np.int32).reshape(len(combos), 3)
    out_idx = np.arange(3 * len(combos), 4 * len(combos), dtype=np.int32)
    table = 0xE8  # majority
    orc.eval_lut_level(wires, np.full(len(combos), 3, np.int32), in_idx, np.full(len(combos), table, np.uint64), out_idx)
    got = ck.decrypt_message_and_carry(wires[out_idx])
    assert [int(g) for g in got] == [(table >> (4 * a + 2 * b + c)) & 1 for a, b, c in combos]


@pytest.mark.parametrize("N,pbs_l", [(1024, 2), (512, 2), (2048, 1)])
def test_other_k2_shapes_stay_unsupported(N, pbs_l):
    p, _, _ = helm_amd.si_named_params("si_toy_1024_k2")
    bad = helm_amd.SiParams.from_buffer_copy(p)
    bad.N, bad.pbs_l = N, pbs_l
    if pbs_l == 2:
        bad.pbs_logB = 12
    h = nv.vp()
    assert nv.hip.helm_si_ctx_create(0, C.byref(bad), C.byref(h)) == -1
    msg = nv.hip.helm_hip_last_error()
    assert b"unsupported" in msg and b"k = 2, N = 1024" in msg, msg


def test_the_3_bit_shape_passes_validation():
    """Without a device the admitted shape gets past every parameter check and fails only where the device is looked up
    (with one, it is created); before this set existed the same call failed with "unsupported"."""
    p, _, _ = helm_amd.si_named_params("shortint_m2c1")
    h = nv.vp()
    rc = nv.hip.helm_si_ctx_create(0, C.byref(p), C.byref(h))
    if rc == 0:
        nv.hip.helm_si_ctx_destroy(h)
        return
    msg = nv.hip.helm_hip_last_error()
    assert b"unsupported" not in msg and b"capacity" not in msg, msg
