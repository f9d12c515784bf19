"""Client side of the bootstrap-first order (helm_si_client_encrypt_small / _decrypt_small, include/helm_client.h) and the
reference the GPU tests of the order compare with (tests/pbs_first.py), on the CPU.

  round trip      every value of t under the small key, toy sets of every shape class
  noise           the phase of a small row is v * delta within 6 sigma of the set's LWE noise, and is not noiseless
  key generation  unchanged: digests of an order-1 key's BSK, KSK and one big ciphertext, recorded on the parent commit
  the reference   pbs_first.py on si_toy_512, against an independent route: decrypt with the LWE secret and compare with the
                  plaintext function, for every input value; a LUT level and a linear combination likewise
  the named set   shortint_m2c2_pbs_ks: m2c2's shape, and the failure probabilities its comment states follow from the
                  formulas of tests/test_gpu_noise.py"""
import hashlib
import math
import os
import sys

import numpy as np
import pytest

import helm_amd
import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pbs_first as PF  # noqa: E402

TOYS = ["si_toy_512", "si_toy_1024", "si_toy_512_k3", "si_toy_1024_k2", "si_toy_1024_mb2", "si_toy_4096"]


@pytest.mark.parametrize("name", TOYS)
def test_small_rows_round_trip_for_every_value(name):
    ck = helm_amd.SiClientKey.generate(name, seed=5)
    p, t = ck.params, ck.t
    v = np.arange(2 * t, dtype=np.uint64)            # values are taken mod t
    ct = ck.encrypt(v, small=True)
    assert ct.shape == (2 * t, p.n + 1) and ct.dtype == np.uint64
    assert list(ck.decrypt_message_and_carry(ct, small=True)) == [int(x) % t for x in v]
    assert list(ck.decrypt(ct, small=True)) == [int(x) % t % p.message_modulus for x in v]
    one = ck.encrypt(3, small=True)
    assert one.shape == (p.n + 1,) and ck.decrypt_message_and_carry(one, small=True) == 3
    # the big-key functions are what they were
    big = ck.encrypt(v)
    assert big.shape == (2 * t, p.k * p.N + 1)
    assert list(ck.decrypt_message_and_carry(big)) == [int(x) % t for x in v]


@pytest.mark.parametrize("name,sigma", [("si_toy_512", 1e-9), ("shortint_m2c2", 0.000007069849454709433)])
def test_small_rows_carry_the_lwe_noise(name, sigma):
    """(the named full-size set's client key is generated with a toy GLWE side: only n and the LWE noise matter here)"""
    p, lwe_std, glwe_std = helm_amd.si_named_params(name)
    assert lwe_std == sigma
    if p.N > 512:
        p.N, p.pbs_logB = 512, 15
    ck = helm_amd.SiClientKey(p, lwe_std, glwe_std, seed=9)
    v = np.arange(4096, dtype=np.uint64) % ck.t
    ct = ck.encrypt(v, small=True)
    err = (ck.phase(ct, small=True) - v * np.uint64(ck.delta)).astype(np.int64).astype(np.float64) / 2.0 ** 64
    assert np.abs(err).max() < 6 * sigma
    assert 0.9 * sigma < err.std() < 1.1 * sigma      # 4096 samples: the estimate is within 3.3 % at 3 standard deviations
    assert abs(err.mean()) < 0.1 * sigma
    masks = ct[:, :p.n]
    assert len(np.unique(masks)) == masks.size        # fresh uniform masks


# recorded on the parent commit (SiClientKey.generate(name, seed=11): sha256 of bsk, ksk, encrypt(arange(t)))
PARENT_DIGESTS = {
    "si_toy_512": ("7f52414b6e728d402b5455da5d8e677a3c56d38c80f269f5b63a63f3a30358d9", "765c41152181593bfee9972dedeb005c6349f30e3224c0aed2c1b46f346fd2ae", "4cd8200cd0132d50a26377fc1de50440774d05ad924f44fef5b03a35b5a8e2e9"),
    "si_toy_1024_mb2": ("f49c0bb9d443a0bf8d45fbe42ffec4af704600f95f3e16ef6fc8d65748f09e98", "b029f29b2f8f24d21e864c60136048a8ef04c97686d0be9c41838da040a7bca8", "f14c66cd79f4768ab89398bbbfa581ea0d768972d8311e7df467abe6f45a1796"),
}


@pytest.mark.parametrize("name", sorted(PARENT_DIGESTS))
def test_key_generation_and_big_encryption_are_the_parents(name):
    ck = helm_amd.SiClientKey.generate(name, seed=11)
    h = lambda a: hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint64).tobytes()).hexdigest()  # noqa: E731
    assert (h(ck.bsk), h(ck.ksk), h(ck.encrypt(np.arange(ck.t, dtype=np.uint64)))) == PARENT_DIGESTS[name]


@pytest.fixture(scope="module")
def toy():
    ck = helm_amd.SiClientKey.generate("si_toy_512", seed=5)
    orc = oracle.Oracle64(ck.params.as_tuple(), ck.bsk, ck.ksk, use_ntt=True)
    return ck, PF.PbsFirst(orc)


def test_the_reference_look_up_decrypts_to_the_function_for_every_input(toy):
    ck, ref = toy
    t = ck.t
    for f in (lambda v: (5 * v + 3) % t, lambda v: v * v % t, lambda v: t - 1 - v):
        lut = ref.orc.make_lut(f)
        rows = ck.encrypt(np.arange(t, dtype=np.uint64), small=True)
        for v in range(t):
            out = ref.apply_lut_small(rows[v], lut)
            assert out.shape == (ck.params.n + 1,)
            assert ref.decrypt(ck.lwe_secret, out) == f(v), v                    # the reference's own decryption
            assert ck.decrypt_message_and_carry(out, small=True) == f(v), v      # the client library's
            # the composition: the big row in between decrypts to the same value under the big key
            assert ck.decrypt_message_and_carry(ref.orc.bootstrap(rows[v], lut)) == f(v)


def test_the_reference_level_and_linear_steps_decrypt(toy):
    ck, ref = toy
    bits = [1, 0, 1, 1]
    w = np.zeros((10, ck.params.n + 1), dtype=np.uint64)
    w[:4] = ck.encrypt(bits, small=True)
    before = w.copy()
    # a full adder on rows 0..2 (sum, carry), a bivariate AND, a negation, a latch that reads a row the level writes in place
    arity = [3, 3, 2, 1, 0, 3]
    in_idx = [[0, 1, 2], [0, 1, 2], [0, 1, -1], [2, -1, -1], [1, -1, -1], [3, 2, 0]]
    table = [0x96, 0xE8, 0x8, 1, 0, 0xCA]
    out = [4, 5, 6, 7, 8, 3]                                                     # gate 5 rewrites its own input row 3
    ref.eval_lut_level(w, arity, in_idx, table, out)
    a, b, c, d = bits
    want = {4: a ^ b ^ c, 5: (a & b) | (a & c) | (b & c), 6: a & b, 8: b, 3: (0xCA >> (d * 4 + c * 2 + a)) & 1}
    for r, v in want.items():
        assert ck.decrypt_message_and_carry(w[r], small=True) == v, r
    assert ck.decrypt_message_and_carry(w[7], small=True) == (ck.t - c) % ck.t      # smart_neg: -x mod t
    assert np.array_equal(w[[0, 1, 2, 9]], before[[0, 1, 2, 9]])
    ref.lincomb(w, [[4, 5, -1], [0, 1, 2]], [[1, 2, 0], [4, 2, 1]], [9, 0], const_add=[3, 0])
    assert ck.decrypt_message_and_carry(w[9], small=True) == (want[4] + 2 * want[5] + 3) % ck.t
    assert ck.decrypt_message_and_carry(w[0], small=True) == 4 * a + 2 * b + c


def test_the_reference_many_lut_outputs_decrypt(toy):
    ck, ref = toy
    t, N = ck.t, ck.params.N
    fs = [lambda v: (3 * v + 1) % t, lambda v: (v + 7) % t, lambda v: (2 * v) % t]
    M = PF.ML.chunks(len(fs))
    tv = PF.ML.many_lut_poly([[f(v) for v in range(t // M)] for f in fs], t, N)
    v = t // M - 1
    row = ck.encrypt(v, small=True)
    outs = ref.many_lut_outputs(row, tv, len(fs), ck.bsk)
    assert [ck.decrypt_message_and_carry(o, small=True) for o in outs] == [f(v) for f in fs]
    assert np.array_equal(outs[0], ref.apply_lut_small(row, tv))     # output 0 is the plain look-up's row, word for word


def _predicted(p, s_lwe, s_glwe):
    """tests/test_gpu_noise.py predicted(), classical blind rotation"""
    B, Bk = 2.0 ** p.pbs_logB, 2.0 ** p.ks_logB
    br = p.n * (p.pbs_l * (p.k + 1) * p.N * ((B * B + 2) / 12) * s_glwe ** 2 + (1 + p.k * p.N / 2) / (24 * B ** (2 * p.pbs_l)))
    ks = p.k * p.N * p.ks_l * ((Bk * Bk + 2) / 12) * s_lwe ** 2 + p.k * p.N / (24 * Bk ** (2 * p.ks_l))
    ms = (1 + p.n / 2) / (48 * p.N * p.N)
    return br, ks, ms


def _log2_pfail(margin, variance):
    return math.log2(math.erfc(margin / math.sqrt(2 * variance)))


def test_the_named_set_for_the_order():
    """shortint_m2c2_pbs_ks is an APPROXIMATE set (helm_client64.cpp): m2c2's shape, an LWE side chosen for order 0, where a
    wire row carries blind rotation + keyswitch noise and the next look-up adds the modulus switch.  The figures its comment
    states are what the formulas give; 2^-40 is the failure probability tfhe quotes for its shortint sets, and m2c2's own LWE
    side misses it in order 0 (which is why the set exists)."""
    p, s_lwe, s_glwe = helm_amd.si_named_params("shortint_m2c2_pbs_ks")
    q, q_lwe, q_glwe = helm_amd.si_named_params("shortint_m2c2")
    assert (p.k, p.N, p.pbs_l, p.pbs_logB, p.message_modulus, p.carry_modulus, p.grouping_factor) == \
           (q.k, q.N, q.pbs_l, q.pbs_logB, q.message_modulus, q.carry_modulus, q.grouping_factor)
    assert s_glwe == q_glwe and q.n < p.n <= 1024 and s_lwe < q_lwe
    assert abs(math.log2(s_lwe) - (-15.58 - 0.02643 * (p.n - 684))) < 0.01       # the security line the comment names
    half_box = 1 / (4 * p.message_modulus * p.carry_modulus)
    br, ks, ms = _predicted(p, s_lwe, s_glwe)
    stated = {1: -84, 5: -72, 21: -46.5}       # fresh output, 2x + y, 4x + 2y + z: sum of squared coefficients
    for amp, want in stated.items():
        got = _log2_pfail(half_box, amp * (br + ks) + ms)
        assert abs(got - want) < 1.0, (amp, got)
        assert got < -40
    br, ks, ms = _predicted(q, q_lwe, q_glwe)
    assert abs(_log2_pfail(half_box, br + ks + ms) - (-40.3)) < 0.1             # the formulas' own check (test_gpu_noise.py)
    assert _log2_pfail(half_box, 21 * (br + ks) + ms) > -10                      # m2c2's LWE side in order 0
