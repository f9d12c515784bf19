"""Admission of keyswitch-first keys (pbs_order = 1) by helm_hip_ctx_create_ex with HELM_HIP_CREATE_KS_PBS = 16, and the client
side of such keys (include/helm_hip.h, include/helm_client.h).  Every refusal comes before a device is touched: no GPU needed."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import helm_amd
from helm_amd import _native as nv
from helm_amd import engine

KS_PBS = 16
ORDER0_MSG = b"only pbs_order = 0 (bootstrap then keyswitch)"
ORDER1_SETS = ["toy_ks_pbs", "toy_k2_ks_pbs", "toy_1024_ks_pbs", "boolean_default_ks_pbs"]


def _create(p, flags):
    h = nv.vp()
    rc = nv.hip.helm_hip_ctx_create_ex(0, C.byref(p), flags, C.byref(h))
    return rc, h, nv.hip.helm_hip_last_error()


def _params(name, **over):
    p, _, _ = helm_amd.named_params(name)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def test_the_header_and_the_python_layer_agree_on_the_flag():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "helm_hip.h")).read()
    assert "HELM_HIP_CREATE_KS_PBS = 16" in header and "helm_hip_wire_words" in header
    assert engine.HIP_CREATE_KS_PBS == KS_PBS


@pytest.mark.parametrize("name,flags", [("toy_ks_pbs", 16), ("toy_ks_pbs", 17), ("toy_ks_pbs", 18), ("toy_k2_ks_pbs", 16),
                                        ("toy_1024_ks_pbs", 16), ("boolean_default_ks_pbs", 16), ("boolean_default_ks_pbs", 17),
                                        ("toy_crt", 17), ("toy_crt", 18)])
def test_order_1_is_admitted_under_the_bit(name, flags):
    """What stops an admitted set on a box without a GPU is the device lookup (HELM_ERR_NO_DEVICE), never HELM_ERR_INVALID;
    with a device the row width is k N + 1 and the class is the shape's own."""
    p = _params(name, pbs_order=1)
    rc, h, err = _create(p, flags)
    if rc == 0:
        assert nv.hip.helm_hip_wire_words(h) == p.k * p.N + 1
        assert nv.hip.helm_hip_kernel_class(h) == (2 if name == "toy_crt" else 0)
        nv.hip.helm_hip_ctx_destroy(h)
    else:
        assert rc != -1, err


def test_a_generic_shape_is_admitted_in_order_1():
    p = _params("toy_k2_ks_pbs", pbs_l=2, pbs_logB=7)  # (2, 512, 2, 7): no tuned build
    rc, h, err = _create(p, 16)
    if rc == 0:
        assert nv.hip.helm_hip_kernel_class(h) == 1
        nv.hip.helm_hip_ctx_destroy(h)
    else:
        assert rc != -1, err


@pytest.mark.parametrize("flags", [19, 20, 24])
@pytest.mark.parametrize("order", [0, 1])
def test_bad_flag_combinations_with_the_bit_are_refused(flags, order):
    rc, h, err = _create(_params("toy_ks_pbs", pbs_order=order), flags)
    assert rc == -1 and not h.value
    assert b"HELM_HIP_CREATE_ALLOW_CRT" in err and b"HELM_HIP_CREATE_FORCE_CRT" in err, err


@pytest.mark.parametrize("flags", [0, 1, 2])
def test_order_1_without_the_bit_is_refused_with_the_message_of_before(flags):
    rc, h, err = _create(_params("toy_ks_pbs"), flags)
    assert rc == -1 and not h.value and err == ORDER0_MSG, err
    h2 = nv.vp()
    assert nv.hip.helm_hip_ctx_create(0, C.byref(_params("toy_ks_pbs")), C.byref(h2)) == -1
    assert nv.hip.helm_hip_last_error() == ORDER0_MSG


@pytest.mark.parametrize("order", [2, -1, 16])
@pytest.mark.parametrize("flags", [16, 17, 18])
def test_an_order_outside_0_and_1_is_refused_under_the_bit(order, flags):
    rc, h, err = _create(_params("toy_ks_pbs", pbs_order=order), flags)
    assert rc == -1 and not h.value and b"pbs_order" in err, err


@pytest.mark.parametrize("what,val,msg", [("n", 1025, b"n must be"), ("grouping_factor", 2, b"grouping_factor"),
                                          ("torus_bits", 64, b"torus_bits"), ("N", 128, b"unsupported"),
                                          ("ks_l", 7, b"keyswitch decomposition"), ("pbs_logB", 14, b"capacity")])
def test_the_other_checks_run_unchanged_under_the_bit(what, val, msg):
    """Byte for byte the refusal of the same parameters in order 0 without the bit."""
    rc, h, err = _create(_params("toy_ks_pbs", **{what: val}), 16)
    assert rc == -1 and not h.value and msg in err, err
    assert _create(_params("toy", **{what: val}), 0)[2] == err


def test_the_bit_with_order_0_passes_validation():
    rc, h, err = _create(_params("toy"), 16)
    if rc == 0:
        assert nv.hip.helm_hip_wire_words(h) == _params("toy").n + 1
        nv.hip.helm_hip_ctx_destroy(h)
    else:
        assert rc != -1, err


def test_wire_words_of_a_null_context_is_an_error():
    assert nv.hip.helm_hip_wire_words(None) < 0


# ---------------------------------------------------------------------------------------------------------------------------
# client
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_named_order_1_sets():
    for name in ORDER1_SETS:
        p, a, b = helm_amd.named_params(name)
        assert p.pbs_order == 1 and p.grouping_factor == 1 and p.torus_bits == 32
    for toy in ("toy", "toy_k2", "toy_1024"):
        p0, a0, b0 = helm_amd.named_params(toy)
        p1, a1, b1 = helm_amd.named_params(toy + "_ks_pbs")
        assert p0.as_tuple7() == p1.as_tuple7() and (a0, b0) == (a1, b1) and p0.pbs_order == 0
    p, a, b = helm_amd.named_params("boolean_default_ks_pbs")
    assert p.as_tuple7() == (664, 2, 512, 3, 6, 4, 3) and a == 0.0000380828277062 and b == 0.00000004990272175010415
    assert p.as_tuple7()[1:] == helm_amd.named_params("boolean_default")[0].as_tuple7()[1:]


@pytest.mark.parametrize("name", ["toy_ks_pbs", "toy_k2_ks_pbs", "boolean_default_ks_pbs"])
def test_order_1_keys_encrypt_and_decrypt_rows_of_kN_plus_1_words(name):
    p, lwe_std, glwe_std = helm_amd.named_params(name)
    if name.startswith("boolean"):
        p.n = 8  # the key material is not under test here: keep key generation short
    ck = helm_amd.ClientKey(p, lwe_std, glwe_std, seed=11)
    kN = p.k * p.N
    assert ck.ct_words() == kN + 1
    bits = np.random.default_rng(3).integers(0, 2, 64).astype(bool)
    ct = ck.encrypt(bits)
    assert ct.shape == (64, kN + 1) and ct.dtype == np.uint32
    assert np.array_equal(ck.decrypt(ct), bits)
    assert ck.decrypt(ct[5]) == bool(bits[5]) and ck.encrypt(True).shape == (kN + 1,)
    # the phase under the GLWE key sits within 6 sigma (glwe_noise_std) of +-1/8
    ph = ck.phase(ct, big=True).astype(np.int64)
    want = np.where(bits, 0x20000000, 0xE0000000).astype(np.int64)
    err = ((ph - want + (1 << 31)) % (1 << 32)) - (1 << 31)
    sigma = glwe_std * 2.0 ** 32
    print(f"{name}: sigma = {sigma:.2f} words, largest |error| = {np.abs(err).max()}")
    assert np.abs(err).max() <= 6 * sigma
    assert np.abs(err).max() > 0  # noise was drawn at all


def test_an_order_0_key_draws_the_words_it_always_drew():
    """Digests taken on the commit before keyswitch-first keys existed: toy, seed 7, eight booleans, and the keyswitching key."""
    ck = helm_amd.ClientKey.generate("toy", seed=7)
    assert ck.ct_words() == ck.params.n + 1
    ct = ck.encrypt(np.array([0, 1, 1, 0, 1, 0, 0, 1], dtype=bool))
    assert hashlib.sha256(ct.tobytes()).hexdigest() == "4387a39061b4de06e83e565ce1b3f779662ee99a9bdca953385c5632f82e13ad"
    assert hashlib.sha256(np.ascontiguousarray(ck.ksk).tobytes()).hexdigest() == \
        "93b27b63b6ef19192816ffd0272325cf83f84623b846cb86fc8a55cef631be6b"


def test_the_key_material_does_not_depend_on_the_order():
    """The server key holds the same two objects in the same layouts: only the encryption key choice differs."""
    a = helm_amd.ClientKey.generate("toy", seed=7)
    b = helm_amd.ClientKey.generate("toy_ks_pbs", seed=7)
    assert np.array_equal(a.bsk, b.bsk) and np.array_equal(a.ksk, b.ksk)
    assert np.array_equal(a.glwe_secret, b.glwe_secret) and np.array_equal(a.lwe_secret, b.lwe_secret)


def test_keygen_refuses_an_order_outside_0_and_1():
    p, a, b = helm_amd.named_params("toy")
    p.pbs_order = 2
    with pytest.raises(helm_amd.HelmError if hasattr(helm_amd, "HelmError") else Exception):
        helm_amd.ClientKey(p, a, b, seed=1)
