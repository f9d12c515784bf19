"""Admission under HELM_SI_CREATE_PBS_KS = 64 (include/helm_shortint.h): the bit chooses the bootstrap-first ciphertext order
and changes no admission rule.  It may stand alone or beside any admitted combination of bits 1, 2, 16, 32; bits 4 and 8 stay
reserved; a call without the bit returns what it returned, message bytes included.  Parameter checks come before the device
lookup, so no GPU is needed: with one, a context is created and the getters are read as well."""
import ctypes as C
import os

import pytest

import helm_amd
from helm_amd import _native as nv

ALLOW, FORCE, MULTIBIT, LARGE, PBS_KS = 1, 2, 16, 32, 64
INVALID = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every combination of bits 1, 2, 16, 32 a call may carry (admitted or not: the status must not depend on bit 64)
COMBOS = [0, ALLOW, FORCE, ALLOW | FORCE, ALLOW | MULTIBIT, FORCE | MULTIBIT, LARGE, ALLOW | LARGE, FORCE | LARGE,
          ALLOW | MULTIBIT | LARGE, FORCE | MULTIBIT | LARGE, MULTIBIT, MULTIBIT | LARGE]

# (k, N, pbs_l, pbs_logB, grouping_factor): twelve shapes over every kernel class, and two no flag admits
SHAPES = [
    (1, 512, 2, 15, 0),    # k_pbs64
    (1, 512, 1, 20, 0),    # k_pbs64, one level
    (1, 1024, 1, 23, 0),   # k_pbs64s
    (1, 2048, 1, 23, 0),   # k_pbs64s (shortint_m2c2's shape)
    (1, 2048, 2, 14, 0),   # k_pbs64s, two levels
    (3, 512, 1, 18, 0),    # k_pbs64k (shortint_m1c1's shape)
    (2, 512, 1, 20, 0),    # k_pbs64k
    (2, 1024, 1, 23, 0),   # k_pbs64k at N = 1024
    (1, 1024, 1, 22, 2),   # k_pbs64s multi-bit
    (1, 2048, 1, 21, 3),   # k_pbs64s multi-bit, groups of 3
    (2, 512, 2, 12, 0),    # k_pbs64_generic (under ALLOW / FORCE only)
    (1, 4096, 1, 22, 0),   # k_pbs64_large (under LARGE only)
    (8, 512, 1, 8, 0),     # outside every domain
    (1, 8192, 1, 20, 0),   # outside every domain
]


def _params(k, N, l, logB, group=0, n=12, msg=4, carry=4):
    p, _, _ = helm_amd.si_named_params("si_toy_512")
    p.n, p.k, p.N, p.pbs_l, p.pbs_logB, p.ks_l, p.ks_logB = n, k, N, l, logB, 3, 5
    p.message_modulus, p.carry_modulus, p.grouping_factor = msg, carry, group
    return p


def _create(p, flags):
    """-> (status, what the context reports) or (status, message)"""
    h = nv.vp()
    rc = nv.hip.helm_si_ctx_create_ex(0, C.byref(p), flags, C.byref(h))
    if rc == 0:
        got = (nv.hip.helm_si_kernel_class(h), nv.hip.helm_si_field_bits(h))
        order, words = nv.hip.helm_si_pbs_order(h), nv.hip.helm_si_wire_words(h)
        nv.hip.helm_si_ctx_destroy(h)
        assert (order, words) == ((0, p.n + 1) if flags & PBS_KS else (1, p.k * p.N + 1))
        return rc, got
    assert not h.value
    return rc, nv.hip.helm_hip_last_error()


def test_the_flag_has_the_headers_value():
    assert helm_amd.shortint.SI_CREATE_PBS_KS == PBS_KS
    header = open(os.path.join(ROOT, "include", "helm_shortint.h")).read()
    assert "HELM_SI_CREATE_PBS_KS = 64" in header
    for name in ("int helm_si_pbs_order(const helm_si_ctx *ctx);", "int64_t helm_si_wire_words(const helm_si_ctx *ctx);"):
        assert name in header


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "k%d_N%d_l%d_B%d_g%d" % s)
def test_the_bit_changes_no_admission_rule(shape):
    """The same status beside every combination of the other bits - and the same message where the call is refused, the same
    kernel class and field where a device is present and the context is made."""
    p = _params(*shape, carry=8 if shape[1] == 4096 else 4)
    admitted = 0
    for flags in COMBOS:
        without, with_bit = _create(p, flags), _create(p, flags | PBS_KS)
        assert with_bit == without, (shape, flags, without, with_bit)
        admitted += without[0] != INVALID
    assert (admitted > 0) == (shape[0] != 8 and shape[1] != 8192)


def test_the_other_checks_still_apply_in_their_order():
    assert _create(_params(1, 512, 2, 15, n=1025), PBS_KS) == (INVALID, b"n must be in [1,1024]")
    p = _params(1, 512, 2, 15)
    p.ks_logB = 8
    rc, msg = _create(p, PBS_KS)
    assert rc == INVALID and b"keyswitch decomposition" in msg
    rc, msg = _create(_params(1, 2048, 1, 25), PBS_KS)
    assert rc == INVALID and b"PBS decomposition" in msg
    # a message that quotes the flags quotes them without the bit, as it does for bit 32
    assert _create(_params(1, 512, 2, 15), MULTIBIT | PBS_KS) == _create(_params(1, 512, 2, 15), MULTIBIT)
    assert b"flags 16:" in _create(_params(1, 512, 2, 15), MULTIBIT | PBS_KS)[1]


@pytest.mark.parametrize("other", COMBOS)
@pytest.mark.parametrize("reserved", [4, 8, 12])
def test_reserved_bits_stay_unknown(reserved, other):
    flags = PBS_KS | reserved | other
    rc, msg = _create(_params(1, 512, 2, 15), flags)
    assert rc == INVALID and msg.startswith(b"unknown bits in flags %d (" % flags), msg
    assert b"HELM_SI_CREATE_PBS_KS = 64" in msg and msg.endswith(b"; 4 and 8 are reserved)"), msg
    assert (b"HELM_SI_CREATE_LARGE_N = 32" in msg) == bool(other & LARGE)


def test_higher_bits_are_unknown_with_and_without_the_bit():
    for flags in (128, 128 | PBS_KS, 1 << 20):
        rc, msg = _create(_params(1, 512, 2, 15), flags)
        assert rc == INVALID and b"unknown bits" in msg
        assert (b"HELM_SI_CREATE_PBS_KS" in msg) == bool(flags & PBS_KS)


def test_without_the_bit_the_unknown_bits_message_is_byte_identical():
    for p in (_params(1, 512, 2, 15), _params(1, 4096, 1, 22, carry=8)):
        assert _create(p, 4)[1] == (b"unknown bits in flags 4 (HELM_SI_CREATE_ALLOW_GENERIC = 1, HELM_SI_CREATE_FORCE_GENERIC = 2, "
                                    b"HELM_SI_CREATE_GENERIC_MULTIBIT = 16; 4 and 8 are reserved)")
        assert _create(p, 8 | LARGE)[1] == (b"unknown bits in flags 40 (HELM_SI_CREATE_ALLOW_GENERIC = 1, "
                                            b"HELM_SI_CREATE_FORCE_GENERIC = 2, HELM_SI_CREATE_GENERIC_MULTIBIT = 16, "
                                            b"HELM_SI_CREATE_LARGE_N = 32; 4 and 8 are reserved)")


def test_getters_refuse_a_null_context():
    assert nv.hip.helm_si_pbs_order(None) == INVALID
    assert nv.hip.helm_si_wire_words(None) == INVALID


def test_server_key_order_argument():
    p = _params(1, 512, 2, 15)
    with pytest.raises(ValueError, match="'ks_pbs' or 'pbs_ks'"):
        helm_amd.SiServerKey(params=p, order="small")
    for order, want in (("ks_pbs", (1, 513)), ("pbs_ks", (0, 13))):
        try:
            sk = helm_amd.SiServerKey(params=p, order=order)
            assert (sk.pbs_order(), sk.wire_words()) == want and sk.dim == 512 and sk.wire_dim == want[1] - 1
            sk.close()
        except helm_amd.HelmError as e:  # no device here: the parameter checks passed
            assert "no HIP device" in str(e), e
    with pytest.raises(helm_amd.HelmError, match="unsupported"):     # the order admits nothing the shape does not
        helm_amd.SiServerKey(params=_params(8, 512, 1, 8), order="pbs_ks")
