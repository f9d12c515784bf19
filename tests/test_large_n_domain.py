"""Admission of the large-N shape (k = 1, N = 4096: the 5-bit shortint sets) under HELM_SI_CREATE_LARGE_N = 32
(include/helm_shortint.h, helm_amd/csrc/helm_pbs64_large_core.inc, helm_pbs64_large.inc).  The bit may stand alone or beside the generic bits; it
matters at N >= 4096 only; without it every call is what it was.  Parameter checks come before the device lookup, so no GPU
is needed."""
import ctypes as C
import os
import sys

import pytest

import helm_amd
from helm_amd import _native as nv

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ks_edges as E  # noqa: E402

ALLOW, FORCE, MULTIBIT, LARGE = 1, 2, 16, 32
INVALID = -1
GENERIC_DOMAIN_TEXT = (b"unsupported (k,N,pbs_l) for the generic kernel: its domain is N in {256,512,1024,2048}, "
                       b"k >= 1 with (k+1) N <= 4096, pbs_l >= 1, grouping_factor <= 1")
TUNED_TEXT = (b"unsupported (k,N,pbs_l): built variants are k = 1, N in {512,1024,2048}, pbs_l in {1,2}; k in {2,3}, N = 512, "
              b"pbs_l = 1; k = 2, N = 1024, pbs_l = 1")

# (k, N, pbs_l, pbs_logB)
ADMITTED = [(1, 4096, 1, 22), (1, 4096, 2, 15), (1, 4096, 3, 8), (1, 4096, 15, 2)]


def _params(k, N, l, logB, n=12, group=0, msg=4, carry=8):
    p, _, _ = helm_amd.si_named_params("si_toy_512")
    p.n, p.k, p.N, p.pbs_l, p.pbs_logB, p.ks_l, p.ks_logB = n, k, N, l, logB, 3, 5
    p.message_modulus, p.carry_modulus, p.grouping_factor = msg, carry, group
    return p


def _create(p, flags, ex=True):
    h = nv.vp()
    rc = nv.hip.helm_si_ctx_create_ex(0, C.byref(p), flags, C.byref(h)) if ex else nv.hip.helm_si_ctx_create(0, C.byref(p), C.byref(h))
    if rc == 0:
        cls = nv.hip.helm_si_kernel_class(h)
        nv.hip.helm_si_ctx_destroy(h)
        return rc, cls
    assert not h.value
    return rc, nv.hip.helm_hip_last_error()


def test_the_flag_has_the_headers_value():
    assert helm_amd.shortint.SI_CREATE_LARGE_N == LARGE
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "helm_shortint.h")).read()
    assert "HELM_SI_CREATE_LARGE_N = 32" in header


@pytest.mark.parametrize("flags", [LARGE, LARGE | ALLOW, LARGE | FORCE])
@pytest.mark.parametrize("shape", ADMITTED)
def test_admitted_shapes_pass_every_parameter_check(shape, flags):
    """What stops an admitted shape on a machine without a GPU is the device lookup, never HELM_ERR_INVALID; with a GPU the
    context is created and reports class 2 under every generic bit."""
    rc, res = _create(_params(*shape), flags)
    if rc == 0:
        assert res == 2
    else:
        assert rc != INVALID and b"no HIP device" in res, res


@pytest.mark.parametrize("shape,group,want", [
    ((1, 4096, 1, 23), 0, b"capacity"),
    ((2, 4096, 1, 20), 0, b"large-N"),
    ((1, 8192, 1, 20), 0, b"large-N"),
    ((1, 4096, 1, 22), 3, b"large-N"),
])
def test_refusals_with_the_bit(shape, group, want):
    rc, msg = _create(_params(*shape, group=group), LARGE)
    assert rc == INVALID and want in msg, msg
    if want == b"large-N":
        assert b"k = 1, N = 4096" in msg and b"HELM_SI_CREATE_LARGE_N" in msg, msg


def test_the_other_checks_still_apply_in_their_order():
    p = _params(1, 4096, 1, 22, n=1025)
    assert _create(p, LARGE) == (INVALID, b"n must be in [1,1024]")
    p = _params(1, 4096, 1, 22)
    p.ks_logB = 8
    rc, msg = _create(p, LARGE)
    assert rc == INVALID and b"keyswitch decomposition" in msg
    p = _params(1, 4096, 1, 22, msg=64, carry=64)    # t = 4096 > N/2
    rc, msg = _create(p, LARGE)
    assert rc == INVALID and b"power of two <= N/2" in msg
    p = _params(1, 4096, 1, 22, msg=32, carry=64)    # t = 2048 = N/2: admitted
    rc, msg = _create(p, LARGE)
    assert rc != INVALID


@pytest.mark.parametrize("flags", [LARGE | 4, LARGE | 8])
def test_reserved_bits_stay_unknown(flags):
    rc, msg = _create(_params(*ADMITTED[0]), flags)
    assert rc == INVALID and b"unknown bits" in msg and str(flags).encode() in msg, msg
    assert b"HELM_SI_CREATE_LARGE_N = 32" in msg, msg      # the bit itself is known: the message lists it beside the others


@pytest.mark.parametrize("shape", [(1, 2048, 1, 23), (2, 512, 2, 12), (1, 512, 2, 15), (8, 512, 1, 8)])
@pytest.mark.parametrize("flags", [0, ALLOW, FORCE, ALLOW | MULTIBIT, MULTIBIT])
def test_the_bit_changes_nothing_below_4096(shape, flags):
    """A tuned shape, generic shapes and a refused one: the same status and the same message (or class) as without the bit."""
    p = _params(*shape, msg=4, carry=4)
    assert _create(p, flags | LARGE) == _create(p, flags), (shape, flags)


def test_without_the_bit_4096_is_refused_as_today():
    p = _params(1, 4096, 1, 22)
    plain = _create(p, 0, ex=False)
    assert plain == (INVALID, TUNED_TEXT)
    assert _create(p, 0) == plain
    assert _create(p, ALLOW) == (INVALID, GENERIC_DOMAIN_TEXT)
    assert _create(p, FORCE) == (INVALID, GENERIC_DOMAIN_TEXT)
    # the unknown-bits message of a call without the bit does not mention it
    rc, msg = _create(p, 4)
    assert msg == (b"unknown bits in flags 4 (HELM_SI_CREATE_ALLOW_GENERIC = 1, HELM_SI_CREATE_FORCE_GENERIC = 2, "
                   b"HELM_SI_CREATE_GENERIC_MULTIBIT = 16; 4 and 8 are reserved)")


def test_server_key_generic_argument():
    p = _params(*ADMITTED[0])
    with pytest.raises(ValueError, match="'large', 'allow\\+large' or 'force\\+large'"):
        helm_amd.SiServerKey(params=p, generic="sometimes")
    with pytest.raises(helm_amd.HelmError, match="unsupported"):
        helm_amd.SiServerKey(params=p)
    for mode in ("large", "allow+large", "force+large"):
        try:
            sk = helm_amd.SiServerKey(params=p, generic=mode)
            assert sk.kernel_class() == "large" and sk.field_bits() == 50
            sk.close()
        except helm_amd.HelmError as e:  # no device here: the parameter checks passed
            assert "no HIP device" in str(e), e


@pytest.mark.parametrize("name,n,ks,t", [("si_toy_4096", 12, (3, 5), 32), ("shortint_m2c3", None, None, 32)])
def test_the_named_sets(name, n, ks, t):
    p, lwe_std, glwe_std = helm_amd.si_named_params(name)
    assert (p.k, p.N, p.pbs_l, p.pbs_logB, p.message_modulus, p.carry_modulus) == (1, 4096, 1, 22, 4, 8)
    assert p.message_modulus * p.carry_modulus == t and 1 <= p.n <= 1024 and p.grouping_factor == 0
    if n is not None:
        assert p.n == n and (p.ks_l, p.ks_logB) == ks
    else:
        assert glwe_std == 2.0 ** -62
    assert 0 < glwe_std < lwe_std < 1e-3
    rc, res = _create(p, LARGE)
    assert rc != INVALID, res
    assert _create(p, 0)[0] == INVALID


def test_the_matrix_core_keyswitch_planes_hold_at_in_dim_4096():
    """k_ks64_mfma sums, per byte plane, digit x (key byte - 128) over in_dim x LP rows into an int32: at most
    in_dim x ks_l x 2^(ks_logB-1) x 128 (padded levels carry zero digits).  For every (ks_l, ks_logB) a context admits,
    at in_dim = 4096: the largest is 4096 x 8 x 2^6 x 128 = 2^28, a factor 8 below 2^31.  The vector-ALU kernel's digit
    buffer, t_chunk x ks_l x 4 B, is 128 KiB at ks_l = 8 unsliced: inside the 160 KiB its launcher asks for."""
    shapes = E.ks_shapes(64)
    assert len(shapes) == 56 and (8, 7) in shapes
    worst = 0
    for l, logB in shapes:
        assert 1 <= logB <= 7 and 1 <= l <= 8 and l * logB <= 63
        worst = max(worst, 4096 * l * (1 << (logB - 1)) * 128)
        assert 4096 * l * (1 << (logB - 1)) * 128 < 2 ** 31
    assert worst == 2 ** 28
    assert max(4096 * l * 4 for l, _ in shapes) == 128 * 1024 <= 160 * 1024
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "helm_amd", "csrc", "helm_shortint.hip")).read()
    assert "hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024" in src
