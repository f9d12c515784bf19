"""The shape domain of the 64-bit engine's generic blind-rotate kernel (helm_amd/csrc/helm_pbs64_generic.inc), reached through
helm_si_ctx_create_ex with HELM_SI_CREATE_ALLOW_GENERIC or HELM_SI_CREATE_FORCE_GENERIC (include/helm_shortint.h): N in
{256, 512, 1024, 2048}, k >= 1 with (k+1) N <= 4096, pbs_l >= 1, no multi-bit, and every other check of
helm_si_ctx_create (the two-prime capacity bound included).  Without a flag nothing changes: the shapes the existing tests
pin keep today's messages.  Parameter checks come before the device lookup, so no GPU is needed."""
import ctypes as C

import pytest

import helm_amd
from helm_amd import _native as nv

ALLOW, FORCE = 1, 2
INVALID = -1


def _params(k, N, l, logB, n=16, ks_l=4, ks_logB=4, group=0):
    p, _, _ = helm_amd.si_named_params("si_toy_512")
    p.n, p.k, p.N, p.pbs_l, p.pbs_logB, p.ks_l, p.ks_logB = n, k, N, l, logB, ks_l, ks_logB
    p.grouping_factor = group
    return p


def _create(p, flags):
    h = nv.vp()
    rc = nv.hip.helm_si_ctx_create_ex(0, C.byref(p), flags, C.byref(h))
    if rc == 0:
        cls = nv.hip.helm_si_kernel_class(h)
        nv.hip.helm_si_ctx_destroy(h)
        return rc, cls
    assert not h.value
    return rc, nv.hip.helm_hip_last_error()


@pytest.mark.parametrize("k,N,l", [(2, 1024, 2), (2, 512, 2), (2, 2048, 1)])
def test_without_flags_the_pinned_k2_shapes_keep_their_message(k, N, l):
    """tests/test_shortint_m2c1_params.py::test_other_k2_shapes_stay_unsupported, through both entry points."""
    p, _, _ = helm_amd.si_named_params("si_toy_1024_k2")
    p.N, p.pbs_l = N, l
    if l == 2:
        p.pbs_logB = 12
    h = nv.vp()
    assert nv.hip.helm_si_ctx_create(0, C.byref(p), C.byref(h)) == INVALID
    old = nv.hip.helm_hip_last_error()
    rc, msg = _create(p, 0)
    assert rc == INVALID and msg == old
    assert b"unsupported" in msg and b"k = 2, N = 1024" in msg, msg


def test_without_flags_every_existing_check_keeps_its_message():
    """tests/test_abi.py::test_shortint_parameter_validation_needs_no_device and test_gpu_shortint.py::test_errors: the
    same failures with byte-identical messages from helm_si_ctx_create and from helm_si_ctx_create_ex(flags = 0)."""
    m2c2, _, _ = helm_amd.si_named_params("shortint_m2c2")
    toy, _, _ = helm_amd.si_named_params("si_toy_512")
    cases = [(m2c2, "k", 2, b"unsupported"), (m2c2, "N", 4096, b"unsupported"), (m2c2, "pbs_logB", 31, b"decomposition"),
             (m2c2, "message_modulus", 3, b"power of two"), (m2c2, "ks_logB", 9, b"keyswitch"),
             (m2c2, "grouping_factor", 4, b"grouping_factor"), (m2c2, "grouping_factor", 3, b"grouping_factor"),
             (m2c2, "pbs_logB", 24, b"capacity"), (toy, "k", 2, b"unsupported")]
    for base, field, value, want in cases:
        bad = helm_amd.SiParams.from_buffer_copy(base)
        setattr(bad, field, value)
        h = nv.vp()
        assert nv.hip.helm_si_ctx_create(0, C.byref(bad), C.byref(h)) == INVALID
        old = nv.hip.helm_hip_last_error()
        rc, msg = _create(bad, 0)
        assert rc == INVALID and msg == old and want in msg, (field, value, msg)


@pytest.mark.parametrize("flags", [ALLOW, FORCE, ALLOW | FORCE])
@pytest.mark.parametrize("k,N,l,logB", [(2, 512, 2, 12), (7, 512, 1, 22), (15, 256, 1, 22), (1, 2048, 3, 8),
                                        (3, 1024, 1, 21), (1, 256, 15, 2), (4, 512, 1, 22), (2, 1024, 2, 12)])
def test_shapes_inside_the_domain_pass_every_parameter_check(k, N, l, logB, flags):
    """What stops an admitted shape on a machine without a GPU is the device lookup (HELM_ERR_NO_DEVICE), never
    HELM_ERR_INVALID; with a GPU the context is created and runs the generic kernel."""
    rc, res = _create(_params(k, N, l, logB), flags)
    if rc == 0:
        assert res == 1
    else:
        assert rc != INVALID and b"no HIP device" in res, res


@pytest.mark.parametrize("k,N,l,logB", [(2, 512, 2, 12), (7, 512, 1, 22), (15, 256, 1, 22), (1, 2048, 3, 8)])
def test_untuned_shapes_stay_refused_without_a_flag(k, N, l, logB):
    rc, msg = _create(_params(k, N, l, logB), 0)
    assert rc == INVALID and b"unsupported" in msg, msg


@pytest.mark.parametrize("k,N,l,logB,want", [
    (1, 4096, 1, 8, b"unsupported"),    # N above the domain: FpG2 has no 2N-th root of unity
    (1, 128, 2, 8, b"unsupported"),     # N below it
    (8, 512, 1, 8, b"unsupported"),     # (k+1) N = 4608 > 4096
    (16, 256, 1, 8, b"unsupported"),    # 4352 > 4096
    (3, 2048, 1, 8, b"unsupported"),    # 8192 > 4096
    (0, 512, 2, 8, b"unsupported"),     # k = 0
    (2, 512, 0, 8, b"unsupported"),     # pbs_l = 0
    (1, 2048, 1, 24, b"capacity"),      # 2 x 2048 x 2^23 x 2^63 = 2^98 > p0 p1 / 2
    (2, 512, 2, 25, b"decomposition"),  # pbs_logB above 24
    (1, 256, 8, 4, b"decomposition"),   # logB l = 32
])
@pytest.mark.parametrize("flags", [ALLOW, FORCE])
def test_shapes_outside_the_domain_are_refused_with_their_reason(k, N, l, logB, want, flags):
    rc, msg = _create(_params(k, N, l, logB), flags)
    assert rc == INVALID and want in msg, msg


def test_the_unsupported_message_names_the_generic_domain():
    rc, msg = _create(_params(1, 4096, 1, 8), ALLOW)
    assert rc == INVALID
    assert b"unsupported" in msg and b"{256,512,1024,2048}" in msg and b"(k+1) N <= 4096" in msg, msg


def test_multi_bit_has_no_generic_form():
    # grouping factor 3 on an untuned shape, with either flag
    for flags in (ALLOW, FORCE):
        rc, msg = _create(_params(2, 1024, 1, 20, n=18, group=3), flags)
        assert rc == INVALID and b"multi-bit" in msg, msg
    # FORCE on the tuned multi-bit set
    mb, _, _ = helm_amd.si_named_params("shortint_m2c2_multibit3")
    rc, msg = _create(mb, FORCE)
    assert rc == INVALID and b"multi-bit" in msg, msg
    # ALLOW leaves the tuned multi-bit set alone: it passes validation
    rc, res = _create(mb, ALLOW)
    assert rc == 0 and res == 0 or (rc != INVALID and b"no HIP device" in res), res


@pytest.mark.parametrize("flags", [4, 8, 5, -1])
def test_unknown_flag_bits_are_refused(flags):
    rc, msg = _create(_params(1, 1024, 1, 20), flags)
    assert rc == INVALID and b"flags" in msg, msg


def test_server_key_generic_argument():
    p = _params(2, 512, 2, 12)
    with pytest.raises(ValueError):
        helm_amd.SiServerKey(params=p, generic="sometimes")
    with pytest.raises(helm_amd.HelmError, match="unsupported"):
        helm_amd.SiServerKey(params=p)
    try:
        helm_amd.SiServerKey(params=p, generic="allow").close()
    except helm_amd.HelmError as e:  # no device here: the parameter checks passed
        assert "no HIP device" in str(e), e
