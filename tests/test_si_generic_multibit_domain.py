"""The shape domain of the generic 64-bit kernel's multi-bit form (helm_amd/csrc/helm_pbs64_generic.inc), opened by
HELM_SI_CREATE_GENERIC_MULTIBIT = 16 together with HELM_SI_CREATE_ALLOW_GENERIC or HELM_SI_CREATE_FORCE_GENERIC
(include/helm_shortint.h): the generic domain's N, k and pbs_l limits with grouping_factor 2 or 3 dividing n, without the
tuned multi-bit build's pbs_l = 1, N >= 1024.  Without the bit every multi-bit refusal stands with its message.  Parameter
checks come before the device lookup, so no GPU is needed."""
import ctypes as C

import pytest

import helm_amd
from helm_amd import _native as nv

ALLOW, FORCE, MULTIBIT = 1, 2, 16
INVALID = -1

# (k, N, pbs_l, pbs_logB, n, grouping_factor)
SHAPES = [(2, 512, 2, 12, 6, 3), (3, 512, 1, 18, 6, 2), (1, 256, 3, 7, 6, 3), (7, 512, 1, 22, 6, 2), (1, 512, 1, 20, 6, 3),
          (1, 2048, 2, 14, 6, 2)]


def _params(k, N, l, logB, n, group):
    p, _, _ = helm_amd.si_named_params("si_toy_512")
    p.n, p.k, p.N, p.pbs_l, p.pbs_logB, p.ks_l, p.ks_logB = n, k, N, l, logB, 4, 4
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


def test_the_flag_has_the_headers_value():
    assert helm_amd.shortint.SI_CREATE_GENERIC_MULTIBIT == MULTIBIT


@pytest.mark.parametrize("flags", [ALLOW | MULTIBIT, FORCE | MULTIBIT, ALLOW | FORCE | MULTIBIT])
@pytest.mark.parametrize("shape", SHAPES)
def test_multi_bit_shapes_inside_the_domain_pass_every_parameter_check(shape, flags):
    """What stops an admitted shape on a machine without a GPU is the device lookup (HELM_ERR_NO_DEVICE), never
    HELM_ERR_INVALID; with a GPU the context is created and runs the generic kernel."""
    rc, res = _create(_params(*shape), flags)
    if rc == 0:
        assert res == 1
    else:
        assert rc != INVALID and b"no HIP device" in res, res


@pytest.mark.parametrize("flags", [MULTIBIT, MULTIBIT | 4, MULTIBIT | 8])
def test_the_bit_alone_and_the_reserved_bits_are_refused(flags):
    rc, msg = _create(_params(*SHAPES[0]), flags)
    assert rc == INVALID and b"flags" in msg, msg


@pytest.mark.parametrize("flags", [ALLOW | MULTIBIT, FORCE | MULTIBIT])
@pytest.mark.parametrize("shape,want", [
    ((2, 512, 2, 12, 8, 4), b"grouping_factor"),   # g = 4
    ((2, 512, 2, 12, 7, 3), b"grouping_factor"),   # g does not divide n
    ((8, 512, 1, 8, 6, 2), b"unsupported"),        # (k+1) N = 4608 > 4096
    ((1, 4096, 1, 8, 6, 3), b"unsupported"),       # N above the domain
])
def test_shapes_outside_the_domain_are_refused_with_their_reason(shape, want, flags):
    rc, msg = _create(_params(*shape), flags)
    assert rc == INVALID and want in msg, msg


@pytest.mark.parametrize("shape", SHAPES)
def test_without_the_bit_the_multi_bit_refusals_stand(shape):
    """Flags 1 and 2 on the same shapes: today's refusals, byte for byte."""
    k, N, l = shape[:3]
    tuned = k == 1 and N in (512, 1024, 2048) and l in (1, 2)  # (the k > 1 builds take no grouping factor at all)
    rc, msg = _create(_params(*shape), ALLOW)
    assert rc == INVALID
    if tuned:  # a tuned classical shape without a tuned multi-bit form
        assert msg == b"multi-bit blind rotation is built for pbs_l = 1, N >= 1024 (every tfhe multi-bit set)", msg
    else:
        assert msg == (b"multi-bit blind rotation (grouping_factor > 1) runs on the tuned builds only: this shape "
                       b"(k,N,pbs_l) has none, and the generic kernel has no multi-bit form"), msg
    rc, msg = _create(_params(*shape), FORCE)
    assert rc == INVALID
    assert msg == b"HELM_SI_CREATE_FORCE_GENERIC: the generic kernel has no multi-bit form (grouping_factor > 1)", msg


def test_shapes_without_grouping_behave_as_under_the_plain_flags():
    for flags in (ALLOW, FORCE):
        for shape in [(2, 512, 2, 12, 6, 0), (1, 4096, 1, 8, 6, 0), (1, 2048, 1, 24, 6, 1)]:
            assert _create(_params(*shape), flags | MULTIBIT) == _create(_params(*shape), flags), (flags, shape)


def test_server_key_generic_argument():
    p = _params(*SHAPES[0])
    with pytest.raises(ValueError):
        helm_amd.SiServerKey(params=p, generic="multibit")
    with pytest.raises(helm_amd.HelmError, match="multi-bit"):
        helm_amd.SiServerKey(params=p, generic="allow")
    for mode in ("allow+multibit", "force+multibit"):
        try:
            helm_amd.SiServerKey(params=p, generic=mode).close()
        except helm_amd.HelmError as e:  # no device here: the parameter checks passed
            assert "no HIP device" in str(e), e
