"""Admission of k = 1, N = 8192 (the 6-bit shortint sets) under HELM_SI_CREATE_N8192 = 256 (include/helm_shortint.h,
helm_amd/csrc/helm_pbs64_large_core.inc, helm_pbs64_n8192.inc).  The bit may stand alone or beside bits 1, 2, 16, 32 and 64; it matters at N = 8192
only; without it every call is what it was, byte for byte.  Parameter checks come before the device lookup, so no GPU is
needed."""
import ctypes as C
import os
import sys

import pytest

import helm_amd
from helm_amd import _native as nv

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ks_edges as E  # noqa: E402
import test_pbs_first_domain as PF  # noqa: E402

ALLOW, FORCE, MULTIBIT, LARGE, PBS_KS, N8192 = 1, 2, 16, 32, 64, 256
INVALID = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the messages of the parent commit for N = 8192 without the bit
LARGE_TEXT = (b"unsupported (k,N,pbs_l) for the large-N kernel: its domain under HELM_SI_CREATE_LARGE_N is "
              b"k = 1, N = 4096, pbs_l >= 1, grouping_factor <= 1 (k > 1 at N = 4096, multi-bit at "
              b"N = 4096 and N = 8192 are out of scope)")
GENERIC_DOMAIN_TEXT = (b"unsupported (k,N,pbs_l) for the generic kernel: its domain is N in {256,512,1024,2048}, "
                       b"k >= 1 with (k+1) N <= 4096, pbs_l >= 1, grouping_factor <= 1")
TUNED_TEXT = (b"unsupported (k,N,pbs_l): built variants are k = 1, N in {512,1024,2048}, pbs_l in {1,2}; k in {2,3}, N = 512, "
              b"pbs_l = 1; k = 2, N = 1024, pbs_l = 1")

# (k, N, pbs_l, pbs_logB)
ADMITTED = [(1, 8192, 1, 21), (1, 8192, 2, 15), (1, 8192, 3, 8), (1, 8192, 15, 2)]


def _params(k, N, l, logB, n=12, group=0, msg=8, carry=8):
    p, _, _ = helm_amd.si_named_params("si_toy_512")
    p.n, p.k, p.N, p.pbs_l, p.pbs_logB, p.ks_l, p.ks_logB = n, k, N, l, logB, 3, 5
    p.message_modulus, p.carry_modulus, p.grouping_factor = msg, carry, group
    return p


def _create(p, flags):
    h = nv.vp()
    rc = nv.hip.helm_si_ctx_create_ex(0, C.byref(p), flags, C.byref(h))
    if rc == 0:
        got = (nv.hip.helm_si_kernel_class(h), nv.hip.helm_si_field_bits(h))
        nv.hip.helm_si_ctx_destroy(h)
        return rc, got
    assert not h.value
    return rc, nv.hip.helm_hip_last_error()


def test_the_flag_has_the_headers_value():
    assert helm_amd.shortint.SI_CREATE_N8192 == N8192
    header = open(os.path.join(ROOT, "include", "helm_shortint.h")).read()
    assert "HELM_SI_CREATE_N8192 = 256" in header
    shim = open(os.path.join(ROOT, "rust", "helm-hip-sys", "src", "lib.rs")).read()
    assert "pub const HELM_SI_CREATE_N8192: i32 = 256;" in shim


@pytest.mark.parametrize("flags", [N8192, N8192 | ALLOW, N8192 | FORCE, N8192 | LARGE, N8192 | PBS_KS])
@pytest.mark.parametrize("shape", ADMITTED)
def test_admitted_shapes_pass_every_parameter_check(shape, flags):
    """What stops an admitted shape on a machine without a GPU is the device lookup, never HELM_ERR_INVALID; with a GPU the
    context is created and reports class 3 in the 50-bit pair beside every other bit."""
    rc, res = _create(_params(*shape), flags)
    if rc == 0:
        assert res == (3, 50)
    else:
        assert rc != INVALID and b"no HIP device" in res, res


@pytest.mark.parametrize("shape,group,want", [
    ((1, 8192, 1, 22), 0, b"capacity"),
    ((2, 8192, 1, 20), 0, b"HELM_SI_CREATE_N8192"),
    ((1, 8192, 1, 21), 3, b"HELM_SI_CREATE_N8192"),
    ((1, 16384, 1, 20), 0, b"HELM_SI_CREATE_N8192"),
])
@pytest.mark.parametrize("beside", [0, LARGE])
def test_refusals_with_the_bit(shape, group, want, beside):
    rc, msg = _create(_params(*shape, group=group), N8192 | beside)
    assert rc == INVALID and want in msg, msg
    if want != b"capacity":
        assert b"k = 1, N = 8192" in msg and b"N >= 16384" in msg, msg


def test_the_other_checks_still_apply_in_their_order():
    assert _create(_params(1, 8192, 2, 15, n=1025), N8192) == (INVALID, b"n must be in [1,1024]")
    p = _params(1, 8192, 2, 15)
    p.ks_logB = 8
    rc, msg = _create(p, N8192)
    assert rc == INVALID and b"keyswitch decomposition" in msg
    rc, msg = _create(_params(1, 8192, 2, 15, msg=128, carry=64), N8192)    # t = 8192 > N/2
    assert rc == INVALID and b"power of two <= N/2" in msg
    rc, msg = _create(_params(1, 8192, 2, 15, msg=64, carry=64), N8192)     # t = 4096 = N/2: admitted
    assert rc != INVALID, msg
    rc, msg = _create(_params(1, 8192, 2, 15), N8192 | MULTIBIT)            # bit 16 still wants 1 or 2 beside it
    assert rc == INVALID and b"HELM_SI_CREATE_GENERIC_MULTIBIT goes with" in msg
    rc, msg = _create(_params(1, 8192, 2, 15), N8192 | MULTIBIT | ALLOW)
    assert rc != INVALID, msg


@pytest.mark.parametrize("shape", [s for s in PF.SHAPES if s[1] < 8192])
def test_the_bit_changes_nothing_below_8192(shape):
    """Every shape of tests/test_pbs_first_domain.py, beside every combination of the other bits: the same status and the same
    message - or the same class and field - as without the bit.  N = 4096 under bit 32 stays the large-N class."""
    assert shape[1] < 8192
    p = PF._params(*shape, carry=8 if shape[1] == 4096 else 4)
    for f in PF.COMBOS + [c | PBS_KS for c in PF.COMBOS]:
        assert PF._create(p, f | N8192) == PF._create(p, f), (shape, f)


@pytest.mark.parametrize("flags,text", [(0, TUNED_TEXT), (ALLOW, GENERIC_DOMAIN_TEXT), (FORCE, GENERIC_DOMAIN_TEXT),
                                        (LARGE, LARGE_TEXT), (LARGE | ALLOW, LARGE_TEXT), (LARGE | PBS_KS, LARGE_TEXT)])
def test_without_the_bit_8192_is_refused_as_before(flags, text):
    assert _create(_params(1, 8192, 2, 15), flags) == (INVALID, text)


def test_unknown_bits():
    p = _params(*ADMITTED[1])
    rc, msg = _create(p, 128)
    assert msg == (b"unknown bits in flags 128 (HELM_SI_CREATE_ALLOW_GENERIC = 1, HELM_SI_CREATE_FORCE_GENERIC = 2, "
                   b"HELM_SI_CREATE_GENERIC_MULTIBIT = 16; 4 and 8 are reserved)")
    assert rc == INVALID
    rc, msg = _create(p, N8192 | 128)
    assert rc == INVALID and b"unknown bits in flags 384" in msg and b"HELM_SI_CREATE_N8192 = 256" in msg
    rc, msg = _create(p, N8192 | 4)
    assert rc == INVALID
    assert msg == (b"unknown bits in flags 260 (HELM_SI_CREATE_ALLOW_GENERIC = 1, HELM_SI_CREATE_FORCE_GENERIC = 2, "
                   b"HELM_SI_CREATE_GENERIC_MULTIBIT = 16, HELM_SI_CREATE_N8192 = 256; 4 and 8 are reserved)")
    rc, msg = _create(p, 4)                                  # a call without the bit does not mention it
    assert rc == INVALID and b"N8192" not in msg
    rc, msg = _create(p, 512)
    assert rc == INVALID and b"unknown bits" in msg and b"N8192" not in msg


def test_server_key_generic_argument():
    p = _params(*ADMITTED[1])
    with pytest.raises(ValueError, match="'large', 'allow\\+large' or 'force\\+large'"):
        helm_amd.SiServerKey(params=p, generic="sometimes")
    with pytest.raises(ValueError, match="'n8192', 'allow\\+n8192', 'force\\+n8192' or 'large\\+n8192'"):
        helm_amd.SiServerKey(params=p, generic="sometimes")
    with pytest.raises(helm_amd.HelmError, match="unsupported"):
        helm_amd.SiServerKey(params=p)
    with pytest.raises(helm_amd.HelmError, match="N = 8192 are out of scope"):
        helm_amd.SiServerKey(params=p, generic="large")
    for mode in ("n8192", "allow+n8192", "force+n8192", "large+n8192"):
        try:
            sk = helm_amd.SiServerKey(params=p, generic=mode)
            assert sk.kernel_class() == "n8192" and sk.field_bits() == 50
            sk.close()
        except helm_amd.HelmError as e:  # no device here: the parameter checks passed
            assert "no HIP device" in str(e), e


@pytest.mark.parametrize("name,n,pbs,ks", [("si_toy_8192", 12, (2, 15), (3, 5)), ("shortint_m3c3", 864, (2, 15), (6, 3))])
def test_the_named_sets(name, n, pbs, ks):
    p, lwe_std, glwe_std = helm_amd.si_named_params(name)
    assert (p.n, p.k, p.N, p.pbs_l, p.pbs_logB, p.ks_l, p.ks_logB) == (n, 1, 8192) + pbs + ks
    assert (p.message_modulus, p.carry_modulus, p.grouping_factor) == (8, 8, 0)
    if name == "shortint_m3c3":
        assert glwe_std == 2.0 ** -62
    else:
        assert (lwe_std, glwe_std) == (1e-9, 1e-17)
    assert 0 < glwe_std < lwe_std < 1e-3
    rc, res = _create(p, N8192)
    assert rc != INVALID, res
    assert _create(p, 0)[0] == INVALID and _create(p, LARGE)[0] == INVALID


def test_keyswitch_bounds_at_in_dim_8192():
    """k_ks64_mfma sums, per byte plane, digit x (key byte - 128) over in_dim x LP rows into an int32: at most
    in_dim x ks_l x 2^(ks_logB-1) x 128.  For every (ks_l, ks_logB) a context admits, at in_dim = 8192: the largest is
    8192 x 8 x 2^6 x 128 = 2^29, a factor 4 below 2^31.  The vector-ALU kernel's digit buffer, t_chunk x ks_l x 4 B, is
    256 KiB at ks_l = 8 unsliced, over the 160 KiB a workgroup can have: vector_geometry's last clause (restated here) adds
    slices until it fits, and never fires at in_dim <= 4096."""
    shapes = E.ks_shapes(64)
    assert len(shapes) == 56 and (8, 7) in shapes
    worst = max(8192 * l * (1 << (logB - 1)) * 128 for l, logB in shapes)
    assert worst == 2 ** 29 < 2 ** 31

    def slices_for(kN, ks_l, count, n=1024, n_cus=256):
        gx, gy, s = (count + 3) // 4, (n + 1 + 255) // 256, 1
        while s < 16 and gx * gy * s < 2 * n_cus and kN // (s * 2) >= 64:
            s *= 2
        grid_only = s
        while -(-kN // s) * ks_l * 4 > 160 * 1024:
            s *= 2
        return grid_only, s

    for l, _ in shapes:
        for count in (1, 40, 156, 159, 2048, 100000):
            for kN in (512, 1024, 2048, 4096):
                a, b = slices_for(kN, l, count)
                assert a == b                                          # every earlier shape keeps its geometry
            a, b = slices_for(8192, l, count)
            assert -(-8192 // b) * l * 4 <= 160 * 1024
            if 8192 * l * 4 > 160 * 1024:
                assert b >= 2
    assert slices_for(8192, 8, 100000) == (1, 2) and slices_for(8192, 5, 100000) == (1, 1)
    src = open(os.path.join(ROOT, "helm_amd", "csrc", "keyswitch.h")).read()
    assert "while ((size_t)((kN + slices - 1) / slices) * ks_l * sizeof(uint32_t) > (size_t)160 * 1024) slices *= 2;" in src
