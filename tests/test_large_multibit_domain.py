"""Admission of multi-bit blind rotation (grouping_factor 2 or 3) at k = 1, N = 4096 and N = 8192 under
HELM_SI_CREATE_LARGE_MULTIBIT = 1024 (include/helm_shortint.h, helm_amd/csrc/helm_pbs64_large_core.inc, helm_pbs64_large.inc, helm_pbs64_n8192.inc).  The
bit goes with bit 32 and/or bit 256; it matters for grouping_factor > 1 at N >= 4096 only; without it every call is what it
was, byte for byte.  Parameter checks come before the device lookup, so no GPU is needed."""
import os
import sys

import pytest

import helm_amd

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_n8192_domain as ND  # noqa: E402
import test_pbs_first_domain as PF  # noqa: E402

ALLOW, FORCE, MULTIBIT, LARGE, PBS_KS, N8192, LARGE_MB = 1, 2, 16, 32, 64, 256, 1024
INVALID = -1
ROOT = ND.ROOT
_params, _create = ND._params, ND._create

# the parent commit's text for a multi-bit shape at N = 8192 under bit 256 (test_n8192_domain.py checks its parts)
N8192_TEXT = (b"unsupported (k,N,pbs_l) for the N = 8192 kernel: its domain under HELM_SI_CREATE_N8192 is "
              b"k = 1, N = 8192, pbs_l >= 1, grouping_factor <= 1 (k > 1 at N = 8192, multi-bit at "
              b"N = 8192 and N >= 16384 are out of scope)")
DECOMPS = [(1, 20), (2, 15), (3, 8)]


def test_the_flag_has_the_headers_value():
    assert helm_amd.shortint.SI_CREATE_LARGE_MULTIBIT == LARGE_MB
    header = open(os.path.join(ROOT, "include", "helm_shortint.h")).read()
    assert "HELM_SI_CREATE_LARGE_MULTIBIT = 1024" in header
    shim = open(os.path.join(ROOT, "rust", "helm-hip-sys", "src", "lib.rs")).read()
    assert "pub const HELM_SI_CREATE_LARGE_MULTIBIT: i32 = 1024;" in shim


# (N, the bits beside the flag): bit 32 alone serves N = 4096 only, bit 256 alone N = 8192 only (test_refusals_by_name)
BESIDE = [(4096, LARGE), (8192, N8192), (4096, LARGE | N8192), (8192, LARGE | N8192), (4096, LARGE | ALLOW), (8192, N8192 | ALLOW),
          (4096, LARGE | N8192 | FORCE | MULTIBIT), (4096, LARGE | PBS_KS), (8192, N8192 | PBS_KS), (8192, LARGE | N8192 | PBS_KS)]


@pytest.mark.parametrize("N,beside", BESIDE, ids=lambda v: str(v))
@pytest.mark.parametrize("l,logB", DECOMPS)
@pytest.mark.parametrize("g", [2, 3])
def test_admitted_shapes_pass_every_parameter_check(g, l, logB, N, beside):
    """What stops an admitted shape on a machine without a GPU is the device lookup, never HELM_ERR_INVALID; with a GPU the
    context is created in the class of its N and the 50-bit pair."""
    rc, res = _create(_params(1, N, l, logB, group=g), LARGE_MB | beside)
    if rc == 0:
        assert res == ((2 if N == 4096 else 3), 50)
    else:
        assert rc != INVALID and b"no HIP device" in res, res


def test_the_flag_goes_with_bit_32_or_256():
    p = _params(1, 4096, 1, 20, group=2)
    for flags in (LARGE_MB, LARGE_MB | ALLOW, LARGE_MB | FORCE, LARGE_MB | ALLOW | MULTIBIT, LARGE_MB | PBS_KS):
        rc, msg = _create(p, flags)
        assert rc == INVALID and msg.startswith(b"flags %d: HELM_SI_CREATE_LARGE_MULTIBIT goes with " % flags), msg
        assert b"HELM_SI_CREATE_LARGE_N" in msg and b"HELM_SI_CREATE_N8192" in msg
    # ... whatever the shape, as bit 16 alone
    rc, msg = _create(_params(1, 512, 2, 15), LARGE_MB)
    assert rc == INVALID and b"HELM_SI_CREATE_LARGE_MULTIBIT goes with" in msg


@pytest.mark.parametrize("shape,group,flags", [
    ((2, 4096, 1, 20), 2, LARGE),                  # k > 1
    ((2, 8192, 1, 20), 3, N8192),
    ((1, 4096, 1, 19), 4, LARGE),                  # grouping factor 4
    ((1, 8192, 2, 15), 4, LARGE | N8192),
    ((1, 16384, 1, 18), 2, N8192),                 # N >= 16384
    ((1, 16384, 1, 18), 3, LARGE | N8192),
    ((1, 8192, 2, 15), 2, LARGE),                  # the bit of the other N
])
def test_refusals_by_name(shape, group, flags):
    rc, msg = _create(_params(*shape, group=group), LARGE_MB | flags)
    assert rc == INVALID and b"HELM_SI_CREATE_LARGE_MULTIBIT" in msg, msg
    assert b"k > 1" in msg and b"grouping_factor >= 4" in msg and b"N >= 16384" in msg, msg
    assert b"k = 1" in msg and b"grouping_factor 2 or 3 dividing n" in msg, msg
    assert _create(_params(*shape, group=group), LARGE_MB | flags | PBS_KS) == (rc, msg)


def test_the_other_checks_still_apply_in_their_order():
    for N, bit in ((4096, LARGE), (8192, N8192)):
        f = LARGE_MB | bit
        assert _create(_params(1, N, 2, 15, n=1026, group=2), f) == (INVALID, b"n must be in [1,1024]")
        for n, g in ((10, 3), (9, 2)):             # a grouping factor that does not divide n
            assert _create(_params(1, N, 2, 15, n=n, group=g), f) == (INVALID, b"grouping_factor must be 0..3 and divide n")
        p = _params(1, N, 2, 15, group=3)
        p.ks_logB = 8
        rc, msg = _create(p, f)
        assert rc == INVALID and b"keyswitch decomposition" in msg
        rc, msg = _create(_params(1, N, 1, 25, group=2), f)
        assert rc == INVALID and b"PBS decomposition" in msg
        rc, msg = _create(_params(1, N, 2, 15, group=2, msg=128, carry=64), f)
        assert rc == INVALID and b"power of two <= N/2" in msg
        rc, msg = _create(_params(1, N, 2, 15, group=3), f | MULTIBIT)            # bit 16 still wants 1 or 2 beside it
        assert rc == INVALID and b"HELM_SI_CREATE_GENERIC_MULTIBIT goes with" in msg
        assert _create(_params(1, N, 2, 15, group=3), f | MULTIBIT | ALLOW)[0] != INVALID
        rc, msg = _create(_params(1, N, 2, 15, group=3), f | FORCE)               # ... and bit 2 wants bit 16 for multi-bit
        assert rc == INVALID and msg.startswith(b"HELM_SI_CREATE_FORCE_GENERIC: the generic kernel has no multi-bit form")
    # the creation-time capacity check stays the classical one: a necessary condition only
    assert b"capacity" in _create(_params(1, 4096, 1, 23, group=2), LARGE_MB | LARGE)[1]
    assert _create(_params(1, 4096, 1, 22, group=3), LARGE_MB | LARGE)[0] != INVALID      # refused at load, not here
    assert b"capacity" in _create(_params(1, 8192, 1, 22, group=2), LARGE_MB | N8192)[1]
    assert _create(_params(1, 8192, 1, 21, group=2), LARGE_MB | N8192)[0] != INVALID      # refused at load, not here


@pytest.mark.parametrize("g", [2, 3])
def test_without_the_flag_multibit_is_refused_in_the_parents_words(g):
    for flags in (LARGE, LARGE | ALLOW, LARGE | PBS_KS):
        assert _create(_params(1, 4096, 1, 20, group=g), flags) == (INVALID, ND.LARGE_TEXT)
        assert _create(_params(1, 8192, 2, 15, group=g), flags) == (INVALID, ND.LARGE_TEXT)
    for flags in (N8192, N8192 | LARGE, N8192 | FORCE | MULTIBIT, N8192 | PBS_KS):
        assert _create(_params(1, 8192, 2, 15, group=g), flags) == (INVALID, N8192_TEXT)
    assert b"k = 1, N = 8192" in N8192_TEXT and b"N >= 16384" in N8192_TEXT and b"HELM_SI_CREATE_N8192" in N8192_TEXT


@pytest.mark.parametrize("shape", PF.SHAPES, ids=lambda s: "k%d_N%d_l%d_B%d_g%d" % s)
def test_the_flag_changes_nothing_elsewhere(shape):
    """Every shape of tests/test_pbs_first_domain.py at grouping_factor <= 1 (any N), and its multi-bit shapes below
    N = 4096, beside bit 32, bit 256 and both, with every combination of the other bits: the same status and message - or
    class and field - as without the flag."""
    assert shape[4] <= 1 or shape[1] < 4096
    p = PF._params(*shape, carry=8 if shape[1] >= 4096 else 4)
    for big in (LARGE, N8192, LARGE | N8192):
        for f in PF.COMBOS + [PBS_KS, ALLOW | PBS_KS]:
            assert PF._create(p, f | big | LARGE_MB) == PF._create(p, f | big), (shape, f, big)


def test_unknown_bits():
    p = _params(1, 8192, 2, 15, group=3)
    rc, msg = _create(p, 128)
    assert msg == (b"unknown bits in flags 128 (HELM_SI_CREATE_ALLOW_GENERIC = 1, HELM_SI_CREATE_FORCE_GENERIC = 2, "
                   b"HELM_SI_CREATE_GENERIC_MULTIBIT = 16; 4 and 8 are reserved)")
    rc, msg = _create(p, 512)
    assert msg == (b"unknown bits in flags 512 (HELM_SI_CREATE_ALLOW_GENERIC = 1, HELM_SI_CREATE_FORCE_GENERIC = 2, "
                   b"HELM_SI_CREATE_GENERIC_MULTIBIT = 16; 4 and 8 are reserved)")
    rc, msg = _create(p, N8192 | 4)
    assert msg == (b"unknown bits in flags 260 (HELM_SI_CREATE_ALLOW_GENERIC = 1, HELM_SI_CREATE_FORCE_GENERIC = 2, "
                   b"HELM_SI_CREATE_GENERIC_MULTIBIT = 16, HELM_SI_CREATE_N8192 = 256; 4 and 8 are reserved)")
    rc, msg = _create(p, LARGE_MB | N8192 | 4)
    assert rc == INVALID
    assert msg == (b"unknown bits in flags 1284 (HELM_SI_CREATE_ALLOW_GENERIC = 1, HELM_SI_CREATE_FORCE_GENERIC = 2, "
                   b"HELM_SI_CREATE_GENERIC_MULTIBIT = 16, HELM_SI_CREATE_N8192 = 256, HELM_SI_CREATE_LARGE_MULTIBIT = 1024; "
                   b"4 and 8 are reserved)")
    for flags in (LARGE_MB | 128, LARGE_MB | LARGE | 512, LARGE_MB | 2048):
        rc, msg = _create(p, flags)
        assert rc == INVALID and msg.startswith(b"unknown bits in flags %d (" % flags), msg
        assert b"HELM_SI_CREATE_LARGE_MULTIBIT = 1024" in msg
    for flags in (4, 128, 512, 2048, LARGE | 8):
        assert b"LARGE_MULTIBIT" not in _create(p, flags)[1]


def test_server_key_generic_argument():
    with pytest.raises(ValueError, match="'large', 'allow\\+large' or 'force\\+large'"):
        helm_amd.SiServerKey(params=_params(1, 8192, 2, 15), generic="multibit")
    with pytest.raises(ValueError, match="'n8192', 'allow\\+n8192', 'force\\+n8192' or 'large\\+n8192'"):
        helm_amd.SiServerKey(params=_params(1, 8192, 2, 15), generic="multibit")
    with pytest.raises(ValueError, match="'large\\+multibit', 'n8192\\+multibit' or 'large\\+n8192\\+multibit'"):
        helm_amd.SiServerKey(params=_params(1, 8192, 2, 15), generic="multibit")
    G = helm_amd.shortint._GENERIC_FLAGS
    assert (G["large+multibit"], G["n8192+multibit"], G["large+n8192+multibit"]) == (1056, 1280, 1312)
    for N, modes, cls in ((4096, ("large+multibit", "large+n8192+multibit"), "large"),
                          (8192, ("n8192+multibit", "large+n8192+multibit"), "n8192")):
        p = _params(1, N, 2, 15, group=3)
        with pytest.raises(helm_amd.HelmError, match="out of scope"):
            helm_amd.SiServerKey(params=p, generic="large+n8192")
        for mode in modes:
            try:
                sk = helm_amd.SiServerKey(params=p, generic=mode)
                assert sk.kernel_class() == cls and sk.field_bits() == 50
                sk.close()
            except helm_amd.HelmError as e:  # no device here: the parameter checks passed
                assert "no HIP device" in str(e), e


@pytest.mark.parametrize("name,N,g,pbs,t", [("si_toy_4096_mb2", 4096, 2, (1, 21), 32), ("si_toy_4096_mb3", 4096, 3, (1, 20), 32),
                                            ("si_toy_8192_mb2", 8192, 2, (2, 15), 64), ("si_toy_8192_mb3", 8192, 3, (2, 15), 64)])
def test_the_toy_sets(name, N, g, pbs, t):
    p, lwe_std, glwe_std = helm_amd.si_named_params(name)
    assert (p.n, p.k, p.N, p.pbs_l, p.pbs_logB, p.ks_l, p.ks_logB) == (12, 1, N) + pbs + (3, 5)
    assert p.message_modulus * p.carry_modulus == t and p.grouping_factor == g and p.n % g == 0
    assert (lwe_std, glwe_std) == (1e-9, 1e-17)
    bit = LARGE if N == 4096 else N8192
    assert _create(p, LARGE_MB | bit)[0] != INVALID
    assert _create(p, bit)[0] == INVALID and _create(p, 0)[0] == INVALID


@pytest.mark.parametrize("name,base,n,N,pbs,bit", [("shortint_m3c3_multibit3", "shortint_m3c3", 864, 8192, (2, 15), N8192),
                                                   ("shortint_m2c3_multibit3", "shortint_m2c3", 1023, 4096, (2, 15), LARGE)])
def test_the_full_size_sets(name, base, n, N, pbs, bit):
    """The approximate multi-bit sets: the classical set's values with grouping factor 3, n a multiple of 3, and a PBS
    decomposition a generated key loads with (two levels of 15 bits; one level of 22 bits cannot, at any grouping)."""
    p, lwe_std, glwe_std = helm_amd.si_named_params(name)
    q, q_lwe, q_glwe = helm_amd.si_named_params(base)
    assert (p.n, p.k, p.N, p.pbs_l, p.pbs_logB) == (n, 1, N) + pbs and p.grouping_factor == 3 and p.n % 3 == 0
    assert (p.ks_l, p.ks_logB, p.message_modulus, p.carry_modulus) == (q.ks_l, q.ks_logB, q.message_modulus, q.carry_modulus)
    assert (lwe_std, glwe_std) == (q_lwe, q_glwe) and abs(p.n - q.n) <= 1
    logN = N.bit_length() - 1
    assert p.pbs_l * 2 ** (p.pbs_logB + 3 + 62 + logN) * 1001 < 5072 ** 4 * 5440 ** 4 // 2 * 1000      # the loader's rule
    assert 2 ** (22 + 2 + 62 + 12) * 1001 >= (5072 ** 4 + 1) * (5440 ** 4 + 1) // 2 * 1000              # 22 x 1 at g = 2, N = 4096
    assert _create(p, LARGE_MB | bit)[0] != INVALID
    assert _create(p, bit)[0] == INVALID and _create(p, 0)[0] == INVALID
