"""Admission of boolean shapes beyond the single-prime capacity bound: helm_hip_ctx_create_ex with HELM_HIP_CREATE_ALLOW_CRT = 1
or HELM_HIP_CREATE_FORCE_CRT = 2 (include/helm_hip.h, helm_amd/csrc/helm_pbs_crt.inc).  The CRT domain is N in {256, 512, 1024,
2048}, k >= 1, (k+1) N <= 4096, pbs_l >= 1, pbs_logB pbs_l <= 31, n <= 1024, pbs_order 0, grouping_factor 1, and it needs no
capacity check.  Every refusal comes before any device is touched - no GPU needed.  Also here: the kernel's CRT lift restated
in Python integers, the creation-time arithmetic, the two new named parameter sets, and the oracle-route trap of
tests/crt_shapes.py pinned."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import helm_amd
import oracle
from helm_amd import _native as nv

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crt_shapes as X  # noqa: E402
import saturation as S  # noqa: E402

ALLOW, FORCE = 1, 2


def _create(p, flags):
    h = nv.vp()
    rc = nv.hip.helm_hip_ctx_create_ex(0, C.byref(p), flags, C.byref(h))
    return rc, h, nv.hip.helm_hip_last_error()


def test_the_header_and_the_python_layer_agree_on_the_flags():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "helm_hip.h")).read()
    assert "HELM_HIP_CREATE_ALLOW_CRT = 1" in header and "HELM_HIP_CREATE_FORCE_CRT = 2" in header
    from helm_amd import engine
    assert (engine.HIP_CREATE_ALLOW_CRT, engine.HIP_CREATE_FORCE_CRT) == (ALLOW, FORCE)


@pytest.mark.parametrize("k,N,l,logB", X.REFUSED_TODAY)
def test_flags_0_refuses_with_capacity_as_before(k, N, l, logB):
    p = X.params(k, N, l, logB)
    rc, h, err = _create(p, 0)
    assert rc == -1 and not h.value and err == b"parameter set exceeds the single-prime NTT capacity", err
    h2 = nv.vp()
    assert nv.hip.helm_hip_ctx_create(0, C.byref(p), C.byref(h2)) == -1
    assert nv.hip.helm_hip_last_error() == err


@pytest.mark.parametrize("flags", [0, ALLOW])
@pytest.mark.parametrize("k,N,l,logB,msg", [(1, 128, 3, 5, b"unsupported"), (4, 2048, 1, 1, b"unsupported"),
                                            (0, 512, 3, 6, b"unsupported"), (1, 256, 8, 4, b"decomposition")])
def test_other_refusals_do_not_depend_on_allow_crt(flags, k, N, l, logB, msg):
    """ALLOW_CRT lifts the capacity refusal only: every other refusal is byte for byte helm_hip_ctx_create's."""
    p = X.params(k, N, l, logB)
    rc, h, err = _create(p, flags)
    h2 = nv.vp()
    assert nv.hip.helm_hip_ctx_create(0, C.byref(p), C.byref(h2)) == -1
    assert rc == -1 and msg in err and err == nv.hip.helm_hip_last_error(), err


@pytest.mark.parametrize("shape", X.SHAPES, ids=X.IDS)
@pytest.mark.parametrize("flags", [ALLOW, FORCE])
def test_crt_shapes_pass_validation(shape, flags):
    """What stops an admitted shape on a box without a GPU is the device lookup (HELM_ERR_NO_DEVICE = -2), never
    HELM_ERR_INVALID; with a device the context is of class 2 and computes in the pair (98)."""
    k, N, l, logB, n = shape
    rc, h, err = _create(X.params(k, N, l, logB, n), flags)
    if rc == 0:
        assert nv.hip.helm_hip_kernel_class(h) == 2 and nv.hip.helm_hip_field_bits(h) == 98
        nv.hip.helm_hip_ctx_destroy(h)
    else:
        assert rc != -1, err


@pytest.mark.parametrize("k,N,l,logB,cls", [(2, 512, 3, 6, 0), (1, 1024, 3, 7, 0), (2, 512, 2, 7, 1), (3, 2048, 1, 2, 1)])
def test_allow_crt_keeps_the_class_of_a_shape_that_fits_the_single_prime(k, N, l, logB, cls):
    rc, h, err = _create(X.params(k, N, l, logB), ALLOW)
    if rc == 0:
        assert nv.hip.helm_hip_kernel_class(h) == cls and nv.hip.helm_hip_field_bits(h) != 98
        nv.hip.helm_hip_ctx_destroy(h)
    else:
        assert rc != -1, err


def test_beyond_the_bound_and_outside_the_lds_budget_is_refused_and_names_the_crt_domain():
    """boolean_default's shape at N = 2048: bound 2^50.2, (k+1) N = 6144 > 4096."""
    rc, h, err = _create(X.params(2, 2048, 3, 6), ALLOW)
    assert rc == -1 and not h.value
    assert b"capacity" in err and b"CRT domain" in err and b"(k+1) N <= 4096" in err, err
    assert _create(X.params(2, 2048, 3, 6), 0)[2] == b"parameter set exceeds the single-prime NTT capacity"


@pytest.mark.parametrize("flags", [3, 4, 8, 5, 6, 0x80000000, 0xFFFFFFFF])
def test_bad_flag_combinations_are_refused(flags):
    rc, h, err = _create(X.params(2, 1024, 1, 23), flags)
    assert rc == -1 and not h.value
    assert b"HELM_HIP_CREATE_ALLOW_CRT" in err and b"HELM_HIP_CREATE_FORCE_CRT" in err, err


@pytest.mark.parametrize("k,N,l,logB", [(3, 2048, 1, 2), (7, 1024, 1, 1), (15, 512, 1, 1), (2, 2048, 3, 6), (1, 4096, 1, 1),
                                        (1, 128, 3, 5), (0, 512, 3, 6)])
def test_force_crt_outside_the_domain_is_refused(k, N, l, logB):
    rc, h, err = _create(X.params(k, N, l, logB), FORCE)
    assert rc == -1 and not h.value
    assert b"HELM_HIP_CREATE_FORCE_CRT" in err and b"(k+1) N <= 4096" in err, err


@pytest.mark.parametrize("what,val", [("n", 1025), ("n", 0), ("pbs_order", 1), ("grouping_factor", 2), ("torus_bits", 64)])
@pytest.mark.parametrize("flags", [ALLOW, FORCE])
def test_the_rest_of_the_crt_domain_is_enforced(what, val, flags):
    p = X.params(2, 1024, 1, 23)
    setattr(p, what, val)
    rc, h, err = _create(p, flags)
    assert rc == -1 and not h.value, err


# ---------------------------------------------------------------------------------------------------------------------------
# the lift of crt_lift32 (helm_pbs_crt.inc) in Python integers
# ---------------------------------------------------------------------------------------------------------------------------
P0, P1 = X.P0, X.P1
P0INV = pow(P0, P1 - 2, P1)
M32, LIM = 1 << 32, 1 << 63


def _centred(v, p):
    v %= p
    return v - p if v > p // 2 else v


def _lift32(r0, r1):
    """(uint32_t)r0 + (uint32_t)p0 (uint32_t)t with t = reduce<F1>(mulmod<F1>(r1 - r0, p0^-1 mod p1)) (tp_quotient,
    pbs_twoprime.h: r1 - r0 goes into the multiplication unreduced, below mulmod's 2^53); every value the kernel forms is
    checked to stay below 2^63 in magnitude (the modular products are fused in mulmod: their operands and results are what
    is formed), r0 and t below 2^51 (to_torus32's range)."""
    t = _centred((r1 - r0) * _centred(P0INV, P1), P1)
    for v in (r0, r1, r1 - r0, t):
        assert abs(v) < LIM
    assert abs(r1 - r0) < 1 << 53
    assert abs(r0) < 1 << 51 and abs(t) < 1 << 51
    word = (r0 % M32) + (P0 % M32) * (t % M32)
    assert word < 1 << 64
    return word % M32


def _residues(x):
    """The recentred residues, and - where a residue lies within 1 of +-p/2, where the kernel's reduce() may return either
    representative (|r| <= p/2 + 1) - the other one too."""
    outs = []
    for r0 in {_centred(x, P0)} | {_centred(x, P0) - s * P0 for s in (1, -1) if abs(_centred(x, P0) - s * P0) <= P0 // 2 + 1}:
        for r1 in {_centred(x, P1)} | {_centred(x, P1) - s * P1 for s in (1, -1) if abs(_centred(x, P1) - s * P1) <= P1 // 2 + 1}:
            outs.append((r0, r1))
    return outs


def test_the_lift_model_equals_x_mod_2_32():
    top = (1 << 78) - 1
    rng = np.random.default_rng(5)
    xs = [0, 1, -1, top, -top, top - 1, 1 - top]
    xs += [s * (LIM + d) for s in (1, -1) for d in (-2, -1, 0, 1, 2)]                 # either side of +-2^63
    xs += [s * (1 << e) + d for s in (1, -1) for e in (31, 32, 51, 62, 64, 77) for d in (-1, 0, 1)]
    for p in (P0, P1):                                                                # residues at +-p/2, multiples of p
        ms = [0, 1, -1, 2, (top // p), -(top // p)] + [int(v) for v in rng.integers(-(top // p), top // p, size=40)]
        for m in ms:
            for off in (0, p // 2, p // 2 + 1, -(p // 2), -(p // 2) - 1, 1, -1):
                xs.append(m * p + off)
    xs += [int.from_bytes(rng.bytes(10), "little", signed=True) >> 1 for _ in range(3000)]   # uniform over +-2^78
    xs += [int(v) for v in rng.integers(-(1 << 62), 1 << 62, size=500)]
    n = 0
    for x in xs:
        if abs(x) > top:
            continue
        for r0, r1 in _residues(x):
            assert _lift32(r0, r1) == x % M32, (x, r0, r1)
            n += 1
    assert n > 3500


def test_the_creation_time_arithmetic():
    """The CRT domain needs no capacity check: its largest bound is below 4096 x 31 x 2^30 x 2^31 < 2^78, and p0 p1 / 2 is
    2^97.5 (the static_assert beside crt_admitted, helm_hip.hip)."""
    worst = 0
    for N in (256, 512, 1024, 2048):
        for k in range(1, 4096 // N):
            for logB in range(1, 32):
                for l in range(1, 31 // logB + 1):
                    worst = max(worst, S.capacity_bound(S.Shape(1024, k, N, l, logB), 32))
    assert worst == 4096 * (1 << 30) * (1 << 31)             # (k+1) N = 4096, one level of 31 bits
    assert worst <= 4096 * 31 * (1 << 30) * (1 << 31) < 1 << 78 < P0 * P1 // 2
    assert 97.4 < np.log2(float(P0 * P1 // 2)) < 97.6
    assert P0 == 5072 ** 4 + 1 and P1 == 5096 ** 4 + 1 and (P1 - 1) % 4096 == 0 and (P1 - 1) % 8192 != 0   # N <= 2048
    assert P0INV * P0 % P1 == 1
    # the LDS layout at the domain's edge (TwoPrimeLds<uint32_t>): acc u32, col 2 doubles, dig 2 D doubles, ms u16
    for N, D in ((1024, 1), (2048, 1), (256, 4)):
        assert 4 * 4096 + 16 * 4096 + 16 * D * N + 2 * 1025 <= 160 * 1024


def test_the_named_sets():
    p, lwe, glwe = helm_amd.named_params("toy_crt")
    assert (p.n, p.k, p.N, p.pbs_l, p.pbs_logB, p.torus_bits, p.pbs_order, p.grouping_factor) == (16, 2, 1024, 1, 23, 32, 0, 1)
    assert glwe < 1e-12      # the toy sets' 1e-9 does not decrypt at one level of 23 bits
    p, lwe, glwe = helm_amd.named_params("boolean_tfhe_lib")
    assert (p.n, p.k, p.N, p.pbs_l, p.pbs_logB, p.ks_l, p.ks_logB) == (830, 2, 1024, 1, 23, 3, 5)
    assert (lwe, glwe) == (1.41e-6, 2.94e-16)
    assert p.torus_bits == 32 and p.pbs_order == 0 and p.grouping_factor == 1
    for name in ("toy_crt", "boolean_tfhe_lib"):
        p, _, _ = helm_amd.named_params(name)
        assert _create(p, 0)[2] == b"parameter set exceeds the single-prime NTT capacity"
        rc, h, err = _create(p, ALLOW)
        assert rc != -1, err
        if rc == 0:
            nv.hip.helm_hip_ctx_destroy(h)


def test_toy_crt_decrypts_under_the_oracle():
    """The set's noise is chosen so that the oracle's own bootstraps decrypt (schoolbook route: the exact one here)."""
    ck = helm_amd.ClientKey.generate("toy_crt", seed=5)
    orc = X.exact_oracle(ck.params, ck.bsk, ck.ksk)
    assert orc._ntt is None
    tv = np.full(ck.params.N, 1 << 29, dtype=np.uint32)
    for bit in (True, False):
        big = orc.bootstrap_noks(ck.encrypt(bit), tv)
        assert bool(ck.decrypt(orc.keyswitch(big))) == bit


def test_the_goldilocks_route_is_not_exact_at_wide_levels():
    """(k, N, l, logB) = (1, 256, 1, 31): column sums pass 2^63, the Goldilocks route differs from the schoolbook route on
    plain random rows, and the schoolbook route is the one that equals the exact integer reference.  Pinned so that nobody
    'fixes' a kernel to match the wrong route; exact_oracle() picks the right one."""
    shape = (1, 256, 1, 31, 16)
    ck = X.toy_key(shape)
    p = ck.params
    assert X.needs_schoolbook(p)
    assert not X.needs_schoolbook(X.params(3, 1024, 2, 15)) and X.needs_schoolbook(X.params(2, 1024, 1, 23))
    school = oracle.Oracle(p.as_tuple7(), ck.bsk, ck.ksk, use_ntt=False)
    gold = oracle.Oracle(p.as_tuple7(), ck.bsk, ck.ksk, use_ntt=True)
    assert X.exact_oracle(p, ck.bsk, ck.ksk)._ntt is None
    rng = np.random.default_rng(3)
    lwe = rng.integers(0, 2**32, size=(3, p.n + 1), dtype=np.uint32)
    tv = rng.integers(0, 2**32, size=p.N, dtype=np.uint32)
    a = [school.bootstrap_noks(lwe[g], tv) for g in range(3)]
    b = [gold.bootstrap_noks(lwe[g], tv) for g in range(3)]
    assert any(not np.array_equal(a[g], b[g]) for g in range(3))
    ref, peak = S.bootstrap_exact(lwe[0], tv, ck.bsk, S.shape_of(p), 32)
    assert np.array_equal(a[0], ref)
    assert peak < S.capacity_bound(S.shape_of(p), 32)
