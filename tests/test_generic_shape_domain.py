"""The shape domain helm_hip_ctx_create admits since the generic blind-rotate kernel exists (include/helm_hip.h,
helm_amd/csrc/helm_pbs_generic.inc): N in {256, 512, 1024, 2048}, k >= 1 with (k+1) N <= 8192 (the kernel's LDS budget),
pbs_l >= 1, and the single-prime capacity bound (k+1) l N 2^(logB-1) 2^31 < p/2.  Shapes just outside are refused with -1
and the reason before any device is touched - no GPU needed."""
import ctypes as C

import pytest

import helm_amd
from helm_amd import _native as nv


def _params(k, N, l, logB, n=16):
    p, _, _ = helm_amd.named_params("toy")
    p.n, p.k, p.N, p.pbs_l, p.pbs_logB, p.ks_l, p.ks_logB = n, k, N, l, logB, 4, 4
    return p


@pytest.mark.parametrize("k,N,l,logB,msg", [
    (1, 128, 3, 5, b"unsupported"),      # N below the domain
    (1, 4096, 1, 1, b"unsupported"),     # N above it
    (4, 2048, 1, 1, b"unsupported"),     # (k+1) N = 10240 > 8192
    (8, 1024, 1, 1, b"unsupported"),     # (k+1) N = 9216 > 8192
    (16, 512, 1, 1, b"unsupported"),     # (k+1) N = 8704 > 8192 (k = 15 at N = 512 is admitted)
    (0, 512, 3, 6, b"unsupported"),      # k = 0
    (2, 512, 0, 6, b"unsupported"),      # pbs_l = 0
    (2, 1024, 3, 7, b"capacity"),        # 2^50.2: would need a two-prime CRT in the 32-bit engine
    (1, 2048, 1, 9, b"capacity"),        # l = 1, logB = 9 at N = 2048
    (1, 1024, 1, 10, b"capacity"),       # l = 1, logB = 10 at N = 1024
    (1, 256, 8, 4, b"decomposition"),    # logB l = 32 > 31
])
def test_shapes_outside_the_domain_are_refused_without_a_device(k, N, l, logB, msg):
    p = _params(k, N, l, logB)
    h = nv.vp()
    assert nv.hip.helm_hip_ctx_create(0, C.byref(p), C.byref(h)) == -1
    err = nv.hip.helm_hip_last_error()
    assert msg in err, err
    assert not h.value


def test_the_unsupported_message_names_the_domain():
    p = _params(1, 4096, 1, 1)
    h = nv.vp()
    assert nv.hip.helm_hip_ctx_create(0, C.byref(p), C.byref(h)) == -1
    err = nv.hip.helm_hip_last_error()
    assert b"256, 512, 1024 or 2048" in err and b"(k+1) N <= 8192" in err, err


@pytest.mark.parametrize("k,N,l,logB", [(3, 256, 2, 8), (4, 256, 3, 6), (2, 512, 2, 7), (2, 1024, 2, 6), (1, 2048, 3, 5),
                                        (15, 512, 1, 1), (7, 1024, 1, 1), (3, 2048, 1, 2)])
def test_shapes_inside_the_domain_pass_validation(k, N, l, logB):
    """Admitted shapes get past every parameter check: what stops them on a box without a GPU is the device lookup
    (HELM_ERR_NO_DEVICE = -2 there), never HELM_ERR_INVALID."""
    p = _params(k, N, l, logB)
    h = nv.vp()
    rc = nv.hip.helm_hip_ctx_create(0, C.byref(p), C.byref(h))
    if rc == 0:
        assert nv.hip.helm_hip_kernel_class(h) == 1
        nv.hip.helm_hip_ctx_destroy(h)
    else:
        assert rc != -1, nv.hip.helm_hip_last_error()


def _digits_32bit(x, logB, l):
    """The generic kernel's digit recurrence (gen_decompose_step, helm_pbs_generic.inc) in exact integers with uint32
    wrap-around: digits[0] the most significant level."""
    rep = logB * l
    state = ((x + (1 << (31 - rep))) & 0xFFFFFFFF) >> (32 - rep)
    half_m1 = (1 << (logB - 1)) - 1
    out = [0] * l
    for lev in range(l - 1, -1, -1):
        tie = 0 if lev == 0 else (state >> (2 * logB - 1)) & 1
        nxt = ((state + half_m1 + tie) & 0xFFFFFFFF) >> logB
        d = (state - (nxt << logB)) & 0xFFFFFFFF
        out[lev] = d - (1 << 32) if d >= 1 << 31 else d
        state = nxt
    return out


@pytest.mark.parametrize("logB,l", [(6, 5), (2, 13), (1, 31), (3, 10), (7, 4), (8, 3), (31, 1), (15, 2), (5, 6)])
def test_generic_digit_recurrence_matches_the_oracle(logB, l):
    """Wide decompositions (logB (l-1) >= 24 carry a state past 2^23, where a 24-bit digit multiply breaks): the
    recurrence the generic kernel runs gives the oracle's digits, boundary values and ties included."""
    import numpy as np
    import oracle
    rng = np.random.default_rng(logB * 100 + l)
    xs = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0xC3F0A5B1] + [int(v) for v in rng.integers(0, 2**32, size=400)]
    rep = logB * l
    xs += [(v << (32 - rep)) & 0xFFFFFFFF for v in range(64)] + [((2 * v + 1) << (31 - rep)) & 0xFFFFFFFF for v in range(64)]
    for x in xs:
        assert _digits_32bit(x, logB, l) == [int(d) for d in oracle.decompose(x, logB, l)], hex(x)
