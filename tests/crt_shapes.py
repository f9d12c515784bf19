"""Shapes of the two-prime blind-rotate kernel (k_pbs_crt, helm_amd/csrc/helm_pbs_crt.inc) and the oracle route that is exact
for each - shared by tests/test_crt_shape_domain.py (CPU) and tests/test_gpu_crt_shapes.py.

THE ORACLE'S ROUTES.  oracle.Oracle(..., use_ntt=True) multiplies in the Goldilocks field (p = 2^64 - 2^32 + 1) and is exact
only while the column sums of an external product stay below 2^63.  The shapes this kernel exists for pass that: at
(k, N, l, logB) = (1, 256, 1, 31) the route already differs from the schoolbook route on plain random rows
(tests/test_crt_shape_domain.py pins it).  use_ntt=False, the schoolbook route with wrapping uint32 sums, is exact for every
shape.  exact_oracle() picks: schoolbook whenever the capacity bound (k+1) l N 2^(logB-1) 2^31 reaches 2^63, and always for
crafted keys at the bound.  A GPU row that differs from the Goldilocks route on such a shape is NOT a GPU error."""
import os
import sys

import helm_amd
import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import saturation as S  # noqa: E402

P0, P1 = S.FPG, S.FPG2   # the CRT pair of k_pbs_crt

# (k, N, pbs_l, pbs_logB, n)
SHAPES = [(2, 1024, 1, 23, 16),    # tfhe boolean TFHE_LIB_PARAMETERS' shape (bound 2^64.6)
          (3, 512, 2, 10, 16),     # the later boolean default's shape (2^52)
          (2, 1024, 3, 7, 16),     # just past the single prime (2^50.2); refused without the flag
          (1, 2048, 1, 9, 16),     # refused without the flag; N = 2048, D = 1
          (1, 1024, 1, 10, 16),    # refused without the flag
          (1, 256, 1, 31, 16),     # logB l = 31 in one level: digits up to 2^30
          (3, 1024, 2, 15, 16),    # the LDS edge (k+1) N = 4096
          (7, 256, 2, 12, 16),     # eight columns; 16 digit polynomials in batches of D = 3: a partial last batch
          (1, 512, 3, 10, 16),     # six digit polynomials one at a time (D <= 1024 / N = 2, and D = 2 would cost a resident workgroup)
          (1, 256, 2, 12, 1024),   # the ms array's ends: the largest n ...
          (1, 256, 2, 12, 1)]      # ... and the smallest; 4 digit polynomials at D = 3: a partial last batch
# the shapes whose last batch of a CMUX step is partial (D > 1 not dividing (k+1) l) on an MI355X: the `cnt < D` path of the
# product loop and of the forward transform.  tests/test_gpu_crt_shapes.py asserts the D the context chose.
PARTIAL_BATCH = [(7, 256, 2, 12, 16), (1, 256, 2, 12, 1)]
IDS = ["k%d_N%d_l%d_B%d_n%d" % s for s in SHAPES]
REFUSED_TODAY = [(2, 1024, 3, 7), (1, 2048, 1, 9), (1, 1024, 1, 10)]   # tests/test_generic_shape_domain.py: "capacity"


def params(k, N, l, logB, n=16):
    p, _, _ = helm_amd.named_params("toy")
    p.n, p.k, p.N, p.pbs_l, p.pbs_logB, p.ks_l, p.ks_logB = n, k, N, l, logB, 4, 4
    return p


def glwe_std(logB):
    """The toy sets' 1e-9 while a level's digits stay small; tfhe's own magnitude for wide levels (one level of 23 bits
    multiplies the key's noise by up to 2^22: 1e-9 does not decrypt there)."""
    return 1e-9 if logB <= 15 else 3e-16


def toy_key(shape, seed=7):
    k, N, l, logB, n = shape
    return helm_amd.ClientKey(params(k, N, l, logB, n), 1e-7, glwe_std(logB), seed=seed)


def needs_schoolbook(p):
    return S.capacity_bound(S.shape_of(p), 32) >= 1 << 63


def exact_oracle(p, bsk, ksk, saturating=False):
    """The oracle on the route that is exact for this shape (module docstring)."""
    return oracle.Oracle(p.as_tuple7(), bsk, ksk, use_ntt=not (saturating or needs_schoolbook(p)))
