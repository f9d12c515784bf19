"""Many-LUT bootstrap (helm_si_make_many_lut / helm_si_apply_many_luts, include/helm_shortint.h): a plain restatement for
the tests - no GPU and no project code.

  many_lut_poly      the test polynomial of n functions in M = the power of two >= n chunks of N / M coefficients
  output_coefficient where output x of n_out is extracted: x * N / M
  extract_at         the sample extract at coefficient h of an accumulator (A_0 .. A_{k-1}, B)
  accumulator_exact  the blind-rotated accumulator of a small-LWE row in exact integers: classical sets through
                     saturation.cmux_step_exact (by import), multi-bit sets through group_step_exact, which mirrors the
                     g > 1 branch of the oracle's orc64_bootstrap
  masks_from_output0 the mask words of the extract at h from the oracle's coefficient-0 output (which holds every mask
                     coefficient of the accumulator: out[r N] = A_r[0], out[r N + u] = -A_r[N - u])
  zero_mask_acc      the accumulator of a row with an all-zero mask: X^(-b~) tv, no step runs

tests/test_many_lut_reference.py pins all of it against the CPU oracle; tests/test_gpu_many_lut.py runs the kernels against it.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import saturation as S  # noqa: E402

W = 64
MOD = 1 << W


def chunks(n):
    """M: the smallest power of two >= n."""
    assert n >= 1
    return 1 << (int(n) - 1).bit_length()


def output_coefficient(x, n_out, N):
    """The accumulator coefficient output x of n_out is extracted at: x * N / M."""
    return x * (N // chunks(n_out))


def many_lut_poly(values, t, N):
    """values: n_funcs lists of t / M function values.  -> N words (numpy uint64), as helm_si_make_many_lut."""
    n_funcs = len(values)
    M = chunks(n_funcs)
    assert M <= t and N % t == 0
    box, per, delta = N // t, t // M, (1 << 63) // t
    acc = [0] * N
    for i in range(n_funcs):
        assert len(values[i]) == per
        for v in range(per):
            for j in range(box):
                acc[(i * per + v) * box + j] = int(values[i][v]) * delta % MOD
    half = box // 2
    for j in range(half):
        acc[j] = -acc[j] % MOD
    return np.array([acc[(j + half) % N] for j in range(N)], dtype=np.uint64)


def extract_at(acc, h):
    """acc: (k+1) polynomials of N integers mod 2^64.  Coefficient j of mask polynomial r goes to word r N + ((h - j) mod N),
    with its own sign for j <= h and negated for j > h; the body is B[h].  -> k N + 1 words (numpy uint64)."""
    k, N = len(acc) - 1, len(acc[0])
    out = [0] * (k * N + 1)
    for r in range(k):
        for j in range(N):
            v = int(acc[r][j])
            out[r * N + (h - j) % N] = v % MOD if j <= h else -v % MOD
    out[k * N] = int(acc[k][h]) % MOD
    return np.array(out, dtype=np.uint64)


def masks_from_output0(out0, k, N, h):
    """The k N mask words of the extract at h, from the coefficient-0 output of the same accumulator (its body is not used):
    word r N + u is A_r[h - u] for u <= h and -A_r[N + h - u] for u > h, with A_r[0] = out0[r N], A_r[j] = -out0[r N + N - j]."""
    out0 = np.asarray(out0, dtype=np.uint64)
    res = np.zeros(k * N, dtype=np.uint64)
    neg = lambda a: (~a + np.uint64(1))
    for r in range(k):
        o = out0[r * N:(r + 1) * N]
        A = np.concatenate([o[:1], neg(o[1:][::-1])])     # A[j] = -o[N - j], j = 1 .. N - 1
        u = np.arange(N)
        src = np.where(u <= h, h - u, N + h - u)
        w = A[src]
        res[r * N:(r + 1) * N] = np.where(u <= h, w, neg(w))
    return res


def zero_mask_acc(tv, bt, k):
    """The accumulator of a row whose mask is all zero and whose body switches to bt: (0, ..., 0, X^(-bt) tv)."""
    tv = np.asarray(tv, dtype=np.uint64)
    N = len(tv)
    idx = (np.arange(N) + int(bt)) % (2 * N)
    b = np.where(idx < N, tv[idx % N], ~tv[idx % N] + np.uint64(1))
    return [[0] * N for _ in range(k)] + [[int(v) for v in b]]


def zero_mask_body(tv, bt, h):
    """Body of the extract at h of a zero-mask row: +-tv[(h + bt) mod N], negated when (h + bt) mod 2N >= N."""
    N = len(tv)
    idx = (h + int(bt)) % (2 * N)
    v = int(tv[idx % N])
    return v % MOD if idx < N else -v % MOD


def group_step_exact(acc, a_tildes, key_group, shape):
    """One multi-bit group step, as the g > 1 branch of orc64_bootstrap: G = sum over the subsets S of the group of
    X^(sum_{i in S} a~_i) * key_group[S] (words mod 2^64), then acc <- G (x) acc - the accumulator's own polynomials are
    decomposed and the result replaces it.  key_group: [2^g][l][k+1][k+1][N] words."""
    g = len(a_tildes)
    k1, N, l = shape.k + 1, shape.N, shape.l
    key_group = np.asarray(key_group, dtype=np.uint64).reshape(1 << g, l, k1, k1, N)
    G = np.zeros((l, k1, k1, N), dtype=np.uint64)
    j = np.arange(N)
    for sub in range(1 << g):
        e = sum(int(a_tildes[i]) for i in range(g) if (sub >> i) & 1) % (2 * N)
        idx = (j - e) % (2 * N)
        src = key_group[sub][..., idx % N]
        G += np.where(idx < N, src, ~src + np.uint64(1))
    dig = np.zeros((k1, l, N), dtype=np.int64)
    for r in range(k1):
        for t in range(N):
            dig[r, :, t] = S.digits(int(acc[r][t]), shape.logB, l, W)
    new = []
    for c in range(k1):
        col = np.zeros(N, dtype=object)
        for r in range(k1):
            for lev in range(l):
                if dig[r, lev].any():
                    col = col + S.negacyclic_exact(dig[r, lev], G[lev, r, c], W)
        new.append([int(v) % MOD for v in col])
    return new


def accumulator_exact(lwe, tv, bsk, shape, group=1):
    """The accumulator after the blind rotation of the small-LWE row `lwe` with test polynomial tv, exact.  group <= 1: a step
    whose switched mask element is 0 is skipped (saturation.cmux_step_exact per active step); group = 2, 3: every group
    step runs (group_step_exact).  -> (k+1) lists of N Python integers mod 2^64."""
    n, k, N = shape.n, shape.k, shape.N
    bt = S.modswitch(lwe[n], N, W)
    acc = [[0] * N for _ in range(k)] + [S.rotate([int(v) for v in tv], (2 * N - bt) % (2 * N), W)]
    a = [S.modswitch(lwe[i], N, W) for i in range(n)]
    if group > 1:
        key = np.asarray(bsk, dtype=np.uint64).reshape(n // group, -1)
        for t in range(n // group):
            acc = group_step_exact(acc, a[t * group:(t + 1) * group], key[t], shape)
        return acc
    key = np.asarray(bsk, dtype=np.uint64).reshape(n, -1)
    for i in range(n):
        if a[i]:
            acc, _ = S.cmux_step_exact(acc, a[i], key[i], shape, W)
    return acc
