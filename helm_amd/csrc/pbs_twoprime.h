// pbs_twoprime.h — what the two "generic, recentre-everywhere" blind-rotate kernels in the CRT pair F0 = FpG, F1 = FpG2 share:
// k_pbs_crt (boolean engine, 32-bit torus: helm_pbs_crt.inc) and k_pbs64_generic (64-bit engine: helm_pbs64_generic.inc).
// Included by the main translation unit of each engine only.  The kernels themselves stay per engine - job type and input
// stage, decomposition, forming the torus word, sample extract and the multi-bit form differ; the LDS layout, the transforms
// over both fields, the classical product accumulation, the CRT quotient and the key conversion after its engine's own loads
// do not, and are here once.
//
// One workgroup of TP_THREADS = 256 threads per bootstrap.  What a bootstrap works on lives in LDS (TwoPrimeLds<Word>, Word
// = the torus word, uint32_t or uint64_t):
//   acc   Word   [k+1][N]      the accumulator GLWE
//   col   double [2][k+1][N]   the k+1 column sums of the external product in both fields, inverse-transformed in place
//   dig   double [2][D][N]     one batch of D digit polynomials in both fields, forward-transformed in place (D N <= 1024,
//                              D <= 4; D = 1 at N = 2048; no larger than keeps the occupancy of D = 1: tp_fit)
//   ms    u16    [n+1]         the modulus-switched input
// At the domain's edge, (k+1) N = 4096, with a 32-bit (64-bit) accumulator: 16 (32) + 64 + 16 (N = 2048: 32) + 2 KiB = 98
// to 114 (114 to 130) KiB of the CU's 160, one workgroup per CU.  The four twiddle tables (forward and inverse, both fields:
// 32 N bytes) are read from global memory, where every workgroup of the device shares them in L2: in LDS they would not fit
// beside the rest at N = 2048.
//
// Per CMUX step: for each batch of digit polynomials q = r l + lev (polynomial r, level lev, 0 = most significant): decompose
// (the engine's own step), forward-transform in both fields (radix-2 Cooley-Tukey, natural order in, bit-reversed out),
// multiply by the key polynomials (r, c, lev) streamed from HBM and add into column c; then inverse-transform the 2 (k+1)
// columns together (Gentleman-Sande, bit-reversed in, natural out; N^-1 is folded into the key) and lift each coefficient's
// two residues to the integer (CRT), taken modulo the engine's torus.
//
// Exactness.  F0 = FpG (p0 = 5072^4 + 1 = 2^49.23, 2^53 / p0 = 13.6), F1 = FpG2 (p1 = 5096^4 + 1 = 2^49.26, 13.4).  Every
// value a transform stage stores is recentred (reduce: |x| <= p/2 + 1), so a butterfly's sum or difference is below 1.1 p and
// a mulmod of it below 0.6 p.  Digits are exact doubles below p/2, the same integer in both fields (their magnitude is the
// engine's: see its file).  A product of a recentred transform output with a key word (|w| <= p/2) is below
// (0.5 + 0.75 (p/2) 2^-52) p = 0.56 p (mulmod's bound); a column sum enters a batch recentred and takes at most D <= 4
// products: <= 0.5 p + 4 x 0.56 p = 2.8 p < 2^53, and it is recentred at the end of every batch - for any (k+1) l.  No lazy
// stage, no short-root stage: nothing here rests on a shape.  The inverse transform's outputs are recentred too:
// r_f = x mod p_f, |r_f| <= p_f/2 + 1, where x is the true integer coefficient of the external product (the bound on |x| is
// the engine's: see its file; it is below p0 p1 / 2 = 2^97.5).  The lift
//   t = reduce<F1>(mulmod<F1>(r1 - r0, p0^-1 mod p1)),   x' = r0 + p0 t          (tp_quotient)
// multiplies an operand of at most (p0 + p1) / 2 + 2 < 2^49.3 (mulmod takes 2^53) and is congruent to x mod p0 p1 with
// |x'| <= p0 p1 / 2 + 1.5 p0 + 1, so |x' - x| < p0 p1 and x' = x.  t is RECENTRED: with t merely below 0.56 p1 (mulmod's
// bound) x' could be x +- p0 p1 once |x| passes 0.78 of the half - what round 16 found in the 64-bit engine's lift_pairs
// (tests/test_multibit_saturating_inputs.py reads the statement off this file).  r0 and t are exact integers below 2^51 in
// magnitude, from which each engine forms x' modulo its torus.
#pragma once
#include "ntt_fp64.h"

#include <algorithm>

namespace helm {

constexpr int TP_THREADS = 256;
constexpr int TP_MAX_D = 4;
static_assert(5072ull * 5072 * 5072 * 5072 + 1 == FpG::P_U64 && 5096ull * 5096 * 5096 * 5096 + 1 == FpG2::P_U64, "the CRT pair");

// digit polynomials transformed together: at most 4 (the column-sum bound above), D N <= 1024 (one at N = 2048)
inline int tp_batch(int N, int k, int l)
{
    int d = std::max(1, 1024 / N);
    d = std::min(d, TP_MAX_D);
    return std::min(d, (k + 1) * l);
}

// LDS layout (bytes), host and device
template <typename Word>
struct TwoPrimeLds {
    size_t acc, col, dig, ms, bytes;
    __host__ __device__ TwoPrimeLds(int N, int K1, int D, int n)
    {
        acc = 0;
        col = acc + sizeof(Word) * (size_t)K1 * N;
        dig = col + sizeof(double) * 2 * (size_t)K1 * N;
        ms = dig + sizeof(double) * 2 * (size_t)D * N;
        bytes = (ms + sizeof(uint16_t) * ((size_t)n + 1) + 15) / 16 * 16;
    }
};

template <typename F>
__device__ __forceinline__ void tp_fwd_bfly(double *y, int t, double w)
{
    const double U = y[0], V = mulmod<F>(y[t], w);
    y[0] = reduce<F>(U + V);
    y[t] = reduce<F>(U - V);
}

template <typename F>
__device__ __forceinline__ void tp_inv_bfly(double *y, int t, double w)
{
    const double U = y[0], V = y[t];
    y[0] = reduce<F>(U + V);
    y[t] = reduce<F>(mulmod<F>(U - V, w));
}

// cnt polynomials per field, field 0 at x[q N], field 1 at x[fstride + q N]: forward negacyclic transform, natural order in,
// bit-reversed out, inputs |x| < 2^52, outputs recentred.  tw0 / tw1: bit-reversed powers of psi in each field (global
// memory).  Ends with a workgroup barrier.
template <int LOGN>
__device__ __forceinline__ void tp_ntt_forward(double *x, int cnt, int fstride, const double *__restrict__ tw0,
                                               const double *__restrict__ tw1)
{
    constexpr int H = 1 << (LOGN - 1);
    const int per_f = cnt * H;
    for (int s = 0; s < LOGN; s++) {
        const int logt = LOGN - 1 - s, t = 1 << logt, m = 1 << s;
        for (int b = (int)threadIdx.x; b < 2 * per_f; b += TP_THREADS) {
            const int f = b >= per_f ? 1 : 0, r = b - f * per_f; // (per_f is a multiple of 64: f is uniform over a wave)
            const int q = r >> (LOGN - 1), k = r & (H - 1), i = k >> logt;
            double *y = x + (size_t)f * fstride + ((size_t)q << LOGN) + (i << (logt + 1)) + (k & (t - 1));
            if (f == 0) tp_fwd_bfly<FpG>(y, t, tw0[m + i]);
            else tp_fwd_bfly<FpG2>(y, t, tw1[m + i]);
        }
        __syncthreads();
    }
}

// inverse: bit-reversed in, natural out, without the 1/N; twi0 / twi1: bit-reversed powers of psi^-1.  Inputs and outputs
// recentred.  Ends with a workgroup barrier.
template <int LOGN>
__device__ __forceinline__ void tp_ntt_inverse(double *x, int cnt, int fstride, const double *__restrict__ twi0,
                                               const double *__restrict__ twi1)
{
    constexpr int H = 1 << (LOGN - 1);
    const int per_f = cnt * H;
    for (int s = 0; s < LOGN; s++) {
        const int logt = s, t = 1 << logt, h = H >> s;
        for (int b = (int)threadIdx.x; b < 2 * per_f; b += TP_THREADS) {
            const int f = b >= per_f ? 1 : 0, r = b - f * per_f;
            const int q = r >> (LOGN - 1), k = r & (H - 1), i = k >> logt;
            double *y = x + (size_t)f * fstride + ((size_t)q << LOGN) + (i << (logt + 1)) + (k & (t - 1));
            if (f == 0) tp_inv_bfly<FpG>(y, t, twi0[h + i]);
            else tp_inv_bfly<FpG2>(y, t, twi1[h + i]);
        }
        __syncthreads();
    }
}

// Classical products into the column sums, for the batch of cnt transformed digit polynomials q0 .. q0 + cnt - 1 in dig
// (field 1 at dig + dstride) and the k+1 columns of col (field 1 at col + cstride; q0 == 0 starts the sums): thread slot
// u = (field, coefficient s) owns that coefficient of every column (no LDS hazard between threads until the barrier).  key:
// the key words of this step, [r][c][lev][f][N]; key polynomial (r, c, lev) of digit q = r l + lev in field f starts at
// (((r (k+1) + c) l + lev) 2 + f) N = koff[q] + (c l 2 + f) N.  Ends with a workgroup barrier (the next batch overwrites dig).
template <int LOGN>
__device__ __forceinline__ void tp_accumulate(const double *dig, int dstride, double *col, int cstride, const double *key, int q0,
                                              int cnt, int K1, int L)
{
    constexpr int N = 1 << LOGN;
    size_t koff[TP_MAX_D];
#pragma unroll
    for (int ql = 0; ql < TP_MAX_D; ql++) {
        const int q = q0 + ql, r = q / L, lev = q - r * L;
        koff[ql] = ((size_t)r * K1 * L + lev) * 2 * N;
    }
    for (int u = (int)threadIdx.x; u < 2 * N; u += TP_THREADS) {
        const int f = u >= N ? 1 : 0, s = u & (N - 1); // (f is uniform over a wave)
        const double *dg = dig + (size_t)f * dstride + s;
        for (int c = 0; c < K1; c++) {
            const double *kc = key + ((size_t)c * L * 2 + f) * N + s;
            double *cs = col + (size_t)f * cstride + (size_t)c * N + s;
            double sum = q0 == 0 ? 0.0 : *cs;
            if (f == 0) {
#pragma unroll
                for (int ql = 0; ql < TP_MAX_D; ql++)
                    if (ql < cnt) sum += mulmod<FpG>(dg[ql << LOGN], kc[koff[ql]]);
                *cs = reduce<FpG>(sum); // <= 0.5 p + D x 0.56 p before (see the head of this file)
            } else {
#pragma unroll
                for (int ql = 0; ql < TP_MAX_D; ql++)
                    if (ql < cnt) sum += mulmod<FpG2>(dg[ql << LOGN], kc[koff[ql]]);
                *cs = reduce<FpG2>(sum);
            }
        }
    }
    __syncthreads();
}

// the CRT quotient t of the integer x = r0 + p0 t with x = r0 (mod p0), x = r1 (mod p1), |x| < p0 p1 / 2 (r0, r1
// recentred), itself recentred: see the head of this file
__device__ __forceinline__ double tp_quotient(double r0, double r1, double p0inv_mod_p1)
{
    return reduce<FpG2>(mulmod<FpG2>(r1 - r0, p0inv_mod_p1));
}

// A key conversion, one workgroup per key polynomial `poly` = blockIdx.x in source order [i][lev][r][c]: load(poly N + j, v0,
// v1) yields coefficient j reduced into both fields (the engine's own: how its key words are read) -> x (LDS, 2 N doubles,
// field 1 at x + N) -> forward transform -> x N^-1, recentred, bit-reversed order -> dst[i][r][c][lev][f][N]: the two fields
// of one key polynomial are adjacent runs of N doubles, so a workgroup's wave reads 512 contiguous bytes per (digit, column)
// in either field - 16 bytes of HBM per key word.
template <int LOGN, typename LOAD>
__device__ __forceinline__ void tp_convert(double *x, const LOAD &load, double *__restrict__ dst, const double *__restrict__ tw0,
                                           const double *__restrict__ tw1, double n_inv0, double n_inv1, int K1, int L)
{
    constexpr int N = 1 << LOGN;
    const size_t poly = blockIdx.x;
    const int c = (int)(poly % K1);
    const int r = (int)((poly / K1) % K1);
    const int lev = (int)((poly / ((size_t)K1 * K1)) % L);
    const size_t i = poly / ((size_t)K1 * K1 * L);
    for (int j = (int)threadIdx.x; j < N; j += TP_THREADS) load(poly * N + j, x[j], x[N + j]);
    __syncthreads();
    tp_ntt_forward<LOGN>(x, 1, N, tw0, tw1);
    double *d = dst + ((((i * K1 + r) * K1 + c) * L + lev) * 2) * N;
    for (int j = (int)threadIdx.x; j < N; j += TP_THREADS) {
        d[j] = reduce<FpG>(mulmod<FpG>(x[j], n_inv0));
        d[N + j] = reduce<FpG2>(mulmod<FpG2>(x[N + j], n_inv1));
    }
}

// Host side of either kernel's context set-up: the dynamic-LDS attribute, the occupancy and the digit batch.  The attribute
// is the kernel's, shared by every context of the process: it is set at the largest layout of this N, so that a context
// created later with a smaller one cannot lower it under an earlier context's launches.  per_cu: resident workgroups per CU
// with one digit polynomial per batch (0: none fits - lds is then that layout's size); d: the most (<= tp_batch) that cost no
// resident workgroup against one per batch; lds: the layout's bytes at d.
struct TwoPrimeFit {
    int per_cu = 0, d = 1;
    size_t lds = 0;
};
template <typename Word>
inline hipError_t tp_fit(const void *kern, int N, int k, int l, int n, TwoPrimeFit &fit)
{
    const int K1max = 4096 / N;
    const size_t lds_max = TwoPrimeLds<Word>(N, K1max, tp_batch(N, K1max - 1, 31), 1024).bytes;
    if (hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max)) return e;
    auto bytes = [&](int d) { return TwoPrimeLds<Word>(N, k + 1, d, n).bytes; };
    fit = TwoPrimeFit{0, 1, bytes(1)};
    if (hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&fit.per_cu, kern, TP_THREADS, fit.lds)) return e;
    if (fit.per_cu < 1) return hipSuccess;
    for (int d = tp_batch(N, k, l); d > 1; d--) {
        int nb = 0;
        if (hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, TP_THREADS, bytes(d))) return e;
        if (nb == fit.per_cu) {
            fit.d = d;
            fit.lds = bytes(d);
            break;
        }
    }
    return hipSuccess;
}

} // namespace helm
