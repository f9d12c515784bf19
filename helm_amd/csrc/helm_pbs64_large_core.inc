// helm_pbs64_large_core.inc — what the two large-N blind-rotate kernels of the 64-bit engine share (included by
// helm_shortint.hip after helm_pbs64_generic.inc and before helm_pbs64_large.inc and helm_pbs64_n8192.inc, main translation
// unit only): k_pbs64_large (k = 1, N = 4096) and k_pbs64_n8192 (k = 1, N = 8192).  Here, once each: the field pair and the
// workgroup width, the two LDS layouts, the radix-2 transforms, a view of the accumulator per kernel (LDS in natural order
// against a global row in n8192_slot order), the prologue, the classical products, the multi-bit subset term, the way of a
// column back into the accumulator (write-back, inverse transform, CRT lift), the sample extract and the key conversion.
// The kernel files keep their __global__ functions and their loop structure: k_pbs64_large forms both columns from one
// forward pass, k_pbs64_n8192 one column after the other.
//
// The pair.  FpG2 (5096^4 + 1) has 2-adicity 2^12, so it holds no 8192-th root of unity; the pair here is L0 = FpG
// (5072^4 + 1, 2^16 | p - 1) and L1 = FpI (5440^4 + 1, 2^24 | p - 1): both hold 16384-th roots of unity, p0 p1 / 2 = 2^97.87.
// One workgroup of 1024 threads (16 waves, four per SIMD, <= 128 VGPRs per lane) per bootstrap; thread `tid` owns the
// PT = N / 1024 positions tid + 1024 m of each field of the transform buffer and of each polynomial of the accumulator.
//
// Exactness.  p0 = 2^49.23 (2^53 / p0 = 13.6), p1 = 2^49.64 (2^53 / p1 = 10.28): the argument is made for p1, the tighter
// field, and holds for p0 a fortiori.  It does not depend on N.  As in k_pbs64_generic there is no lazy stage and no
// short-root stage: every value a transform stage stores is recentred (reduce: |x| <= p/2 + 1).
//   * mulmod(a, w), |w| <= p/2: |r| <= (0.5 + 0.75 |a| 2^-52) p.  For a recentred a (|a| <= p1/2 + 1 = 2^48.64) that is
//     (0.5 + 0.75 x 2^-3.36) p = 0.573 p, "below about 0.58 p".
//   * forward butterfly: U +- mulmod(V, w) with U, V recentred: <= 0.5 p + 0.58 p = 1.08 p < 2^53, then recentred.
//   * inverse butterfly: U +- V <= p + 2 (recentred next, or multiplied: mulmod of |a| <= p + 2 = 2^49.64 is below
//     (0.5 + 0.75 x 2^-2.36) p = 0.65 p, then recentred).
//   * digits are at most 2^23 < p/2 in magnitude, the same integer in both fields.
//   * a column sum takes a product of a recentred transform output with a key word (|w| <= p/2): each below 0.58 p.  It is
//     recentred after at most FOUR products (l64_mac's `fold`, which the callers set after every fourth product, and when it
//     is written back): <= 0.5 p + 4 x 0.58 p = 2.82 p < 10.28 p = 2^53, for any l.
//   * the inverse transform's outputs are recentred: r_f = x mod p_f, |r_f| <= p_f/2 + 1, where x is the true integer
//     coefficient of the external product, |x| <= (k+1) l N 2^(logB-1) 2^63 < p0 p1 / 2 / 1.001 (the capacity check of
//     helm_si_ctx_create_ex with THIS pair's product; the figures at each N stand at the head of the kernel files).
//   * the lift: t = (r1 - r0) p0^-1 mod p1 (l64_quotient).  |r1 - r0| <= p0/2 + p1/2 + 2 < 2^49.5, so the mulmod is below
//     0.63 p1 and its recentring gives |t| <= p1/2 + 1 < 2^48.7 < 2^51 - the quotient is recentred, as in the generic and
//     multi-bit lifts.  x' = r0 + p0 t is congruent to x mod p0 p1 and |x'| <= p0 p1 / 2 + 1.5 p0 + 1, so |x' - x| <
//     p0 p1 (1 - 0.0005) + 1.5 p0 + 1 < p0 p1 and x' = x exactly; it is formed mod 2^64 from the two exact int64 values
//     (to_int64: |r0|, |t| < 2^51, HELM_BOUND slot 4).
// The torus arithmetic is therefore the exact negacyclic product mod 2^64 for every admitted shape
// (tests/test_large_n_bounds.py and tests/test_n8192_bounds.py restate these bounds with exact fractions).
//
// Multi-bit form (the kernels' template argument GG = grouping factor 2 or 3, HELM_SI_CREATE_LARGE_MULTIBIT; GG = 0 is the
// classical form).  The algorithm is the one at the head of helm_pbs64_generic.inc: per group t < n / GG ONE external
// product, acc <- (sum_S X^(e_S) GGSW_{t,S}) (x) acc with e_S = sum_{i in S} a~_i mod 2N (uniform over the workgroup, in
// scalar registers).  The digits are those of the accumulator itself at the thread's own positions (no rotation, no
// difference), the column sums are sum_S sum_q (d^_q . M(e_S)) . K^_{t,S}[q][c], and the lifted value REPLACES the
// accumulator.  No group is skipped, not one whose rotations are all 0: the oracle does not skip either, and the step is not
// the identity on the low bits.  M(e)[s] = psi^(expo(s) e), expo(s) = 2 rev(s) + 1: l64_ntt_forward has the generic kernel's
// Cooley-Tukey structure (twiddle m + i), so position s holds the value at psi^(2 rev(s) + 1).  M is read per use from the
// context's table of the 2N powers of psi in each field of this pair ([2][2N] doubles in global memory, written once at
// creation).
// Exactness of the multi-bit form, for p1.  d^ is recentred and |M| <= p/2, so d^ M = mulmod(d^, M) is below 0.58 p; its
// product with a key word is below (0.5 + 0.75 x 0.58 p 2^-52) p < 0.59 p.  A sum is recentred after every four products
// (the 2^GG subsets of one digit polynomial in runs of four): <= 0.5 p + 4 x 0.59 p < 2.9 p < 2^53 = 10.28 p.  The true
// integer coefficient is bounded by helm_si_load_bootstrap_key's group-sum rule for the key at hand (below p0 p1 / 2 / 1.001
// with THIS pair's product), so the recentred lift is exact (tests/test_large_multibit_bounds.py restates these numbers).

using L0 = FpG;
using L1 = FpI;

constexpr int L64_THREADS = 1024;
constexpr int N8192_LOGN = 13;
template <int LOGN>
constexpr int L64_PT = (1 << LOGN) / L64_THREADS; // positions per thread and field

// LDS layout of k_pbs64_large (bytes), host and device
struct Large64Lds {
    size_t acc, buf, ms, bytes;
    __host__ __device__ Large64Lds(int N, int n)
    {
        acc = 0;
        buf = acc + sizeof(uint64_t) * 2 * (size_t)N;
        ms = buf + sizeof(double) * 2 * (size_t)N;
        bytes = (ms + sizeof(uint16_t) * ((size_t)n + 1) + 15) / 16 * 16;
    }
};

// LDS layout of k_pbs64_n8192 (bytes), host and device
struct N8192Lds {
    size_t buf, ms, bytes;
    __host__ __device__ N8192Lds(int n)
    {
        buf = 0;
        ms = buf + sizeof(double) * 2 * ((size_t)1 << N8192_LOGN);
        bytes = (ms + sizeof(uint16_t) * ((size_t)n + 1) + 15) / 16 * 16;
    }
};

// One polynomial per field, field 0 at x[0 .. N), field 1 at x[N .. 2N): forward negacyclic transform, natural order in,
// bit-reversed out, inputs |x| < 2^52, outputs recentred.  tw0 / tw1: bit-reversed powers of psi in each field (global
// memory).  N / 2 / L64_THREADS butterflies per thread, field and stage, one field after the other within a stage: a thread's
// butterflies of one field are in flight together, not all of the stage (fewer registers live beside the sums and the
// states).  Ends with a workgroup barrier.
template <int LOGN>
__device__ __forceinline__ void l64_ntt_forward(double *x, const double *__restrict__ tw0, const double *__restrict__ tw1)
{
    constexpr int N = 1 << LOGN, H = N / 2;
    static_assert(H % L64_THREADS == 0, "whole rounds of butterflies per field");
    for (int s = 0; s < LOGN; s++) {
        const int logt = LOGN - 1 - s, t = 1 << logt, m = 1 << s;
#pragma unroll
        for (int b0 = 0; b0 < H; b0 += L64_THREADS) {
            const int k = b0 + (int)threadIdx.x, i = k >> logt;
            tp_fwd_bfly<L0>(x + (i << (logt + 1)) + (k & (t - 1)), t, tw0[m + i]);
        }
#pragma unroll
        for (int b0 = 0; b0 < H; b0 += L64_THREADS) {
            const int k = b0 + (int)threadIdx.x, i = k >> logt;
            tp_fwd_bfly<L1>(x + N + (i << (logt + 1)) + (k & (t - 1)), t, tw1[m + i]);
        }
        __syncthreads();
    }
}

// inverse: bit-reversed in, natural out, without the 1/N; twi0 / twi1: bit-reversed powers of psi^-1.  Inputs and outputs
// recentred.  Ends with a workgroup barrier.
template <int LOGN>
__device__ __forceinline__ void l64_ntt_inverse(double *x, const double *__restrict__ twi0, const double *__restrict__ twi1)
{
    constexpr int N = 1 << LOGN, H = N / 2;
    for (int s = 0; s < LOGN; s++) {
        const int logt = s, t = 1 << logt, h = H >> s;
#pragma unroll
        for (int b0 = 0; b0 < H; b0 += L64_THREADS) {
            const int k = b0 + (int)threadIdx.x, i = k >> logt;
            tp_inv_bfly<L0>(x + (i << (logt + 1)) + (k & (t - 1)), t, twi0[h + i]);
        }
#pragma unroll
        for (int b0 = 0; b0 < H; b0 += L64_THREADS) {
            const int k = b0 + (int)threadIdx.x, i = k >> logt;
            tp_inv_bfly<L1>(x + N + (i << (logt + 1)) + (k & (t - 1)), t, twi1[h + i]);
        }
        __syncthreads();
    }
}

// ---- the accumulator GLWE as each kernel holds it: own(r, m) is the thread's word of polynomial r at its position
// tid + 1024 m, at(r, j) any coefficient j < N (another thread's, in general) -------------------------------------------

// k_pbs64_large: [2][N] words of LDS in natural order
template <int LOGN>
struct L64LdsAcc {
    static constexpr int N = 1 << LOGN;
    uint64_t *p;
    __device__ __forceinline__ uint64_t &own(int r, int m) const { return p[(size_t)r * N + (int)threadIdx.x + m * L64_THREADS]; }
    __device__ __forceinline__ uint64_t &at(int r, int j) const { return p[(size_t)r * N + j]; }
};

// Where coefficient j of a polynomial lies in its N words of an accumulator row of k_pbs64_n8192: thread j mod 1024 owns it,
// and a thread's eight coefficients lie side by side, so that its own accesses are one address and constant offsets (with
// the natural order they were sixteen 64-bit addresses per thread, which the compiler kept in registers over the whole
// rotation).
__device__ __forceinline__ unsigned n8192_slot(int j) { return (((unsigned)j & (L64_THREADS - 1)) << 3) | ((unsigned)j >> 10); }

// k_pbs64_n8192: a row of [2][N] words of global memory, each polynomial in n8192_slot order (not __restrict__: read at other
// threads' positions); base = n8192_slot(tid), so n8192_slot(tid + 1024 m) = base + m
struct N8192RowAcc {
    static constexpr int N = 1 << N8192_LOGN;
    uint64_t *p;
    unsigned base;
    __device__ __forceinline__ uint64_t &own(int r, int m) const { return (p + (size_t)r * N)[base + m]; }
    __device__ __forceinline__ uint64_t &at(int r, int j) const { return (p + (size_t)r * N)[n8192_slot(j)]; }
};

// ---- the prologue: the modulus switch into MS, then the accumulator as (0, X^{-b~} lut).  The caller places the barrier
// that orders the accumulator's words for other threads. -------------------------------------------------------------------
template <int LOGN, class Acc>
__device__ __forceinline__ void l64_prologue(Acc acc, uint16_t *MS, const Pbs64Job &job, const uint64_t *__restrict__ small,
                                             const uint64_t *__restrict__ luts, int n)
{
    constexpr int N = 1 << LOGN, PT = L64_PT<LOGN>;
    const int tid = (int)threadIdx.x;
    switch_row(MS, job_row(job, small, n), n, tid, L64_THREADS, LOGN + 1);
    __syncthreads();
    const int bt = (int)MS[n];
    const uint64_t *tv = luts + (size_t)job.lut * N;
#pragma unroll
    for (int m = 0; m < PT; m++) {
        const uint64_t v = lut_rotated(tv, tid + m * L64_THREADS, bt, N);
        acc.own(0, m) = 0;
        acc.own(1, m) = v;
    }
}

// One product per field onto a column sum (first: the sum starts with it).  fold: recentre the sum - the callers fold after
// every fourth product (see the head of this file): <= 0.5 p + 4 x 0.59 p before.
__device__ __forceinline__ void l64_mac(double &a0, double &a1, double v0, double v1, bool first, bool fold)
{
    double s0 = first ? v0 : a0 + v0, s1 = first ? v1 : a1 + v1;
    if (fold) {
        s0 = reduce<L0>(s0);
        s1 = reduce<L1>(s1);
    }
    a0 = s0;
    a1 = s1;
}

// ---- the classical products: the transformed digit polynomial in buf times one column's key words at this thread's
// positions, onto sum[field][position].  kc: key polynomial (r, c, lev), field f at kc + f N. -----------------------------
template <int LOGN>
__device__ __forceinline__ void l64_products(double (&sum)[2][L64_PT<LOGN>], const double *buf, const double *__restrict__ kc,
                                             bool first, bool fold)
{
    constexpr int N = 1 << LOGN, PT = L64_PT<LOGN>;
#pragma unroll
    for (int m = 0; m < PT; m++) {
        const int s = (int)threadIdx.x + m * L64_THREADS;
        l64_mac(sum[0][m], sum[1][m], mulmod<L0>(buf[s], kc[s]), mulmod<L1>(buf[N + s], kc[N + s]), first, fold);
    }
}

// ---- the multi-bit subset term: for subset S of the group (bit i of S = member i, am[] the members' rotations in scalar
// registers) d^ M(e_S) at this thread's positions, then its product with subset S's key word of each of the caller's NC
// columns, recentred after every fourth subset.  kS: key polynomial (r, c, lev) of GGSW (t, S) for the first of them, the
// next column's col_words further.  (A position's d^ M(e_S) serves its NC products at once: formed per column by a caller
// that holds both columns' sums, it costs k_pbs64_large<12, 2 / 3> ten registers and a wave of occupancy.) ---------------
template <int LOGN, int GG, int NC>
__device__ __forceinline__ void l64_subset_term(double (&sum)[NC][2][L64_PT<LOGN>], const double *buf,
                                                const double *__restrict__ kS, size_t col_words,
                                                const double *__restrict__ psi_pow, const int (&am)[GG], int S)
{
    constexpr int N = 1 << LOGN, PT = L64_PT<LOGN>;
    int eS = 0; // e_S = sum of the members' rotations mod 2N
#pragma unroll
    for (int i = 0; i < GG; i++) eS += (S >> i) & 1 ? am[i] : 0;
    eS &= 2 * N - 1;
    const bool fold = (S & 3) == 3;
#pragma unroll
    for (int m = 0; m < PT; m++) {
        const int s = (int)threadIdx.x + m * L64_THREADS;
        double d0 = buf[s], d1 = buf[N + s];
        if (S) { // (M(0) = 1)
            const int ex = 2 * (int)(__brev((unsigned)s) >> (32 - LOGN)) + 1; // expo(s): see the head of this file
            const int at = (ex * eS) & (2 * N - 1);
            d0 = mulmod<L0>(d0, psi_pow[at]);
            d1 = mulmod<L1>(d1, psi_pow[2 * N + at]);
        }
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const double *kc = kS + (size_t)c * col_words;
            l64_mac(sum[c][0][m], sum[c][1][m], mulmod<L0>(d0, kc[s]), mulmod<L1>(d1, kc[N + s]), false, fold);
        }
    }
}

// the lift's quotient t = (r1 - r0) p0^-1 mod p1, recentred
__device__ __forceinline__ double l64_quotient(double r0, double r1, double p0inv_mod_p1)
{
    return reduce<L1>(mulmod<L1>(r1 - r0, p0inv_mod_p1));
}

// ---- a column back into the accumulator: the sums into buf, recentred; inverse transform (N^-1 is folded into the key);
// CRT lift of each coefficient's two residues to the exact integer mod 2^64 at the thread's own positions of polynomial c -
// added to the accumulator's word (classical) or, REPLACE, put in its place (multi-bit). ----------------------------------
template <int LOGN, bool REPLACE, class Acc>
__device__ __forceinline__ void l64_column_back(Acc acc, int c, double *buf, const double (&sum)[2][L64_PT<LOGN>],
                                                const double *__restrict__ twi0, const double *__restrict__ twi1,
                                                double p0inv_mod_p1)
{
    constexpr int N = 1 << LOGN, PT = L64_PT<LOGN>;
    const int tid = (int)threadIdx.x;
#pragma unroll
    for (int m = 0; m < PT; m++) {
        const int s = tid + m * L64_THREADS;
        buf[s] = reduce<L0>(sum[0][m]);
        buf[N + s] = reduce<L1>(sum[1][m]);
    }
    __syncthreads();
    l64_ntt_inverse<LOGN>(buf, twi0, twi1);
#pragma unroll
    for (int m = 0; m < PT; m++) {
        const int j = tid + m * L64_THREADS;
        const double r0 = buf[j], r1 = buf[N + j];
        const double t = l64_quotient(r0, r1, p0inv_mod_p1);
        HELM_BOUND(__builtin_fabs(r0) < 0x1p51 && __builtin_fabs(t) < 0x1p51, 4);
        const uint64_t x = (uint64_t)to_int64(r0) + L0::P_U64 * (uint64_t)to_int64(t);
        uint64_t &w = acc.own(c, m);
        w = REPLACE ? x : w + x;
    }
}

// ---- sample extract: every output of the job (extract_put; pad = 0: the one at coefficient 0) into rows of N + 1 words ----
template <int LOGN, class Acc>
__device__ __forceinline__ void l64_sample_extract(Acc acc, const Pbs64Job &job, uint64_t *__restrict__ out)
{
    constexpr int N = 1 << LOGN, PT = L64_PT<LOGN>;
    const int tid = (int)threadIdx.x;
    const int n_out = pbs64_job_outputs(job.pad), ls = pbs64_job_log_stride(job.pad);
    for (int x = 0; x < n_out; x++) {
        const int h = x << ls;
        uint64_t *ob = big_row(out, job.out_row + x, 1, N);
#pragma unroll
        for (int m = 0; m < PT; m++) extract_put(ob, N, h, tid + m * L64_THREADS, acc.own(0, m));
        if (tid == 0) ob[N] = acc.at(1, h); // body = B[h]
    }
}

// ---- the key conversion.  One workgroup per key polynomial: standard-domain u64 coefficients (taken as signed) -> both
// fields -> forward transform -> x N^-1, recentred, bit-reversed order: dst[i][r][c][lev][f][N] (src is [i][lev][r][c][N]).
// k_bsk_convert64_generic's sibling for the pair (L0, L1) and 1024 threads.  The two-field buffer, [2][N] doubles, is
// dynamic LDS: at N = 8192 it is 128 KiB, over the static limit (the launcher's context raises the kernel's limit). --------
template <int LOGN>
__global__ __launch_bounds__(L64_THREADS) void k_bsk_convert64_large(const uint64_t *__restrict__ src, double *__restrict__ dst,
                                                                     const double *__restrict__ tw0,
                                                                     const double *__restrict__ tw1, double n_inv0,
                                                                     double n_inv1, double two32_0, double two32_1, int K1,
                                                                     int L)
{
    constexpr int N = 1 << LOGN;
    extern __shared__ __align__(16) unsigned char smem_c64[];
    double *x = reinterpret_cast<double *>(smem_c64); // [2][N]
    const size_t poly = blockIdx.x; // index in src order
    const int c = (int)(poly % K1);
    const int r = (int)((poly / K1) % K1);
    const int lev = (int)((poly / ((size_t)K1 * K1)) % L);
    const size_t i = poly / ((size_t)K1 * K1 * L);
    for (int j = (int)threadIdx.x; j < N; j += L64_THREADS) {
        const uint64_t v = src[poly * N + j];
        // v = hi 2^32 + lo with hi signed: reduce in each field
        const double hi = (double)(int32_t)(uint32_t)(v >> 32), lo = (double)(uint32_t)v;
        x[j] = reduce<L0>(mulmod<L0>(hi, two32_0) + lo);
        x[N + j] = reduce<L1>(mulmod<L1>(hi, two32_1) + lo);
    }
    __syncthreads();
    l64_ntt_forward<LOGN>(x, tw0, tw1);
    double *d = dst + ((((i * K1 + r) * K1 + c) * L + lev) * 2) * N;
    for (int j = (int)threadIdx.x; j < N; j += L64_THREADS) {
        d[j] = reduce<L0>(mulmod<L0>(x[j], n_inv0));
        d[N + j] = reduce<L1>(mulmod<L1>(x[N + j], n_inv1));
    }
}
