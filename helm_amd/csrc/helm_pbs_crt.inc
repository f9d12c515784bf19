// helm_pbs_crt.inc — the two-prime blind-rotate kernel of the boolean engine (included by helm_hip.hip, main translation unit
// only).  Every other boolean kernel works in ONE prime below 2^51, so a shape runs only while its exact products stay below
// p/2: (k+1) l N 2^(logB-1) 2^31 < 2^49.6 (helm_hip_ctx_create's capacity check).  Shapes with few, wide decomposition levels
// lie beyond that - tfhe's boolean TFHE_LIB_PARAMETERS (k = 2, N = 1024, one level of 23 bits: 2^64.6), the later boolean
// default (k = 3, N = 512, two levels of 10 bits: 2^52).  k_pbs_crt is k_pbs_generic done in two fields, F0 = FpG and
// F1 = FpG2 (the CRT pair of the 64-bit engine's k_pbs64_generic), with a CRT lift to the torus: k, pbs_l and pbs_logB at run
// time, the domain helm_hip_ctx_create_ex admits under HELM_HIP_CREATE_ALLOW_CRT / HELM_HIP_CREATE_FORCE_CRT - N in {256,
// 512, 1024, 2048} (FpG2's 2-adicity is 2^12: 2N <= 4096), k >= 1, (k+1) N <= 4096, pbs_l >= 1, pbs_logB pbs_l <= 31,
// n <= 1024.  Same jobs, wires, raw inputs, test vectors and output rows as k_pbs_generic.
//
// One workgroup of 256 threads per bootstrap.  What a bootstrap works on lives in LDS (CrtLds):
//   acc   u32    [k+1][N]      the accumulator GLWE
//   col   double [2][k+1][N]   the k+1 column sums of the external product in both fields, inverse-transformed in place
//   dig   double [2][D][N]     one batch of D digit polynomials in both fields, forward-transformed in place (D N <= 1024,
//                              D <= 4; D = 1 at N = 2048; no larger than keeps the occupancy of D = 1: setup_crt)
//   ms    u16    [n+1]         the modulus-switched input
// At the domain's edge, (k+1) N = 4096: 16 + 64 + 16 (N = 2048: 32) + 2 = 98 (114) KiB of the CU's 160, one workgroup per CU.
// The four twiddle tables (forward and inverse, both fields: 32 N bytes) are read from global memory, where every workgroup of
// the device shares them in L2, as in k_pbs64_generic: in LDS they would not fit beside the rest at N = 2048.
//
// Per CMUX step: for each batch of digit polynomials q = r l + lev (polynomial r of X^a acc - acc, level lev, 0 = most
// significant): decompose (gen_decompose_step), forward-transform in both fields (radix-2 Cooley-Tukey, natural order in,
// bit-reversed out), multiply by the key polynomials (r, c, lev) streamed from HBM and add into column c; then
// inverse-transform the 2 (k+1) columns together (Gentleman-Sande, bit-reversed in, natural out; N^-1 is folded into the key),
// lift each coefficient's two residues to the integer mod 2^32 and add it into the accumulator; sample extract at the end.
//
// Decomposition at rep = logB l = 31, re-derived: round_off = 1 << (31 - rep) = 1 and the shift 32 - rep = 1, so the state is
// (x + 1) >> 1 < 2^31 - the closest multiple of 2 (x = 2^32 - 1 wraps to state 0: the torus element 0, correct).  One level
// of 31 bits: last = true (no tie bit; 2 logB - 1 = 61 is never used as a shift), half_m1 = 2^30 - 1, state + half_m1 < 2^32,
// next is 0 or 1, digit = state - next 2^31 in [-2^30 + 1, 2^30].  Several levels: logB <= 15, the tie shift 2 logB - 1 <= 29,
// and the state stays below 2^31 + 1 after each level (gen_decompose_step's 32-bit recurrence holds for any logB l <= 31).
//
// Exactness.  F0 = FpG (p0 = 5072^4 + 1 = 2^49.23, 2^53 / p0 = 13.6), F1 = FpG2 (p1 = 5096^4 + 1 = 2^49.26, 13.4).  Every
// value a transform stage stores is recentred (reduce: |x| <= p/2 + 1), so a butterfly's sum or difference is below 1.1 p and
// a mulmod of it below 0.6 p.  Digits are at most 2^30 in magnitude (logB = 31, l = 1): exact doubles below p/2 = 2^48.2, the
// same integer in both fields.  A product of a recentred transform output with a key word (|w| <= p/2) is below
// (0.5 + 0.75 (p/2) 2^-52) p = 0.56 p (mulmod's bound); a column sum enters a batch recentred and takes at most D <= 4
// products: <= 0.5 p + 4 x 0.56 p = 2.8 p < 2^53, and it is recentred at the end of every batch - for any (k+1) l.  No lazy
// stage, no short-root stage: nothing here rests on a shape.  The inverse transform's outputs are recentred too:
// r_f = x mod p_f, |r_f| <= p_f/2 + 1, where x is the true integer coefficient of the external product (key words taken as
// centred 32-bit integers), |x| <= (k+1) l N 2^(logB-1) 2^31 <= 4096 x 31 x 2^30 x 2^31 < 2^78 over the whole domain, against
// p0 p1 / 2 = 2^97.5: the domain needs no capacity check (helm_hip.hip restates this as a static_assert).  The lift
//   t = reduce<F1>(mulmod<F1>(reduce<F1>(r1 - r0), p0^-1 mod p1)),   x' = r0 + p0 t
// is congruent to x mod p0 p1 with |x'| <= p0 p1 / 2 + 1.5 p0 + 1, so |x' - x| < p0 p1 and x' = x.  t is RECENTRED: with t
// merely below 0.56 p1 (mulmod's bound) x' could be x +- p0 p1 once |x| passes 0.78 of the half - what round 16 found in the
// 64-bit engine's lift_pairs.  The torus word x mod 2^32 is formed from the two exact values in 32-bit arithmetic,
// (uint32_t)r0 + (uint32_t)p0 (uint32_t)t (to_torus32: |r0|, |t| < 2^51) - no value of magnitude 2^63 or more is ever formed,
// although |x| itself passes 2^63 (TFHE_LIB's shape: 2^64.6).  The torus arithmetic is therefore the exact negacyclic product
// mod 2^32 whatever the shape.  mulmod, reduce and to_torus32 carry ntt_fp64.h's HELM_BOUND checks, but the bound-checking
// build does not run this kernel: it is built like k_pbs64_generic, whose -O0 counting build faulted on its first launch for
// a cause not found (DESIGN.md 4.4.1), so that build refuses a CRT context at creation (setup_crt).

using CrtF0 = FpG;
using CrtF1 = FpG2;
constexpr int CRT_THREADS = 256;
constexpr int CRT_MAX_D = 4;
static_assert(5072ull * 5072 * 5072 * 5072 + 1 == CrtF0::P_U64 && 5096ull * 5096 * 5096 * 5096 + 1 == CrtF1::P_U64, "the CRT pair");

// digit polynomials transformed together: at most 4 (the column-sum bound above), D N <= 1024 (one at N = 2048)
static inline int crt_batch(int N, int k, int l)
{
    int d = std::max(1, 1024 / N);
    d = std::min(d, CRT_MAX_D);
    return std::min(d, (k + 1) * l);
}

// LDS layout of k_pbs_crt (bytes), host and device
struct CrtLds {
    size_t acc, col, dig, ms, bytes;
    __host__ __device__ CrtLds(int N, int K1, int D, int n)
    {
        acc = 0;
        col = acc + sizeof(uint32_t) * (size_t)K1 * N;
        dig = col + sizeof(double) * 2 * (size_t)K1 * N;
        ms = dig + sizeof(double) * 2 * (size_t)D * N;
        bytes = (ms + sizeof(uint16_t) * ((size_t)n + 1) + 15) / 16 * 16;
    }
};

template <typename F>
__device__ __forceinline__ void crt_fwd_bfly(double *y, int t, double w)
{
    const double U = y[0], V = mulmod<F>(y[t], w);
    y[0] = reduce<F>(U + V);
    y[t] = reduce<F>(U - V);
}

template <typename F>
__device__ __forceinline__ void crt_inv_bfly(double *y, int t, double w)
{
    const double U = y[0], V = y[t];
    y[0] = reduce<F>(U + V);
    y[t] = reduce<F>(mulmod<F>(U - V, w));
}

// cnt polynomials per field, field 0 at x[q N], field 1 at x[fstride + q N]: forward negacyclic transform, natural order in,
// bit-reversed out, inputs |x| < 2^52, outputs recentred.  tw0 / tw1: bit-reversed powers of psi in each field (global
// memory).  Ends with a workgroup barrier.
template <int LOGN>
__device__ __forceinline__ void crt_ntt_forward(double *x, int cnt, int fstride, const double *__restrict__ tw0,
                                                const double *__restrict__ tw1)
{
    constexpr int H = 1 << (LOGN - 1);
    const int per_f = cnt * H;
    for (int s = 0; s < LOGN; s++) {
        const int logt = LOGN - 1 - s, t = 1 << logt, m = 1 << s;
        for (int b = (int)threadIdx.x; b < 2 * per_f; b += CRT_THREADS) {
            const int f = b >= per_f ? 1 : 0, r = b - f * per_f; // (per_f is a multiple of 64: f is uniform over a wave)
            const int q = r >> (LOGN - 1), k = r & (H - 1), i = k >> logt;
            double *y = x + (size_t)f * fstride + ((size_t)q << LOGN) + (i << (logt + 1)) + (k & (t - 1));
            if (f == 0) crt_fwd_bfly<CrtF0>(y, t, tw0[m + i]);
            else crt_fwd_bfly<CrtF1>(y, t, tw1[m + i]);
        }
        __syncthreads();
    }
}

// inverse: bit-reversed in, natural out, without the 1/N; twi0 / twi1: bit-reversed powers of psi^-1.  Inputs and outputs
// recentred.  Ends with a workgroup barrier.
template <int LOGN>
__device__ __forceinline__ void crt_ntt_inverse(double *x, int cnt, int fstride, const double *__restrict__ twi0,
                                                const double *__restrict__ twi1)
{
    constexpr int H = 1 << (LOGN - 1);
    const int per_f = cnt * H;
    for (int s = 0; s < LOGN; s++) {
        const int logt = s, t = 1 << logt, h = H >> s;
        for (int b = (int)threadIdx.x; b < 2 * per_f; b += CRT_THREADS) {
            const int f = b >= per_f ? 1 : 0, r = b - f * per_f;
            const int q = r >> (LOGN - 1), k = r & (H - 1), i = k >> logt;
            double *y = x + (size_t)f * fstride + ((size_t)q << LOGN) + (i << (logt + 1)) + (k & (t - 1));
            if (f == 0) crt_inv_bfly<CrtF0>(y, t, twi0[h + i]);
            else crt_inv_bfly<CrtF1>(y, t, twi1[h + i]);
        }
        __syncthreads();
    }
}

// the integer x with x = r0 (mod p0), x = r1 (mod p1), |x| < p0 p1 / 2, taken mod 2^32 (r0, r1 recentred): see the head of
// this file
__device__ __forceinline__ uint32_t crt_lift32(double r0, double r1, double p0inv_mod_p1)
{
    const double t = reduce<CrtF1>(mulmod<CrtF1>(reduce<CrtF1>(r1 - r0), p0inv_mod_p1));
    return to_torus32(r0) + (uint32_t)CrtF0::P_U64 * to_torus32(t);
}

// bsk: [i][r][c][lev][f][N] in the transform domain (bit-reversed order), times N^-1, recentred (k_bsk_convert_crt)
template <int LOGN>
__global__ __launch_bounds__(CRT_THREADS) void k_pbs_crt(const PbsJob *__restrict__ jobs,
                                                      const uint32_t *__restrict__ wires,  // rows of n+1
                                                      const uint32_t *__restrict__ raw_in, // rows of n+1
                                                      const uint32_t *__restrict__ tvs,    // rows of N
                                                      const double *__restrict__ bsk,
                                                      const double *__restrict__ tw0, const double *__restrict__ tw1,
                                                      const double *__restrict__ twi0, const double *__restrict__ twi1,
                                                      uint32_t *__restrict__ out_big, // rows of K*N+1
                                                      int n, int K, int L, int logB, int D, double p0inv_mod_p1)
{
    constexpr int N = 1 << LOGN;
    const int K1 = K + 1, QN = K1 * L, tid = (int)threadIdx.x;
    extern __shared__ __align__(16) unsigned char smem_crt[];
    const CrtLds lay(N, K1, D, n);
    uint32_t *acc = reinterpret_cast<uint32_t *>(smem_crt + lay.acc);
    double *col = reinterpret_cast<double *>(smem_crt + lay.col);
    double *dig = reinterpret_cast<double *>(smem_crt + lay.dig);
    uint16_t *MS = reinterpret_cast<uint16_t *>(smem_crt + lay.ms);
    const PbsJob job = jobs[blockIdx.x];
    const size_t row = (size_t)n + 1;

    // ---- gate linear step + modulus switch ---------------------------------------------------
    {
        const uint32_t *a0 = nullptr, *a1 = nullptr, *a2 = nullptr;
        if (job.op < 0) a0 = raw_in + row * (size_t)job.in0;
        else {
            if (job.in0 >= 0) a0 = wires + row * (size_t)job.in0;
            if (job.in1 >= 0) a1 = wires + row * (size_t)job.in1;
            if (job.in2 >= 0) a2 = wires + row * (size_t)job.in2;
        }
        for (int i = tid; i <= n; i += CRT_THREADS) {
            uint32_t v;
            if (job.op < 0) v = a0[i];
            else v = gate_lincomb(job.op, job.which, a0 ? a0[i] : 0u, a1 ? a1[i] : 0u, a2 ? a2[i] : 0u, i == n);
            MS[i] = (uint16_t)modswitch(v, LOGN + 1);
        }
    }
    __syncthreads();
    // ---- accumulator init: (0, ..., 0, X^{-b~} tv) -----------------------------------------
    {
        const int bt = (int)MS[n];
        const uint32_t *tv = tvs + (size_t)job.tv * N;
        for (int idx = tid; idx < K1 * N; idx += CRT_THREADS) {
            const int r = idx >> LOGN, j = idx & (N - 1);
            uint32_t v = 0;
            if (r == K) {
                const int s = (j + bt) & (2 * N - 1);
                v = tv[s & (N - 1)];
                if (s >= N) v = 0u - v;
            }
            acc[idx] = v;
        }
    }
    __syncthreads();

    // ---- blind rotation: acc += BSK_i (x) (X^{a_i} acc - acc) ------------------------------
    const int rep = logB * L; // <= 31
    const uint32_t round_off = 1u << (31 - rep), half_m1 = (1u << (logB - 1)) - 1u;
    const size_t step_words = (size_t)K1 * K1 * L * 2 * N; // key words of one LWE coefficient
    const int cstride = K1 * N, dstride = D * N;           // field 1's columns / digits
    for (int i = 0; i < n; i++) {
        const int a = (int)MS[i];
        const double *key = bsk + (size_t)i * step_words;
        for (int q0 = 0; q0 < QN; q0 += D) {
            const int cnt = QN - q0 < D ? QN - q0 : D;
            // digits of polynomials q0 .. q0 + cnt - 1, the same integers in both fields
            for (int idx = tid; idx < (cnt << LOGN); idx += CRT_THREADS) {
                const int q = q0 + (idx >> LOGN), j = idx & (N - 1);
                const int r = q / L, lev = q - r * L;
                const uint32_t *ar = acc + r * N;
                const int s = (j - a) & (2 * N - 1); // (X^a acc_r)[j] = +-acc_r[j - a]
                const uint32_t rot = s < N ? ar[s] : 0u - ar[s - N];
                uint32_t state = (rot - ar[j] + round_off) >> (32 - rep);
                // digit lev is the (L - lev)-th the recurrence yields (least significant level first): the levels below it
                // are recomputed for every digit polynomial, as in k_pbs_generic
                int d = 0;
                for (int lv = L - 1; lv >= lev; lv--) d = gen_decompose_step(state, logB, half_m1, lv == 0);
                dig[idx] = (double)d;
                dig[dstride + idx] = (double)d;
            }
            __syncthreads();
            crt_ntt_forward<LOGN>(dig, cnt, dstride, tw0, tw1);
            // products into the column sums: thread slot u = (field, coefficient s) owns that coefficient of every column
            // (no LDS hazard between threads until the inverse transform's barrier).  Key polynomial (r, c, lev) of digit
            // q = r l + lev in field f starts at (((r (k+1) + c) l + lev) 2 + f) N = koff[q] + (c l 2 + f) N.
            size_t koff[CRT_MAX_D];
#pragma unroll
            for (int ql = 0; ql < CRT_MAX_D; ql++) {
                const int q = q0 + ql, r = q / L, lev = q - r * L;
                koff[ql] = ((size_t)r * K1 * L + lev) * 2 * N;
            }
            for (int u = tid; u < 2 * N; u += CRT_THREADS) {
                const int f = u >= N ? 1 : 0, s = u & (N - 1); // (f is uniform over a wave)
                const double *dg = dig + (size_t)f * dstride + s;
                for (int c = 0; c < K1; c++) {
                    const double *kc = key + ((size_t)c * L * 2 + f) * N + s;
                    double *cs = col + (size_t)f * cstride + (size_t)c * N + s;
                    double sum = q0 == 0 ? 0.0 : *cs;
                    if (f == 0) {
#pragma unroll
                        for (int ql = 0; ql < CRT_MAX_D; ql++)
                            if (ql < cnt) sum += mulmod<CrtF0>(dg[ql << LOGN], kc[koff[ql]]);
                        *cs = reduce<CrtF0>(sum); // <= 0.5 p + D x 0.56 p before (see the head of this file)
                    } else {
#pragma unroll
                        for (int ql = 0; ql < CRT_MAX_D; ql++)
                            if (ql < cnt) sum += mulmod<CrtF1>(dg[ql << LOGN], kc[koff[ql]]);
                        *cs = reduce<CrtF1>(sum);
                    }
                }
            }
            __syncthreads(); // the next batch overwrites dig
        }
        crt_ntt_inverse<LOGN>(col, K1, cstride, twi0, twi1);
        // CRT lift of each coefficient's two residues to the exact integer, accumulated mod 2^32
        for (int idx = tid; idx < K1 * N; idx += CRT_THREADS) acc[idx] += crt_lift32(col[idx], col[cstride + idx], p0inv_mod_p1);
        __syncthreads();
    }

    // ---- sample extract (coefficient 0) ----------------------------------------------------
    uint32_t *ob = out_big + (size_t)blockIdx.x * ((size_t)K * N + 1);
    for (int idx = tid; idx < K * N; idx += CRT_THREADS) {
        const int r = idx >> LOGN, t = idx & (N - 1);
        // out[r N + t] = (t == 0) ? A_r[0] : -A_r[N - t]
        ob[idx] = t == 0 ? acc[r * N] : 0u - acc[r * N + N - t];
    }
    if (tid == 0) ob[K * N] = acc[K * N]; // body = B[0]
}

// One workgroup per key polynomial: standard-domain u32 coefficients (taken as signed: |v| <= 2^31 < p/2, the same integer in
// both fields) -> forward transform in both fields -> x N^-1, recentred, bit-reversed order.  dst[i][r][c][lev][f][N] (src is
// [i][lev][r][c][N]): the two fields of one key polynomial are adjacent runs of N doubles, so a workgroup's wave reads 512
// contiguous bytes per (digit, column) in either field - 16 bytes of HBM per key word.
template <int LOGN>
__global__ __launch_bounds__(CRT_THREADS) void k_bsk_convert_crt(const uint32_t *__restrict__ src, double *__restrict__ dst,
                                                              const double *__restrict__ tw0, const double *__restrict__ tw1,
                                                              double n_inv0, double n_inv1, int K1, int L)
{
    constexpr int N = 1 << LOGN;
    __shared__ double x[2 * N];
    const size_t poly = blockIdx.x; // index in src order
    const int c = (int)(poly % K1);
    const int r = (int)((poly / K1) % K1);
    const int lev = (int)((poly / ((size_t)K1 * K1)) % L);
    const size_t i = poly / ((size_t)K1 * K1 * L);
    for (int j = (int)threadIdx.x; j < N; j += CRT_THREADS) {
        const double v = (double)(int32_t)src[poly * N + j];
        x[j] = v;
        x[N + j] = v;
    }
    __syncthreads();
    crt_ntt_forward<LOGN>(x, 1, N, tw0, tw1);
    double *d = dst + ((((i * K1 + r) * K1 + c) * L + lev) * 2) * N;
    for (int j = (int)threadIdx.x; j < N; j += CRT_THREADS) {
        d[j] = reduce<CrtF0>(mulmod<CrtF0>(x[j], n_inv0));
        d[N + j] = reduce<CrtF1>(mulmod<CrtF1>(x[N + j], n_inv1));
    }
}

// NTT self-test of the CRT class: forward in both fields, x N^-1, inverse, lift; must reproduce the input exactly.
template <int LOGN>
__global__ __launch_bounds__(CRT_THREADS) void k_ntt_roundtrip_crt(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst,
                                                                const double *__restrict__ tw0, const double *__restrict__ tw1,
                                                                const double *__restrict__ twi0, const double *__restrict__ twi1,
                                                                double n_inv0, double n_inv1, double p0inv_mod_p1)
{
    constexpr int N = 1 << LOGN;
    __shared__ double x[2 * N];
    const size_t base = (size_t)blockIdx.x * N;
    for (int j = (int)threadIdx.x; j < N; j += CRT_THREADS) {
        const double v = (double)(int32_t)src[base + j];
        x[j] = v;
        x[N + j] = v;
    }
    __syncthreads();
    crt_ntt_forward<LOGN>(x, 1, N, tw0, tw1);
    for (int j = (int)threadIdx.x; j < N; j += CRT_THREADS) {
        x[j] = reduce<CrtF0>(mulmod<CrtF0>(x[j], n_inv0));
        x[N + j] = reduce<CrtF1>(mulmod<CrtF1>(x[N + j], n_inv1));
    }
    __syncthreads();
    crt_ntt_inverse<LOGN>(x, 1, N, twi0, twi1);
    for (int j = (int)threadIdx.x; j < N; j += CRT_THREADS) dst[base + j] = crt_lift32(x[j], x[N + j], p0inv_mod_p1);
}
