// helm_pbs_generic.inc — the generic blind-rotate kernel of the boolean engine (included by helm_hip.hip, main translation
// unit only).  The tuned builds above hard-wire k and pbs_l into wave maps and register layouts and cover N = 512 and 1024;
// this one takes k and pbs_l at run time and serves every other admitted shape (helm_hip_ctx_create: N in {256, 512, 1024,
// 2048}, (k+1) N <= 8192, the single-prime capacity bound), and any shape under HELM_HIP_PBS_VARIANT=10.
//
// One workgroup of 256 threads per bootstrap.  Everything a bootstrap touches lives in LDS (GenLds):
//   col   double [k+1][N]   the k+1 column sums of the external product, inverse-transformed in place
//   dig   double [D][N]     one batch of D digit polynomials (D <= 4, D N <= 2048, and no larger than keeps the occupancy
//                           of D = 1: helm_hip_ctx_create), forward-transformed in place
//   tw    double [2][N]     the context's bit-reversed psi and psi^-1 tables (setup_field_tables)
//   acc   u32    [k+1][N]   the accumulator GLWE
//   ms    u16    [n+1]      the modulus-switched input
// At the budget's edge ((k+1) N = 8192, N = 2048, D = 1, n = 1024) that is 64 + 16 + 32 + 32 + 2 = 146 KiB of the CU's 160.
//
// Per CMUX step: for each batch of digit polynomials q = r l + lev (polynomial r of X^a acc - acc, decomposition level lev,
// 0 = most significant, the order of the key's levels): decompose, forward-transform (radix-2 Cooley-Tukey stages, natural
// order in, bit-reversed out), multiply by the key polynomials (r, c, lev) streamed from HBM and add into column c; then
// inverse-transform the k+1 columns together (Gentleman-Sande, bit-reversed in, natural out; N^-1 is folded into the key),
// lift to the torus and add into the accumulator.
//
// Exactness, in FpH (p = 6432^4 + 1, 2^53 / p = 5.26) only: every value a transform stage stores is recentred (reduce:
// |x| <= p/2 + eps), so a butterfly's sum or difference is below 1.14 p and a mulmod of it below 0.83 p.  A product of a
// recentred transform output with a key word (|w| <= p/2) is below (0.5 + 0.75 (p/2) 2^-52) p = 0.64 p (mulmod's bound); a
// column sum enters a batch recentred and takes at most D <= 4 products: <= 0.5 p + 4 x 0.64 p = 3.07 p < 2^53, and it is
// recentred at the end of every batch - for any (k+1) l the domain admits.  The true integer coefficients of the external
// product are below (k+1) l N 2^(logB-1) 2^31 < p/2 (the capacity check), so the recentred inverse outputs are those
// integers, and to_torus32 takes them mod 2^32.  Why not the lazy fields: FpG and FpI skip recentrings on the strength of
// bounds derived for the tuned kernels' fixed shapes and of per-key norms; the generic kernel recentres everywhere and needs
// no shape-specific argument.  mulmod, reduce and to_torus32 carry ntt_fp64.h's HELM_BOUND checks, so the check build counts
// violations here as well.

constexpr int GEN_THREADS = 256;
constexpr int GEN_MAX_D = 4;

// digit polynomials transformed together: at most 4 (the column-sum bound above), D N <= 2048
static inline int gen_batch(int N, int k, int l)
{
    int d = std::max(1, 2048 / N);
    d = std::min(d, GEN_MAX_D);
    return std::min(d, (k + 1) * l);
}

// decompose_step (helm_hip.hip) with a full 32-bit multiply: that one computes the digit with a 24-bit multiply, exact only
// while the carried state stays below 2^23, i.e. logB (l-1) <= 22 - which the generic domain (logB l <= 31 under the capacity
// bound) does not guarantee: l = 5, logB = 6 reaches 2^24 after the first level.  Same recurrence otherwise (tfhe's
// SignedDecomposer, closest representable, balanced digits); the digit is state - next B computed mod 2^32 (|digit| <= B/2).
__device__ __forceinline__ int gen_decompose_step(uint32_t &state, int logB, uint32_t half_m1, bool last)
{
    const uint32_t s = state;
    const uint32_t tie = last ? 0u : (s >> (2 * logB - 1)) & 1u; // not last: l >= 2, so 2 logB - 1 <= 29
    const uint32_t next = (s + half_m1 + tie) >> logB;
    state = next;
    return (int)(s - (next << logB));
}

// LDS layout of k_pbs_generic (bytes), host and device
struct GenLds {
    size_t col, dig, tw, acc, ms, bytes;
    __host__ __device__ GenLds(int N, int K1, int D, int n)
    {
        col = 0;
        dig = col + sizeof(double) * (size_t)K1 * N;
        tw = dig + sizeof(double) * (size_t)D * N;
        acc = tw + sizeof(double) * 2 * (size_t)N;
        ms = acc + sizeof(uint32_t) * (size_t)K1 * N;
        bytes = (ms + sizeof(uint16_t) * ((size_t)n + 1) + 15) / 16 * 16;
    }
};

// cnt polynomials x[q N .. q N + N) (|coefficient| < 2^53, recentred on output): forward negacyclic transform, natural order
// in, bit-reversed out; tw: bit-reversed powers of psi.  Ends with a workgroup barrier.
template <int LOGN>
__device__ __forceinline__ void gen_ntt_forward(double *x, int cnt, const double *tw)
{
    constexpr int H = 1 << (LOGN - 1);
    for (int s = 0; s < LOGN; s++) {
        const int logt = LOGN - 1 - s, t = 1 << logt, m = 1 << s;
        for (int b = (int)threadIdx.x; b < cnt * H; b += GEN_THREADS) {
            const int q = b >> (LOGN - 1), k = b & (H - 1);
            const int i = k >> logt;
            double *y = x + ((size_t)q << LOGN) + (i << (logt + 1)) + (k & (t - 1));
            const double U = y[0], V = mulmod<FpH>(y[t], tw[m + i]);
            y[0] = reduce<FpH>(U + V);
            y[t] = reduce<FpH>(U - V);
        }
        __syncthreads();
    }
}

// inverse: bit-reversed in, natural out, without the 1/N; tw: bit-reversed powers of psi^-1.  Inputs recentred, outputs
// recentred.  Ends with a workgroup barrier.
template <int LOGN>
__device__ __forceinline__ void gen_ntt_inverse(double *x, int cnt, const double *tw)
{
    constexpr int H = 1 << (LOGN - 1);
    for (int s = 0; s < LOGN; s++) {
        const int logt = s, t = 1 << logt, h = H >> s;
        for (int b = (int)threadIdx.x; b < cnt * H; b += GEN_THREADS) {
            const int q = b >> (LOGN - 1), k = b & (H - 1);
            const int i = k >> logt;
            double *y = x + ((size_t)q << LOGN) + (i << (logt + 1)) + (k & (t - 1));
            const double U = y[0], V = y[t];
            y[0] = reduce<FpH>(U + V);
            y[t] = reduce<FpH>(mulmod<FpH>(U - V, tw[h + i]));
        }
        __syncthreads();
    }
}

// bsk: [i][r][c][lev][N] in the transform domain (bit-reversed order), times N^-1, recentred (k_bsk_convert_generic)
template <int LOGN>
__global__ __launch_bounds__(GEN_THREADS) void k_pbs_generic(const PbsJob *__restrict__ jobs,
                                                          const uint32_t *__restrict__ wires,  // rows of n+1
                                                          const uint32_t *__restrict__ raw_in, // rows of n+1
                                                          const uint32_t *__restrict__ tvs,    // rows of N
                                                          const double *__restrict__ bsk, const double *__restrict__ tw_fwd,
                                                          const double *__restrict__ tw_inv,
                                                          uint32_t *__restrict__ out_big, // rows of K*N+1
                                                          int n, int K, int L, int logB, int D)
{
    constexpr int N = 1 << LOGN;
    const int K1 = K + 1, QN = K1 * L, tid = (int)threadIdx.x;
    extern __shared__ __align__(16) unsigned char smem_gen[];
    const GenLds lay(N, K1, D, n);
    double *col = reinterpret_cast<double *>(smem_gen + lay.col);
    double *dig = reinterpret_cast<double *>(smem_gen + lay.dig);
    double *twf = reinterpret_cast<double *>(smem_gen + lay.tw);
    double *twi = twf + N;
    uint32_t *acc = reinterpret_cast<uint32_t *>(smem_gen + lay.acc);
    uint16_t *MS = reinterpret_cast<uint16_t *>(smem_gen + lay.ms);
    const PbsJob job = jobs[blockIdx.x];
    const size_t row = (size_t)n + 1;

    // ---- gate linear step + modulus switch, twiddle tables --------------------------------
    switch_row(MS, GateRows(job, wires, raw_in, row), n, tid, GEN_THREADS, LOGN + 1);
    for (int j = tid; j < N; j += GEN_THREADS) {
        twf[j] = tw_fwd[j];
        twi[j] = tw_inv[j];
    }
    __syncthreads();
    // ---- accumulator init: (0, ..., 0, X^{-b~} tv) -----------------------------------------
    {
        const int bt = (int)MS[n];
        const uint32_t *tv = tvs + (size_t)job.tv * N;
        for (int idx = tid; idx < K1 * N; idx += GEN_THREADS) {
            const int r = idx >> LOGN, j = idx & (N - 1);
            acc[idx] = r == K ? lut_rotated(tv, j, bt, N) : 0u;
        }
    }
    __syncthreads();

    // ---- blind rotation: acc += BSK_i (x) (X^{a_i} acc - acc) ------------------------------
    const int rep = logB * L;
    const uint32_t round_off = 1u << (31 - rep), half_m1 = (1u << (logB - 1)) - 1u;
    const size_t step_words = (size_t)K1 * K1 * L * N; // key words of one LWE coefficient
    for (int i = 0; i < n; i++) {
        const int a = (int)MS[i];
        const double *key = bsk + (size_t)i * step_words;
        for (int q0 = 0; q0 < QN; q0 += D) {
            const int cnt = QN - q0 < D ? QN - q0 : D;
            // digits of polynomials q0 .. q0 + cnt - 1
            for (int idx = tid; idx < (cnt << LOGN); idx += GEN_THREADS) {
                const int q = q0 + (idx >> LOGN), j = idx & (N - 1);
                const int r = q / L, lev = q - r * L;
                const uint32_t *ar = acc + r * N;
                const int s = (j - a) & (2 * N - 1); // (X^a acc_r)[j] = +-acc_r[j - a]
                const uint32_t rot = s < N ? ar[s] : 0u - ar[s - N];
                uint32_t state = (rot - ar[j] + round_off) >> (32 - rep);
                // digit lev is the (L - lev)-th the recurrence yields (least significant level first): the levels below it
                // are recomputed for every digit polynomial - O(l^2) cheap integer steps per coefficient, deliberate (no
                // per-coefficient state kept across batches; the transforms dominate for the l of real parameter sets)
                int d = 0;
                for (int lv = L - 1; lv >= lev; lv--) d = gen_decompose_step(state, logB, half_m1, lv == 0);
                dig[idx] = (double)d;
            }
            __syncthreads();
            gen_ntt_forward<LOGN>(dig, cnt, twf);
            // products into the column sums: each thread owns coefficients s of every column (no LDS hazard between
            // threads until the inverse transform's barrier).  Key polynomial (r, c, lev) of digit q = r l + lev starts at
            // ((r (k+1) + c) l + lev) N = koff[q] + c l N.
            size_t koff[GEN_MAX_D];
#pragma unroll
            for (int ql = 0; ql < GEN_MAX_D; ql++) {
                const int q = q0 + ql, r = q / L, lev = q - r * L;
                koff[ql] = ((size_t)r * K1 * L + lev) * N;
            }
            for (int s = tid; s < N; s += GEN_THREADS) {
                for (int c = 0; c < K1; c++) {
                    const double *kc = key + (size_t)c * L * N + s;
                    double sum = q0 == 0 ? 0.0 : col[c * N + s];
#pragma unroll
                    for (int ql = 0; ql < GEN_MAX_D; ql++)
                        if (ql < cnt) sum += mulmod<FpH>(dig[(ql << LOGN) + s], kc[koff[ql]]);
                    col[c * N + s] = reduce<FpH>(sum); // <= 0.5 p + D x 0.64 p before (see the head of this file)
                }
            }
            __syncthreads(); // the next batch overwrites dig
        }
        gen_ntt_inverse<LOGN>(col, K1, twi);
        for (int idx = tid; idx < K1 * N; idx += GEN_THREADS) acc[idx] += to_torus32(col[idx]);
        __syncthreads();
    }

    // ---- sample extract (coefficient 0) ----------------------------------------------------
    uint32_t *ob = big_row(out_big, blockIdx.x, K, N);
    for (int idx = tid; idx < K * N; idx += GEN_THREADS) {
        const int r = idx >> LOGN, t = idx & (N - 1);
        // out[r N + t] = (t == 0) ? A_r[0] : -A_r[N - t]
        ob[idx] = t == 0 ? acc[r * N] : 0u - acc[r * N + N - t];
    }
    if (tid == 0) ob[K * N] = acc[K * N]; // body = B[0]
}

// One workgroup per key polynomial: standard-domain u32 coefficients (taken as signed) -> forward transform -> x N^-1,
// recentred, bit-reversed order: dst[i][r][c][lev][N] (src is [i][lev][r][c][N]).
template <int LOGN>
__global__ __launch_bounds__(GEN_THREADS) void k_bsk_convert_generic(const uint32_t *__restrict__ src, double *__restrict__ dst,
                                                                  const double *__restrict__ tw_fwd, double n_inv, int K1, int L)
{
    constexpr int N = 1 << LOGN;
    __shared__ double x[N];
    const size_t poly = blockIdx.x; // index in src order
    const int c = (int)(poly % K1);
    const int r = (int)((poly / K1) % K1);
    const int lev = (int)((poly / ((size_t)K1 * K1)) % L);
    const size_t i = poly / ((size_t)K1 * K1 * L);
    for (int j = (int)threadIdx.x; j < N; j += GEN_THREADS) x[j] = (double)(int32_t)src[poly * N + j];
    __syncthreads();
    gen_ntt_forward<LOGN>(x, 1, tw_fwd);
    double *d = dst + (((i * K1 + r) * K1 + c) * L + lev) * N;
    for (int j = (int)threadIdx.x; j < N; j += GEN_THREADS) d[j] = reduce<FpH>(mulmod<FpH>(x[j], n_inv));
}

// NTT self-test of the generic class: forward, x N^-1, inverse; must reproduce the input exactly.
template <int LOGN>
__global__ __launch_bounds__(GEN_THREADS) void k_ntt_roundtrip_generic(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst,
                                                                    const double *__restrict__ tw_fwd,
                                                                    const double *__restrict__ tw_inv, double n_inv)
{
    constexpr int N = 1 << LOGN;
    __shared__ double x[N];
    const size_t base = (size_t)blockIdx.x * N;
    for (int j = (int)threadIdx.x; j < N; j += GEN_THREADS) x[j] = (double)(int32_t)src[base + j];
    __syncthreads();
    gen_ntt_forward<LOGN>(x, 1, tw_fwd);
    for (int j = (int)threadIdx.x; j < N; j += GEN_THREADS) x[j] = reduce<FpH>(mulmod<FpH>(x[j], n_inv));
    __syncthreads();
    gen_ntt_inverse<LOGN>(x, 1, tw_inv);
    for (int j = (int)threadIdx.x; j < N; j += GEN_THREADS) dst[base + j] = to_torus32(x[j]);
}
