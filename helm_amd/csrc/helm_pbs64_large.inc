// helm_pbs64_large.inc — the large-N blind-rotate kernel of the 64-bit engine (included by helm_shortint.hip after
// helm_pbs64_generic.inc, main translation unit only).  k = 1, N = 4096: the shape of the 5-bit shortint sets
// (message_modulus * carry_modulus = 32), admitted by helm_si_ctx_create_ex under HELM_SI_CREATE_LARGE_N.  pbs_l, pbs_logB and
// n come at run time.  Same jobs and buffers as k_pbs64_generic: modulus switch, classical blind rotation with the job's
// look-up table, sample extract (many-LUT: extracts at 0, N/M, 2N/M, ...) into rows of N + 1 words.
//
// Why it is its own kernel.  (1) The field: FpG2 (5096^4 + 1) has 2-adicity 2^12, so it holds no 8192-th root of unity; the
// pair here is L0 = FpG (5072^4 + 1, 2^16 | p - 1) and L1 = FpI (5440^4 + 1, 2^24 | p - 1), p0 p1 / 2 = 2^97.87.  (2) LDS:
// TwoPrimeLds<uint64_t> at k = 1, N = 4096 would be 64 (acc) + 128 (col, both fields) + 64 (dig) KiB.  (3) One workgroup per
// CU is all that fits, so the workgroup is wide.
//
// One workgroup of 1024 threads (16 waves, four per SIMD, <= 128 VGPRs per lane) per bootstrap.  LDS (Large64Lds):
//   acc   u64    [2][N]    the accumulator GLWE                                                      64 KiB
//   buf   double [2][N]    ONE transform buffer, both fields: a digit polynomial going forward,
//                          then a column of the external product going back                          64 KiB
//   ms    u16    [n+1]     the modulus-switched input                                                <= 2 KiB
// 130 KiB of the CU's 160: one workgroup per CU.  Thread `tid` owns the PT = N / 1024 = 4 positions tid + 1024 m of each
// field of buf: it writes the digits there, multiplies the spectrum there, and lifts the coefficients there - so the only
// barriers are those of the transforms' stages, one before a transform (the stages read other threads' positions) and one
// after a step's last lift (the next step's digits read the accumulator at rotated positions).
//
// Per CMUX step (skipped when the rotation is 0): for each digit polynomial q = r l + lev of X^a acc - acc (r < 2, level 0 =
// most significant; the digit recurrence of k_pbs64_generic): digits into buf, the same integers in both fields; forward
// transform in both fields at once (radix-2 Cooley-Tukey, natural in, bit-reversed out); each thread multiplies its 4
// positions per field by the key words of both columns (streamed from HBM / L2) and keeps the 2 columns x 2 fields x 4 = 16
// column sums in registers.  After the last digit polynomial, per column: the sums go back into buf, recentred; inverse
// transform (Gentleman-Sande, bit-reversed in, natural out; N^-1 is folded into the key); CRT lift of each coefficient's two
// residues to the integer mod 2^64, added into the accumulator.  Twiddles come from global memory (4 tables of 32 KiB, shared
// by every workgroup in L2).
//
// Exactness.  p0 = 2^49.23 (2^53 / p0 = 13.6), p1 = 2^49.64 (2^53 / p1 = 10.28): the argument is made for p1, the tighter
// field, and holds for p0 a fortiori.  As in k_pbs64_generic there is no lazy stage and no short-root stage: every value a
// transform stage stores is recentred (reduce: |x| <= p/2 + 1).
//   * mulmod(a, w), |w| <= p/2: |r| <= (0.5 + 0.75 |a| 2^-52) p.  For a recentred a (|a| <= p1/2 + 1 = 2^48.64) that is
//     (0.5 + 0.75 x 2^-3.36) p = 0.573 p, "below about 0.58 p".
//   * forward butterfly: U +- mulmod(V, w) with U, V recentred: <= 0.5 p + 0.58 p = 1.08 p < 2^53, then recentred.
//   * inverse butterfly: U +- V <= p + 2 (recentred next, or multiplied: mulmod of |a| <= p + 2 = 2^49.64 is below
//     (0.5 + 0.75 x 2^-2.36) p = 0.65 p, then recentred).
//   * digits are at most 2^23 < p/2 in magnitude, the same integer in both fields.
//   * a column sum takes a product of a recentred transform output with a key word (|w| <= p/2): each below 0.58 p.  It is
//     recentred after at most FOUR products (after q = 3, 7, ..., and when it is written back): <= 0.5 p + 4 x 0.58 p =
//     2.82 p < 10.28 p = 2^53, for any l.
//   * the inverse transform's outputs are recentred: r_f = x mod p_f, |r_f| <= p_f/2 + 1, where x is the true integer
//     coefficient of the external product, |x| <= (k+1) l N 2^(logB-1) 2^63 = l 2^(75+logB) < p0 p1 / 2 / 1.001 (the capacity
//     check of helm_si_ctx_create_ex with THIS pair's product: (l, logB) = (1, 22) is at 0.547 of p0 p1 / 2, (1, 23) is
//     refused).
//   * the lift: t = (r1 - r0) p0^-1 mod p1.  |r1 - r0| <= p0/2 + p1/2 + 2 < 2^49.5, so the mulmod is below 0.63 p1 and its
//     recentring gives |t| <= p1/2 + 1 < 2^48.7 < 2^51 - the quotient is recentred, as in the generic and multi-bit lifts.
//     x' = r0 + p0 t is congruent to x mod p0 p1 and |x'| <= p0 p1 / 2 + 1.5 p0 + 1, so |x' - x| < p0 p1 (1 - 0.0005) +
//     1.5 p0 + 1 < p0 p1 and x' = x exactly; it is formed mod 2^64 from the two exact int64 values (to_int64: |r0|, |t| <
//     2^51, HELM_BOUND slot 4).
// The torus arithmetic is therefore the exact negacyclic product mod 2^64 for every admitted shape
// (tests/test_large_n_bounds.py restates these bounds with exact fractions).
//
// Multi-bit form (template argument GG = grouping factor 2 or 3, HELM_SI_CREATE_LARGE_MULTIBIT; GG = 0 is the classical form
// above).  The algorithm is the one at the head of helm_pbs64_generic.inc: per group t < n / GG ONE external product,
// acc <- (sum_S X^(e_S) GGSW_{t,S}) (x) acc with e_S = sum_{i in S} a~_i mod 2N (uniform over the workgroup, in scalar
// registers).  The digits are those of the accumulator itself at the thread's own positions (no rotation, no difference), the
// column sums are sum_S sum_q (d^_q . M(e_S)) . K^_{t,S}[q][c], and the lifted value REPLACES the accumulator.  No group is
// skipped, not one whose rotations are all 0: the oracle does not skip either, and the step is not the identity on the low
// bits.  M(e)[s] = psi^(expo(s) e), expo(s) = 2 rev(s) + 1: l64_ntt_forward has the generic kernel's Cooley-Tukey structure
// (twiddle m + i), so position s holds the value at psi^(2 rev(s) + 1).  M is read per use from the context's table of the 2N
// powers of psi in each field of this pair ([2][2N] doubles in global memory, written once at creation).  All 2 l digit
// polynomials go forward once, the 16 sums stay in registers, both columns are lifted after the last digit polynomial; the
// barriers stand where they stood (a step reads the accumulator at own positions only; the one that ends a step still orders
// the body coefficient for the sample extract).
// Exactness of the multi-bit form, for p1.  d^ is recentred and |M| <= p/2, so d^ M = mulmod(d^, M) is below 0.58 p; its
// product with a key word is below (0.5 + 0.75 x 0.58 p 2^-52) p < 0.59 p.  A sum is recentred after every four products
// (the 2^GG subsets of one digit polynomial in runs of four): <= 0.5 p + 4 x 0.59 p < 2.9 p < 2^53 = 10.28 p.  The true
// integer coefficient is bounded by helm_si_load_bootstrap_key's group-sum rule for the key at hand (below p0 p1 / 2 / 1.001
// with THIS pair's product), so the recentred lift is exact (tests/test_large_multibit_bounds.py restates these numbers).

using L0 = FpG;
using L1 = FpI;

constexpr int L64_THREADS = 1024;

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

// One polynomial per field, field 0 at x[0 .. N), field 1 at x[N .. 2N): forward negacyclic transform, natural order in,
// bit-reversed out, inputs |x| < 2^52, outputs recentred.  tw0 / tw1: bit-reversed powers of psi in each field (global
// memory).  N / L64_THREADS butterflies per thread and stage, the field uniform over a wave.  Ends with a workgroup barrier.
template <int LOGN>
__device__ __forceinline__ void l64_ntt_forward(double *x, const double *__restrict__ tw0, const double *__restrict__ tw1)
{
    constexpr int N = 1 << LOGN, H = N / 2;
    static_assert(H % L64_THREADS == 0, "whole rounds of butterflies per field");
    for (int s = 0; s < LOGN; s++) {
        const int logt = LOGN - 1 - s, t = 1 << logt, m = 1 << s;
#pragma unroll
        for (int b0 = 0; b0 < 2 * H; b0 += L64_THREADS) {
            const int b = b0 + (int)threadIdx.x, k = b & (H - 1), i = k >> logt;
            double *y = x + (b0 >= H ? N : 0) + (i << (logt + 1)) + (k & (t - 1));
            if (b0 < H) tp_fwd_bfly<L0>(y, t, tw0[m + i]);
            else tp_fwd_bfly<L1>(y, t, tw1[m + i]);
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
        for (int b0 = 0; b0 < 2 * H; b0 += L64_THREADS) {
            const int b = b0 + (int)threadIdx.x, k = b & (H - 1), i = k >> logt;
            double *y = x + (b0 >= H ? N : 0) + (i << (logt + 1)) + (k & (t - 1));
            if (b0 < H) tp_inv_bfly<L0>(y, t, twi0[h + i]);
            else tp_inv_bfly<L1>(y, t, twi1[h + i]);
        }
        __syncthreads();
    }
}

// bsk: [i][r][c][lev][f][N] in the transform domain (bit-reversed order), times N^-1, recentred (k_bsk_convert64_large);
// GG > 0 (multi-bit): i = t 2^GG + S, n a multiple of GG, psi_pow the 2N powers of psi per field ([2][2N])
template <int LOGN, int GG = 0>
__global__ __launch_bounds__(L64_THREADS) void k_pbs64_large(const Pbs64Job *__restrict__ jobs,
                                                             const uint64_t *__restrict__ small, // rows of n+1
                                                             const uint64_t *__restrict__ luts,  // rows of N
                                                             const double *__restrict__ bsk,
                                                             const double *__restrict__ tw0, const double *__restrict__ tw1,
                                                             const double *__restrict__ twi0, const double *__restrict__ twi1,
                                                             const double *__restrict__ psi_pow,
                                                             uint64_t *__restrict__ out, // rows of N+1
                                                             int n, int L, int logB, double p0inv_mod_p1)
{
    constexpr int N = 1 << LOGN, PT = N / L64_THREADS;
    static_assert(PT >= 1 && N % L64_THREADS == 0, "whole positions per thread");
    const int tid = (int)threadIdx.x;
    extern __shared__ __align__(16) unsigned char smem_l64[];
    const Large64Lds lay(N, n);
    uint64_t *acc = reinterpret_cast<uint64_t *>(smem_l64 + lay.acc);
    double *buf = reinterpret_cast<double *>(smem_l64 + lay.buf);
    uint16_t *MS = reinterpret_cast<uint16_t *>(smem_l64 + lay.ms);
    const Pbs64Job job = jobs[blockIdx.x];

    // ---- modulus switch --------------------------------------------------------------------
    const uint64_t *lwe = small + (size_t)job.in_row * ((size_t)n + 1);
    for (int i = tid; i <= n; i += L64_THREADS) MS[i] = (uint16_t)modswitch64(lwe[i], LOGN + 1);
    __syncthreads();
    // ---- accumulator: (0, X^{-b~} lut) -----------------------------------------------------
    {
        const int bt = (int)MS[n];
        const uint64_t *tv = luts + (size_t)job.lut * N;
#pragma unroll
        for (int m = 0; m < PT; m++) {
            const int j = tid + m * L64_THREADS, s = (j + bt) & (2 * N - 1);
            const uint64_t v = tv[s & (N - 1)];
            acc[j] = 0;
            acc[N + j] = s >= N ? 0ull - v : v;
        }
    }
    __syncthreads();

    // ---- blind rotation: acc += BSK_i (x) (X^{a_i} acc - acc) ------------------------------
    const int rep = logB * L; // <= 31
    const uint64_t round_off = 1ull << (63 - rep);
    const uint32_t half_m1 = (1u << (logB - 1)) - 1u;
    const size_t step_words = (size_t)4 * L * 2 * N; // key words of one GGSW
    if constexpr (GG == 0) // (classical form; the multi-bit form is the else branch below)
    for (int i = 0; i < n; i++) {
        const int a = (int)MS[i];
        if (a == 0) continue; // uniform over the workgroup
        const double *key = bsk + (size_t)i * step_words;
        double sum[2][2][PT]; // [column][field][position]: registers (every index below is a compile-time constant)
        for (int q = 0; q < 2 * L; q++) {
            const int r = q >= L ? 1 : 0, lev = q - r * L;
            // digits of polynomial q at this thread's positions, the same integers in both fields
            const uint64_t *ar = acc + (size_t)r * N;
#pragma unroll
            for (int m = 0; m < PT; m++) {
                const int j = tid + m * L64_THREADS;
                const int s = (j - a) & (2 * N - 1); // (X^a acc_r)[j] = +-acc_r[j - a]
                const uint64_t rot = s < N ? ar[s] : 0ull - ar[s - N];
                uint32_t state = (uint32_t)((rot - ar[j] + round_off) >> (64 - rep));
                int d = 0; // digit lev is the (L - lev)-th the recurrence yields (least significant level first)
                for (int lv = L - 1; lv >= lev; lv--) d = g64_decompose_step(state, logB, half_m1);
                buf[j] = (double)d;
                buf[N + j] = (double)d;
            }
            __syncthreads();
            l64_ntt_forward<LOGN>(buf, tw0, tw1);
            // products at this thread's positions: key polynomial (r, c, lev) in field f starts at
            // (((r 2 + c) l + lev) 2 + f) N
            const bool fold = (q & 3) == 3; // recentre after every fourth product (see the head of this file)
#pragma unroll
            for (int c = 0; c < 2; c++) {
                const double *kc = key + (((size_t)(r * 2 + c) * L + lev) * 2) * N;
#pragma unroll
                for (int m = 0; m < PT; m++) {
                    const int s = tid + m * L64_THREADS;
                    const double v0 = mulmod<L0>(buf[s], kc[s]), v1 = mulmod<L1>(buf[N + s], kc[N + s]);
                    double s0 = q == 0 ? v0 : sum[c][0][m] + v0, s1 = q == 0 ? v1 : sum[c][1][m] + v1;
                    if (fold) {
                        s0 = reduce<L0>(s0); // <= 0.5 p + 4 x 0.58 p before
                        s1 = reduce<L1>(s1);
                    }
                    sum[c][0][m] = s0;
                    sum[c][1][m] = s1;
                }
            }
            // (no barrier: the next digits, or the column below, overwrite this thread's own positions only)
        }
#pragma unroll
        for (int c = 0; c < 2; c++) {
#pragma unroll
            for (int m = 0; m < PT; m++) {
                const int s = tid + m * L64_THREADS;
                buf[s] = reduce<L0>(sum[c][0][m]);
                buf[N + s] = reduce<L1>(sum[c][1][m]);
            }
            __syncthreads();
            l64_ntt_inverse<LOGN>(buf, twi0, twi1);
            // CRT lift of each coefficient's two residues to the exact integer, accumulated mod 2^64
#pragma unroll
            for (int m = 0; m < PT; m++) {
                const int j = tid + m * L64_THREADS;
                const double r0 = buf[j], r1 = buf[N + j];
                const double t = reduce<L1>(mulmod<L1>(r1 - r0, p0inv_mod_p1));
                HELM_BOUND(__builtin_fabs(r0) < 0x1p51 && __builtin_fabs(t) < 0x1p51, 4);
                acc[(size_t)c * N + j] += (uint64_t)to_int64(r0) + L0::P_U64 * (uint64_t)to_int64(t);
            }
        }
        __syncthreads(); // the next step's digits read the accumulator at rotated positions
    }
    // ---- multi-bit blind rotation: acc <- (sum_S X^(e_S) BSK_{t,S}) (x) acc ------------------
    else
    for (int t = 0; t < n / GG; t++) {
        constexpr int SUB = 1 << GG;
        // the group's rotations, uniform over the workgroup: scalar registers
        int am[GG];
#pragma unroll
        for (int i = 0; i < GG; i++) am[i] = __builtin_amdgcn_readfirstlane((int)MS[t * GG + i]);
        const double *key = bsk + (size_t)t * SUB * step_words;
        double sum[2][2][PT]; // [column][field][position]: registers (every index below is a compile-time constant)
#pragma unroll
        for (int m = 0; m < PT; m++) sum[0][0][m] = sum[0][1][m] = sum[1][0][m] = sum[1][1][m] = 0.0;
        for (int q = 0; q < 2 * L; q++) {
            const int r = q >= L ? 1 : 0, lev = q - r * L;
            // digits of the accumulator's polynomial itself at this thread's positions
#pragma unroll
            for (int m = 0; m < PT; m++) {
                const int j = tid + m * L64_THREADS;
                uint32_t state = (uint32_t)((acc[(size_t)r * N + j] + round_off) >> (64 - rep));
                int d = 0;
                for (int lv = L - 1; lv >= lev; lv--) d = g64_decompose_step(state, logB, half_m1);
                buf[j] = (double)d;
                buf[N + j] = (double)d;
            }
            __syncthreads();
            l64_ntt_forward<LOGN>(buf, tw0, tw1);
            // per subset S (one at a time): d^ M(e_S) at this thread's positions, then its products with the key words of
            // GGSW (t, S), polynomial (r, c, lev), for both columns; recentred after every fourth subset
#pragma unroll 1
            for (int S = 0; S < SUB; S++) {
                int eS = 0; // e_S = sum of the members' rotations mod 2N (bit i of S = member i)
#pragma unroll
                for (int i = 0; i < GG; i++) eS += (S >> i) & 1 ? am[i] : 0;
                eS &= 2 * N - 1;
                const double *kS = key + (size_t)S * step_words + ((size_t)(r * 2) * L + lev) * 2 * N;
                const bool fold = (S & 3) == 3;
#pragma unroll
                for (int m = 0; m < PT; m++) {
                    const int s = tid + m * L64_THREADS;
                    double d0 = buf[s], d1 = buf[N + s];
                    if (S) { // (M(0) = 1)
                        const int ex = 2 * (int)(__brev((unsigned)s) >> (32 - LOGN)) + 1; // expo(s): see the head of this file
                        const int at = (ex * eS) & (2 * N - 1);
                        d0 = mulmod<L0>(d0, psi_pow[at]);
                        d1 = mulmod<L1>(d1, psi_pow[2 * N + at]);
                    }
#pragma unroll
                    for (int c = 0; c < 2; c++) {
                        const double *kc = kS + (size_t)c * L * 2 * N;
                        double s0 = sum[c][0][m] + mulmod<L0>(d0, kc[s]), s1 = sum[c][1][m] + mulmod<L1>(d1, kc[N + s]);
                        if (fold) {
                            s0 = reduce<L0>(s0); // <= 0.5 p + 4 x 0.59 p before
                            s1 = reduce<L1>(s1);
                        }
                        sum[c][0][m] = s0;
                        sum[c][1][m] = s1;
                    }
                }
            }
            // (no barrier: the next digits, or the column below, overwrite this thread's own positions only)
        }
#pragma unroll
        for (int c = 0; c < 2; c++) {
#pragma unroll
            for (int m = 0; m < PT; m++) {
                const int s = tid + m * L64_THREADS;
                buf[s] = reduce<L0>(sum[c][0][m]);
                buf[N + s] = reduce<L1>(sum[c][1][m]);
            }
            __syncthreads();
            l64_ntt_inverse<LOGN>(buf, twi0, twi1);
            // CRT lift as above; the lifted value replaces the accumulator
#pragma unroll
            for (int m = 0; m < PT; m++) {
                const int j = tid + m * L64_THREADS;
                const double r0 = buf[j], r1 = buf[N + j];
                const double tq = reduce<L1>(mulmod<L1>(r1 - r0, p0inv_mod_p1));
                HELM_BOUND(__builtin_fabs(r0) < 0x1p51 && __builtin_fabs(tq) < 0x1p51, 4);
                acc[(size_t)c * N + j] = (uint64_t)to_int64(r0) + L0::P_U64 * (uint64_t)to_int64(tq);
            }
        }
        __syncthreads(); // orders the body coefficient for the sample extract (and the next step's digits after the lifts)
    }

    // ---- sample extract: every output of the job (extract_put; pad = 0: the one at coefficient 0) ----------
    const int n_out = pbs64_job_outputs(job.pad), ls = pbs64_job_log_stride(job.pad);
    for (int x = 0; x < n_out; x++) {
        const int h = x << ls;
        uint64_t *ob = out + (size_t)(job.out_row + x) * ((size_t)N + 1);
#pragma unroll
        for (int m = 0; m < PT; m++) {
            const int j = tid + m * L64_THREADS;
            extract_put(ob, N, h, j, acc[j]);
        }
        if (tid == 0) ob[N] = acc[(size_t)N + h]; // body = B[h]
    }
}

// One workgroup per key polynomial: standard-domain u64 coefficients (taken as signed) -> both fields -> forward transform ->
// x N^-1, recentred, bit-reversed order: dst[i][r][c][lev][f][N] (src is [i][lev][r][c][N]).  k_bsk_convert64_generic's
// sibling for the pair (L0, L1) and 1024 threads.
template <int LOGN>
__global__ __launch_bounds__(L64_THREADS) void k_bsk_convert64_large(const uint64_t *__restrict__ src, double *__restrict__ dst,
                                                                     const double *__restrict__ tw0,
                                                                     const double *__restrict__ tw1, double n_inv0,
                                                                     double n_inv1, double two32_0, double two32_1, int K1,
                                                                     int L)
{
    constexpr int N = 1 << LOGN;
    __shared__ double x[2 * N];
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
