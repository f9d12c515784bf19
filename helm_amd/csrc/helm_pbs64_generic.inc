// helm_pbs64_generic.inc — the generic blind-rotate kernel of the 64-bit engine (included by helm_shortint.hip, main
// translation unit only).  The tuned builds (k_pbs64, k_pbs64k, k_pbs64s) hard-wire k and pbs_l into wave maps and register
// layouts; this one takes k, pbs_l and pbs_logB at run time and serves every shape of the generic domain a context admits
// under HELM_SI_CREATE_ALLOW_GENERIC (helm_si_ctx_create_ex: N in {256, 512, 1024, 2048}, (k+1) N <= 4096, the two-prime
// capacity bound), and every shape under HELM_SI_CREATE_FORCE_GENERIC.  Same jobs and buffers as launch_pbs64: modulus switch,
// blind rotation with the job's look-up table, sample extract into a row of k N + 1 words.
//
// One workgroup of 256 threads per bootstrap.  What a bootstrap works on lives in LDS (Gen64Lds):
//   acc   u64    [k+1][N]      the accumulator GLWE
//   col   double [2][k+1][N]   the k+1 column sums of the external product in both CRT fields, inverse-transformed in place
//   dig   double [2][D][N]     one batch of D digit polynomials in both fields, forward-transformed in place (D N <= 1024,
//                              D <= 4; D = 1 at N = 2048)
//   ms    u16    [n+1]         the modulus-switched input
// At the domain's edge, (k+1) N = 4096: 32 + 64 + 16 (N = 2048: 32) + 2 = 114 (130) KiB of the CU's 160, one workgroup per
// CU.  The twiddle tables of both fields (forward and inverse: 32 N bytes) are read from global memory, where every workgroup
// of the device shares them in L2: in LDS they would not fit beside the rest at N = 2048.
//
// Per CMUX step (skipped when the rotation is 0, as in the tuned kernels: its digits are all zero): for each batch of digit
// polynomials q = r l + lev (polynomial r of X^a acc - acc, level lev, 0 = most significant): decompose (tfhe's balanced
// digits, the recurrence of pbs64_body), forward-transform in both fields (radix-2 Cooley-Tukey, natural order in,
// bit-reversed out), multiply by the key polynomials (r, c, lev) streamed from HBM and add into column c; then
// inverse-transform the 2 (k+1) columns together (Gentleman-Sande, bit-reversed in, natural out; N^-1 is folded into the
// key), lift each coefficient's two residues to the integer mod 2^64 (CRT) and add it into the accumulator.
//
// Exactness.  F0 = FpG (p0 = 2^49.23, 2^53 / p0 = 13.6), F1 = FpG2 (p1 = 2^49.26, 13.4).  Every value a transform stage
// stores is recentred (reduce: |x| <= p/2 + 1), so a butterfly's sum or difference is below 1.1 p and a mulmod of it below
// 0.6 p.  Digits are at most 2^23 < p/2 in magnitude, the same integer in both fields.  A product of a recentred transform
// output with a key word (|w| <= p/2) is below (0.5 + 0.75 (p/2) 2^-52) p = 0.56 p (mulmod's bound); a column sum enters a
// batch recentred and takes at most D <= 4 products: <= 0.5 p + 4 x 0.56 p = 2.8 p < 2^53, and it is recentred at the end of
// every batch - for any (k+1) l.  The inverse transform's outputs are recentred too: r_f = x mod p_f with |r_f| <= p_f/2 + 1,
// where x is the true integer coefficient of the external product, |x| <= (k+1) l N 2^(logB-1) 2^63, below p0 p1 / 2 / 1.001
// (the capacity check of helm_si_ctx_create_ex).  The lift x' = r0 + p0 t with t = (r1 - r0) p0^-1 mod p1 recentred
// (|t| <= p1/2 + 1) is congruent to x mod p0 p1 and |x'| <= p0 p1 / 2 + 1.5 p0 + 1; |x' - x| < p0 p1 then, so x' = x
// exactly, and it is formed mod 2^64 from the two exact int64 values (to_int64: |r0|, |t| < 2^51).  The torus arithmetic
// is therefore the exact negacyclic product mod 2^64, as in the tuned kernels, whatever the shape.  Unlike those, the
// generic kernel recentres everywhere (no lazy stage, no short-root stage) and so needs no argument tied to a shape.
// mulmod and reduce carry ntt_fp64.h's HELM_BOUND checks, and the lift checks its to_int64 range (slot 4); the bound-checking
// build does not run this kernel yet (setup_generic, DESIGN.md 4.4.1).
//
// Multi-bit form (template argument GG = grouping factor 2 or 3, HELM_SI_CREATE_GENERIC_MULTIBIT; GG = 0 is the classical
// form above).  Per group t < n / GG of mask words ONE external product, acc <- (sum_S X^(e_S) GGSW_{t,S}) (x) acc with
// e_S = sum_{i in S} a~_i mod 2N over the 2^GG subsets S of the group (tfhe's MultiBitPBS; GGSW index t 2^GG + S, bit i of S
// = member i, same layout per GGSW as above).  The digits are those of the accumulator itself (no rotation, no difference),
// the column sums are  sum_S sum_q (d^_q . M(e_S)) . K^_{t,S}[q][c],  and the lifted value REPLACES the accumulator.  No
// group is skipped, not one whose rotations are all 0: the oracle does not skip either, and at e = 0 the step is not the
// identity on the accumulator's low bits.  M(e)[s] = psi^(expo(s) e) is the spectrum of the monomial X^e: g64_ntt_forward
// leaves at position s the value at psi^(2 rev(s) + 1) (rev: bit reversal over log2 N bits - the Cooley-Tukey recursion
// splits on X^(N/m) = psi^(N/m (2 rev(i) + 1)) at twiddle m + i), so expo(s) = 2 rev(s) + 1 and M(e)[s] is read from the
// context's table of the 2N powers of psi (global memory: 32 N bytes shared in L2, no LDS).
// Exactness of the multi-bit form.  M(e)[s] is a table entry, |M| <= p/2, and d^ is recentred, so d^ M = mulmod(d^, M) is
// below 0.56 p; its product with a key word is below (0.5 + 0.75 x 0.56 p 2^-52) p < 0.57 p (mulmod's bound with
// p 2^-52 < 0.15).  A column sum is recentred after every four products (the 2^GG subsets of one digit polynomial in
// runs of four): <= 0.5 p + 4 x 0.57 p = 2.8 p < 2^53 as above, for any D, (k+1) l and GG.  The true integer coefficient
// is now  x = sum_S sum_q (d_q X^(e_S) K_{t,S}[q][c])  with the key words taken as centred 64-bit integers: congruent mod
// 2^64 to the oracle's (which sums the rotated keys mod 2^64 first), and |x| <= 2^(logB-1) x the largest l1-norm over the
// 2^GG (k+1) l key polynomials of a group that meet in one column.  That is 2^GG times the classical worst case, which the
// creation-time check does not cover: helm_si_load_bootstrap_key computes the bound from the key at hand and refuses a key
// beyond p0 p1 / 2 / 1.001, so the lift is exact for every key a context holds.

constexpr int G64_THREADS = 256;
constexpr int G64_MAX_D = 4;

// digit polynomials transformed together: at most 4 (the column-sum bound above), D N <= 1024 (one at N = 2048)
static inline int gen64_batch(int N, int k, int l)
{
    int d = std::max(1, 1024 / N);
    d = std::min(d, G64_MAX_D);
    return std::min(d, (k + 1) * l);
}

// one level of tfhe's signed decomposition, least significant first: the digit is what the state loses when B/2 - 1 + (bit
// 2 logB - 1 of the state) is added and logB bits are shifted out (as pbs64_body does).  The state has at most
// logB l <= 31 bits, so the sum stays below 2^32 and the digit, computed mod 2^32, is in [-B/2, B/2].
__device__ __forceinline__ int g64_decompose_step(uint32_t &state, int logB, uint32_t half_m1)
{
    const uint32_t s = state;
    const uint32_t tie = 2 * logB - 1 < 32 ? (s >> (2 * logB - 1)) & 1u : 0u;
    const uint32_t next = (s + half_m1 + tie) >> logB;
    state = next;
    return (int)(s - (next << logB));
}

// LDS layout of k_pbs64_generic (bytes), host and device
struct Gen64Lds {
    size_t acc, col, dig, ms, bytes;
    __host__ __device__ Gen64Lds(int N, int K1, int D, int n)
    {
        acc = 0;
        col = acc + sizeof(uint64_t) * (size_t)K1 * N;
        dig = col + sizeof(double) * 2 * (size_t)K1 * N;
        ms = dig + sizeof(double) * 2 * (size_t)D * N;
        bytes = (ms + sizeof(uint16_t) * ((size_t)n + 1) + 15) / 16 * 16;
    }
};

template <typename F>
__device__ __forceinline__ void g64_fwd_bfly(double *y, int t, double w)
{
    const double U = y[0], V = mulmod<F>(y[t], w);
    y[0] = reduce<F>(U + V);
    y[t] = reduce<F>(U - V);
}

template <typename F>
__device__ __forceinline__ void g64_inv_bfly(double *y, int t, double w)
{
    const double U = y[0], V = y[t];
    y[0] = reduce<F>(U + V);
    y[t] = reduce<F>(mulmod<F>(U - V, w));
}

// cnt polynomials per field, field 0 at x[q N], field 1 at x[fstride + q N]: forward negacyclic transform, natural order in,
// bit-reversed out, inputs |x| < 2^52, outputs recentred.  tw0 / tw1: bit-reversed powers of psi in each field (global
// memory).  Ends with a workgroup barrier.
template <int LOGN>
__device__ __forceinline__ void g64_ntt_forward(double *x, int cnt, int fstride, const double *__restrict__ tw0,
                                                const double *__restrict__ tw1)
{
    constexpr int H = 1 << (LOGN - 1);
    const int per_f = cnt * H;
    for (int s = 0; s < LOGN; s++) {
        const int logt = LOGN - 1 - s, t = 1 << logt, m = 1 << s;
        for (int b = (int)threadIdx.x; b < 2 * per_f; b += G64_THREADS) {
            const int f = b >= per_f ? 1 : 0, r = b - f * per_f; // (per_f is a multiple of 64: f is uniform over a wave)
            const int q = r >> (LOGN - 1), k = r & (H - 1), i = k >> logt;
            double *y = x + (size_t)f * fstride + ((size_t)q << LOGN) + (i << (logt + 1)) + (k & (t - 1));
            if (f == 0) g64_fwd_bfly<F0>(y, t, tw0[m + i]);
            else g64_fwd_bfly<F1>(y, t, tw1[m + i]);
        }
        __syncthreads();
    }
}

// inverse: bit-reversed in, natural out, without the 1/N; twi0 / twi1: bit-reversed powers of psi^-1.  Inputs and outputs
// recentred.  Ends with a workgroup barrier.
template <int LOGN>
__device__ __forceinline__ void g64_ntt_inverse(double *x, int cnt, int fstride, const double *__restrict__ twi0,
                                                const double *__restrict__ twi1)
{
    constexpr int H = 1 << (LOGN - 1);
    const int per_f = cnt * H;
    for (int s = 0; s < LOGN; s++) {
        const int logt = s, t = 1 << logt, h = H >> s;
        for (int b = (int)threadIdx.x; b < 2 * per_f; b += G64_THREADS) {
            const int f = b >= per_f ? 1 : 0, r = b - f * per_f;
            const int q = r >> (LOGN - 1), k = r & (H - 1), i = k >> logt;
            double *y = x + (size_t)f * fstride + ((size_t)q << LOGN) + (i << (logt + 1)) + (k & (t - 1));
            if (f == 0) g64_inv_bfly<F0>(y, t, twi0[h + i]);
            else g64_inv_bfly<F1>(y, t, twi1[h + i]);
        }
        __syncthreads();
    }
}

// bsk: [i][r][c][lev][f][N] in the transform domain (bit-reversed order), times N^-1, recentred (k_bsk_convert64_generic);
// GG > 0 (multi-bit): i = t 2^GG + S, n a multiple of GG, psi_pow the 2N powers of psi per field ([2][2N])
template <int LOGN, int GG = 0>
__global__ __launch_bounds__(G64_THREADS) void k_pbs64_generic(const Pbs64Job *__restrict__ jobs,
                                                            const uint64_t *__restrict__ small, // rows of n+1
                                                            const uint64_t *__restrict__ luts,  // rows of N
                                                            const double *__restrict__ bsk,
                                                            const double *__restrict__ tw0, const double *__restrict__ tw1,
                                                            const double *__restrict__ twi0, const double *__restrict__ twi1,
                                                            const double *__restrict__ psi_pow,
                                                            uint64_t *__restrict__ out, // rows of k*N+1
                                                            int n, int K, int L, int logB, int D, double p0inv_mod_p1)
{
    constexpr int N = 1 << LOGN;
    const int K1 = K + 1, QN = K1 * L, tid = (int)threadIdx.x;
    extern __shared__ __align__(16) unsigned char smem_g64[];
    const Gen64Lds lay(N, K1, D, n);
    uint64_t *acc = reinterpret_cast<uint64_t *>(smem_g64 + lay.acc);
    double *col = reinterpret_cast<double *>(smem_g64 + lay.col);
    double *dig = reinterpret_cast<double *>(smem_g64 + lay.dig);
    uint16_t *MS = reinterpret_cast<uint16_t *>(smem_g64 + lay.ms);
    const Pbs64Job job = jobs[blockIdx.x];

    // ---- modulus switch --------------------------------------------------------------------
    const uint64_t *lwe = small + (size_t)job.in_row * ((size_t)n + 1);
    for (int i = tid; i <= n; i += G64_THREADS) MS[i] = (uint16_t)modswitch64(lwe[i], LOGN + 1);
    __syncthreads();
    // ---- accumulator: (0, ..., 0, X^{-b~} lut) ---------------------------------------------
    {
        const int bt = (int)MS[n];
        const uint64_t *tv = luts + (size_t)job.lut * N;
        for (int idx = tid; idx < K1 * N; idx += G64_THREADS) {
            uint64_t v = 0;
            if (idx >= K * N) {
                const int s = ((idx - K * N) + bt) & (2 * N - 1);
                v = tv[s & (N - 1)];
                if (s >= N) v = 0ull - v;
            }
            acc[idx] = v;
        }
    }
    __syncthreads();

    // ---- blind rotation: acc += BSK_i (x) (X^{a_i} acc - acc) ------------------------------
    const int rep = logB * L; // <= 31
    const uint64_t round_off = 1ull << (63 - rep);
    const uint32_t half_m1 = (1u << (logB - 1)) - 1u;
    const size_t step_words = (size_t)K1 * K1 * L * 2 * N; // key words of one GGSW (classical: of one LWE coefficient)
    const int cstride = K1 * N, dstride = D * N;           // field 1's columns / digits
    if constexpr (GG == 0) // (classical form; the multi-bit form is the else branch below)
    for (int i = 0; i < n; i++) {
        const int a = (int)MS[i];
        if (a == 0) continue; // uniform over the workgroup
        const double *key = bsk + (size_t)i * step_words;
        for (int q0 = 0; q0 < QN; q0 += D) {
            const int cnt = QN - q0 < D ? QN - q0 : D;
            // digits of polynomials q0 .. q0 + cnt - 1, the same integers in both fields
            for (int idx = tid; idx < (cnt << LOGN); idx += G64_THREADS) {
                const int q = q0 + (idx >> LOGN), j = idx & (N - 1);
                const int r = q / L, lev = q - r * L;
                const uint64_t *ar = acc + (size_t)r * N;
                const int s = (j - a) & (2 * N - 1); // (X^a acc_r)[j] = +-acc_r[j - a]
                const uint64_t rot = s < N ? ar[s] : 0ull - ar[s - N];
                uint32_t state = (uint32_t)((rot - ar[j] + round_off) >> (64 - rep));
                // digit lev is the (L - lev)-th the recurrence yields (least significant level first): the levels below it
                // are recomputed for every digit polynomial - O(l^2) integer steps per coefficient, against the transforms'
                // O(log N) modular ones
                int d = 0;
                for (int lv = L - 1; lv >= lev; lv--) d = g64_decompose_step(state, logB, half_m1);
                dig[idx] = (double)d;
                dig[dstride + idx] = (double)d;
            }
            __syncthreads();
            g64_ntt_forward<LOGN>(dig, cnt, dstride, tw0, tw1);
            // products into the column sums: thread slot u = (field, coefficient s) owns that coefficient of every column
            // (no LDS hazard between threads until the inverse transform's barrier).  Key polynomial (r, c, lev) of digit
            // q = r l + lev in field f starts at (((r (k+1) + c) l + lev) 2 + f) N = koff[q] + (c l 2 + f) N.
            size_t koff[G64_MAX_D];
#pragma unroll
            for (int ql = 0; ql < G64_MAX_D; ql++) {
                const int q = q0 + ql, r = q / L, lev = q - r * L;
                koff[ql] = ((size_t)r * K1 * L + lev) * 2 * N;
            }
            for (int u = tid; u < 2 * N; u += G64_THREADS) {
                const int f = u >= N ? 1 : 0, s = u & (N - 1); // (f is uniform over a wave)
                const double *dg = dig + (size_t)f * dstride + s;
                for (int c = 0; c < K1; c++) {
                    const double *kc = key + ((size_t)c * L * 2 + f) * N + s;
                    double *cs = col + (size_t)f * cstride + (size_t)c * N + s;
                    double sum = q0 == 0 ? 0.0 : *cs;
                    if (f == 0) {
#pragma unroll
                        for (int ql = 0; ql < G64_MAX_D; ql++)
                            if (ql < cnt) sum += mulmod<F0>(dg[ql << LOGN], kc[koff[ql]]);
                        *cs = reduce<F0>(sum); // <= 0.5 p + D x 0.56 p before (see the head of this file)
                    } else {
#pragma unroll
                        for (int ql = 0; ql < G64_MAX_D; ql++)
                            if (ql < cnt) sum += mulmod<F1>(dg[ql << LOGN], kc[koff[ql]]);
                        *cs = reduce<F1>(sum);
                    }
                }
            }
            __syncthreads(); // the next batch overwrites dig
        }
        g64_ntt_inverse<LOGN>(col, K1, cstride, twi0, twi1);
        // CRT lift of each coefficient's two residues to the exact integer, accumulated mod 2^64
        for (int idx = tid; idx < K1 * N; idx += G64_THREADS) {
            const double r0 = col[idx], r1 = col[cstride + idx];
            const double t = reduce<F1>(mulmod<F1>(r1 - r0, p0inv_mod_p1));
            HELM_BOUND(__builtin_fabs(r0) < 0x1p51 && __builtin_fabs(t) < 0x1p51, 4);
            acc[idx] += (uint64_t)to_int64(r0) + F0::P_U64 * (uint64_t)to_int64(t);
        }
        __syncthreads();
    }
    // ---- multi-bit blind rotation: acc <- (sum_S X^(e_S) BSK_{t,S}) (x) acc ------------------
    else
    for (int t = 0; t < n / GG; t++) {
        constexpr int SUB = 1 << GG;
        int e[SUB]; // e_S, uniform over the workgroup: e_S = e_(S without its lowest member) + a~ of that member
        e[0] = 0;
#pragma unroll
        for (int S = 1; S < SUB; S++) e[S] = (e[S & (S - 1)] + (int)MS[t * GG + __builtin_ctz(S)]) & (2 * N - 1);
        const double *key = bsk + (size_t)t * SUB * step_words;
        for (int q0 = 0; q0 < QN; q0 += D) {
            const int cnt = QN - q0 < D ? QN - q0 : D;
            // digits of the accumulator's polynomials themselves
            for (int idx = tid; idx < (cnt << LOGN); idx += G64_THREADS) {
                const int q = q0 + (idx >> LOGN), j = idx & (N - 1);
                const int r = q / L, lev = q - r * L;
                uint32_t state = (uint32_t)((acc[(size_t)r * N + j] + round_off) >> (64 - rep));
                int d = 0;
                for (int lv = L - 1; lv >= lev; lv--) d = g64_decompose_step(state, logB, half_m1);
                dig[idx] = (double)d;
                dig[dstride + idx] = (double)d;
            }
            __syncthreads();
            g64_ntt_forward<LOGN>(dig, cnt, dstride, tw0, tw1);
            // thread slot u = (field, coefficient s) as in the classical form; per digit polynomial the 2^GG products
            // d^ M(e_S) once, then per column their products with the subsets' key words, recentred every four
            auto products = [&](auto field, int f, int s) {
                using F = decltype(field);
                const int ex = 2 * (int)(__brev((unsigned)s) >> (32 - LOGN)) + 1; // expo(s): see the head of this file
                const double *pw = psi_pow + (size_t)f * 2 * N;
                double m[SUB];
#pragma unroll
                for (int S = 1; S < SUB; S++) m[S] = pw[(ex * e[S]) & (2 * N - 1)];
                const double *dg = dig + (size_t)f * dstride + s;
                for (int ql = 0; ql < cnt; ql++) {
                    const int q = q0 + ql, r = q / L, lev = q - r * L;
                    double dm[SUB];
                    dm[0] = dg[ql << LOGN]; // M(0) = 1
#pragma unroll
                    for (int S = 1; S < SUB; S++) dm[S] = mulmod<F>(dm[0], m[S]);
                    const double *kq = key + (((size_t)r * K1 * L + lev) * 2 + f) * N + s;
                    for (int c = 0; c < K1; c++) {
                        const double *kc = kq + (size_t)c * L * 2 * N;
                        double *cs = col + (size_t)f * cstride + (size_t)c * N + s;
                        double sum = q == 0 ? 0.0 : *cs;
#pragma unroll
                        for (int S = 0; S < SUB; S++) {
                            sum += mulmod<F>(dm[S], kc[(size_t)S * step_words]);
                            if ((S & 3) == 3) sum = reduce<F>(sum); // <= 0.5 p + 4 x 0.57 p before
                        }
                        *cs = sum;
                    }
                }
            };
            for (int u = tid; u < 2 * N; u += G64_THREADS) {
                const int s = u & (N - 1); // (the field is uniform over a wave)
                if (u < N) products(F0{}, 0, s);
                else products(F1{}, 1, s);
            }
            __syncthreads(); // the next batch overwrites dig
        }
        g64_ntt_inverse<LOGN>(col, K1, cstride, twi0, twi1);
        // CRT lift as above; the lifted value replaces the accumulator
        for (int idx = tid; idx < K1 * N; idx += G64_THREADS) {
            const double r0 = col[idx], r1 = col[cstride + idx];
            const double tq = reduce<F1>(mulmod<F1>(r1 - r0, p0inv_mod_p1));
            HELM_BOUND(__builtin_fabs(r0) < 0x1p51 && __builtin_fabs(tq) < 0x1p51, 4);
            acc[idx] = (uint64_t)to_int64(r0) + F0::P_U64 * (uint64_t)to_int64(tq);
        }
        __syncthreads();
    }

    // ---- sample extract: every output of the job (extract_put; pad = 0: the one at coefficient 0) ----------
    const int n_out = pbs64_job_outputs(job.pad), ls = pbs64_job_log_stride(job.pad);
    for (int x = 0; x < n_out; x++) {
        const int h = x << ls;
        uint64_t *ob = out + (size_t)(job.out_row + x) * ((size_t)K * N + 1);
        for (int idx = tid; idx < K * N; idx += G64_THREADS) {
            const int r = idx >> LOGN, j = idx & (N - 1);
            extract_put(ob + (size_t)r * N, N, h, j, acc[idx]);
        }
        if (tid == 0) ob[(size_t)K * N] = acc[(size_t)K * N + h]; // body = B[h]
    }
}

// One workgroup per key polynomial: standard-domain u64 coefficients (taken as signed) -> both fields -> forward transform ->
// x N^-1, recentred, bit-reversed order: dst[i][r][c][lev][f][N] (src is [i][lev][r][c][N]).
template <int LOGN>
__global__ __launch_bounds__(G64_THREADS) void k_bsk_convert64_generic(const uint64_t *__restrict__ src, double *__restrict__ dst,
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
    for (int j = (int)threadIdx.x; j < N; j += G64_THREADS) {
        const uint64_t v = src[poly * N + j];
        // v = hi 2^32 + lo with hi signed: reduce in each field
        const double hi = (double)(int32_t)(uint32_t)(v >> 32), lo = (double)(uint32_t)v;
        x[j] = reduce<F0>(mulmod<F0>(hi, two32_0) + lo);
        x[N + j] = reduce<F1>(mulmod<F1>(hi, two32_1) + lo);
    }
    __syncthreads();
    g64_ntt_forward<LOGN>(x, 1, N, tw0, tw1);
    double *d = dst + ((((i * K1 + r) * K1 + c) * L + lev) * 2) * N;
    for (int j = (int)threadIdx.x; j < N; j += G64_THREADS) {
        d[j] = reduce<F0>(mulmod<F0>(x[j], n_inv0));
        d[N + j] = reduce<F1>(mulmod<F1>(x[N + j], n_inv1));
    }
}
