// helm_pbs64_generic.inc — the generic blind-rotate kernel of the 64-bit engine (included by helm_shortint.hip, main
// translation unit only).  The tuned builds (k_pbs64, k_pbs64k, k_pbs64s) hard-wire k and pbs_l into wave maps and register
// layouts; this one takes k, pbs_l and pbs_logB at run time and serves every shape of the generic domain a context admits
// under HELM_SI_CREATE_ALLOW_GENERIC (helm_si_ctx_create_ex: N in {256, 512, 1024, 2048}, (k+1) N <= 4096, the two-prime
// capacity bound), and every shape under HELM_SI_CREATE_FORCE_GENERIC.  Same jobs and buffers as launch_pbs64: modulus switch,
// blind rotation with the job's look-up table, sample extract into a row of k N + 1 words.
//
// One workgroup of TP_THREADS per bootstrap; the LDS layout (TwoPrimeLds<uint64_t>), the transforms over both fields, the
// classical product accumulation, the CRT quotient and the key conversion's tail are pbs_twoprime.h's, shared with the
// boolean engine's k_pbs_crt, and so are the description of a CMUX step and the exactness argument.  This engine's own part:
// a step is skipped when the rotation is 0, as in the tuned kernels (its digits are all zero); the digits are tfhe's
// balanced ones (the recurrence of pbs64_body), at most 2^23 < p/2 in magnitude; the true integer coefficient x of the
// external product has |x| <= (k+1) l N 2^(logB-1) 2^63, below p0 p1 / 2 / 1.001 (the capacity check of
// helm_si_ctx_create_ex), so tp_quotient's lift x' = r0 + p0 t is exact, and it is formed mod 2^64 from the two exact int64
// values (to_int64: |r0|, |t| < 2^51).  The torus arithmetic is therefore the exact negacyclic product mod 2^64, as
// in the tuned kernels, whatever the shape.  Unlike those, the generic kernel recentres everywhere (no lazy stage, no
// short-root stage) and so needs no argument tied to a shape.  mulmod and reduce carry ntt_fp64.h's HELM_BOUND checks, and
// the lift checks its to_int64 range (slot 4); the bound-checking build does not run this kernel yet (setup_generic,
// DESIGN.md 4.4.1).
//
// Multi-bit form (template argument GG = grouping factor 2 or 3, HELM_SI_CREATE_GENERIC_MULTIBIT; GG = 0 is the classical
// form above).  Per group t < n / GG of mask words ONE external product, acc <- (sum_S X^(e_S) GGSW_{t,S}) (x) acc with
// e_S = sum_{i in S} a~_i mod 2N over the 2^GG subsets S of the group (tfhe's MultiBitPBS; GGSW index t 2^GG + S, bit i of S
// = member i, same layout per GGSW as above).  The digits are those of the accumulator itself (no rotation, no difference),
// the column sums are  sum_S sum_q (d^_q . M(e_S)) . K^_{t,S}[q][c],  and the lifted value REPLACES the accumulator.  No
// group is skipped, not one whose rotations are all 0: the oracle does not skip either, and at e = 0 the step is not the
// identity on the accumulator's low bits.  M(e)[s] = psi^(expo(s) e) is the spectrum of the monomial X^e: tp_ntt_forward
// leaves at position s the value at psi^(2 rev(s) + 1) (rev: bit reversal over log2 N bits - the Cooley-Tukey recursion
// splits on X^(N/m) = psi^(N/m (2 rev(i) + 1)) at twiddle m + i), so expo(s) = 2 rev(s) + 1 and M(e)[s] is read from the
// context's table of the 2N powers of psi (global memory: 32 N bytes shared in L2, no LDS).
// Exactness of the multi-bit form.  M(e)[s] is a table entry, |M| <= p/2, and d^ is recentred, so d^ M = mulmod(d^, M) is
// below 0.56 p; its product with a key word is below (0.5 + 0.75 x 0.56 p 2^-52) p < 0.57 p (mulmod's bound with
// p 2^-52 < 0.15).  A column sum is recentred after every four products (the 2^GG subsets of one digit polynomial in
// runs of four): <= 0.5 p + 4 x 0.57 p = 2.8 p < 2^53 as there, for any D, (k+1) l and GG.  The true integer coefficient
// is now  x = sum_S sum_q (d_q X^(e_S) K_{t,S}[q][c])  with the key words taken as centred 64-bit integers: congruent mod
// 2^64 to the oracle's (which sums the rotated keys mod 2^64 first), and |x| <= 2^(logB-1) x the largest l1-norm over the
// 2^GG (k+1) l key polynomials of a group that meet in one column.  That is 2^GG times the classical worst case, which the
// creation-time check does not cover: helm_si_load_bootstrap_key computes the bound from the key at hand and refuses a key
// beyond p0 p1 / 2 / 1.001, so the lift is exact for every key a context holds.

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

// bsk: [i][r][c][lev][f][N] in the transform domain (bit-reversed order), times N^-1, recentred (k_bsk_convert64_generic);
// GG > 0 (multi-bit): i = t 2^GG + S, n a multiple of GG, psi_pow the 2N powers of psi per field ([2][2N])
template <int LOGN, int GG = 0>
__global__ __launch_bounds__(TP_THREADS) void k_pbs64_generic(const Pbs64Job *__restrict__ jobs,
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
    const TwoPrimeLds<uint64_t> lay(N, K1, D, n);
    uint64_t *acc = reinterpret_cast<uint64_t *>(smem_g64 + lay.acc);
    double *col = reinterpret_cast<double *>(smem_g64 + lay.col);
    double *dig = reinterpret_cast<double *>(smem_g64 + lay.dig);
    uint16_t *MS = reinterpret_cast<uint16_t *>(smem_g64 + lay.ms);
    const Pbs64Job job = jobs[blockIdx.x];

    // ---- modulus switch --------------------------------------------------------------------
    switch_row(MS, job_row(job, small, n), n, tid, TP_THREADS, LOGN + 1);
    __syncthreads();
    // ---- accumulator: (0, ..., 0, X^{-b~} lut) ---------------------------------------------
    {
        const int bt = (int)MS[n];
        const uint64_t *tv = luts + (size_t)job.lut * N;
        for (int idx = tid; idx < K1 * N; idx += TP_THREADS)
            acc[idx] = idx >= K * N ? lut_rotated(tv, idx - K * N, bt, N) : 0ull;
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
            for (int idx = tid; idx < (cnt << LOGN); idx += TP_THREADS) {
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
            tp_ntt_forward<LOGN>(dig, cnt, dstride, tw0, tw1);
            tp_accumulate<LOGN>(dig, dstride, col, cstride, key, q0, cnt, K1, L);
        }
        tp_ntt_inverse<LOGN>(col, K1, cstride, twi0, twi1);
        // CRT lift of each coefficient's two residues to the exact integer, accumulated mod 2^64
        for (int idx = tid; idx < K1 * N; idx += TP_THREADS) {
            const double r0 = col[idx], r1 = col[cstride + idx];
            const double t = tp_quotient(r0, r1, p0inv_mod_p1);
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
            for (int idx = tid; idx < (cnt << LOGN); idx += TP_THREADS) {
                const int q = q0 + (idx >> LOGN), j = idx & (N - 1);
                const int r = q / L, lev = q - r * L;
                uint32_t state = (uint32_t)((acc[(size_t)r * N + j] + round_off) >> (64 - rep));
                int d = 0;
                for (int lv = L - 1; lv >= lev; lv--) d = g64_decompose_step(state, logB, half_m1);
                dig[idx] = (double)d;
                dig[dstride + idx] = (double)d;
            }
            __syncthreads();
            tp_ntt_forward<LOGN>(dig, cnt, dstride, tw0, tw1);
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
            for (int u = tid; u < 2 * N; u += TP_THREADS) {
                const int s = u & (N - 1); // (the field is uniform over a wave)
                if (u < N) products(F0{}, 0, s);
                else products(F1{}, 1, s);
            }
            __syncthreads(); // the next batch overwrites dig
        }
        tp_ntt_inverse<LOGN>(col, K1, cstride, twi0, twi1);
        // CRT lift as above; the lifted value replaces the accumulator
        for (int idx = tid; idx < K1 * N; idx += TP_THREADS) {
            const double r0 = col[idx], r1 = col[cstride + idx];
            const double tq = tp_quotient(r0, r1, p0inv_mod_p1);
            HELM_BOUND(__builtin_fabs(r0) < 0x1p51 && __builtin_fabs(tq) < 0x1p51, 4);
            acc[idx] = (uint64_t)to_int64(r0) + F0::P_U64 * (uint64_t)to_int64(tq);
        }
        __syncthreads();
    }

    // ---- sample extract: every output of the job (extract_put; pad = 0: the one at coefficient 0) ----------
    const int n_out = pbs64_job_outputs(job.pad), ls = pbs64_job_log_stride(job.pad);
    for (int x = 0; x < n_out; x++)
        sample_extract_lds<LOGN>(big_row(out, job.out_row + x, K, N), acc, K, x << ls, tid, TP_THREADS);
}

// One workgroup per key polynomial: standard-domain u64 coefficients (taken as signed) -> both fields -> tp_convert:
// dst[i][r][c][lev][f][N] (src is [i][lev][r][c][N]).
template <int LOGN>
__global__ __launch_bounds__(TP_THREADS) void k_bsk_convert64_generic(const uint64_t *__restrict__ src, double *__restrict__ dst,
                                                                    const double *__restrict__ tw0,
                                                                    const double *__restrict__ tw1, double n_inv0,
                                                                    double n_inv1, double two32_0, double two32_1, int K1,
                                                                    int L)
{
    constexpr int N = 1 << LOGN;
    __shared__ double x[2 * N];
    auto load = [&](size_t at, double &v0, double &v1) {
        const uint64_t v = src[at];
        // v = hi 2^32 + lo with hi signed: reduce in each field
        const double hi = (double)(int32_t)(uint32_t)(v >> 32), lo = (double)(uint32_t)v;
        v0 = reduce<F0>(mulmod<F0>(hi, two32_0) + lo);
        v1 = reduce<F1>(mulmod<F1>(hi, two32_1) + lo);
    };
    tp_convert<LOGN>(x, load, dst, tw0, tw1, n_inv0, n_inv1, K1, L);
}
