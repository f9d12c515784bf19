// helm_pbs64_large.inc — the large-N blind-rotate kernel of the 64-bit engine (included by helm_shortint.hip after
// helm_pbs64_large_core.inc, main translation unit only).  k = 1, N = 4096: the shape of the 5-bit shortint sets
// (message_modulus * carry_modulus = 32), admitted by helm_si_ctx_create_ex under HELM_SI_CREATE_LARGE_N.  pbs_l, pbs_logB and
// n come at run time.  Same jobs and buffers as k_pbs64_generic: modulus switch, classical blind rotation with the job's
// look-up table, sample extract (many-LUT: extracts at 0, N/M, 2N/M, ...) into rows of N + 1 words.  The pair, the
// transforms, the pieces of a step and the exactness argument are those of helm_pbs64_large_core.inc.
//
// Why it is its own kernel.  (1) The field: the generic kernel's FpG2 holds no 8192-th root of unity (the core's head).
// (2) LDS: TwoPrimeLds<uint64_t> at k = 1, N = 4096 would be 64 (acc) + 128 (col, both fields) + 64 (dig) KiB.  (3) One
// workgroup per CU is all that fits, so the workgroup is wide.
//
// LDS (Large64Lds):
//   acc   u64    [2][N]    the accumulator GLWE                                                      64 KiB
//   buf   double [2][N]    ONE transform buffer, both fields: a digit polynomial going forward,
//                          then a column of the external product going back                          64 KiB
//   ms    u16    [n+1]     the modulus-switched input                                                <= 2 KiB
// 130 KiB of the CU's 160: one workgroup per CU.  Thread `tid` owns the PT = 4 positions tid + 1024 m of each field of buf:
// it writes the digits there, multiplies the spectrum there, and lifts the coefficients there - so the only barriers are
// those of the transforms' stages, one before a transform (the stages read other threads' positions) and one after a step's
// last lift (the next step's digits read the accumulator at rotated positions).
//
// Per CMUX step (skipped when the rotation is 0): for each digit polynomial q = r l + lev of X^a acc - acc (r < 2, level 0 =
// most significant; the digit recurrence of k_pbs64_generic): digits into buf, the same integers in both fields; forward
// transform in both fields; each thread multiplies its 4 positions per field by the key words of BOTH columns (streamed from
// HBM / L2) and keeps the 2 columns x 2 fields x 4 = 16 column sums in registers (at PT = 8 they would spill: k_pbs64_n8192).
// After the last digit polynomial, per column: l64_column_back.  Twiddles come from global memory (4 tables of 32 KiB, shared
// by every workgroup in L2).
//
// Capacity at this N: |x| <= (k+1) l N 2^(logB-1) 2^63 = l 2^(75+logB): (l, logB) = (1, 22) is at 0.547 of p0 p1 / 2,
// (1, 23) is refused (tests/test_large_n_bounds.py).
//
// Multi-bit form (GG = 2 or 3): all 2 l digit polynomials go forward once, the 16 sums stay in registers, both columns are
// lifted after the last digit polynomial; the barriers stand where they stood (a step reads the accumulator at own positions
// only; the one that ends a step still orders the body coefficient for the sample extract).

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
    constexpr int N = 1 << LOGN, PT = L64_PT<LOGN>;
    static_assert(PT >= 1 && N % L64_THREADS == 0, "whole positions per thread");
    const int tid = (int)threadIdx.x;
    extern __shared__ __align__(16) unsigned char smem_l64[];
    const Large64Lds lay(N, n);
    const L64LdsAcc<LOGN> acc{reinterpret_cast<uint64_t *>(smem_l64 + lay.acc)};
    double *buf = reinterpret_cast<double *>(smem_l64 + lay.buf);
    uint16_t *MS = reinterpret_cast<uint16_t *>(smem_l64 + lay.ms);
    const Pbs64Job job = jobs[blockIdx.x];

    l64_prologue<LOGN>(acc, MS, job, small, luts, n);
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
#pragma unroll
            for (int m = 0; m < PT; m++) {
                const int j = tid + m * L64_THREADS;
                const int s = (j - a) & (2 * N - 1); // (X^a acc_r)[j] = +-acc_r[j - a]
                const uint64_t rot = s < N ? acc.at(r, s) : 0ull - acc.at(r, s - N);
                uint32_t state = (uint32_t)((rot - acc.own(r, m) + round_off) >> (64 - rep));
                int d = 0; // digit lev is the (L - lev)-th the recurrence yields (least significant level first)
                for (int lv = L - 1; lv >= lev; lv--) d = g64_decompose_step(state, logB, half_m1);
                buf[j] = (double)d;
                buf[N + j] = (double)d;
            }
            __syncthreads();
            l64_ntt_forward<LOGN>(buf, tw0, tw1);
            // key polynomial (r, c, lev) in field f starts at (((r 2 + c) l + lev) 2 + f) N
            const bool fold = (q & 3) == 3; // recentre after every fourth product (see the head of the core)
#pragma unroll
            for (int c = 0; c < 2; c++)
                l64_products<LOGN>(sum[c], buf, key + (((size_t)(r * 2 + c) * L + lev) * 2) * N, q == 0, fold);
            // (no barrier: the next digits, or the column below, overwrite this thread's own positions only)
        }
#pragma unroll
        for (int c = 0; c < 2; c++) l64_column_back<LOGN, false>(acc, c, buf, sum[c], twi0, twi1, p0inv_mod_p1);
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
                uint32_t state = (uint32_t)((acc.own(r, m) + round_off) >> (64 - rep));
                int d = 0;
                for (int lv = L - 1; lv >= lev; lv--) d = g64_decompose_step(state, logB, half_m1);
                buf[j] = (double)d;
                buf[N + j] = (double)d;
            }
            __syncthreads();
            l64_ntt_forward<LOGN>(buf, tw0, tw1);
            // per subset S (one at a time), for both columns: the key words of GGSW (t, S), polynomial (r, c, lev)
#pragma unroll 1
            for (int S = 0; S < SUB; S++) {
                const double *kS = key + (size_t)S * step_words + ((size_t)(r * 2) * L + lev) * 2 * N;
                l64_subset_term<LOGN, GG>(sum, buf, kS, (size_t)L * 2 * N, psi_pow, am, S);
            }
            // (no barrier: the next digits, or the column below, overwrite this thread's own positions only)
        }
#pragma unroll
        for (int c = 0; c < 2; c++) l64_column_back<LOGN, true>(acc, c, buf, sum[c], twi0, twi1, p0inv_mod_p1);
        __syncthreads(); // orders the body coefficient for the sample extract (and the next step's digits after the lifts)
    }

    l64_sample_extract<LOGN>(acc, job, out);
}
