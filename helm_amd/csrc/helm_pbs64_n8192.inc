// helm_pbs64_n8192.inc — the N = 8192 blind-rotate kernel of the 64-bit engine (included by helm_shortint.hip after
// helm_pbs64_large_core.inc and helm_pbs64_large.inc, main translation unit only).  k = 1, N = 8192: the shape of the 6-bit
// shortint sets (message_modulus * carry_modulus = 64), admitted by helm_si_ctx_create_ex under HELM_SI_CREATE_N8192.  pbs_l,
// pbs_logB and n come at run time.  Same jobs, buffers and epilogue as k_pbs64_large: modulus switch (to 2N = 16384: the u16
// `ms` array holds it), classical blind rotation with the job's look-up table, sample extract (many-LUT: extracts at 0, N/M,
// 2N/M, ...) into rows of N + 1 words.  The pair, the transforms, the pieces of a step and the exactness argument are those
// of helm_pbs64_large_core.inc.
//
// Why it is its own kernel.  k_pbs64_large one size up would hold 128 KiB of accumulator and 128 KiB of transform buffer in
// LDS (a CU has 160), and its 32 column sums per thread (2 columns x 2 fields x 8 positions) spill.  Here:
//   * the accumulator GLWE lives in a row of GLOBAL memory per workgroup, [2][N] u64 = 128 KiB (it stays in L2; within a
//     polynomial the coefficients are in the order of n8192_slot, a thread's eight side by side: N8192RowAcc): row
//     blockIdx.x of a buffer of the launching context (helm_si_ctx::d_acc8192), so a launch has at most as many workgroups
//     as the buffer has rows - launch_pbs64_n8192 cuts wider batches into chunks;
//   * the columns of the external product are computed ONE AFTER THE OTHER: for column c all 2 l digit polynomials go
//     forward and are multiplied by column c's key words only, so a thread holds 1 column x 2 fields x 8 = 16 sums, the
//     register footprint of k_pbs64_large.  The forward transforms are repeated per column: 4 l + 2 transforms per step
//     instead of 2 l + 2.
// LDS (N8192Lds):
//   buf   double [2][N]    ONE transform buffer, both fields                                           128 KiB
//   ms    u16    [n+1]     the modulus-switched input                                                  <= 2 KiB
// 130 KiB of the CU's 160: one workgroup of 1024 threads per CU.  Thread `tid` owns the PT = 8 positions tid + 1024 m of each
// field of buf and of each polynomial of the accumulator row.
//
// Per CMUX step (skipped when the rotation is 0, uniformly over the workgroup):
//   1. each thread reads the accumulator row at its own and at the rotated positions (other threads' positions), once per
//      GLWE polynomial, and keeps the rounded, shifted difference X^a acc_r - acc_r as the decomposition's start state: 2 x 8
//      u32.  These are the only reads of other threads' positions, and they happen before anything of this step is written;
//      both columns form their digits from these states, so column 1 sees the accumulator as it was before column 0's
//      product was added.
//   2. per column c, per polynomial r, per level in the order the digit recurrence yields them (least significant first, one
//      running state per position; the sums commute, only the key polynomial (r, c, lev) has to match): digits into buf, the
//      same integers in both fields; forward transform; products with the key words of (r, c, lev) added to the 16 sums,
//      recentred after every fourth product.  Then l64_column_back: the coefficient is added to the accumulator row at the
//      thread's OWN positions.
// Barriers and what they order (__syncthreads() makes a workgroup's global stores visible to the workgroup):
//   (A) the one after the first digits of a step (it stands before every forward transform): every thread's rotated reads
//       of step 1 are done before any thread passes it, and the first accumulator write of the step comes after it;
//   (B) the one that ends a step: the step's accumulator writes before the next step's rotated reads, and before the sample
//       extract's read of the body coefficient;
//   (C) the one after the accumulator is set up: before the first step's rotated reads.
//
// Capacity at this N: |x| <= (k+1) l N 2^(logB-1) 2^63 = l 2^(76+logB), which helm_si_ctx_create_ex holds below
// p0 p1 / 2 / 1.001 = 2^97.87 / 1.001: (l, logB) = (1, 21) is at 0.547 of p0 p1 / 2, (1, 22) is refused; tfhe's (2, 15) is at
// 2^92 (tests/test_n8192_bounds.py).
//
// Multi-bit form (GG = 2 or 3), the columns one after the other as above.  The start states (acc + round_off) >> (64 - rep)
// are taken at the thread's own eight positions before column 0's lift replaces polynomial 0 - a multi-bit step reads no
// other thread's position.  Per column, polynomial and level: digits, forward transform, then per subset S, ONE AT A TIME
// (the loop is rolled: the 2^GG table values and products are never live together), l64_subset_term.  The barriers stand
// where they stood; (B) still orders the body coefficient for the sample extract.

// bsk: [i][r][c][lev][f][N] in the transform domain (bit-reversed order), times N^-1, recentred (k_bsk_convert64_large<13>)
// acc_rows: rows of 2N words, one per workgroup of the launch (gridDim.x rows at least)
// GG > 0 (multi-bit): i = t 2^GG + S, n a multiple of GG, psi_pow the 2N powers of psi per field ([2][2N])
template <int GG = 0>
__global__ __launch_bounds__(L64_THREADS) void k_pbs64_n8192(const Pbs64Job *__restrict__ jobs,
                                                             const uint64_t *__restrict__ small, // rows of n+1
                                                             const uint64_t *__restrict__ luts,  // rows of N
                                                             const double *__restrict__ bsk,
                                                             const double *__restrict__ tw0, const double *__restrict__ tw1,
                                                             const double *__restrict__ twi0, const double *__restrict__ twi1,
                                                             const double *__restrict__ psi_pow,
                                                             uint64_t *__restrict__ out, // rows of N+1
                                                             uint64_t *acc_rows, int n, int L, int logB, double p0inv_mod_p1)
{
    constexpr int LOGN = N8192_LOGN, N = 1 << LOGN, PT = L64_PT<LOGN>;
    static_assert(PT == 8, "eight positions per thread");
    const int tid = (int)threadIdx.x;
    extern __shared__ __align__(16) unsigned char smem_n8192[];
    const N8192Lds lay(n);
    double *buf = reinterpret_cast<double *>(smem_n8192 + lay.buf);
    uint16_t *MS = reinterpret_cast<uint16_t *>(smem_n8192 + lay.ms);
    const N8192RowAcc acc{acc_rows + (size_t)blockIdx.x * 2 * N, (unsigned)tid << 3};
    const Pbs64Job job = jobs[blockIdx.x];

    l64_prologue<LOGN>(acc, MS, job, small, luts, n);
    __syncthreads(); // (C)

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
        // the decomposition's start states of both polynomials, from the accumulator before this step touches it
        uint32_t init[2][PT];
#pragma unroll
        for (int r = 0; r < 2; r++) {
#pragma unroll
            for (int m = 0; m < PT; m++) {
                const int j = tid + m * L64_THREADS;
                const int s = (j - a) & (2 * N - 1); // (X^a acc_r)[j] = +-acc_r[j - a]
                const uint64_t w = acc.at(r, s & (N - 1));
                const uint64_t rot = s < N ? w : 0ull - w;
                init[r][m] = (uint32_t)((rot - acc.own(r, m) + round_off) >> (64 - rep));
            }
        }
#pragma unroll 1
        for (int c = 0; c < 2; c++) {
            double sum[2][PT]; // [field][position]: registers (every index below is a compile-time constant)
#pragma unroll
            for (int m = 0; m < PT; m++) sum[0][m] = sum[1][m] = 0.0;
            int products = 0;
#pragma unroll
            for (int r = 0; r < 2; r++) {
                uint32_t state[PT];
#pragma unroll
                for (int m = 0; m < PT; m++) state[m] = init[r][m];
                // levels in recurrence order: the least significant level (lev = L - 1) first
                for (int lev = L - 1; lev >= 0; lev--) {
#pragma unroll
                    for (int m = 0; m < PT; m++) {
                        const int j = tid + m * L64_THREADS;
                        const double d = (double)g64_decompose_step(state[m], logB, half_m1);
                        buf[j] = d;
                        buf[N + j] = d;
                    }
                    __syncthreads(); // (A)
                    l64_ntt_forward<LOGN>(buf, tw0, tw1);
                    // key polynomial (r, c, lev) in field f starts at (((r 2 + c) l + lev) 2 + f) N
                    const bool fold = (products & 3) == 3; // recentre after every fourth product (see the head of the core)
                    products++;
                    l64_products<LOGN>(sum, buf, key + (((size_t)(r * 2 + c) * L + lev) * 2) * N, false, fold);
                    // (no barrier: the next digits, or the column below, overwrite this thread's own positions only)
                }
            }
            l64_column_back<LOGN, false>(acc, c, buf, sum, twi0, twi1, p0inv_mod_p1);
        }
        __syncthreads(); // (B)
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
        // the decomposition's start states of polynomial 0 at own positions, before column 0's lift replaces it (polynomial
        // 1 is replaced by column 1's lift, after its last use: its states are read from the row again per column)
        uint32_t init0[PT];
#pragma unroll
        for (int m = 0; m < PT; m++) init0[m] = (uint32_t)((acc.own(0, m) + round_off) >> (64 - rep));
#pragma unroll 1
        for (int c = 0; c < 2; c++) {
            double sum[1][2][PT]; // [the one column][field][position]: registers (every index is a compile-time constant)
#pragma unroll
            for (int m = 0; m < PT; m++) sum[0][0][m] = sum[0][1][m] = 0.0;
#pragma unroll
            for (int r = 0; r < 2; r++) {
                uint32_t state[PT];
#pragma unroll
                for (int m = 0; m < PT; m++)
                    state[m] = r == 0 ? init0[m] : (uint32_t)((acc.own(1, m) + round_off) >> (64 - rep));
                // levels in recurrence order: the least significant level (lev = L - 1) first
                for (int lev = L - 1; lev >= 0; lev--) {
#pragma unroll
                    for (int m = 0; m < PT; m++) {
                        const int j = tid + m * L64_THREADS;
                        const double d = (double)g64_decompose_step(state[m], logB, half_m1);
                        buf[j] = d;
                        buf[N + j] = d;
                    }
                    __syncthreads(); // (A)
                    l64_ntt_forward<LOGN>(buf, tw0, tw1);
                    // per subset S, one at a time: the key word of GGSW (t, S), polynomial (r, c, lev)
                    const double *kq = key + (((size_t)(r * 2 + c) * L + lev) * 2) * N;
#pragma unroll 1
                    for (int S = 0; S < SUB; S++) {
                        // (the transformed digits are read from buf again per subset: hoisted out of this loop, their 16
                        // values would stay live beside the sums)
                        asm volatile("" ::: "memory");
                        l64_subset_term<LOGN, GG>(sum, buf, kq + (size_t)S * step_words, 0, psi_pow, am, S);
                    }
                    // (no barrier: the next digits, or the column below, overwrite this thread's own positions only)
                }
            }
            l64_column_back<LOGN, true>(acc, c, buf, sum[0], twi0, twi1, p0inv_mod_p1);
        }
        __syncthreads(); // (B)
    }

    l64_sample_extract<LOGN>(acc, job, out);
}
