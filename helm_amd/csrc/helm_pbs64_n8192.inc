// helm_pbs64_n8192.inc — the N = 8192 blind-rotate kernel of the 64-bit engine (included by helm_shortint.hip after
// helm_pbs64_large.inc, main translation unit only).  k = 1, N = 8192: the shape of the 6-bit shortint sets
// (message_modulus * carry_modulus = 64), admitted by helm_si_ctx_create_ex under HELM_SI_CREATE_N8192.  pbs_l, pbs_logB and n
// come at run time.  Same jobs, buffers and epilogue as k_pbs64_large: modulus switch (to 2N = 16384: the u16 `ms` array
// holds it), classical blind rotation with the job's look-up table, sample extract (many-LUT: extracts at 0, N/M, 2N/M, ...)
// into rows of N + 1 words.  Same pair L0 = FpG, L1 = FpI (2^16 | FpG - 1, 2^24 | FpI - 1: both hold 16384-th roots of
// unity), the same radix-2 transforms and butterflies (n8192_ntt_forward / n8192_ntt_inverse below), the same all-recentred
// arithmetic.
//
// Why it is its own kernel.  k_pbs64_large one size up would hold 128 KiB of accumulator and 128 KiB of transform buffer in
// LDS (a CU has 160), and its 32 column sums per thread (2 columns x 2 fields x 8 positions) spill.  Here:
//   * the accumulator GLWE lives in a row of GLOBAL memory per workgroup, [2][N] u64 = 128 KiB (it stays in L2; within a
//     polynomial the coefficients are in the order of n8192_slot, a thread's eight side by side): row
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
//      recentred after every fourth product.  Then the sums go back into buf, recentred; inverse transform; CRT lift; the
//      coefficient is added to the accumulator row at the thread's OWN positions.
// Barriers and what they order (__syncthreads() makes a workgroup's global stores visible to the workgroup):
//   (A) the one after the first digits of a step (it stands before every forward transform): every thread's rotated reads
//       of step 1 are done before any thread passes it, and the first accumulator write of the step comes after it;
//   (B) the one that ends a step: the step's accumulator writes before the next step's rotated reads, and before the sample
//       extract's read of the body coefficient;
//   (C) the one after the accumulator is set up: before the first step's rotated reads.
//
// Exactness.  The argument at the head of helm_pbs64_large.inc does not depend on N: every value a transform stage stores is
// recentred (|x| <= p/2 + 1), a product with a table or key word is below 0.58 p, a forward butterfly below 1.08 p, an inverse
// butterfly's product below 0.65 p, digits are at most 2^23 in magnitude, and a column sum takes at most FOUR products between
// two recentrings: <= 0.5 p + 4 x 0.58 p = 2.82 p < 10.28 p = 2^53 in the tighter field, for any l.  What depends on N is the
// capacity: the true integer coefficient of the external product is |x| <= (k+1) l N 2^(logB-1) 2^63 = l 2^(76+logB), which
// helm_si_ctx_create_ex holds below p0 p1 / 2 / 1.001 = 2^97.87 / 1.001 with this pair's product: (l, logB) = (1, 21) is at
// 0.547 of p0 p1 / 2, (1, 22) is refused; tfhe's (2, 15) is at 2^92.  The lift then returns x exactly, as there
// (tests/test_n8192_bounds.py restates these numbers with exact fractions).
//
// Multi-bit form (template argument GG = grouping factor 2 or 3, HELM_SI_CREATE_LARGE_MULTIBIT; GG = 0 is the classical form
// above).  The algorithm is the one at the head of helm_pbs64_generic.inc, in this kernel's form (a), the columns one after
// the other: per group t < n / GG ONE external product, acc <- (sum_S X^(e_S) GGSW_{t,S}) (x) acc, e_S = sum_{i in S} a~_i
// mod 2N (the members' rotations live in scalar registers).  The start states (acc + round_off) >> (64 - rep) are taken at
// the thread's own eight positions before column 0's lift replaces polynomial 0 - a multi-bit step reads no other thread's
// position.  Per column, polynomial and level: digits, forward transform, then per subset S, ONE AT A TIME (the loop is
// rolled: the 2^GG table values and products are never live together), d^ M(e_S) and its product with the key word of GGSW
// (t, S), recentred after every fourth subset.  M(e)[s] = psi^((2 rev(s) + 1) e) is read per use from the context's table of
// the 2N powers of psi per field ([2][2N] doubles in global memory).  The lifted value REPLACES the accumulator row's word.  No
// group is skipped, not one whose rotations are all 0.  The barriers stand where they stood; (B) still orders the body
// coefficient for the sample extract.
// Exactness of the multi-bit form, for p1: d^ M is below 0.58 p, its product with a key word below (0.5 + 0.75 x 0.58 p
// 2^-52) p < 0.59 p, four of them on a recentred sum <= 0.5 p + 4 x 0.59 p < 2.9 p < 2^53 = 10.28 p; the true coefficient is
// bounded by helm_si_load_bootstrap_key's group-sum rule for the key at hand with this pair's product, so the recentred lift
// is exact (tests/test_large_multibit_bounds.py).

constexpr int N8192_LOGN = 13;

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

// Where coefficient j of a polynomial lies in its N words of an accumulator row: thread j mod 1024 owns it, and a thread's
// eight coefficients lie side by side, so that its own accesses are one address and constant offsets (with the natural
// order they were sixteen 64-bit addresses per thread, which the compiler kept in registers over the whole rotation).
__device__ __forceinline__ unsigned n8192_slot(int j) { return (((unsigned)j & (L64_THREADS - 1)) << 3) | ((unsigned)j >> 10); }

// l64_ntt_forward / l64_ntt_inverse at LOGN = 13, one field after the other within a stage: a thread's four butterflies of a
// field are in flight together, not all eight of the stage (fewer registers live beside the sums and the states)
__device__ __forceinline__ void n8192_ntt_forward(double *x, const double *__restrict__ tw0, const double *__restrict__ tw1)
{
    constexpr int LOGN = N8192_LOGN, N = 1 << LOGN, H = N / 2;
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

__device__ __forceinline__ void n8192_ntt_inverse(double *x, const double *__restrict__ twi0, const double *__restrict__ twi1)
{
    constexpr int LOGN = N8192_LOGN, N = 1 << LOGN, H = N / 2;
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

// bsk: [i][r][c][lev][f][N] in the transform domain (bit-reversed order), times N^-1, recentred (k_bsk_convert64_n8192)
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
    constexpr int LOGN = N8192_LOGN, N = 1 << LOGN, PT = N / L64_THREADS;
    static_assert(PT == 8, "eight positions per thread");
    const int tid = (int)threadIdx.x;
    extern __shared__ __align__(16) unsigned char smem_n8192[];
    const N8192Lds lay(n);
    double *buf = reinterpret_cast<double *>(smem_n8192 + lay.buf);
    uint16_t *MS = reinterpret_cast<uint16_t *>(smem_n8192 + lay.ms);
    uint64_t *acc = acc_rows + (size_t)blockIdx.x * 2 * N; // (not __restrict__: read at other threads' positions)
    const Pbs64Job job = jobs[blockIdx.x];
    const unsigned own = (unsigned)tid << 3; // n8192_slot(tid + 1024 m) = own + m

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
            acc[own + m] = 0;
            acc[N + own + m] = s >= N ? 0ull - v : v;
        }
    }
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
            const uint64_t *ar = acc + (size_t)r * N;
#pragma unroll
            for (int m = 0; m < PT; m++) {
                const int j = tid + m * L64_THREADS;
                const int s = (j - a) & (2 * N - 1); // (X^a acc_r)[j] = +-acc_r[j - a]
                const uint64_t w = ar[n8192_slot(s & (N - 1))];
                const uint64_t rot = s < N ? w : 0ull - w;
                init[r][m] = (uint32_t)((rot - ar[own + m] + round_off) >> (64 - rep));
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
                    n8192_ntt_forward(buf, tw0, tw1);
                    // products at this thread's positions: key polynomial (r, c, lev) in field f starts at
                    // (((r 2 + c) l + lev) 2 + f) N
                    const double *kc = key + (((size_t)(r * 2 + c) * L + lev) * 2) * N;
                    const bool fold = (products & 3) == 3; // recentre after every fourth product (see the head of this file)
                    products++;
#pragma unroll
                    for (int m = 0; m < PT; m++) {
                        const int s = tid + m * L64_THREADS;
                        double s0 = sum[0][m] + mulmod<L0>(buf[s], kc[s]), s1 = sum[1][m] + mulmod<L1>(buf[N + s], kc[N + s]);
                        if (fold) {
                            s0 = reduce<L0>(s0); // <= 0.5 p + 4 x 0.58 p before
                            s1 = reduce<L1>(s1);
                        }
                        sum[0][m] = s0;
                        sum[1][m] = s1;
                    }
                    // (no barrier: the next digits, or the column below, overwrite this thread's own positions only)
                }
            }
#pragma unroll
            for (int m = 0; m < PT; m++) {
                const int s = tid + m * L64_THREADS;
                buf[s] = reduce<L0>(sum[0][m]);
                buf[N + s] = reduce<L1>(sum[1][m]);
            }
            __syncthreads();
            n8192_ntt_inverse(buf, twi0, twi1);
            // CRT lift of each coefficient's two residues to the exact integer, accumulated mod 2^64 at own positions
#pragma unroll
            for (int m = 0; m < PT; m++) {
                const int j = tid + m * L64_THREADS;
                const double r0 = buf[j], r1 = buf[N + j];
                const double t = reduce<L1>(mulmod<L1>(r1 - r0, p0inv_mod_p1));
                HELM_BOUND(__builtin_fabs(r0) < 0x1p51 && __builtin_fabs(t) < 0x1p51, 4);
                acc[(unsigned)c * N + own + m] += (uint64_t)to_int64(r0) + L0::P_U64 * (uint64_t)to_int64(t);
            }
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
        for (int m = 0; m < PT; m++) init0[m] = (uint32_t)((acc[own + m] + round_off) >> (64 - rep));
#pragma unroll 1
        for (int c = 0; c < 2; c++) {
            double sum[2][PT]; // [field][position]: registers (every index below is a compile-time constant)
#pragma unroll
            for (int m = 0; m < PT; m++) sum[0][m] = sum[1][m] = 0.0;
#pragma unroll
            for (int r = 0; r < 2; r++) {
                uint32_t state[PT];
#pragma unroll
                for (int m = 0; m < PT; m++)
                    state[m] = r == 0 ? init0[m] : (uint32_t)((acc[N + own + m] + round_off) >> (64 - rep));
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
                    n8192_ntt_forward(buf, tw0, tw1);
                    // per subset S, one at a time: d^ M(e_S) at this thread's positions, then its product with the key word
                    // of GGSW (t, S), polynomial (r, c, lev); recentred after every fourth subset
                    const double *kq = key + (((size_t)(r * 2 + c) * L + lev) * 2) * N;
#pragma unroll 1
                    for (int S = 0; S < SUB; S++) {
                        int eS = 0; // e_S = sum of the members' rotations mod 2N (bit i of S = member i)
#pragma unroll
                        for (int i = 0; i < GG; i++) eS += (S >> i) & 1 ? am[i] : 0;
                        eS &= 2 * N - 1;
                        const double *kc = kq + (size_t)S * step_words;
                        const bool fold = (S & 3) == 3;
                        // (the transformed digits are read from buf again per subset: hoisted out of this loop, their 16
                        // values would stay live beside the sums)
                        asm volatile("" ::: "memory");
#pragma unroll
                        for (int m = 0; m < PT; m++) {
                            const int s = tid + m * L64_THREADS;
                            double d0 = buf[s], d1 = buf[N + s];
                            if (S) { // (M(0) = 1)
                                const int ex = 2 * (int)(__brev((unsigned)s) >> (32 - LOGN)) + 1; // expo(s)
                                const int at = (ex * eS) & (2 * N - 1);
                                d0 = mulmod<L0>(d0, psi_pow[at]);
                                d1 = mulmod<L1>(d1, psi_pow[2 * N + at]);
                            }
                            double s0 = sum[0][m] + mulmod<L0>(d0, kc[s]), s1 = sum[1][m] + mulmod<L1>(d1, kc[N + s]);
                            if (fold) {
                                s0 = reduce<L0>(s0); // <= 0.5 p + 4 x 0.59 p before
                                s1 = reduce<L1>(s1);
                            }
                            sum[0][m] = s0;
                            sum[1][m] = s1;
                        }
                    }
                    // (no barrier: the next digits, or the column below, overwrite this thread's own positions only)
                }
            }
#pragma unroll
            for (int m = 0; m < PT; m++) {
                const int s = tid + m * L64_THREADS;
                buf[s] = reduce<L0>(sum[0][m]);
                buf[N + s] = reduce<L1>(sum[1][m]);
            }
            __syncthreads();
            n8192_ntt_inverse(buf, twi0, twi1);
            // CRT lift as above; the lifted value replaces the accumulator row's word at own positions
#pragma unroll
            for (int m = 0; m < PT; m++) {
                const int j = tid + m * L64_THREADS;
                const double r0 = buf[j], r1 = buf[N + j];
                const double tq = reduce<L1>(mulmod<L1>(r1 - r0, p0inv_mod_p1));
                HELM_BOUND(__builtin_fabs(r0) < 0x1p51 && __builtin_fabs(tq) < 0x1p51, 4);
                acc[(unsigned)c * N + own + m] = (uint64_t)to_int64(r0) + L0::P_U64 * (uint64_t)to_int64(tq);
            }
        }
        __syncthreads(); // (B)
    }

    // ---- sample extract: every output of the job (extract_put; pad = 0: the one at coefficient 0) ----------
    const int n_out = pbs64_job_outputs(job.pad), ls = pbs64_job_log_stride(job.pad);
    for (int x = 0; x < n_out; x++) {
        const int h = x << ls;
        uint64_t *ob = out + (size_t)(job.out_row + x) * ((size_t)N + 1);
#pragma unroll
        for (int m = 0; m < PT; m++) {
            const int j = tid + m * L64_THREADS;
            extract_put(ob, N, h, j, acc[own + m]);
        }
        if (tid == 0) ob[N] = acc[N + n8192_slot(h)]; // body = B[h]
    }
}

// k_bsk_convert64_large's sibling for N = 8192: the two-field buffer is 128 KiB, over the static LDS limit, so it is dynamic
// (the launcher raises the kernel's limit: setup_n8192).  One workgroup per key polynomial: standard-domain u64 coefficients
// (taken as signed) -> both fields -> forward transform -> x N^-1, recentred, bit-reversed order: dst[i][r][c][lev][f][N]
// (src is [i][lev][r][c][N]).
__global__ __launch_bounds__(L64_THREADS) void k_bsk_convert64_n8192(const uint64_t *__restrict__ src, double *__restrict__ dst,
                                                                     const double *__restrict__ tw0,
                                                                     const double *__restrict__ tw1, double n_inv0,
                                                                     double n_inv1, double two32_0, double two32_1, int K1,
                                                                     int L)
{
    constexpr int N = 1 << N8192_LOGN;
    extern __shared__ __align__(16) unsigned char smem_c8192[];
    double *x = reinterpret_cast<double *>(smem_c8192); // [2][N]
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
    l64_ntt_forward<N8192_LOGN>(x, tw0, tw1);
    double *d = dst + ((((i * K1 + r) * K1 + c) * L + lev) * 2) * N;
    for (int j = (int)threadIdx.x; j < N; j += L64_THREADS) {
        d[j] = reduce<L0>(mulmod<L0>(x[j], n_inv0));
        d[N + j] = reduce<L1>(mulmod<L1>(x[N + j], n_inv1));
    }
}
