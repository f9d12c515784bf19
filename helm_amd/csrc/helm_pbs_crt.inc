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
// One workgroup of TP_THREADS per bootstrap; the LDS layout (TwoPrimeLds<uint32_t>), the transforms over both fields, the
// product accumulation, the CRT quotient and the key conversion's tail are pbs_twoprime.h's, shared with k_pbs64_generic, and
// so is the exactness argument.  This engine's own part of it: the digits, the bound on |x| and the torus word.
//
// Decomposition at rep = logB l = 31, re-derived: round_off = 1 << (31 - rep) = 1 and the shift 32 - rep = 1, so the state is
// (x + 1) >> 1 < 2^31 - the closest multiple of 2 (x = 2^32 - 1 wraps to state 0: the torus element 0, correct).  One level
// of 31 bits: last = true (no tie bit; 2 logB - 1 = 61 is never used as a shift), half_m1 = 2^30 - 1, state + half_m1 < 2^32,
// next is 0 or 1, digit = state - next 2^31 in [-2^30 + 1, 2^30].  Several levels: logB <= 15, the tie shift 2 logB - 1 <= 29,
// and the state stays below 2^31 + 1 after each level (gen_decompose_step's 32-bit recurrence holds for any logB l <= 31).
//
// Exactness.  Digits are at most 2^30 in magnitude (logB = 31, l = 1): exact doubles below p/2 = 2^48.2.  The true integer
// coefficient x of the external product (key words taken as centred 32-bit integers) has
// |x| <= (k+1) l N 2^(logB-1) 2^31 <= 4096 x 31 x 2^30 x 2^31 < 2^78 over the whole domain, against p0 p1 / 2 = 2^97.5: the
// domain needs no capacity check (helm_hip.hip restates this as a static_assert), and tp_quotient's lift is exact.  The torus
// word x mod 2^32 is formed from the two exact values in 32-bit arithmetic, (uint32_t)r0 + (uint32_t)p0 (uint32_t)t
// (to_torus32: |r0|, |t| < 2^51) - no value of magnitude 2^63 or more is ever formed, although |x| itself passes 2^63
// (TFHE_LIB's shape: 2^64.6).  The torus arithmetic is therefore the exact negacyclic product mod 2^32 whatever the shape.
// mulmod, reduce and to_torus32 carry ntt_fp64.h's HELM_BOUND checks, but the bound-checking build does not run this kernel:
// it is built like k_pbs64_generic, whose -O0 counting build faulted on its first launch for a cause not found (DESIGN.md
// 4.4.1), so that build refuses a CRT context at creation (setup_crt).

// the integer x with x = r0 (mod p0), x = r1 (mod p1), |x| < p0 p1 / 2, taken mod 2^32 (r0, r1 recentred)
__device__ __forceinline__ uint32_t crt_lift32(double r0, double r1, double p0inv_mod_p1)
{
    const double t = tp_quotient(r0, r1, p0inv_mod_p1);
    return to_torus32(r0) + (uint32_t)FpG::P_U64 * to_torus32(t);
}

// bsk: [i][r][c][lev][f][N] in the transform domain (bit-reversed order), times N^-1, recentred (k_bsk_convert_crt)
template <int LOGN>
__global__ __launch_bounds__(TP_THREADS) void k_pbs_crt(const PbsJob *__restrict__ jobs,
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
    const TwoPrimeLds<uint32_t> lay(N, K1, D, n);
    uint32_t *acc = reinterpret_cast<uint32_t *>(smem_crt + lay.acc);
    double *col = reinterpret_cast<double *>(smem_crt + lay.col);
    double *dig = reinterpret_cast<double *>(smem_crt + lay.dig);
    uint16_t *MS = reinterpret_cast<uint16_t *>(smem_crt + lay.ms);
    const PbsJob job = jobs[blockIdx.x];
    const size_t row = (size_t)n + 1;

    // ---- gate linear step + modulus switch ---------------------------------------------------
    switch_row(MS, GateRows(job, wires, raw_in, row), n, tid, TP_THREADS, LOGN + 1);
    __syncthreads();
    // ---- accumulator init: (0, ..., 0, X^{-b~} tv) -----------------------------------------
    {
        const int bt = (int)MS[n];
        const uint32_t *tv = tvs + (size_t)job.tv * N;
        for (int idx = tid; idx < K1 * N; idx += TP_THREADS) {
            const int r = idx >> LOGN, j = idx & (N - 1);
            acc[idx] = r == K ? lut_rotated(tv, j, bt, N) : 0u;
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
            for (int idx = tid; idx < (cnt << LOGN); idx += TP_THREADS) {
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
            tp_ntt_forward<LOGN>(dig, cnt, dstride, tw0, tw1);
            tp_accumulate<LOGN>(dig, dstride, col, cstride, key, q0, cnt, K1, L);
        }
        tp_ntt_inverse<LOGN>(col, K1, cstride, twi0, twi1);
        // CRT lift of each coefficient's two residues to the exact integer, accumulated mod 2^32
        for (int idx = tid; idx < K1 * N; idx += TP_THREADS) acc[idx] += crt_lift32(col[idx], col[cstride + idx], p0inv_mod_p1);
        __syncthreads();
    }

    // ---- sample extract (coefficient 0) ----------------------------------------------------
    uint32_t *ob = big_row(out_big, blockIdx.x, K, N);
    for (int idx = tid; idx < K * N; idx += TP_THREADS) {
        const int r = idx >> LOGN, t = idx & (N - 1);
        // out[r N + t] = (t == 0) ? A_r[0] : -A_r[N - t]
        ob[idx] = t == 0 ? acc[r * N] : 0u - acc[r * N + N - t];
    }
    if (tid == 0) ob[K * N] = acc[K * N]; // body = B[0]
}

// One workgroup per key polynomial: standard-domain u32 coefficients (taken as signed: |v| <= 2^31 < p/2, the same integer in
// both fields) -> tp_convert: dst[i][r][c][lev][f][N] (src is [i][lev][r][c][N]).
template <int LOGN>
__global__ __launch_bounds__(TP_THREADS) void k_bsk_convert_crt(const uint32_t *__restrict__ src, double *__restrict__ dst,
                                                             const double *__restrict__ tw0, const double *__restrict__ tw1,
                                                             double n_inv0, double n_inv1, int K1, int L)
{
    constexpr int N = 1 << LOGN;
    __shared__ double x[2 * N];
    auto load = [&](size_t at, double &v0, double &v1) {
        const double v = (double)(int32_t)src[at];
        v0 = v;
        v1 = v;
    };
    tp_convert<LOGN>(x, load, dst, tw0, tw1, n_inv0, n_inv1, K1, L);
}

// NTT self-test of the CRT class: forward in both fields, x N^-1, inverse, lift; must reproduce the input exactly.
template <int LOGN>
__global__ __launch_bounds__(TP_THREADS) void k_ntt_roundtrip_crt(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst,
                                                                const double *__restrict__ tw0, const double *__restrict__ tw1,
                                                                const double *__restrict__ twi0, const double *__restrict__ twi1,
                                                                double n_inv0, double n_inv1, double p0inv_mod_p1)
{
    constexpr int N = 1 << LOGN;
    __shared__ double x[2 * N];
    const size_t base = (size_t)blockIdx.x * N;
    for (int j = (int)threadIdx.x; j < N; j += TP_THREADS) {
        const double v = (double)(int32_t)src[base + j];
        x[j] = v;
        x[N + j] = v;
    }
    __syncthreads();
    tp_ntt_forward<LOGN>(x, 1, N, tw0, tw1);
    for (int j = (int)threadIdx.x; j < N; j += TP_THREADS) {
        x[j] = reduce<FpG>(mulmod<FpG>(x[j], n_inv0));
        x[N + j] = reduce<FpG2>(mulmod<FpG2>(x[N + j], n_inv1));
    }
    __syncthreads();
    tp_ntt_inverse<LOGN>(x, 1, N, twi0, twi1);
    for (int j = (int)threadIdx.x; j < N; j += TP_THREADS) dst[base + j] = crt_lift32(x[j], x[N + j], p0inv_mod_p1);
}
