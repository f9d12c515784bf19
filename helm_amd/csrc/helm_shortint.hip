// helm_shortint.hip — gfx950 kernels + C ABI (include/helm_shortint.h) of the LUT-mode /
// arithmetic-mode engine: 64-bit torus, KS_PBS order.  Replaces the tfhe::shortint
// ServerKey calls HELM issues per LUT gate (reference src/gates.rs:754-785) and, through
// the radix layer built on the same two primitives, per arithmetic operator
// (src/gates.rs:306-702):
//
//   k_lincomb64     out = sum coef * in + const                      (no bootstrap)
//   k_keyswitch64   big LWE (k*N) -> small LWE (n), four ciphertexts per key pass
//   k_pbs64         modulus switch + blind rotate with a per-ciphertext look-up table +
//                   sample extract.  One workgroup per ciphertext, one wave per
//                   (accumulator polynomial, CRT prime): the exact negacyclic products of
//                   a 64-bit torus need ~2^97, i.e. two of the fp64 NTT fields of
//                   ntt_fp64.h and a CRT lift mod 2^64 after the inverse transforms.
//   k_bsk_convert64 standard-domain key -> both NTT fields (once per key)
//
// There is no CPU fallback in this file.
#include "../../include/helm_shortint.h"
#include "../../include/helm_comm.h"
#include "ntt_fp64.h"
#include "many_lut_rule.h"
#include "keyswitch.h"
#include "pbs_frame.h"
#include "with_logn.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#ifndef HELM_SI_TU
#define HELM_SI_TU 0 // 1: the max-ILP translation unit (two launchers only)
#endif
#ifndef HELM_SI_SPLIT_TU
#define HELM_SI_SPLIT_TU 0
#endif
using namespace helm;

int helm_hip_fail_(int code, const std::string &msg); // helm_hip.hip: sets helm_hip_last_error()
#define fail helm_hip_fail_
int helm_hip_runtime_guard_(const char *where); // helm_comm.cpp: one HIP runtime per process, or HELM_ERR_STATE naming the copies
#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t e__ = (expr);                                                                    \
        if (e__ != hipSuccess)                                                                      \
            return fail(HELM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));          \
    } while (0)

namespace {

// CRT pair: two 49-bit primes whose 2^53 / p >= 13.3 headroom lets a whole forward transform (up to
// 11 stages, digits below 2^23: <= 9.6 p), the pointwise products and their sums (<= 11.4 p, the largest bound in this
// file) run without recentring.  Round 4: the pair is 5072^4 + 1 and 5096^4 + 1 (ntt_fp64.h FpG, FpG2; rounds 1-3:
// Fp<49>, Fp49b with 2^53 / p = 14.2) - their fourth root of unity psi^(N/2) = +-b^2 is 25 bits long, so stage 1 of a
// forward transform on digits (|d| <= 2^23: the split kernel is only chosen for pbs_logB <= 24) is ONE multiplication,
// exact and inside (-p/2, p/2), instead of a modular one (p0 p1 / 2 = 2^97.5 covers more than before;
// profiles/r04/short_roots_field.txt).
using F0 = FpG;
using F1 = FpG2;
// Round 6: the 46-bit pair (ntt_fp64.h FpJ, FpJ2) for k_pbs64k contexts whose LOADED key keeps the exact products below
// p p' / 2 = 2^90.62 (helm_si_load_bootstrap_key; helm_si_field_bits() says which pair a context computes in)
using J0 = FpJ;
using J1 = FpJ2;
__device__ __forceinline__ double stage1_digit_product(double digit, double w1)
{
    return digit * w1; // |digit| <= 2^23, |w1| = b^2 < 2^24.7: exact, < p/2
}

#ifdef HELM_WIDE_STAMPS
__device__ unsigned long long g_stamps64[8 * 8];
#define STAMP_DECL unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t0 = 0, t1;
#define STAMP_BEGIN                        \
    t0 = __builtin_amdgcn_s_memtime();     \
    __builtin_amdgcn_s_waitcnt(0xC07F);
#define STAMP(k)                           \
    t1 = __builtin_amdgcn_s_memtime();     \
    __builtin_amdgcn_s_waitcnt(0xC07F);    \
    ph[k] += t1 - t0;                      \
    t0 = t1;
#define STAMP_END(wave)                    \
    if (blockIdx.x == 0 && lane == 0)      \
        for (int q = 0; q < 8; q++) g_stamps64[(wave) * 8 + q] = ph[q];
#else
#define STAMP_DECL
#define STAMP_BEGIN
#define STAMP(k)
#define STAMP_END(wave)
#endif

struct Pbs64Job {
    int32_t in_row;  // row of the small-LWE buffer (n+1 words)
    int32_t lut;     // row of the look-up-table buffer (N words)
    int32_t out_row; // row of the destination table (k*N+1 words)
    int32_t pad;     // programmable bootstrap: 0 = one output, sample extract at coefficient 0; many-LUT (helm_si_apply_many_luts):
                     // (n_out - 1) | log2(stride) << 16 - output x < n_out is the extract at coefficient x * stride, written to
                     // row out_row + x.  Modes 1 and 2 of k_pbs64 (the WoP-PBS path): the index of the job's key.
};
__host__ __device__ __forceinline__ int pbs64_job_outputs(int32_t pad) { return (pad & 0xFFFF) + 1; }
__host__ __device__ __forceinline__ int pbs64_job_log_stride(int32_t pad) { return pad >> 16; }

struct Ks64Job {
    int32_t in_row;  // row of the big table
    int32_t out_row; // row of the small-LWE buffer
};

// the input row of a job: row in_row of `small` as it is
__device__ __forceinline__ PlainRow<uint64_t> job_row(const Pbs64Job &job, const uint64_t *small, int n)
{
    return PlainRow<uint64_t>(small, job.in_row, n);
}

// exact integer in a double (|v| < 2^51) -> two's complement int64
__device__ __forceinline__ int64_t to_int64(double v)
{
    const double m = v + 6755399441055744.0; // 1.5 * 2^52: mantissa = 2^51 + v
    const uint32_t lo = (uint32_t)__double2loint(m);
    const int32_t hi = (int32_t)((uint32_t)__double2hiint(m) & 0xFFFFFu) - 0x80000;
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | lo);
}

// The epilogue of the tuned bootstrap kernels: every output of the job (pbs64_job_outputs(pad), pad = 0: the one at
// coefficient 0).  A mask wave (p < K) holds slots s0 .. s0 + CNT - 1 of polynomial p (coefficient jA(lane, slot)); one lane
// of the workgroup (`body`) writes B[h].  acc_at(j): coefficient j of this wave's polynomial, complete in LDS since the
// blind rotation's final barrier.
template <typename G, int K, int CNT, typename ACC>
__device__ __forceinline__ void sample_extract_outputs(uint64_t *__restrict__ out, int32_t out_row, int32_t pad, int p, int s0,
                                                       bool body, int lane, const ACC &acc_at)
{
    constexpr int N = G::N;
    const int n_out = pbs64_job_outputs(pad), ls = pbs64_job_log_stride(pad);
    for (int x = 0; x < n_out; x++) {
        const int h = x << ls;
        uint64_t *ob = big_row(out, out_row + x, K, N);
        if (p < K) {
#pragma unroll
            for (int e = 0; e < CNT; e++) {
                const int j = G::jA(lane, s0 + e);
                extract_put(ob + (size_t)p * N, N, h, j, acc_at(j));
            }
        } else if (body) {
            ob[K * N] = acc_at(h);
        }
    }
}

// ------------------------------------------------------------------------------------
// k_pbs64<LOGN, L>: k = 1.  Waves w = 0..3: polynomial p = w >> 1, field f = w & 1.
// Per CMUX step, wave (p, f): rotate/subtract polynomial p (u64, LDS), signed-decompose,
// per level forward NTT in field f and multiply by the two key polynomials of row p; the
// product for the other polynomial goes to the partner (1-p, f) through this wave's
// scratch; inverse NTT of the own sum; the two residues of each coefficient meet in the
// wave that owns that half of the polynomial, which lifts them (CRT) to the exact integer
// mod 2^64 and accumulates.
// ------------------------------------------------------------------------------------
template <int LOGN_, int L_>
struct Pbs64Cfg {
    static constexpr int LOGN = LOGN_, L = L_, K = 1, K1 = 2, NW = 4;
    using G = Geo<LOGN>;
    static constexpr int MAX_SMALL_N = 1024;
    static constexpr size_t X_OFF = 0;                                            // double [NW][XPAD]
    // twiddles per field: index table for blocks A, B (N >> BC entries) + lane table for block C
    static constexpr int TW_IDX = G::N >> G::BC, TW_FIELD = TW_IDX + G::TWC * 64;
    static constexpr size_t TW_OFF = X_OFF + sizeof(double) * NW * G::XPAD;       // double [2][TW_FIELD]
    static constexpr size_t ACC_OFF = TW_OFF + sizeof(double) * 2 * TW_FIELD;     // u64 [K1][N]
    static constexpr size_t MS_OFF = ACC_OFF + sizeof(uint64_t) * K1 * G::N;      // u16 [n+1]
    static constexpr size_t BYTES = (MS_OFF + sizeof(uint16_t) * (MAX_SMALL_N + 1) + 15) / 16 * 16;
};

template <typename C, typename F, int MODE>
__device__ __forceinline__ void pbs64_body(unsigned char *smem, const double *__restrict__ bsk, int n, int logB,
                                           double p0inv_mod_p1, int p, int f, int lane,
                                           const uint64_t *__restrict__ alt_p)
{
    constexpr int LOGN = C::LOGN, L = C::L, K1 = C::K1;
    using G = Geo<LOGN>;
    constexpr int N = G::N, E = G::E, H = E / 2;
    double *X = reinterpret_cast<double *>(smem + C::X_OFF);
    uint64_t *ACC = reinterpret_cast<uint64_t *>(smem + C::ACC_OFF);
    const uint16_t *MS = reinterpret_cast<const uint16_t *>(smem + C::MS_OFF);
    const int w = p * 2 + f;
    double *xb = X + (size_t)w * G::XPAD;                       // own scratch
    const double *x_poly = X + (size_t)((1 - p) * 2 + f) * G::XPAD; // same field, other polynomial
    const double *x_field = X + (size_t)(p * 2 + (1 - f)) * G::XPAD; // same polynomial, other field
    uint64_t *acc_p = ACC + (size_t)p * N;
    const double *twt = reinterpret_cast<const double *>(smem + C::TW_OFF) + (size_t)f * C::TW_FIELD;
    TwHybrid<LOGN, false> twf{twt, twt + C::TW_IDX + lane};
    TwHybrid<LOGN, true> twi{twt, twt + C::TW_IDX + (63 - lane)};

    // key words of step i for this wave: [i][row p][c][lev][f][e/2][lane] as double2
    const size_t per_poly = (size_t)2 * (N / 2); // both fields
    const size_t bsk_step = (size_t)K1 * K1 * L * per_poly;
    const double2 *bsk_w = reinterpret_cast<const double2 *>(bsk) + ((size_t)p * K1 * L * 2 + f) * (N / 2) + lane;

    STAMP_DECL
    for (int i = 0; i < n; i++) {
        const int a = __builtin_amdgcn_readfirstlane((int)MS[i]);
        if (a == 0) continue; // uniform over the workgroup: every wave skips the same steps
        STAMP_BEGIN
        const double2 *bp_i = bsk_w + (size_t)i * bsk_step;

        // ---- rotate / subtract, decomposition state (least significant level first; the
        //      rounded value has logB * L <= 32 bits) --------------------------------------------
        uint32_t state[E];
        {
            const int rep = logB * L;
#pragma unroll
            for (int e = 0; e < E; e++) {
                const int j = G::jA(lane, e);
                uint64_t v;
                if constexpr (MODE == 2) {
                    v = alt_p[j]; // CMUX of two given ciphertexts: c1 - c0
                } else {
                    const int src = (j - a) & (2 * N - 1);
                    v = acc_p[src & (N - 1)];
                    if (src >= N) v = 0ull - v;
                }
                v -= acc_p[j];
                state[e] = (uint32_t)((v + (1ull << (63 - rep))) >> (64 - rep));
            }
        }
        double mine[E], other[E];
        const uint32_t half_m1 = (1u << (logB - 1)) - 1u;
    [[maybe_unused]] const uint32_t bmask = (1u << logB) - 1u;
#pragma unroll
        for (int lev = L - 1; lev >= 0; lev--) {
            double x[1][E];
#pragma unroll
            for (int e = 0; e < E; e++) {
                // tfhe's carry rule as one addition (see decompose_step in helm_hip.hip): the digit is what
                // the state loses when B/2 - 1 + (bit 2 logB - 1) is added and logB bits are shifted out
                const uint32_t s = state[e];
                const uint32_t next = (s + half_m1 + __builtin_amdgcn_ubfe(s, 2 * logB - 1, 1)) >> logB;
                state[e] = next;
                x[0][e] = (double)((int32_t)s - (int32_t)(next << logB));
            }
            // key words in chunks of E/4 (two per column), software-pipelined: the first chunk is
            // fetched before the transform, each next one just before the products of the previous
            // (at most two chunks = 64 registers in flight; whole columns spilled to AGPRs)
            constexpr int CH = E / 4; // double2 per chunk
            auto fetch = [&](int q, double2 (&dst)[CH]) { // chunk q of 4: column q / 2, half q % 2
                const double2 *kp = bp_i + (size_t)((q >> 1) * L + lev) * per_poly + (size_t)(q & 1) * CH * 64;
#pragma unroll
                for (int u = 0; u < CH; u++) dst[u] = kp[u * 64];
            };
            auto products = [&](int q, const double2 (&kq)[CH]) {
                const int c = q >> 1, e20 = (q & 1) * CH;
#pragma unroll
                for (int u = 0; u < CH; u++) {
                    const int e2 = e20 + u;
                    const double t0 = mulmod<F>(x[0][2 * e2], kq[u].x), t1 = mulmod<F>(x[0][2 * e2 + 1], kq[u].y);
                    if (c == p) {
                        mine[2 * e2] = lev == L - 1 ? t0 : mine[2 * e2] + t0;
                        mine[2 * e2 + 1] = lev == L - 1 ? t1 : mine[2 * e2 + 1] + t1;
                    } else {
                        other[2 * e2] = lev == L - 1 ? t0 : other[2 * e2] + t0;
                        other[2 * e2 + 1] = lev == L - 1 ? t1 : other[2 * e2 + 1] + t1;
                    }
                }
            };
            double2 ka[CH], kb2[CH];
            fetch(0, ka);
            __builtin_amdgcn_sched_barrier(0);
            STAMP(0) // rotation, decomposition, first key chunk issued
            ntt_forward<F, LOGN, 1, decltype(twf), 0, NoHook, 1>(x, xb, twf, lane); // (digits: stage 1 plain)
            STAMP(1) // forward transform
            __builtin_amdgcn_sched_barrier(0);
            fetch(1, kb2);
            __builtin_amdgcn_sched_barrier(0);
            products(0, ka);
            __builtin_amdgcn_sched_barrier(0);
            fetch(2, ka);
            __builtin_amdgcn_sched_barrier(0);
            products(1, kb2);
            __builtin_amdgcn_sched_barrier(0);
            fetch(3, kb2);
            __builtin_amdgcn_sched_barrier(0);
            products(2, ka);
            products(3, kb2);
        }
        // hand the other polynomial's partial sum over through the (now idle) scratch
#pragma unroll
        for (int e = 0; e < E; e++) xb[e * 64 + lane] = reduce<F>(other[e]);
        STAMP(2) // products, hand-over written
        lds_block_sync();
        STAMP(3) // barrier 1
#pragma unroll
        for (int e = 0; e < E; e++) mine[e] = reduce<F>(reduce<F>(mine[e]) + x_poly[e * 64 + lane]);
        lds_block_sync(); // hand-over slots read: scratch free again
        STAMP(4) // sum + barrier 2

        ntt_inverse<F, LOGN>(mine, xb, twi, lane);
        STAMP(5) // inverse transform

        // ---- CRT: field-f wave lifts slots [f*H, f*H+H); it needs the other field's
        //      residues for those and provides its own for the other half ----------------
#pragma unroll
        for (int e = 0; e < H; e++) xb[e * 64 + lane] = mine[(1 - f) * H + e];
        lds_block_sync();
#pragma unroll
        for (int e = 0; e < H; e++) {
            const double own = mine[f * H + e], oth = x_field[e * 64 + lane];
            const double r0 = f == 0 ? own : oth, r1 = f == 0 ? oth : own;
            // x = r0 + p0 * t,  t = (r1 - r0) * p0^-1 mod p1 : the exact integer (|x| < p0 p1 / 2)
            const double t = mulmod<F1>(r1 - r0, p0inv_mod_p1);
            const uint64_t xv = (uint64_t)to_int64(r0) + F0::P_U64 * (uint64_t)to_int64(t);
            acc_p[G::jA(lane, f * H + e)] += xv;
        }
        lds_block_sync(); // accumulator complete before the next step's rotated reads
        STAMP(6) // CRT exchange, lift, accumulate, barriers 3 and 4
    }
    STAMP_END(p * 2 + f)
}

// MODE 0: programmable bootstrap (job: in_row of `small`, lut row of N words, out_row of k*N+1 words).
// MODE 1: blind rotation of a given GLWE with a per-job GGSW stack, sample extract - the tail of vertical packing
//         (job: in_row = row of `small` holding the synthetic rotation amounts, lut = row of (k+1) N words in
//         `luts`, pad = index of the job's key, key_stride doubles apart).
// MODE 2: one CMUX  out = c0 + GGSW (x) (c1 - c0)  (job: lut = row of c0, in_row = row of c1, both rows of
//         (k+1) N words of `luts`; pad = key index; the GGSW is entry key_first of that key; out rows of (k+1) N).
template <typename C, int MODE>
__global__ __launch_bounds__(64 * C::NW, 1) void k_pbs64(const Pbs64Job *__restrict__ jobs,
                                                         const uint64_t *__restrict__ small, // rows of n+1
                                                         const uint64_t *__restrict__ luts,  // rows of N
                                                         const double *__restrict__ bsk,     // NTT domain, both fields
                                                         const double *__restrict__ tw0,
                                                         const double *__restrict__ tw1,
                                                         uint64_t *__restrict__ out, // rows of k*N+1
                                                         int n, int logB, double p0inv_mod_p1, size_t key_stride,
                                                         int key_first)
{
    constexpr int LOGN = C::LOGN, K = C::K;
    using G = Geo<LOGN>;
    constexpr int N = G::N, E = G::E, H = E / 2;
    extern __shared__ __align__(16) unsigned char smem[];
    uint64_t *ACC = reinterpret_cast<uint64_t *>(smem + C::ACC_OFF);
    uint16_t *MS = reinterpret_cast<uint16_t *>(smem + C::MS_OFF);
    double *TW = reinterpret_cast<double *>(smem + C::TW_OFF);

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int p = w >> 1, f = w & 1;
    const Pbs64Job job = jobs[blockIdx.x];
    if constexpr (MODE == 2) {
        if (tid == 0) MS[0] = 1, MS[1] = 0;
    } else switch_row(MS, job_row(job, small, n), n, tid, 64 * C::NW, LOGN + 1);
    for (int i = tid; i < C::TW_IDX; i += 64 * C::NW) {
        TW[i] = tw0[i];
        TW[C::TW_FIELD + i] = tw1[i];
    }
    for (int r = w; r < G::TWC; r += C::NW) { // lane-table rows of block C (slots TWB.. of tw_lane_index)
        const int idx = tw_lane_index<LOGN>(G::TWB + r, lane);
        TW[C::TW_IDX + r * 64 + lane] = tw0[idx];
        TW[C::TW_FIELD + C::TW_IDX + r * 64 + lane] = tw1[idx];
    }
    __syncthreads();
    // accumulator: (0, X^{-b~} * lut); MODE 1, 2: the given GLWE as it is
    if constexpr (MODE == 0) {
        const int bt = (int)MS[n];
        const uint64_t *tv = luts + (size_t)job.lut * N;
        for (int j = tid; j < (K + 1) * N; j += 64 * C::NW) ACC[j] = j >= K * N ? lut_rotated(tv, j - K * N, bt, N) : 0ull;
    } else {
        const uint64_t *c0 = luts + (size_t)job.lut * ((size_t)(K + 1) * N);
        for (int j = tid; j < (K + 1) * N; j += 64 * C::NW) ACC[j] = c0[j];
    }
    __syncthreads();

    const double *key = bsk;
    const uint64_t *alt_p = nullptr;
    if constexpr (MODE != 0) key += (size_t)job.pad * key_stride + (size_t)key_first * ((size_t)(K + 1) * (K + 1) * C::L * 2 * N);
    if constexpr (MODE == 2) alt_p = luts + (size_t)job.in_row * ((size_t)(K + 1) * N) + (size_t)p * N;
    const int steps = MODE == 2 ? 1 : n;
    if (f == 0) pbs64_body<C, F0, MODE>(smem, key, steps, logB, p0inv_mod_p1, p, 0, lane, alt_p);
    else pbs64_body<C, F1, MODE>(smem, key, steps, logB, p0inv_mod_p1, p, 1, lane, alt_p);

    const uint64_t *acc_p = ACC + (size_t)p * N;
    if constexpr (MODE == 2) { // the whole GLWE
        uint64_t *og = out + (size_t)job.out_row * ((size_t)(K + 1) * N) + (size_t)p * N;
#pragma unroll
        for (int e = 0; e < H; e++) {
            const int j = G::jA(lane, f * H + e);
            og[j] = acc_p[j];
        }
        return;
    }
    // ---- sample extract; wave (p, f) writes its half of the slots (MODE 1: pad is the key index, one output) ------
    sample_extract_outputs<G, K, H>(out, job.out_row, MODE == 0 ? job.pad : 0, p, f * H, f == 0 && lane == 0, lane,
                                    [&](int j) { return acc_p[j]; });
}

// ------------------------------------------------------------------------------------
// k_pbs64k<LOGN, K>: the programmable bootstrap for k > 1 and one decomposition level - the
// parameter set the reference binary installs for LUT mode, PARAM_MESSAGE_1_CARRY_1_KS_PBS
// (reference src/bin/helm.rs:301: k = 3, N = 512 [dimensions recalled]).  2 (k+1) waves:
// wave w = (polynomial p = w >> 1, field f = w & 1), as k_pbs64; what changes with k + 1 > 2
// polynomials is the hand-over: every wave publishes the spectrum of its digit polynomial, and wave
// (p, f) gathers column p's sum from all k + 1 of them (see pbs64k_body).  Five workgroup barriers
// per step; 64 KB of LDS and at most 128 registers: TWO ciphertexts per CU.  Measured against the
// forms they replaced (profiles/r03/si_kernel_experiments.txt): the gather form against a ds_add_f64
// scatter +6.4 %; the accumulator stored as [acc | -acc] (16) and the digits split between the two
// field waves of a polynomial (17) each kept.
// ------------------------------------------------------------------------------------
//
// N = 1024 (k = 2, the 3-bit set shortint_m2c1): the same six waves and two ciphertexts per CU, but the LDS of the N = 512
// layout would be 93 KB (scratch 51 KB + twiddles 16 KB + accumulator 24 KB, 48 KB as [acc | -acc]).  So the accumulator
// has no region of its own (ACC_X): wave (p, f) keeps the half of polynomial p it lifts in the CRT (slots f H .. f H + H,
// coefficients f N/2 .. f N/2 + N/2) in registers, and publishes it in the upper half of its own transform scratch, which is
// free from the CRT of one step to the decomposition of the next.  The digit hand-over moves to the lower halves.  LDS
// 70.4 KB per ciphertext.
template <int LOGN_, int K_>
struct Pbs64kCfg {
    static constexpr int LOGN = LOGN_, L = 1, K = K_, K1 = K_ + 1, NW = 2 * K1;
    using G = Geo<LOGN>;
    static constexpr int MAX_SMALL_N = 1024;
    static constexpr bool ACC_X = LOGN >= 10;                                     // the accumulator lives in the scratch
    static constexpr size_t X_OFF = 0;                                            // double [NW][XPAD]: transform scratch,
                                                                                  // and between two barriers the column sums
    static constexpr int TW_IDX = G::N >> G::BC, TW_FIELD = TW_IDX + G::TWC * 64;
    static constexpr size_t TW_OFF = X_OFF + sizeof(double) * NW * G::XPAD;       // double [2][TW_FIELD]
    static constexpr size_t ACC_OFF = TW_OFF + sizeof(double) * 2 * TW_FIELD;     // u64 [K1][N] (none: ACC_X)
    // every polynomial is stored as [acc | -acc] (2N words): a rotated read X^a acc is then ONE indexed read,
    // no sign logic (5 vector instructions per coefficient in a kernel that is bound by its instruction stream)
    static constexpr int ACC_LEN = ACC_X ? G::N : 2 * G::N;
    static constexpr size_t MS_OFF = ACC_OFF + (ACC_X ? 0 : sizeof(uint64_t) * K1 * ACC_LEN); // u16 [n+1]
    static constexpr size_t BYTES = (MS_OFF + sizeof(uint16_t) * (MAX_SMALL_N + 1) + 15) / 16 * 16;
    static_assert(NW <= 16, "a workgroup holds at most 16 waves");
    static_assert(2 * BYTES <= 160 * 1024, "two ciphertexts per CU");
    // ACC_X: coefficient j of polynomial p, in the upper half of the scratch of wave (p, j >= N/2)
    __device__ static __forceinline__ int acc_x(int p, int j)
    {
        return (p * 2 + (j >> (LOGN - 1))) * G::XPAD + G::N / 2 + (j & (G::N / 2 - 1));
    }
};

// F: this wave's field; FA, FB: the CRT pair (F is one of them)
template <typename C, typename F, typename FA, typename FB>
__device__ __forceinline__ void pbs64k_body(unsigned char *smem, const double *__restrict__ bsk, int n, int logB,
                                            double p0inv_mod_p1, int p, int f, int lane)
{
    constexpr int LOGN = C::LOGN, K1 = C::K1;
    // 46-bit pair: both leading forward stages plain on the digits (|d| <= 2^17), no recentring of the column sums - the
    // inverse transform takes them unreduced (ntt_inverse, WIDE)
    constexpr bool WIDE = wide_headroom<F>::value;
    constexpr int DIG = WIDE ? 2 : 1;
    using G = Geo<LOGN>;
    constexpr int N = G::N, E = G::E, H = E / 2;
    double *X = reinterpret_cast<double *>(smem + C::X_OFF);
    uint64_t *ACC = reinterpret_cast<uint64_t *>(smem + C::ACC_OFF);
    const uint16_t *MS = reinterpret_cast<const uint16_t *>(smem + C::MS_OFF);
    double *xb = X + (size_t)(p * 2 + f) * G::XPAD;                          // own scratch
    const double *x_field = X + (size_t)(p * 2 + (1 - f)) * G::XPAD;         // same polynomial, other field
    uint64_t *acc_p = ACC + (size_t)p * C::ACC_LEN;
    const double *twt = reinterpret_cast<const double *>(smem + C::TW_OFF) + (size_t)f * C::TW_FIELD;
    TwHybrid<LOGN, false> twf{twt, twt + C::TW_IDX + lane};
    TwHybrid<LOGN, true> twi{twt, twt + C::TW_IDX + (63 - lane)};
    // key words of step i for this wave: [i][row p][c][f][e/2][lane] as double2 (the layout k_bsk_convert64 writes)
    // read with buffer loads: one descriptor in scalar registers, a scalar byte offset per (step, column), one lane
    // register and an immediate per word (plain pointers cost an address register pair per word and spill at 128)
    const unsigned poly_bytes = (unsigned)(N / 2) * 16u;      // one key polynomial in one field
    const unsigned col_bytes = 2u * poly_bytes;               // both fields
    const unsigned step_bytes = (unsigned)(K1 * K1) * col_bytes;
    const unsigned row_off = (unsigned)p * col_bytes + (unsigned)f * poly_bytes;
    KeyBuf kb;
    kb.init(bsk, (size_t)n * step_bytes, lane);
    const uint32_t half_m1 = (1u << (logB - 1)) - 1u;
    [[maybe_unused]] const uint32_t bmask = (1u << logB) - 1u;
    // ACC_X: the accumulator as published in the scratch upper halves (Pbs64kCfg::acc_x), and this wave's half in registers
    [[maybe_unused]] const uint64_t *Xu = reinterpret_cast<const uint64_t *>(X);
    [[maybe_unused]] uint64_t *xb_acc = reinterpret_cast<uint64_t *>(xb) + N / 2 + lane;
    [[maybe_unused]] uint64_t acc_own[C::ACC_X ? H : 1];
    if constexpr (C::ACC_X) {
#pragma unroll
        for (int e = 0; e < H; e++) acc_own[e] = xb_acc[e * 64];
    }
    for (int i = 0; i < n; i++) {
        const int a = __builtin_amdgcn_readfirstlane((int)MS[i]);
        if (a == 0) continue; // uniform over the workgroup
        const unsigned so_i = (unsigned)i * step_bytes + row_off;
        // Gather form of the hand-over: wave (p, f) owns OUTPUT column p.  Every wave publishes the spectrum of its digit
        // polynomial in its scratch; after the barrier each wave reads all K1 spectra and multiplies them with the key
        // words of column p (rows 0..k): the column sum stays in registers - no LDS atomics, no clear, no data-dependent
        // branch, and the own spectrum's registers are free during the products.
        double2 kw[H][K1];
        auto fetch = [&](int u) {
#pragma unroll
            for (int r = 0; r < K1; r++) kw[u][r] = kb.load(so_i + (unsigned)(r * K1) * col_bytes, u * 1024);
        };
#pragma unroll
        for (int u = 0; u < H / 2; u++) fetch(u);
        double mine[E];
        {
            double x[1][E];
            auto digit = [&](int e, [[maybe_unused]] int eo) { // eo: slot e - f H of acc_own (ACC_X)
                const int j = G::jA(lane, e);
                const int src = (j - a) & (2 * N - 1);
                uint64_t v;
                if constexpr (C::ACC_X) {
                    v = Xu[C::acc_x(p, src & (N - 1))];
                    if (src >= N) v = 0ull - v;
                    v -= acc_own[eo];
                } else {
                    v = acc_p[src];
                    v -= acc_p[j];
                }
                const uint32_t st = (uint32_t)((v + (1ull << (63 - logB))) >> (64 - logB));
                return (double)((int)((st + half_m1) & bmask) - (int)half_m1); // st <= B/2 stays, above it st - B
            };
            // the two field waves of a polynomial need the same digits: each makes half of them and hands them to the other
            // through the other's (free) transform scratch - one more barrier, half the decomposition work
            // (ACC_X: through the lower halves - the upper ones hold the accumulator until the barrier)
            double *xb_field = X + (size_t)(p * 2 + (1 - f)) * G::XPAD;
            constexpr int XO = C::ACC_X ? 0 : 1; // slot offset of the hand-over: (XO f H + e) * 64
#pragma unroll
            for (int e = 0; e < H; e++) {
                x[0][f * H + e] = digit(f * H + e, e);
                xb_field[(XO * f * H + e) * 64 + lane] = x[0][f * H + e];
            }
            lds_block_sync();
#pragma unroll
            for (int e = 0; e < H; e++) x[0][(1 - f) * H + e] = xb[(XO * (1 - f) * H + e) * 64 + lane];
            ntt_forward<F, LOGN, 1, decltype(twf), 0, NoHook, DIG>(x, xb, twf, lane); // (digits: stage 1 - 46-bit pair: stages 1 and 2 - plain)
#pragma unroll
            for (int e = 0; e < E; e++) xb[e * 64 + lane] = x[0][e];
        }
        lds_block_sync(); // every spectrum published
        const double *xs = X + (size_t)f * G::XPAD + lane; // spectrum of polynomial r: xs + r * 2 * XPAD
        auto products = [&](int u) {
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int r = 0; r < K1; r++) { // |t| <= 1.5 p each: the sum of K1 <= 4 stays below 6 p < 2^53, exact
                const double *xr = xs + (size_t)r * 2 * G::XPAD;
                const double t0 = mulmod<F>(xr[(2 * u) * 64], kw[u][r].x), t1 = mulmod<F>(xr[(2 * u + 1) * 64], kw[u][r].y);
                s0 = r == 0 ? t0 : s0 + t0;
                s1 = r == 0 ? t1 : s1 + t1;
            }
            mine[2 * u] = WIDE ? s0 : reduce<F>(s0);   // (WIDE: |s| <= 4.5 p, what ntt_inverse's WIDE form takes)
            mine[2 * u + 1] = WIDE ? s1 : reduce<F>(s1);
        };
#pragma unroll
        for (int u = 0; u < H; u++) {
            if (u + H / 2 < H) {
                fetch(u + H / 2);
                __builtin_amdgcn_sched_barrier(0);
            }
            products(u);
            __builtin_amdgcn_sched_barrier(0);
        }
        lds_block_sync(); // every wave has read: the scratches are free for the inverse transforms
        // WIDE: the outputs stay unreduced (<= 21 p): the CRT below reduces the DIFFERENCE of the two residues once instead of
        // both residues (X = r0 + p0 t equals the exact integer for any representative r0 with |r0| + |V| + p0 |t| < p0 p1)
        ntt_inverse<F, LOGN, decltype(twi), 0, !WIDE>(mine, xb, twi, lane);
        // ---- CRT: field-f wave lifts slots [f*H, f*H+H) of its polynomial ---------------------
#pragma unroll
        for (int e = 0; e < H; e++) xb[e * 64 + lane] = mine[(1 - f) * H + e];
        lds_block_sync();
#pragma unroll
        for (int e = 0; e < H; e++) {
            const double own = mine[f * H + e], oth = x_field[e * 64 + lane];
            const double r0 = f == 0 ? own : oth, r1 = f == 0 ? oth : own;
            const double t = mulmod<FB>(WIDE ? reduce<FB>(r1 - r0) : r1 - r0, p0inv_mod_p1);
            const uint64_t xv = (uint64_t)to_int64(r0) + FA::P_U64 * (uint64_t)to_int64(t);
            const int j = G::jA(lane, f * H + e);
            if constexpr (C::ACC_X) { // (the upper half of the own scratch: the other waves read only lower halves here)
                acc_own[e] += xv;
                xb_acc[e * 64] = acc_own[e];
            } else {
                const uint64_t nv = acc_p[j] + xv;
                acc_p[j] = nv;
                acc_p[j + N] = 0ull - nv;
            }
        }
        lds_block_sync(); // accumulator complete before the next step's rotated reads; scratch free again
    }
}

template <typename C, typename FA, typename FB>
__global__ __launch_bounds__(64 * C::NW, C::NW / 2) void k_pbs64k(const Pbs64Job *__restrict__ jobs,
                                                          const uint64_t *__restrict__ small, // rows of n+1
                                                          const uint64_t *__restrict__ luts,  // rows of N
                                                          const double *__restrict__ bsk,     // NTT domain, both fields
                                                          const double *__restrict__ tw0, const double *__restrict__ tw1,
                                                          uint64_t *__restrict__ out, // rows of k*N+1
                                                          int n, int logB, double p0inv_mod_p1)
{
    constexpr int LOGN = C::LOGN, K = C::K;
    using G = Geo<LOGN>;
    constexpr int N = G::N, E = G::E, H = E / 2;
    extern __shared__ __align__(16) unsigned char smem[];
    uint64_t *ACC = reinterpret_cast<uint64_t *>(smem + C::ACC_OFF);
    uint16_t *MS = reinterpret_cast<uint16_t *>(smem + C::MS_OFF);
    double *TW = reinterpret_cast<double *>(smem + C::TW_OFF);
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int p = w >> 1, f = w & 1;
    const Pbs64Job job = jobs[blockIdx.x];
    switch_row(MS, job_row(job, small, n), n, tid, 64 * C::NW, LOGN + 1);
    for (int i = tid; i < C::TW_IDX; i += 64 * C::NW) {
        TW[i] = tw0[i];
        TW[C::TW_FIELD + i] = tw1[i];
    }
    for (int r = w; r < G::TWC; r += C::NW) { // lane-table rows of block C
        const int idx = tw_lane_index<LOGN>(G::TWB + r, lane);
        TW[C::TW_IDX + r * 64 + lane] = tw0[idx];
        TW[C::TW_FIELD + C::TW_IDX + r * 64 + lane] = tw1[idx];
    }
    __syncthreads();
    { // accumulator: (0, ..., 0, X^{-b~} * lut)
        const int bt = (int)MS[n];
        const uint64_t *tv = luts + (size_t)job.lut * N;
        for (int j = tid; j < (K + 1) * N; j += 64 * C::NW) {
            const uint64_t v = j >= K * N ? lut_rotated(tv, j - K * N, bt, N) : 0ull;
            const int pp = j / N, jj = j - pp * N;
            if constexpr (C::ACC_X) reinterpret_cast<uint64_t *>(smem + C::X_OFF)[C::acc_x(pp, jj)] = v;
            else {
                ACC[(size_t)pp * C::ACC_LEN + jj] = v;
                ACC[(size_t)pp * C::ACC_LEN + N + jj] = 0ull - v;
            }
        }
    }
    __syncthreads();
    if (f == 0) pbs64k_body<C, FA, FA, FB>(smem, bsk, n, logB, p0inv_mod_p1, p, 0, lane);
    else pbs64k_body<C, FB, FA, FB>(smem, bsk, n, logB, p0inv_mod_p1, p, 1, lane);
    // ---- sample extract; wave (p, f) writes its half of the slots ------
    const uint64_t *acc_p = ACC + (size_t)p * C::ACC_LEN;
    const uint64_t *acc_xp = reinterpret_cast<const uint64_t *>(smem + C::X_OFF);
    auto acc_at = [&](int j) { return C::ACC_X ? acc_xp[C::acc_x(p, j)] : acc_p[j]; };
    sample_extract_outputs<G, K, H>(out, job.out_row, job.pad, p, f * H, f == 0 && lane == 0, lane, acc_at);
}

// ------------------------------------------------------------------------------------
// k_pbs64s<LOGN>: the same bootstrap with EIGHT waves per ciphertext (two per SIMD), L = 1:
// wave w = (polynomial p, field f, half h).  A size-N negacyclic transform splits, after its
// first butterfly stage (pairs j, j + N/2, twiddle psi^(N/2)), into two independent size-N/2
// transforms whose twiddles are slices of the full table: half h, stage with m' groups, group i'
// uses table[2m' + h m' + i'].  So wave (p, f, h) transforms half h with the LOGN-1 machinery of
// ntt_fp64.h on a derived table; by the mirror identity the inverse of half h reads the table of
// half 1-h mirrored.  The halves meet once per step, in the last inverse stage.
// Per step: (1) each of the four waves of a polynomial decomposes a quarter of its coefficients
// and publishes the digits (int32, LDS); (2) stage 1 + half transform + products with the key
// words of its half of the spectrum; other-polynomial sum handed over; (3) half inverse, then ONE
// exchange among the four waves of the polynomial, after which each computes the last stage of a
// quarter of the slots in both fields and lifts them with the CRT (lift_pairs), accumulating.  Five
// workgroup barriers per step, no redundant work except the 16 stage-1 products per lane.
// ------------------------------------------------------------------------------------
// LDS flags between two waves of a workgroup (LDS-only fences, as lds_block_sync: global loads stay in flight).
// set: everything this wave wrote to or read from LDS before is done when the value shows; wait: nothing this wave does
// to LDS afterwards starts before the value was seen.
[[maybe_unused]] __device__ __forceinline__ void lds_flag_set(uint32_t *flag, uint32_t v)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __hip_atomic_store(flag, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
[[maybe_unused]] __device__ __forceinline__ void lds_flag_wait(const uint32_t *flag, uint32_t v)
{
    while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != v) __builtin_amdgcn_s_sleep(1);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// the half transforms of k_pbs64s (a one-transpose form of the 1,024-point half - lane-bit stages through row swaps - was
// bit-identical and measured -0.4 % / +0.7 %: profiles/r03/si_kernel_experiments.txt; removed in round 6)
template <typename F, int LOGH, typename TW, int PRIO, typename HOOK = NoHook>
__device__ __forceinline__ void half_forward(double (&x)[1][Geo<LOGH>::E], double *xb, const TW &tw, int lane,
                                             const HOOK &hook = HOOK())
{
    ntt_forward<F, LOGH, 1, TW, PRIO, HOOK>(x, xb, tw, lane, hook);
}
template <typename F, int LOGH, typename TW, int PRIO, bool CENTRE, typename HOOK = NoHook>
__device__ __forceinline__ void half_inverse(double (&x)[Geo<LOGH>::E], double *xb, const TW &tw, int lane,
                                             const HOOK &hook = HOOK())
{
    ntt_inverse<F, LOGH, TW, PRIO, CENTRE, HOOK>(x, xb, tw, lane, hook);
}

template <int LOGN_, int L_ = 1>
struct Pbs64sCfg {
    static constexpr int LOGN = LOGN_, L = L_, K = 1, K1 = 2, NW = 8;
    using G = Geo<LOGN>;      // decomposition geometry: E coefficients per lane
    using GS = Geo<LOGN - 1>; // half transforms
    static constexpr int MAX_SMALL_N = 1024;
    static constexpr int TW_IDX = GS::N >> GS::BC, TW_PART = TW_IDX + GS::TWC * 64; // per (field, half)
    static constexpr size_t X_OFF = 0;                                              // double [NW][GS::XPAD]
    static constexpr size_t TW_OFF = X_OFF + sizeof(double) * NW * GS::XPAD;        // double [2][2][TW_PART]
    static constexpr size_t ACC_OFF = TW_OFF + sizeof(double) * 4 * TW_PART;        // u64 [K1][N]
    // digits: int32 for one level (23-bit digits), int16 for two (pbs_logB <= 15: |digit| <= 2^14) - the LDS of a CU
    // does not hold two levels of int32 next to the rest at N = 2048
    using dig_t = std::conditional_t<L == 1, int32_t, int16_t>;
    static constexpr size_t DIG_OFF = ACC_OFF + sizeof(uint64_t) * K1 * G::N;       // dig_t [K1][L][N]
    static constexpr size_t MS_OFF = DIG_OFF + sizeof(dig_t) * K1 * L * G::N;       // u16 [n+1]
    static constexpr size_t FLAG_OFF = (MS_OFF + sizeof(uint16_t) * (MAX_SMALL_N + 1) + 15) / 16 * 16; // u32 [2][NW]
    static constexpr size_t BYTES = FLAG_OFF + sizeof(uint32_t) * 2 * NW;
};

// The last inverse stage and the CRT of k_pbs64s, lifted in PAIRS: wave (f, h) owns slots
// [(2 f + h) E/4, + E/4) of BOTH halves of its polynomial - from its own value of the slot and the three others' (other
// half, other field, other field's other half) it computes the last stage of both outputs j and j + N/2 in both fields and
// lifts both.  Against "every wave lifts the slots of its own half": 12 LDS reads per wave instead of 24 (and 12 values
// published instead of 16) in the phase that is bound by the LDS pipe, and the sixteen modular multiplications of the
// (a1 - a0) psi^(N/2) outputs spread evenly over the waves instead of sitting on the h = 1 ones.  Same values.
template <typename C, typename F, int h, bool ADD>
__device__ __forceinline__ void lift_pairs(const double (&mine)[C::GS::E], const double *x_half, const double *x_field,
                                           const double *x_fh, uint64_t *acc_p, int f, double w1, double w1o,
                                           double p0inv_mod_p1, int lane)
{
    using FO = std::conditional_t<std::is_same<F, F0>::value, F1, F0>;
    constexpr int EH = C::GS::E, QS = EH / 4, N = C::G::N;
    const int s0 = (f * 2 + h) * QS;
#pragma unroll
    for (int e = 0; e < QS; e++) {
        const int s = s0 + e;
        const double a = mine[s], o = x_half[s * 64 + lane], a2 = x_field[s * 64 + lane], o2 = x_fh[s * 64 + lane];
        const double e0 = h ? o : a, e1 = h ? a : o, g0 = h ? o2 : a2, g1 = h ? a2 : o2; // halves 0 and 1, own / other field
        // y[j] = a0 + a1 ; y[j + N/2] = (a1 - a0) * psi^(N/2)
        const double own[2] = {reduce<F>(e0 + e1), reduce<F>(mulmod<F>(e1 - e0, w1))};
        const double oth[2] = {reduce<FO>(g0 + g1), reduce<FO>(mulmod<FO>(g1 - g0, w1o))};
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const double r0 = f == 0 ? own[u] : oth[u], r1 = f == 0 ? oth[u] : own[u];
            // The quotient leaves mulmod within (0.5 + 0.75 |r1 - r0| 2^-52) p1 = 0.61 p1, so taken as it comes the lifted
            // value is the exact integer only up to 0.78 of p0 p1 / 2: enough for the classical step (ADD), whose shapes end
            // at 0.71 of it by their creation bound.  The multi-bit group step is admitted by its key up to the half itself
            // (helm_si_load_bootstrap_key) and recentres the quotient, as k_pbs64_generic does.
            const double tq = mulmod<F1>(r1 - r0, p0inv_mod_p1);
            const double t = ADD ? tq : reduce<F1>(tq);
            const uint64_t xv = (uint64_t)to_int64(r0) + F0::P_U64 * (uint64_t)to_int64(t);
            uint64_t *dst = acc_p + u * (N / 2) + s * 64 + lane;
            *dst = ADD ? *dst + xv : xv;
        }
    }
}

template <typename C, typename F, int h, int P>
__device__ __forceinline__ void pbs64s_body(unsigned char *smem, const double *__restrict__ bsk, int n, int logB,
                                            double p0inv_mod_p1, double w1, double w1o, int p, int f, int lane)
{
    constexpr int LOGN = C::LOGN, K1 = C::K1, L = C::L;
    using G = typename C::G;
    using GS = typename C::GS;
    constexpr int N = G::N, E = G::E, EH = GS::E, Q = E / 4, HC = EH / 2;
    // entry priority of the transforms (stepped down block by block inside them)
    constexpr int PH = 3;
    constexpr bool SRC1 = L == 1; // stage 1 where the digits are made (+1.6 %, profiles/r03/si_kernel_experiments.txt)
    double *X = reinterpret_cast<double *>(smem + C::X_OFF);
    uint64_t *ACC = reinterpret_cast<uint64_t *>(smem + C::ACC_OFF);
    using dig_t = typename C::dig_t;
    dig_t *DIG = reinterpret_cast<dig_t *>(smem + C::DIG_OFF);
    const uint16_t *MS = reinterpret_cast<const uint16_t *>(smem + C::MS_OFF);
    auto wave_of = [](int pp, int ff, int hh) { return (pp * 2 + ff) * 2 + hh; };
    double *xb = X + (size_t)wave_of(p, f, h) * GS::XPAD;
    const double *x_poly = X + (size_t)wave_of(1 - p, f, h) * GS::XPAD;  // same field and half, other polynomial
    const double *x_half = X + (size_t)wave_of(p, f, 1 - h) * GS::XPAD;  // same polynomial and field, other half
    const double *x_field = X + (size_t)wave_of(p, 1 - f, h) * GS::XPAD; // same polynomial and half, other field
    uint64_t *acc_p = ACC + (size_t)p * N;
    dig_t *dig_p = DIG + (size_t)p * L * N; // [level][N]
    const double *twt = reinterpret_cast<const double *>(smem + C::TW_OFF);
    const double *tw_own = twt + (size_t)(f * 2 + h) * C::TW_PART, *tw_oth = twt + (size_t)(f * 2 + (1 - h)) * C::TW_PART;
    // block-C twiddles of both transforms in registers where the kernel has them to spare (one level, classical: 176 + 60;
    // +1.2 %, profiles/r03/si_kernel_experiments.txt)
    constexpr bool TWC_REGS = L == 1;
    std::conditional_t<TWC_REGS, TwHybridC<LOGN - 1, false>, TwHybrid<LOGN - 1, false>> twf;
    std::conditional_t<TWC_REGS, TwHybridC<LOGN - 1, true>, TwHybrid<LOGN - 1, true>> twi;
    twf.t = tw_own, twi.t = tw_oth;
    if constexpr (TWC_REGS) {
        twf.load(tw_own + C::TW_IDX + lane);
        twi.load(tw_oth + C::TW_IDX + (63 - lane));
    } else {
        twf.base = tw_own + C::TW_IDX + lane;
        twi.base = tw_oth + C::TW_IDX + (63 - lane);
    }
    const int quarter = f * 2 + h; // which E/4 slots of the polynomial this wave decomposes

    // key words of this wave: [i][row p][c][level][f][h][e/2][lane] as double2
    const size_t part = (size_t)(GS::N / 2);
    const size_t bsk_step = (size_t)K1 * K1 * L * 4 * part;
    const double2 *bsk_w = reinterpret_cast<const double2 *>(bsk) + ((size_t)p * K1 * L * 4 + f * 2 + h) * part + lane;
    const uint32_t half_m1 = (1u << (logB - 1)) - 1u;
    [[maybe_unused]] const uint32_t bmask = (1u << logB) - 1u;

    STAMP_DECL
    for (int i = 0; i < n; i++) {
        const int a = __builtin_amdgcn_readfirstlane((int)MS[i]);
        if (a == 0) continue; // uniform over the workgroup
        STAMP_BEGIN
        [[maybe_unused]] const double2 *bp_i = bsk_w + (size_t)i * bsk_step;
        auto key = [&](int col_lev, int u) { return (bp_i + (size_t)col_lev * 4 * part)[u * 64]; };
        // ---- (1) digits of this wave's quarter of polynomial p -------------------------------
        if constexpr (SRC1) {
            // L = 1: the quarter is Q/2 PAIRS (j, j + N/2); stage 1 of the full transform is done here, once per pair
            // and field (U + V psi^(N/2) for half 0, U - V psi^(N/2) for half 1), and the four results go straight
            // into the transform scratches of the four waves that transform them - no digit buffer, no conversions and
            // no stage-1 product on the consumers' side (they used to compute all sixteen, each half redundantly)
            double *x_f0 = X + (size_t)wave_of(p, f, 0) * GS::XPAD + lane, *x_f1 = X + (size_t)wave_of(p, f, 1) * GS::XPAD + lane;
            double *x_o0 = X + (size_t)wave_of(p, 1 - f, 0) * GS::XPAD + lane, *x_o1 = X + (size_t)wave_of(p, 1 - f, 1) * GS::XPAD + lane;
            auto digit = [&](int j) {
                const int src = (j - a) & (2 * N - 1);
                uint64_t v = acc_p[src & (N - 1)];
                if (src >= N) v = 0ull - v;
                v -= acc_p[j];
                const uint32_t st = (uint32_t)((v + (1ull << (63 - logB))) >> (64 - logB));
                return (double)((int)((st + half_m1) & bmask) - (int)half_m1); // st <= B/2 stays, above it st - B
            };
#pragma unroll
            for (int u = 0; u < Q / 2; u++) {
                const int e = quarter * (Q / 2) + u;
                const double U = digit(G::jA(lane, e)), D1 = digit(G::jA(lane, e + EH));
                const double Vf = stage1_digit_product(D1, w1), Vo = stage1_digit_product(D1, w1o);
                x_f0[e * 64] = U + Vf;
                x_f1[e * 64] = U - Vf;
                x_o0[e * 64] = U + Vo;
                x_o1[e * 64] = U - Vo;
            }
        } else
#pragma unroll
        for (int u = 0; u < Q; u++) {
            const int j = G::jA(lane, quarter * Q + u);
            const int src = (j - a) & (2 * N - 1);
            uint64_t v = acc_p[src & (N - 1)];
            if (src >= N) v = 0ull - v;
            v -= acc_p[j];
            if constexpr (L == 1) {
                const uint32_t st = (uint32_t)((v + (1ull << (63 - logB))) >> (64 - logB));
                // nothing is left above the digit, the carry decides between d and d - B (d > B/2)
                dig_p[j] = (int)st - (int)(((st + half_m1) >> logB) << logB);
            } else { // least significant level first, the one-addition carry rule of pbs64_body
                const int rep = logB * L;
                uint32_t st = (uint32_t)((v + (1ull << (63 - rep))) >> (64 - rep));
#pragma unroll
                for (int lev = L - 1; lev >= 0; lev--) {
                    const uint32_t next = (st + half_m1 + __builtin_amdgcn_ubfe(st, 2 * logB - 1, 1)) >> logB;
                    dig_p[lev * N + j] = (dig_t)((int)st - (int)(next << logB));
                    st = next;
                }
            }
        }
        // first key column of this wave's half (E/4 double2 per column)
        double2 kw[K1][HC];
#pragma unroll
        for (int u = 0; u < HC; u++) kw[0][u] = key(0 * L, u);
        STAMP(0) // quarter decomposition
        lds_block_sync(); // digits published
        STAMP(1) // barrier 1
        // ---- (2) stage 1 of the full transform, half transform, products ---------------------
        // the two waves of a SIMD (polynomials 0 and 1 of one field and half) run every phase together;
        // stepping the issue priority down block by block keeps them abreast, so that neither finishes
        // the phase alone (a lone wave cannot hide its LDS latencies)
        double mine[EH], other[EH];
#pragma unroll
        for (int lev = 0; lev < L; lev++) {
            if (lev > 0) {
#pragma unroll
                for (int u = 0; u < HC; u++) kw[0][u] = key(0 * L + lev, u);
            }
            __builtin_amdgcn_s_setprio(PH);
            double x[1][EH];
            if constexpr (SRC1) {
#pragma unroll
                for (int e = 0; e < EH; e++) x[0][e] = xb[e * 64 + lane];
            } else {
                const dig_t *dg = dig_p + lev * N + lane;
#pragma unroll
                for (int e = 0; e < EH; e++) {
                    const double U = (double)dg[64 * e], V = stage1_digit_product((double)dg[64 * (e + EH)], w1);
                    x[0][e] = h ? U - V : U + V;
                }
            }
            // the second column is asked for between the transform's second transpose and its last block: behind both
            // LDS round trips (fetching it before the transform was measured 1 % slower,
            // profiles/r02/si_kernel_experiments.txt, after it 0.6 %, profiles/r03/si_kernel_experiments.txt), with a
            // block of arithmetic to cover the latency
            auto fetch_kw1 = [&]() {
#pragma unroll
                for (int u = 0; u < HC; u++) kw[1][u] = key(1 * L + lev, u);
            };
            half_forward<F, LOGN - 1, decltype(twf), PH>(x, xb, twf, lane, fetch_kw1);
            __builtin_amdgcn_s_setprio(0);
            if (lev == 0) {
                STAMP(2) // digits read, stage 1, half transform
            }
#pragma unroll
            for (int c = 0; c < K1; c++) {
#pragma unroll
                for (int u = 0; u < HC; u++) {
                    const double t0 = mulmod<F>(x[0][2 * u], kw[c][u].x), t1 = mulmod<F>(x[0][2 * u + 1], kw[c][u].y);
                    if (c == p) {
                        mine[2 * u] = lev == 0 ? t0 : mine[2 * u] + t0;
                        mine[2 * u + 1] = lev == 0 ? t1 : mine[2 * u + 1] + t1;
                    } else {
                        other[2 * u] = lev == 0 ? t0 : other[2 * u] + t0;
                        other[2 * u + 1] = lev == 0 ? t1 : other[2 * u + 1] + t1;
                    }
                }
            }
        }
        // a product is below 1.5 p (mulmod: (0.5 + 0.75 |a| 2^-52) p with |a| <= 9.6 p): the 2 L of a column are
        // summed as they are and recentred once (L <= 2: below 6 p)
#pragma unroll
        for (int e = 0; e < EH; e++) xb[e * 64 + lane] = other[e];
        STAMP(3) // products
        lds_block_sync();
#pragma unroll
        for (int e = 0; e < EH; e++) mine[e] = reduce<F>(mine[e] + x_poly[e * 64 + lane]);
        lds_block_sync(); // hand-over read: scratch free again
        STAMP(4) // barrier 2, sum, barrier 3
        // ---- (3) half inverse, meet the other half, last stage -------------------------------
        __builtin_amdgcn_s_setprio(PH);
        // a_h[e * 64 + lane], uncentred: the last stage recentres anyway (centring here measured 1.3 % slower,
        // profiles/r03/si_kernel_experiments.txt)
        half_inverse<F, LOGN - 1, decltype(twi), PH, false>(mine, xb, twi, lane);
        __builtin_amdgcn_s_setprio(0);
        STAMP(5) // half inverse
        // ---- (3b, 4) one exchange for the last inverse stage and the CRT (two barriers instead of four): every wave
        //      publishes its half inverse, and lift_pairs computes the last stage of its slots in both fields and lifts them
#pragma unroll
        for (int e = 0; e < EH; e++)
            if (e / (EH / 4) != f * 2 + h) xb[e * 64 + lane] = mine[e]; // own slots stay
        lds_block_sync();
        lift_pairs<C, F, h, true>(mine, x_half, x_field, X + (size_t)wave_of(p, 1 - f, 1 - h) * GS::XPAD, acc_p, f, w1, w1o,
                                  p0inv_mod_p1, lane);
        lds_block_sync(); // accumulator complete, scratch free again
        STAMP(7) // last stage and CRT, barriers 4 and 5
    }
    STAMP_END((p * 2 + f) * 2 + h)
}

__host__ __device__ constexpr int bitrev_c(int v, int bits)
{
    int r = 0;
    for (int b = 0; b < bits; b++) r |= ((v >> b) & 1) << (bits - 1 - b);
    return r;
}

// Multi-bit blind rotation (tfhe MultiBitPBS, grouping factor g <= 3; reference src/bin/helm.rs:83 installs
// the g = 3 set for arithmetic mode): per group of g mask words ONE external product
//     acc <- ( sum_S X^(e_S) * GGSW_S ) (x) acc,      e_S = sum_{i in S} a~_i,
// evaluated as  sum_S ( NTT(digits(acc)) .* M(e_S) ) .* K_S  in the transform domain: multiplying by the monomial
// X^e is a pointwise product with M(e)[j] = psi^(expo[j] * e), expo[j] the (odd) exponent of the evaluation
// point of spectrum position j (probed once per context through the key-conversion kernel) and psi_pow the 2N
// powers of psi.  Same wave roles, transforms, hand-over and CRT as pbs64s_body; n/g steps instead of n, the
// accumulator is replaced instead of added to.
template <typename C, typename F, int h, int P>
__device__ __forceinline__ void pbs64s_mb_body(unsigned char *smem, const double *__restrict__ bsk, int n, int logB,
                                               double p0inv_mod_p1, double w1, double w1o, int p, int f, int lane, int g,
                                               const uint16_t *__restrict__ expo, const double *__restrict__ psi_pow)
{
    constexpr int LOGN = C::LOGN, K1 = C::K1;
    using G = typename C::G;
    using GS = typename C::GS;
    constexpr int PH = 3;
    constexpr int N = G::N, E = G::E, EH = GS::E, Q = E / 4, HC = EH / 2;
    double *X = reinterpret_cast<double *>(smem + C::X_OFF);
    uint64_t *ACC = reinterpret_cast<uint64_t *>(smem + C::ACC_OFF);
    using dig_t = typename C::dig_t;
    dig_t *DIG = reinterpret_cast<dig_t *>(smem + C::DIG_OFF);
    const uint16_t *MS = reinterpret_cast<const uint16_t *>(smem + C::MS_OFF);
    auto wave_of = [](int pp, int ff, int hh) { return (pp * 2 + ff) * 2 + hh; };
    double *xb = X + (size_t)wave_of(p, f, h) * GS::XPAD;
    const double *x_poly = X + (size_t)wave_of(1 - p, f, h) * GS::XPAD;
    const double *x_half = X + (size_t)wave_of(p, f, 1 - h) * GS::XPAD;
    const double *x_field = X + (size_t)wave_of(p, 1 - f, h) * GS::XPAD;
    uint64_t *acc_p = ACC + (size_t)p * N;
    [[maybe_unused]] dig_t *dig_p = DIG + (size_t)p * N;
    const double *twt = reinterpret_cast<const double *>(smem + C::TW_OFF);
    const double *tw_own = twt + (size_t)(f * 2 + h) * C::TW_PART, *tw_oth = twt + (size_t)(f * 2 + (1 - h)) * C::TW_PART;
    TwHybrid<LOGN - 1, false> twf{tw_own, tw_own + C::TW_IDX + lane};
    TwHybrid<LOGN - 1, true> twi{tw_oth, tw_oth + C::TW_IDX + (63 - lane)};
    const int quarter = f * 2 + h;
    const size_t part = (size_t)(GS::N / 2);
    const size_t bsk_step = (size_t)K1 * K1 * 4 * part; // one GGSW
    const uint32_t half_m1 = (1u << (logB - 1)) - 1u;
    [[maybe_unused]] const uint32_t bmask = (1u << logB) - 1u;
    const int subsets = 1 << g;
    // exponent of this lane's first spectrum position (slot e = 0 of the key-word order)
    const int c_lane = (int)expo[((size_t)h * HC * 64 + lane) * 2];
    // omega^k, k < EH (omega = psi^(2N/EH)), held by lane k: read with v_readlane by a uniform index
    const double om_tab = psi_pow[(lane & (EH - 1)) * (2 * N / EH)];
    const int om_lo = __double2loint(om_tab), om_hi = __double2hiint(om_tab);
    // key words through buffer loads: descriptor in scalar registers, scalar byte offset per (group, subset, column)
    const unsigned ggsw_bytes = (unsigned)(bsk_step * 16), col_bytes = (unsigned)(4 * part * 16);
    const unsigned wave_off = (unsigned)(((size_t)p * K1 * 4 + f * 2 + h) * part * 16);
    KeyBuf kbuf;
    kbuf.init(bsk, (size_t)(n / g) * subsets * ggsw_bytes, lane);
    for (int t = 0; t < n / g; t++) {
        int am[3];
#pragma unroll
        for (int q = 0; q < 3; q++) am[q] = q < g ? __builtin_amdgcn_readfirstlane((int)MS[t * g + q]) : 0;
        // psi^(c_lane a_q) of the group's members: in flight during the decomposition and the transform
        double bq[3];
#pragma unroll
        for (int q = 0; q < 3; q++) bq[q] = psi_pow[(c_lane * am[q]) & (2 * N - 1)];
        // ---- (1) digits of this wave's quarter of polynomial p ----------------------------------
#pragma unroll
        for (int u = 0; u < Q; u++) {
            const int j = G::jA(lane, quarter * Q + u);
            const uint64_t v = acc_p[j];
            const uint32_t st = (uint32_t)((v + (1ull << (63 - logB))) >> (64 - logB));
            dig_p[j] = (int)st - (int)(((st + half_m1) >> logB) << logB);
        }
        lds_block_sync(); // digits published
        // ---- (2) stage 1 of the full transform, half transform ----------------------------------
        __builtin_amdgcn_s_setprio(PH);
        double x[1][EH];
        {
            const dig_t *dg = dig_p + lane;
#pragma unroll
            for (int e = 0; e < EH; e++) {
                const double U = (double)dg[64 * e], V = stage1_digit_product((double)dg[64 * (e + EH)], w1);
                x[0][e] = h ? U - V : U + V;
            }
        }
        half_forward<F, LOGN - 1, decltype(twf), PH>(x, xb, twf, lane);
        __builtin_amdgcn_s_setprio(0);
        // ---- the group's key in the transform domain, G[c] = sum_S M(e_S) .* K_S[p][c], in NESTED form, and the products
        //      x .* G[c].  M(e_S) is the product of its members' monomial vectors M_i = M(a~_i), so
        //        G = (K_000 + M_0 K_001) + M_1 (K_010 + M_0 K_011) + M_2 [(K_100 + M_0 K_101) + M_1 (K_110 + M_0 K_111)]:
        //      2^g - 1 modular multiplications per spectrum position and column instead of 2 (2^g - 1) (one per subset for
        //      the monomial's own value, one with the key word), plus g per position for the M_i.  The spectrum positions
        //      of a lane are expo(lane, e) = c_lane + (2N/EH) rev(e), so M_i[e] = psi^(c_lane a~_i) * omega^(a~_i rev(e)):
        //      one gathered power per lane and member (bq, fetched at the top of the step) times a wave-uniform power of
        //      omega read out of a lane-held table with v_readlane.  Walked slot pair by slot pair and column by column:
        //      the 2^g key words of one (slot pair, column) are fetched one iteration ahead (buffer loads: scalar offsets).
        //      (The flat sum, one product per subset, measured 16.6 % slower: profiles/r03/si_kernel_experiments.txt.)
        static_assert(K1 == 2, "two key columns");
        double mine[EH], oth[EH];
        auto key_products = [&](auto g_const) {
            constexpr int GG = decltype(g_const)::value, SUB = 1 << GG; // compile-time group size: no branches in the walk
            const unsigned so_t = (unsigned)t * (unsigned)SUB * ggsw_bytes + wave_off;
            double2 kq[2][SUB];
            auto fetch = [&](int it, double2 (&dst)[SUB]) { // it = 2 u + c
                const int u = it >> 1, c = it & 1;
#pragma unroll
                for (int S = 0; S < SUB; S++)
                    dst[S] = kbuf.load(so_t + (unsigned)S * ggsw_bytes + (unsigned)c * col_bytes + (unsigned)(u >> 2) * 4096u, (u & 3) * 1024);
            };
            fetch(0, kq[0]);
            double m[GG][2];
#pragma unroll
            for (int it = 0; it < 2 * HC; it++) {
                const int u = it >> 1, c = it & 1;
                if (it + 1 < 2 * HC) fetch(it + 1, kq[(it + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
                if (c == 0) { // the members' monomial values at the two positions of this slot pair
#pragma unroll
                    for (int q = 0; q < GG; q++)
#pragma unroll
                        for (int z = 0; z < 2; z++) {
                            const int k = (am[q] * bitrev_c(2 * u + z, GS::LOGE)) & (EH - 1);
                            const double om = __hiloint2double(__builtin_amdgcn_readlane(om_hi, k), __builtin_amdgcn_readlane(om_lo, k));
                            m[q][z] = mulmod<F>(bq[q], om);
                        }
                }
                // |K| <= 0.5 p, |M| <= 0.56 p: 1.1 p, 1.8 p, 2.4 p after the three levels - far below 2^53 = 14.2 p
                double2(&v)[SUB] = kq[it & 1];
#pragma unroll
                for (int q = 0; q < GG; q++)
#pragma unroll
                    for (int S = 0; S < SUB; S++)
                        if (!(S & ((2 << q) - 1))) {
                            v[S].x += mulmod<F>(v[S | (1 << q)].x, m[q][0]);
                            v[S].y += mulmod<F>(v[S | (1 << q)].y, m[q][1]);
                        }
                const double c0 = mulmod<F>(x[0][2 * u], reduce<F>(v[0].x)), c1 = mulmod<F>(x[0][2 * u + 1], reduce<F>(v[0].y)); // <= 1.5 p
                if (c == p) {
                    mine[2 * u] = c0;
                    mine[2 * u + 1] = c1;
                } else {
                    oth[2 * u] = c0;
                    oth[2 * u + 1] = c1;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        if (g == 3) key_products(std::integral_constant<int, 3>());
        else key_products(std::integral_constant<int, 2>());
#pragma unroll
        for (int e = 0; e < EH; e++) xb[e * 64 + lane] = oth[e];
        lds_block_sync();
#pragma unroll
        for (int e = 0; e < EH; e++) mine[e] = reduce<F>(mine[e] + x_poly[e * 64 + lane]); // <= 11.4 p before
        lds_block_sync(); // hand-over read: scratch free again
        // ---- (3) half inverse, meet the other half, last stage -----------------------------------
        __builtin_amdgcn_s_setprio(PH);
        half_inverse<F, LOGN - 1, decltype(twi), PH, false>(mine, xb, twi, lane); // uncentred, as in pbs64s_body
        __builtin_amdgcn_s_setprio(0);
#pragma unroll
        for (int e = 0; e < EH; e++)
            if (e / (EH / 4) != f * 2 + h) xb[e * 64 + lane] = mine[e]; // own slots stay
        lds_block_sync();
        // the lifted value REPLACES the accumulator
        lift_pairs<C, F, h, false>(mine, x_half, x_field, X + (size_t)wave_of(p, 1 - f, 1 - h) * GS::XPAD, acc_p, f, w1, w1o,
                                   p0inv_mod_p1, lane);
        lds_block_sync(); // accumulator complete, scratch free again
    }
}

template <typename C, bool MB>
__global__ __launch_bounds__(64 * C::NW, 1) void k_pbs64s(const Pbs64Job *__restrict__ jobs,
                                                          const uint64_t *__restrict__ small,
                                                          const uint64_t *__restrict__ luts,
                                                          const double *__restrict__ bsk,    // split layout
                                                          const double *__restrict__ tw_sub, // [2 fields][2 halves][N/2]
                                                          const double *__restrict__ tw0, const double *__restrict__ tw1,
                                                          uint64_t *__restrict__ out, int n, int logB,
                                                          double p0inv_mod_p1, int g,
                                                          const uint16_t *__restrict__ expo, // multi-bit: [2 halves][N/2]
                                                          const double *__restrict__ psi_pow) // multi-bit: [2 fields][2N]
{
    constexpr int LOGN = C::LOGN, K = C::K;
    using G = typename C::G;
    using GS = typename C::GS;
    constexpr int N = G::N, E = G::E;
    extern __shared__ __align__(16) unsigned char smem[];
    uint64_t *ACC = reinterpret_cast<uint64_t *>(smem + C::ACC_OFF);
    uint16_t *MS = reinterpret_cast<uint16_t *>(smem + C::MS_OFF);
    double *TW = reinterpret_cast<double *>(smem + C::TW_OFF);
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the waves of polynomial 1 take the halves the other way round: each SIMD (wave index mod 4) then holds one wave of
    // either half - the last inverse stage costs the h = 1 waves sixteen modular multiplications more than the h = 0 waves
    // (+1.2 %, profiles/r03/si_kernel_experiments.txt)
    const int p = w >> 2, f = (w >> 1) & 1, h = (w & 1) ^ p;
    const Pbs64Job job = jobs[blockIdx.x];
    switch_row(MS, job_row(job, small, n), n, tid, 64 * C::NW, LOGN + 1);
    if (tid < 2 * C::NW) reinterpret_cast<uint32_t *>(smem + C::FLAG_OFF)[tid] = 0u;
    // derived tables: index part for blocks A, B and lane table for block C, per (field, half)
    for (int q = 0; q < 4; q++) {
        const double *src = tw_sub + (size_t)q * GS::N;
        double *dst = TW + (size_t)q * C::TW_PART;
        for (int i = tid; i < C::TW_IDX; i += 64 * C::NW) dst[i] = src[i];
        for (int r = w; r < GS::TWC; r += C::NW) dst[C::TW_IDX + r * 64 + lane] = src[tw_lane_index<LOGN - 1>(GS::TWB + r, lane)];
    }
    __syncthreads();
    {
        const int bt = (int)MS[n];
        const uint64_t *tv = luts + (size_t)job.lut * N;
        for (int j = tid; j < (K + 1) * N; j += 64 * C::NW) ACC[j] = j >= K * N ? lut_rotated(tv, j - K * N, bt, N) : 0ull;
    }
    __syncthreads();
    // psi^(N/2): entry 1 of the full forward table of this wave's field
    const double w1 = f == 0 ? tw0[1] : tw1[1], w1o = f == 0 ? tw1[1] : tw0[1];
    // one specialisation per (field, transform half, polynomial): all three are uniform over the wave
    // (the polynomial as a literal too: the bodies are inlined, so `c == p` in the products and the row offsets fold - 66
    // v_cndmask per wave-step gone from the classical kernel, +3.4 %, profiles/r03/si_kernel_experiments.txt)
#define HELM_SI_BODY(FN, FT, HH, FF, ...)                                                                                    \
    do {                                                                                                                     \
        if (p == 0) FN<C, FT, HH, 0>(smem, bsk, n, logB, p0inv_mod_p1, w1, w1o, 0, FF, lane, ##__VA_ARGS__);                 \
        else FN<C, FT, HH, 1>(smem, bsk, n, logB, p0inv_mod_p1, w1, w1o, 1, FF, lane, ##__VA_ARGS__);                        \
    } while (0)
    if constexpr (MB) {
        if (f == 0) {
            if (h == 0) HELM_SI_BODY(pbs64s_mb_body, F0, 0, 0, g, expo, psi_pow);
            else HELM_SI_BODY(pbs64s_mb_body, F0, 1, 0, g, expo, psi_pow);
        } else {
            if (h == 0) HELM_SI_BODY(pbs64s_mb_body, F1, 0, 1, g, expo, psi_pow + 2 * N);
            else HELM_SI_BODY(pbs64s_mb_body, F1, 1, 1, g, expo, psi_pow + 2 * N);
        }
    } else if (f == 0) {
        if (h == 0) HELM_SI_BODY(pbs64s_body, F0, 0, 0);
        else HELM_SI_BODY(pbs64s_body, F0, 1, 0);
    } else {
        if (h == 0) HELM_SI_BODY(pbs64s_body, F1, 0, 1);
        else HELM_SI_BODY(pbs64s_body, F1, 1, 1);
    }
#undef HELM_SI_BODY

    // ---- sample extract; wave (p, f, h) writes its quarter of the slots ------
    const uint64_t *acc_p = ACC + (size_t)p * N;
    const int quarter = f * 2 + h;
    sample_extract_outputs<G, K, E / 4>(out, job.out_row, job.pad, p, quarter * (E / 4), w == K * 4 && lane == 0, lane,
                                        [&](int j) { return acc_p[j]; });
}

// key conversion for k_pbs64s: standard-domain u64 -> field F, stage 1 + half transform h, times N^-1:
//   dst[i][r][c][lev][f][h][e/2][lane][e&1]    (src is [i][lev][r][c][N]); one wave per (polynomial, half)
template <typename F, int LOGN>
__global__ __launch_bounds__(64) void k_bsk_convert64s(const uint64_t *__restrict__ src, double *__restrict__ dst,
                                                       const double *__restrict__ tw_full, const double *__restrict__ tw_sub_f,
                                                       double n_inv, double two32, int K1, int f, int L)
{
    using G = Geo<LOGN>;
    using GS = Geo<LOGN - 1>;
    constexpr int N = G::N, EH = GS::E;
    __shared__ double xbuf[GS::XPAD];
    const int lane = threadIdx.x;
    const size_t poly = blockIdx.x >> 1;
    const int h = blockIdx.x & 1;
    const int c = poly % K1;
    const int r = (poly / K1) % K1;
    const int lev = (poly / ((size_t)K1 * K1)) % L;
    const size_t i = poly / ((size_t)K1 * K1 * L);
    const double w1 = tw_full[1];
    auto load = [&](int j) {
        const uint64_t v = src[poly * N + j];
        const double hi = (double)(int32_t)(uint32_t)(v >> 32), lo = (double)(uint32_t)v;
        return reduce<F>(mulmod<F>(hi, two32) + lo);
    };
    double x[1][EH];
#pragma unroll
    for (int e = 0; e < EH; e++) {
        const double U = load(e * 64 + lane), V = mulmod<F>(load(e * 64 + lane + N / 2), w1);
        x[0][e] = reduce<F>(h ? U - V : U + V);
    }
    ntt_forward<F, LOGN - 1, 1>(x, xbuf, TwMem{tw_sub_f + (size_t)h * GS::N}, lane);
    const size_t dpoly = (((((i * K1 + r) * K1 + c) * L + lev) * 2 + f) * 2 + h);
    double *d = dst + dpoly * GS::N;
#pragma unroll
    for (int e = 0; e < EH; e++) d[((e >> 1) * 64 + lane) * 2 + (e & 1)] = reduce<F>(mulmod<F>(x[0][e], n_inv));
}

// ------------------------------------------------------------------------------------
// The keyswitch kernels, big LWE (k*N) -> small LWE (n): wrappers over the bodies of keyswitch.h for Ks64Job rows.
//   k_keyswitch64                     vector-ALU form, four ciphertexts per key pass
//   k_ks64_digits / k_ks64_mfma       matrix-core form: the level count padded to LP in {1, 2, 4, 8}, the key's EIGHT byte
//                                     planes; one wave = 64 ciphertexts x 16 key columns x 8 planes (128 accumulator registers)
// ------------------------------------------------------------------------------------
struct Ks64Rows {
    using Job = Ks64Job;
    using Word = uint64_t;
    const uint64_t *in;
    __device__ __forceinline__ Ks64Rows(const Ks64Job &job, const uint64_t *big, size_t row) : in(big + row * (size_t)job.in_row) {}
    __device__ __forceinline__ uint64_t word(int t) const { return in[t]; }
    __device__ __forceinline__ uint64_t body(int kN) const { return in[kN]; }
    static __device__ __forceinline__ int out_row(const Ks64Job &job, int) { return job.out_row; }
};
constexpr int ks64_padded_levels(int ks_l) { return ks_l <= 1 ? 1 : ks_l <= 2 ? 2 : ks_l <= 4 ? 4 : 8; }

template <int KSL>
__global__ __launch_bounds__(256) void k_keyswitch64(const Ks64Job *__restrict__ jobs, const uint64_t *__restrict__ big,
                                                     const uint64_t *__restrict__ ksk, uint64_t *__restrict__ out,
                                                     int n, int kN, int logB, int count, int t_chunk)
{
    helm_ks::vector_body<KSL, Ks64Rows>(jobs, big, ksk, out, n, kN, logB, count, t_chunk);
}

template <int KSL>
__global__ __launch_bounds__(256) void k_ks64_digits(const Ks64Job *__restrict__ jobs, const uint64_t *__restrict__ big,
                                                     int8_t *__restrict__ dig, int32_t *__restrict__ dsum,
                                                     uint64_t *__restrict__ body, int kN, int logB, int count, int kchunks)
{
    helm_ks::digits_body<KSL, ks64_padded_levels(KSL), Ks64Rows>(jobs, big, dig, dsum, body, kN, logB, count, kchunks);
}

__global__ __launch_bounds__(64) void k_ks64_mfma(const Ks64Job *__restrict__ jobs, const int8_t *__restrict__ dig,
                                                  const int32_t *__restrict__ dsum, const uint64_t *__restrict__ body,
                                                  const int8_t *__restrict__ kplanes, uint64_t *__restrict__ out, int n,
                                                  int count, int kchunks, int ctiles)
{
    helm_ks::product_body<1, Ks64Rows>(jobs, dig, dsum, body, kplanes, out, n, count, kchunks, ctiles);
}

// out row = sum coef * in rows + const (body only).  One workgroup per output row.
__global__ __launch_bounds__(256) void k_lincomb64(const int32_t *__restrict__ in_idx, const int64_t *__restrict__ coef,
                                                   const uint64_t *__restrict__ body_add,
                                                   const int32_t *__restrict__ out_idx, const uint64_t *__restrict__ src,
                                                   uint64_t *__restrict__ dst, int terms, int dim)
{
    const int g = blockIdx.x;
    const size_t row = (size_t)dim + 1;
    uint64_t *o = dst + row * (size_t)(out_idx ? out_idx[g] : g);
    for (int i = threadIdx.x; i <= dim; i += 256) {
        uint64_t v = i == dim ? body_add[g] : 0ull;
        for (int t = 0; t < terms; t++) {
            const int r = in_idx[(size_t)g * terms + t];
            if (r >= 0) v += (uint64_t)coef[(size_t)g * terms + t] * src[row * (size_t)r + i];
        }
        o[i] = v;
    }
}

// a gate of a level must not read a row another gate of the level writes; in-place rows
// (out == in of the SAME gate) are common in the radix layer, so sums go through a staging
// buffer first when asked to
__global__ __launch_bounds__(256) void k_rows64(const uint64_t *__restrict__ src, const int32_t *__restrict__ src_row,
                                                uint64_t *__restrict__ dst, const int32_t *__restrict__ dst_row,
                                                int dim)
{
    const size_t row = (size_t)dim + 1;
    const int s = src_row ? src_row[blockIdx.x] : (int)blockIdx.x;
    const int d = dst_row ? dst_row[blockIdx.x] : (int)blockIdx.x;
    if (d < 0) return;
    for (int i = threadIdx.x; i <= dim; i += 256) dst[row * (size_t)d + i] = s < 0 ? 0ull : src[row * (size_t)s + i];
}

__global__ __launch_bounds__(256) void k_set_trivial64(const int32_t *__restrict__ idx, const uint64_t *__restrict__ body,
                                                       uint64_t *__restrict__ wires, int dim)
{
    const size_t row = (size_t)dim + 1;
    uint64_t *dst = wires + row * (size_t)idx[blockIdx.x];
    for (int i = threadIdx.x; i <= dim; i += 256) dst[i] = i == dim ? body[blockIdx.x] : 0ull;
}

// standard-domain u64 (taken as signed) -> NTT domain of field F, times N^-1, in the lane
// order k_pbs64 reads: dst[i][r][c][lev][f][e/2][lane][e&1]   (src is [i][lev][r][c][N])
template <typename F, int LOGN>
__global__ __launch_bounds__(64) void k_bsk_convert64(const uint64_t *__restrict__ src, double *__restrict__ dst,
                                                      const double *__restrict__ tw_fwd, double n_inv, double two32,
                                                      int K1, int L, int f)
{
    using G = Geo<LOGN>;
    constexpr int N = G::N, E = G::E;
    __shared__ double xbuf[G::XPAD];
    const int lane = threadIdx.x;
    const size_t poly = blockIdx.x;
    const int c = poly % K1;
    const int r = (poly / K1) % K1;
    const int lev = (poly / ((size_t)K1 * K1)) % L;
    const size_t i = poly / ((size_t)K1 * K1 * L);
    double x[1][E];
#pragma unroll
    for (int e = 0; e < E; e++) {
        const uint64_t v = src[poly * N + G::jA(lane, e)];
        // v = hi * 2^32 + lo with hi signed: reduce in the field
        const double hi = (double)(int32_t)(uint32_t)(v >> 32), lo = (double)(uint32_t)v;
        x[0][e] = reduce<F>(mulmod<F>(hi, two32) + lo);
    }
    ntt_forward<F, LOGN, 1>(x, xbuf, TwMem{tw_fwd}, lane);
    const size_t dpoly = (((i * K1 + r) * K1 + c) * L + lev) * 2 + f;
    double *d = dst + dpoly * N;
#pragma unroll
    for (int e = 0; e < E; e++) d[((e >> 1) * 64 + lane) * 2 + (e & 1)] = reduce<F>(mulmod<F>(x[0][e], n_inv));
}

// ------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------
template <typename T> struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    int ensure(size_t n)
    {
        if (n <= cap) return 0;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = std::max(n + n / 2, (size_t)64);
        if (hipMalloc(&p, want * sizeof(T)) != hipSuccess) return -1;
        cap = want;
        return 0;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

} // namespace

struct helm_si_wires {
    helm_si_ctx *owner;
    uint64_t *d;
    int64_t n_rows;
};

// Which bootstrap kernel a context runs: decided once, by si_admit() from (params, flags), and only read afterwards (the
// setup of the class at creation, convert_bootstrap_key and launch_pbs64 switch on it; the table of forms is at
// convert_bootstrap_key and in DESIGN.md 4.4.3).
enum SiClass { SI_TUNED = 0, SI_GENERIC = 1, SI_LARGE = 2, SI_N8192 = 3 }; // the values helm_si_kernel_class returns
enum SiForm {
    SI_NO_FORM,  // classes 1 to 3: one kernel each
    SI_WIDE,     // k_pbs64: N = 512 at k = 1, two levels with wide digits, HELM_SI_SPLIT=0
    SI_SPLIT,    // k_pbs64s<., false>: k = 1, N >= 1024, grouping 1
    SI_SPLIT_MB, // k_pbs64s<., true>: grouping > 1
    SI_K         // k_pbs64k: k = 2 or 3
};
struct SiKernelForm {
    SiClass cls = SI_TUNED;
    SiForm form = SI_WIDE; // of class 0
    bool split_key() const { return form == SI_SPLIT || form == SI_SPLIT_MB; } // reads bsk_split through tw_sub
};

// What a key load decides: the tables of the CRT pair, the keys in their device layouts and the settings that go with them.
// A primary context owns one (helm_si_ctx::own_keys); a lane holds its primary's, so a key loaded into the primary - which
// may move the pair and rewrite every table - is what each lane launches with from then on.
struct SiKeyState {
    SiKernelForm run;            // helm_si_ctx_create_ex: what every bootstrap launch of the context and its lanes runs
    double *tw[2] = {nullptr, nullptr};
    double n_inv[2] = {0, 0}, two32[2] = {0, 0};
    double p0inv_mod_p1 = 0;
    int pair = 0;                // CRT pair of the tables above: 0 = FpG / FpG2 (49 bits), 1 = FpJ / FpJ2 (46 bits: k_pbs64k contexts
                                 // whose loaded key fits, helm_si_load_bootstrap_key), 2 = FpG / FpI (k_pbs64_large: N = 4096,
                                 // k_pbs64_n8192: N = 8192)
    double *bsk = nullptr;
    double *bsk_split = nullptr; // layout of k_pbs64s (N >= 1024, pbs_l = 1)
    double *tw_sub = nullptr;    // derived half-transform tables [2 fields][2 halves][N/2]
    int group = 1;               // multi-bit grouping factor (1: classical blind rotation)
    uint16_t *expo = nullptr;    // multi-bit: exponent of the evaluation point per spectrum position [2 halves][N/2]
    double *psi_pow = nullptr;   // multi-bit: psi^t, t < 2N, per field
    // classes 1 to 3 (setup_generic, setup_large, setup_n8192): the launch sizing of the class's kernel and its inverse tables
    size_t lds = 0;                       // LDS bytes per workgroup (TwoPrimeLds<uint64_t>, Large64Lds, N8192Lds)
    int per_cu = 1;                       // resident workgroups per CU at lds (class 3: 1, launch_pbs64_n8192)
    int gen_d = 1;                        // class 1: digit polynomials per batch (tp_batch, tp_fit)
    double *twi[2] = {nullptr, nullptr};  // bit-reversed powers of psi^-1 per field (the kernels' inverse transforms)
    uint64_t *ksk = nullptr;
    int8_t *ksk_planes = nullptr; // matrix-core keyswitch: eight byte planes as signed bytes, B-fragment order
    int ks_kchunks = 0, ks_ctiles = 0, ks_mfma = 1; // HELM_HIP_KS_MFMA=0: the vector-ALU keyswitch for every launch
    bool have_bsk = false, have_ksk = false;
    SiKeyState() = default;
    SiKeyState(const SiKeyState &) = delete;
    SiKeyState &operator=(const SiKeyState &) = delete;
    ~SiKeyState() // (the owner's device is current: helm_si_ctx_destroy)
    {
        for (void *p : {(void *)tw[0], (void *)tw[1], (void *)twi[0], (void *)twi[1], (void *)tw_sub, (void *)bsk,
                        (void *)bsk_split, (void *)expo, (void *)psi_pow, (void *)ksk, (void *)ksk_planes})
            (void)hipFree(p);
    }
};

struct helm_si_ctx {
    int device = 0;
    helm_si_ctx *lane_of = nullptr;     // helm_si_ctx_fork(): the primary this lane was forked from
    std::vector<helm_si_ctx *> lanes;   // of a primary: its lanes (a key load waits for the stream of each)
    std::unique_ptr<SiKeyState> own_keys; // of a primary
    SiKeyState *keys = nullptr;         // own_keys, or the primary's: the one place shared state is read from
    helm_si_params P{};
    int logN = 0;
    // helm_si_pbs_order: 1 = keyswitch, then bootstrap (table rows under the big key), 0 = bootstrap, then keyswitch
    // (HELM_SI_CREATE_PBS_KS: table rows under the small key).  The one place the width of a wire row comes from.
    int order = 1;
    size_t wire_dim() const { return order ? (size_t)P.k * P.N : (size_t)P.n; } // mask words of a wire row
    size_t wire_row() const { return wire_dim() + 1; }
    hipStream_t own_stream = nullptr, stream = nullptr;
    bool high_priority = false; // own_stream was created at the device's highest priority (helm_si_set_priority)
    DevBuf<int8_t> d_ksdig;
    DevBuf<int32_t> d_ksdsum;
    DevBuf<uint64_t> d_ksbody;
    uint64_t delta = 0;
    int n_cus = 256;
    int64_t round_capacity = 0; // bootstraps resident at once (CUs x workgroups per CU of the set's kernel), probed on first need
    // per-call scratch
    DevBuf<Pbs64Job> d_pbs;
    DevBuf<Ks64Job> d_ks;
    DevBuf<uint64_t> d_small, d_luts, d_stage, d_body;
    DevBuf<int32_t> d_idx, d_idx2;
    DevBuf<int64_t> d_coef;
    // k_pbs64_n8192: the accumulator rows of this context's launches, [n_cus][2][N] words, allocated when the context is made
    // (alloc_acc8192).  A lane has its own (it launches on its own stream); launches of one context follow each other on its
    // stream, so they share the rows.
    uint64_t *d_acc8192 = nullptr;
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pbs, ev_ks, ev_lin;
    helm_si_timing tacc{};
    std::vector<helm_si_wires *> child_wires; // released with the context (see helm_hip.hip)
    // Call slots: helm_si_lincomb / helm_si_apply_luts copy their index arrays into a slot's pinned arena, issue ONE
    // asynchronous copy of it and launch - no stream synchronisation inside the call, so the host plans the next
    // batched round of the radix layer while the GPU runs this one (a round used to leave the GPU idle for ~1 ms of
    // host planning, copies and synchronisations out of ~8 ms).  A slot is reused three calls later, after its event.
    struct CallSlot {
        char *host = nullptr, *dev = nullptr;
        size_t cap = 0, used = 0;
        hipEvent_t done = nullptr;
        bool busy = false;
    } slots[3];
    int next_slot = 0;
    uint64_t luts_hash = 0; // of the look-up tables resident in d_luts (re-uploaded only when they change)
    std::vector<uint64_t> luts_host; // host copy of the resident tables: compared word for word when the hash matches
    size_t luts_words = 0;
    // multi-GPU (helm_si_set_exchange): every bootstrap batch of at least x_min ciphertexts is split
    // into x_world contiguous chunks, this rank bootstraps chunk x_rank into x_stage, the caller's
    // collective fills x_gather with every rank's chunk and the rows are scattered into the table
    // helm_si_set_audit: every helm_si_lincomb / helm_si_apply_luts call hands its operand rows and results to the host
    helm_si_audit_fn audit_fn = nullptr;
    void *audit_user = nullptr;
    bool level_many = false; // helm_si_set_level_many_lut: the gates of a LUT level that share an input tuple share a rotation
    int x_rank = 0, x_world = 1;
    int64_t x_min = 0, x_cap = 0;
    uint64_t *x_stage = nullptr, *x_gather = nullptr;
    helm_si_exchange_fn x_fn = nullptr;
    void *x_user = nullptr;
    // helm_si_set_exchange_comm: the collective is the library's own ncclAllGather through x_comm; the gather buffer is
    // the context's (x_own), this rank's chunk is computed straight into its slot of it (all-gather in place)
    helm_comm *x_comm = nullptr;
    uint64_t *x_own = nullptr;
    bool x_on = false; // sharding active (world = 1 with a collective installed counts: the single-GPU test of the path)
    int64_t x_batches = 0, x_rows = 0;
    // where this rank's chunk of a sharded batch goes, and the exchange that follows it
    uint64_t *x_slot(int64_t rows) const
    {
        return x_comm ? x_gather + (size_t)x_rank * (size_t)rows * wire_row() : x_stage;
    }
};

namespace {

// a lane works on the tables of the context it was forked from
bool owns(const helm_si_ctx *ctx, const helm_si_wires *w)
{
    return w->owner == ctx || (ctx->lane_of && w->owner == ctx->lane_of);
}

struct Timed {
    helm_si_ctx *ctx;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> *list;
    hipEvent_t a = nullptr, b = nullptr;
    Timed(helm_si_ctx *c, std::vector<std::pair<hipEvent_t, hipEvent_t>> *l) : ctx(c), list(l)
    {
        if (ctx->timing) {
            (void)hipEventCreate(&a);
            (void)hipEventCreate(&b);
            (void)hipEventRecord(a, ctx->stream);
        }
    }
    ~Timed()
    {
        if (ctx->timing) {
            (void)hipEventRecord(b, ctx->stream);
            list->push_back({a, b});
        }
    }
};

bool si_supported(const helm_si_params &P)
{
    // k > 1: k_pbs64k, one level, N = 512 (PARAM_MESSAGE_1_CARRY_1_KS_PBS of helm.rs:301 has k = 3); k = 2 also at
    // N = 1024 (the 3-bit set shortint_m2c1)
    if (P.k == 2 || P.k == 3)
        return (P.N == 512 || (P.k == 2 && P.N == 1024)) && P.pbs_l == 1 && P.grouping_factor <= 1;
    if (P.k != 1) return false;
    if (!(P.N == 512 || P.N == 1024 || P.N == 2048)) return false;
    return P.pbs_l == 1 || P.pbs_l == 2;
}

// the shapes k_pbs64_generic takes (helm_si_ctx_create_ex with a HELM_SI_CREATE_* flag): N stops at 2048 because FpG2 has
// 2-adicity 2^12 (no 2N-th root of unity beyond), (k+1) N <= 4096 is its LDS budget (helm_pbs64_generic.inc); its multi-bit
// form (grouping_factor 2 or 3, which must divide n) is on request only: HELM_SI_CREATE_GENERIC_MULTIBIT
bool si_generic_domain(const helm_si_params &P, bool multibit)
{
    return (P.N == 256 || P.N == 512 || P.N == 1024 || P.N == 2048) && P.k >= 1 && (int64_t)(P.k + 1) * P.N <= 4096 &&
           P.pbs_l >= 1 && P.grouping_factor <= (multibit ? 3 : 1);
}

// the shapes the tuned multi-bit build (k_pbs64s) serves
bool si_tuned_multibit(const helm_si_params &P)
{
    return P.k == 1 && P.pbs_l == 1 && (P.N == 1024 || P.N == 2048);
}

// The dynamic-LDS limit of a launcher's kernels, set once per device (the attribute belongs to the device's code object).
// `done` is the launcher's own flag set, one per kernel build; atomic because rank threads of one process launch concurrently.
hipError_t lds_attr_once(std::atomic<bool> (&done)[64], int device, std::initializer_list<const void *> kernels, size_t bytes)
{
    if (done[device & 63]) return hipSuccess;
    for (const void *k : kernels) {
        hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
    }
    done[device & 63] = true;
    return hipSuccess;
}

template <typename C>
hipError_t launch_pbs64k_c(helm_si_ctx *ctx, const Pbs64Job *jobs, int64_t count, const uint64_t *small,
                           const uint64_t *luts, uint64_t *out, int *per_cu = nullptr)
{
    static std::atomic<bool> attr_done[64];
    const SiKeyState &K = *ctx->keys; // (the CRT pair follows the key loaded last, on a lane too)
    // (the 46-bit pair is built for N = 512 only: helm_si_load_bootstrap_key never chooses it at another N)
    auto kern_j = [] {
        if constexpr (C::LOGN == 9) return k_pbs64k<C, J0, J1>;
        else return k_pbs64k<C, F0, F1>;
    }();
    if (K.pair && C::LOGN != 9) return hipErrorInvalidValue;
    auto kern = K.pair ? kern_j : k_pbs64k<C, F0, F1>;
    if (hipError_t e = lds_attr_once(attr_done, ctx->device, {reinterpret_cast<const void *>(k_pbs64k<C, F0, F1>),
                                                              reinterpret_cast<const void *>(kern_j)}, C::BYTES))
        return e;
    if (per_cu) return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, kern, 64 * C::NW, C::BYTES);
    hipLaunchKernelGGL(kern, dim3((unsigned)count), dim3(64 * C::NW), C::BYTES, ctx->stream, jobs, small, luts, K.bsk,
                       K.tw[0], K.tw[1], out, ctx->P.n, ctx->P.pbs_logB, K.p0inv_mod_p1);
    return hipGetLastError();
}

template <typename C, int MODE = 0>
hipError_t launch_pbs64_c(helm_si_ctx *ctx, const Pbs64Job *jobs, int64_t count, const uint64_t *small,
                          const uint64_t *luts, uint64_t *out, const double *key = nullptr, int n_steps = -1,
                          int logB = 0, size_t key_stride = 0, int key_first = 0, int *per_cu = nullptr)
{
    static std::atomic<bool> attr_done[64];
    const SiKeyState &K = *ctx->keys;
    auto kern = k_pbs64<C, MODE>;
    if (hipError_t e = lds_attr_once(attr_done, ctx->device, {reinterpret_cast<const void *>(kern)}, C::BYTES)) return e;
    if (per_cu) return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, kern, 64 * C::NW, C::BYTES);
    hipLaunchKernelGGL(kern, dim3((unsigned)count), dim3(64 * C::NW), C::BYTES, ctx->stream, jobs, small, luts,
                       key ? key : K.bsk, K.tw[0], K.tw[1], out, n_steps >= 0 ? n_steps : ctx->P.n,
                       logB ? logB : ctx->P.pbs_logB, K.p0inv_mod_p1, key_stride, key_first);
#ifdef HELM_WIDE_STAMPS
    {
        unsigned long long v[8 * 8];
        (void)hipStreamSynchronize(ctx->stream);
        if (hipMemcpyFromSymbol(v, HIP_SYMBOL(g_stamps64), sizeof(v)) == hipSuccess)
            for (int w = 0; w < C::NW; w++)
                fprintf(stderr, "[stamps k_pbs64: prep | fwd | products | bar1 | sum+bar2 | inverse | crt+bars] wave %d: %llu %llu %llu %llu %llu %llu %llu cycles/step\n",
                        w, v[w * 8] / ctx->P.n, v[w * 8 + 1] / ctx->P.n, v[w * 8 + 2] / ctx->P.n, v[w * 8 + 3] / ctx->P.n,
                        v[w * 8 + 4] / ctx->P.n, v[w * 8 + 5] / ctx->P.n, v[w * 8 + 6] / ctx->P.n);
    }
#endif
    return hipGetLastError();
}

template <typename C, bool MB>
hipError_t launch_pbs64s_c(helm_si_ctx *ctx, const Pbs64Job *jobs, int64_t count, const uint64_t *small,
                           const uint64_t *luts, uint64_t *out, int *per_cu = nullptr)
{
    static std::atomic<bool> attr_done[64];
    const SiKeyState &K = *ctx->keys;
    auto kern = k_pbs64s<C, MB>;
    if (hipError_t e = lds_attr_once(attr_done, ctx->device, {reinterpret_cast<const void *>(kern)}, C::BYTES)) return e;
    if (per_cu) return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, kern, 64 * C::NW, C::BYTES);
    hipLaunchKernelGGL(kern, dim3((unsigned)count), dim3(64 * C::NW), C::BYTES, ctx->stream, jobs, small, luts,
                       K.bsk_split, K.tw_sub, K.tw[0], K.tw[1], out, ctx->P.n, ctx->P.pbs_logB, K.p0inv_mod_p1, K.group,
                       K.expo, K.psi_pow);
#ifdef HELM_WIDE_STAMPS
    {
        unsigned long long v[8 * 8];
        (void)hipStreamSynchronize(ctx->stream);
        if (hipMemcpyFromSymbol(v, HIP_SYMBOL(g_stamps64), sizeof(v)) == hipSuccess)
            for (int w = 0; w < C::NW; w++) {
                fprintf(stderr, "[stamps k_pbs64s: digits | bar1 | fwd | products | sum+bars | inverse | halves+bars | crt+bars] wave %d:", w);
                for (int q = 0; q < 8; q++) fprintf(stderr, " %llu", v[w * 8 + q] / ctx->P.n);
                fprintf(stderr, " cycles/step\n");
            }
    }
#endif
    return hipGetLastError();
}

// The run-time grouping factor as the kernels' compile-time GG: f(std::integral_constant<int, GG>) with GG = 3 or 2 for the
// multi-bit forms, 0 (the classical form) for anything else.
template <class F>
auto with_group(int group, F &&f)
{
    if (group == 3) return f(std::integral_constant<int, 3>{});
    if (group == 2) return f(std::integral_constant<int, 2>{});
    return f(std::integral_constant<int, 0>{});
}

// Two translation units from this one source (Makefile).  The compiler's max-ILP scheduling strategy
// (-mllvm -amdgpu-sched-strategy=max-ilp; there is no per-function switch) is worth +3.7 % on k_pbs64k and +2.0 % on the
// multi-bit k_pbs64s, and costs the classical k_pbs64s 0.8 % and its two-level build 1.8 % (same box, alternating,
// identical ciphertexts: profiles/r03/si_kernel_experiments.txt (15)).  So the launchers of the first two are compiled a
// second time with -DHELM_SI_TU=1 under that strategy - nothing else of the file is - and the main unit
// (-DHELM_SI_SPLIT_TU=1), which instantiates none of their kernels, calls them through this one function.  Without the two
// macros the file is a single unit that holds the function itself.  It serves the forms SI_K and SI_SPLIT_MB.
} // namespace
__attribute__((visibility("hidden"))) hipError_t helm_si_tu1_launch_pbs64(helm_si_ctx *ctx, const void *jobs, int64_t count,
                                                                        const uint64_t *small, const uint64_t *luts,
                                                                        uint64_t *out, int *per_cu);
#if !HELM_SI_SPLIT_TU
hipError_t helm_si_tu1_launch_pbs64(helm_si_ctx *ctx, const void *jobs_v, int64_t count, const uint64_t *small,
                                    const uint64_t *luts, uint64_t *out, int *per_cu)
{
    const Pbs64Job *jobs = static_cast<const Pbs64Job *>(jobs_v);
    switch (ctx->keys->run.form) {
    case SI_K: // (k, N) = (3, 512), (2, 512), (2, 1024): si_supported
        if (ctx->P.k == 3) return launch_pbs64k_c<Pbs64kCfg<9, 3>>(ctx, jobs, count, small, luts, out, per_cu);
        if (ctx->logN == 10) return launch_pbs64k_c<Pbs64kCfg<10, 2>>(ctx, jobs, count, small, luts, out, per_cu);
        return launch_pbs64k_c<Pbs64kCfg<9, 2>>(ctx, jobs, count, small, luts, out, per_cu);
    case SI_SPLIT_MB:
        return with_logn<10, 11>(ctx->logN, hipErrorInvalidValue, [&](auto ln) {
            return launch_pbs64s_c<Pbs64sCfg<decltype(ln)::value>, true>(ctx, jobs, count, small, luts, out, per_cu);
        });
    default: return hipErrorInvalidValue;
    }
}
#endif
#if HELM_SI_TU == 0 // ==== everything below: the main unit only ===============================================
#include "pbs_twoprime.h" // what k_pbs64_generic shares with the boolean engine's k_pbs_crt
namespace {

// k_pbs64_generic: k, pbs_l and pbs_logB at run time (helm_si_ctx_create_ex)
#include "helm_pbs64_generic.inc"

// what the two large-N kernels share: the pair FpG / FpI, the transforms, the pieces of a step, the key conversion
#include "helm_pbs64_large_core.inc"

// k_pbs64_large: k = 1, N = 4096 (helm_si_ctx_create_ex with HELM_SI_CREATE_LARGE_N)
#include "helm_pbs64_large.inc"

hipError_t launch_pbs64_large(helm_si_ctx *ctx, const Pbs64Job *jobs, int64_t count, const uint64_t *small,
                              const uint64_t *luts, uint64_t *out)
{
    // (the dynamic LDS attribute is set by helm_si_ctx_create_ex: setup_large)
    const SiKeyState &K = *ctx->keys;
    if (ctx->logN != 12 || ctx->P.k != 1) return hipErrorInvalidValue;
    if (K.group > 1 && !K.psi_pow) return hipErrorInvalidValue;
    with_group(K.group, [&](auto g) {
        hipLaunchKernelGGL((k_pbs64_large<12, decltype(g)::value>), dim3((unsigned)count), dim3(L64_THREADS), K.lds,
                           ctx->stream, jobs, small, luts, K.bsk, K.tw[0], K.tw[1], K.twi[0], K.twi[1], K.psi_pow, out, ctx->P.n,
                           ctx->P.pbs_l, ctx->P.pbs_logB, K.p0inv_mod_p1);
    });
    return hipGetLastError();
}

// group: the multi-bit grouping factor (2 or 3), anything else: the classical form
const void *pbs64_large_kernel(int group)
{
    return with_group(group, [](auto g) { return reinterpret_cast<const void *>(k_pbs64_large<12, decltype(g)::value>); });
}

// k_pbs64_n8192: k = 1, N = 8192 (helm_si_ctx_create_ex with HELM_SI_CREATE_N8192)
#include "helm_pbs64_n8192.inc"

// The kernel's accumulator rows are indexed by blockIdx.x, so a launch is at most as wide as the context's row buffer: one
// round (a workgroup per CU).  A wider batch goes out in chunks of a round, one after the other on the context's stream.
hipError_t launch_pbs64_n8192(helm_si_ctx *ctx, const Pbs64Job *jobs, int64_t count, const uint64_t *small,
                              const uint64_t *luts, uint64_t *out)
{
    // (the dynamic LDS attribute is set by helm_si_ctx_create_ex: setup_n8192)
    const SiKeyState &K = *ctx->keys;
    if (ctx->logN != N8192_LOGN || ctx->P.k != 1) return hipErrorInvalidValue;
    const int64_t rows = std::max(ctx->n_cus, 1); // (the rows of d_acc8192: alloc_acc8192)
    if (!ctx->d_acc8192) return hipErrorInvalidValue;
    if (K.group > 1 && !K.psi_pow) return hipErrorInvalidValue;
    for (int64_t off = 0; off < count; off += rows) {
        const int64_t chunk = std::min(rows, count - off);
        with_group(K.group, [&](auto g) {
            hipLaunchKernelGGL(k_pbs64_n8192<decltype(g)::value>, dim3((unsigned)chunk), dim3(L64_THREADS), K.lds,
                               ctx->stream, jobs + off, small, luts, K.bsk, K.tw[0], K.tw[1], K.twi[0], K.twi[1], K.psi_pow, out,
                               ctx->d_acc8192, ctx->P.n, ctx->P.pbs_l, ctx->P.pbs_logB, K.p0inv_mod_p1);
        });
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

// group: the multi-bit grouping factor (2 or 3), anything else: the classical form
const void *pbs64_n8192_kernel(int group)
{
    return with_group(group, [](auto g) { return reinterpret_cast<const void *>(k_pbs64_n8192<decltype(g)::value>); });
}

hipError_t launch_pbs64_generic(helm_si_ctx *ctx, const Pbs64Job *jobs, int64_t count, const uint64_t *small,
                                const uint64_t *luts, uint64_t *out)
{
    // (the dynamic LDS attribute is set by helm_si_ctx_create_ex, at the largest layout of this N)
    const SiKeyState &K = *ctx->keys;
    return with_logn<8, 11>(ctx->logN, hipErrorInvalidValue, [&](auto ln) {
        with_group(K.group, [&](auto g) {
            hipLaunchKernelGGL((k_pbs64_generic<decltype(ln)::value, decltype(g)::value>), dim3((unsigned)count),
                               dim3(TP_THREADS), K.lds, ctx->stream, jobs, small, luts, K.bsk, K.tw[0], K.tw[1], K.twi[0],
                               K.twi[1], K.psi_pow, out, ctx->P.n, ctx->P.k, ctx->P.pbs_l, ctx->P.pbs_logB, K.gen_d,
                               K.p0inv_mod_p1);
        });
        return hipGetLastError();
    });
}

// group: the multi-bit grouping factor (2 or 3), anything else: the classical form
const void *pbs64_generic_kernel(int logN, int group)
{
    return with_logn<8, 11>(logN, (const void *)nullptr, [&](auto ln) {
        return with_group(group, [](auto g) {
            return reinterpret_cast<const void *>(k_pbs64_generic<decltype(ln)::value, decltype(g)::value>);
        });
    });
}

// per_cu: not a launch but the question helm_si_round_capacity asks - how many workgroups of the context's kernel a CU holds
// (classes 1 to 3: what their setup stored; a tuned form: the occupancy of the build it would launch)
hipError_t launch_pbs64(helm_si_ctx *ctx, const Pbs64Job *jobs, int64_t count, const uint64_t *small,
                        const uint64_t *luts, uint64_t *out, int *per_cu = nullptr)
{
    const SiKeyState &K = *ctx->keys;
    if (per_cu && K.run.cls != SI_TUNED) {
        *per_cu = K.per_cu;
        return hipSuccess;
    }
    switch (K.run.cls) {
    case SI_N8192: return launch_pbs64_n8192(ctx, jobs, count, small, luts, out);
    case SI_LARGE: return launch_pbs64_large(ctx, jobs, count, small, luts, out);
    case SI_GENERIC: return launch_pbs64_generic(ctx, jobs, count, small, luts, out);
    case SI_TUNED: break;
    }
    switch (K.run.form) {
    case SI_K:
    case SI_SPLIT_MB: return helm_si_tu1_launch_pbs64(ctx, jobs, count, small, luts, out, per_cu); // the max-ILP unit's
    case SI_SPLIT: // (one or two levels: si_supported)
        if (ctx->P.pbs_l == 1)
            return with_logn<10, 11>(ctx->logN, hipErrorInvalidValue, [&](auto ln) {
                return launch_pbs64s_c<Pbs64sCfg<decltype(ln)::value>, false>(ctx, jobs, count, small, luts, out, per_cu);
            });
        return with_logn<10, 11>(ctx->logN, hipErrorInvalidValue, [&](auto ln) {
            return launch_pbs64s_c<Pbs64sCfg<decltype(ln)::value, 2>, false>(ctx, jobs, count, small, luts, out, per_cu);
        });
    case SI_WIDE:
        return with_logn<9, 11>(ctx->logN, hipErrorInvalidValue, [&](auto ln) {
            constexpr int LN = decltype(ln)::value;
            return ctx->P.pbs_l == 1 ? launch_pbs64_c<Pbs64Cfg<LN, 1>>(ctx, jobs, count, small, luts, out, nullptr, -1, 0, 0, 0, per_cu)
                                     : launch_pbs64_c<Pbs64Cfg<LN, 2>>(ctx, jobs, count, small, luts, out, nullptr, -1, 0, 0, 0, per_cu);
        });
    case SI_NO_FORM: break;
    }
    return hipErrorInvalidValue;
}

// A keyswitching key on the device: in_dim input words (+ body) -> out_dim mask words + body.  The context's own
// key (big -> small) and the WoP-PBS path's extra keys go through the same kernels.
using KsKey = helm_ks::Key<uint64_t>;

// Where the output rows of a keyswitch launch lie, for the sliced vector-ALU form, whose partial sums meet in rows zeroed
// beforehand.  Without one the jobs write rows 0 .. count-1 of `out` (every order-1 launch).  The order-0 launches write
// elsewhere: `rows` (with `none`, as many -1 entries: k_rows64 writes a zero row for a negative source) names the rows of a
// wire table one by one - the other rows of the table are not touched - and without `rows` the first `dense` rows are zeroed
// (a rank's exchange slot, where skipped many-LUT outputs leave gaps).
struct KsOutRows {
    int64_t dense = 0;
    const int32_t *rows = nullptr, *none = nullptr;
};

// What the 64-bit engine's keyswitch launches have of their own (helm_ks::launch): every ks_l in 1..8 with the level count
// padded to 1, 2, 4 or 8 on the matrix cores, one column tile per product wave, the 160 KiB dynamic-LDS limit on the vector
// kernels (an unsliced digit buffer is up to 128 KiB at in_dim = 4096), and output rows named by KsOutRows.
struct KsEngine64 {
    using Word = uint64_t;
    using Ctx = helm_si_ctx;
    using OutJob = Ks64Job;
    using Where = const KsOutRows *;
    using VectorLevels = std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 7, 8>;
    using DigitLevels = VectorLevels;
    static constexpr int CT = 1;
    static constexpr int padded_levels(int ks_l) { return ks64_padded_levels(ks_l); }
    static auto product_kernel() { return k_ks64_mfma; }
    // narrow batches stay on the vector-ALU kernel, whose key rows are split over workgroup slices: a matrix-core
    // wave walks the whole key column by column tile (0.23 ms whatever the width; vector ALU: 0.11 ms for 64, 0.37 ms
    // for 256 ciphertexts under PARAM_MESSAGE_2_CARRY_2)
    static bool matrix_path(const Ctx *ctx, const KsKey &K, int64_t count) { return K.planes && ctx->keys->ks_mfma && count >= 160; }
    static hipError_t zero_rows(Ctx *ctx, const Ks64Job *, Where where, uint64_t *out, int64_t count, int n)
    {
        if (where && where->rows) {
            hipLaunchKernelGGL(k_rows64, dim3((unsigned)count), dim3(256), 0, ctx->stream, out, where->none, out, where->rows, n);
            return hipGetLastError();
        }
        return hipMemsetAsync(out, 0, (size_t)(where ? where->dense : count) * ((size_t)n + 1) * sizeof(uint64_t), ctx->stream);
    }
    template <typename> static hipError_t allow_lds(Ctx *ctx, const void *kernel)
    {
        static bool done[64] = {false}; // per kernel and device: the attribute belongs to the device's code object
        if (done[ctx->device & 63]) return hipSuccess;
        hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        done[ctx->device & 63] = e == hipSuccess;
        return e;
    }
};

// `out`: rows of out_dim+1 words (job g writes row jobs[g].out_row)
hipError_t launch_ks64_key(helm_si_ctx *ctx, const KsKey &K, const Ks64Job *jobs, int64_t count, const uint64_t *big,
                           uint64_t *out, const KsOutRows *where = nullptr)
{
    return helm_ks::launch<KsEngine64>(
        ctx, K, jobs, jobs, count, big, out, where, [](auto lv) { return k_ks64_digits<decltype(lv)::value>; },
        [](auto lv) { return k_keyswitch64<decltype(lv)::value>; });
}

hipError_t launch_ks64(helm_si_ctx *ctx, const Ks64Job *jobs, int64_t count, const uint64_t *big, uint64_t *out,
                       const KsOutRows *where = nullptr)
{
    KsKey K;
    K.key = ctx->keys->ksk;
    K.planes = ctx->keys->ksk_planes;
    K.in_dim = ctx->P.k * ctx->P.N;
    K.out_dim = ctx->P.n;
    K.l = ctx->P.ks_l;
    K.logB = ctx->P.ks_logB;
    K.kchunks = ctx->keys->ks_kchunks;
    K.ctiles = ctx->keys->ks_ctiles;
    return launch_ks64_key(ctx, K, jobs, count, big, out, where);
}

int check_rows(const helm_si_wires *w, const int32_t *idx, int64_t count, bool allow_neg)
{
    for (int64_t i = 0; i < count; i++)
        if (idx[i] >= w->n_rows || (idx[i] < 0 && !(allow_neg && idx[i] == -1)))
            return fail(HELM_ERR_INVALID, "row index " + std::to_string(idx[i]) + " out of range at position " +
                                              std::to_string(i));
    return 0;
}

// Per-context scratch is refilled from pageable host memory by every call; such a copy is not
// guaranteed to queue behind kernels still reading the previous contents, so callers drain the
// stream (drain()) before their first upload.
int drain(helm_si_ctx *ctx)
{
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

template <typename T>
int upload(helm_si_ctx *ctx, DevBuf<T> &buf, const T *host, size_t n)
{
    if (buf.ensure(n)) return fail(HELM_ERR_OOM, "device scratch");
    HIP_TRY(hipMemcpyAsync(buf.p, host, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return 0;
}

// ---- call slots (see helm_si_ctx) -------------------------------------------------------------------------
int slot_begin(helm_si_ctx *ctx, size_t need, helm_si_ctx::CallSlot **out)
{
    helm_si_ctx::CallSlot &S = ctx->slots[ctx->next_slot];
    ctx->next_slot = (ctx->next_slot + 1) % 3;
    if (!S.done) HIP_TRY(hipEventCreateWithFlags(&S.done, hipEventDisableTiming));
    if (S.busy) HIP_TRY(hipEventSynchronize(S.done)); // two calls later at the earliest: normally long complete
    S.busy = false;
    need += 4096;
    if (need > S.cap) {
        if (S.host) (void)hipHostFree(S.host);
        if (S.dev) (void)hipFree(S.dev);
        S.host = S.dev = nullptr;
        S.cap = 0;
        const size_t want = std::max(need * 2, (size_t)1 << 20);
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&S.host), want, hipHostMallocDefault));
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&S.dev), want));
        S.cap = want;
    }
    S.used = 0;
    *out = &S;
    return 0;
}
template <typename T> T *slot_put(helm_si_ctx::CallSlot &S, const T *src, size_t n)
{
    S.used = (S.used + 255) / 256 * 256;
    std::memcpy(S.host + S.used, src, n * sizeof(T));
    T *d = reinterpret_cast<T *>(S.dev + S.used);
    S.used += n * sizeof(T);
    return d;
}
int slot_flush(helm_si_ctx *ctx, helm_si_ctx::CallSlot &S)
{
    if (S.used) HIP_TRY(hipMemcpyAsync(S.dev, S.host, S.used, hipMemcpyHostToDevice, ctx->stream));
    return 0;
}
int slot_end(helm_si_ctx *ctx, helm_si_ctx::CallSlot &S)
{
    HIP_TRY(hipEventRecord(S.done, ctx->stream));
    S.busy = true;
    return 0;
}
// the look-up tables of a call: resident already (same words as the last upload) or uploaded after a drain
int luts_resident(helm_si_ctx *ctx, const uint64_t *luts_host, size_t words)
{
    uint64_t h = 0x9E3779B97F4A7C15ull ^ words;
    for (size_t i = 0; i < words; i++) h = (h ^ luts_host[i]) * 0x100000001B3ull + (h >> 29);
    // the hash only says "probably": the words themselves decide (a collision would bootstrap with the previous call's
    // tables and return wrong ciphertexts without an error; the WoP-PBS path swaps tables on one context all the time)
    if (ctx->d_luts.p && ctx->luts_words == words && ctx->luts_hash == h && ctx->luts_host.size() == words &&
        std::memcmp(ctx->luts_host.data(), luts_host, words * sizeof(uint64_t)) == 0)
        return 0;
    HIP_TRY(hipStreamSynchronize(ctx->stream)); // a running bootstrap may still read the old tables
    if (ctx->d_luts.ensure(words)) return fail(HELM_ERR_OOM, "look-up tables");
    HIP_TRY(hipMemcpy(ctx->d_luts.p, luts_host, words * sizeof(uint64_t), hipMemcpyHostToDevice));
    ctx->luts_host.assign(luts_host, luts_host + words);
    ctx->luts_hash = h;
    ctx->luts_words = words;
    return 0;
}

// keyswitch + bootstrap of `count` rows of `src` (big) into rows of `dst` (big)
int apply_luts_device(helm_si_ctx *ctx, const uint64_t *src, uint64_t *dst, const std::vector<Ks64Job> &ks,
                      const std::vector<Pbs64Job> &pbs, const uint64_t *luts_host, int64_t n_luts,
                      const KsKey *other_key = nullptr) // other_key: keyswitch from another big key (WoP-PBS path)
{
    const helm_si_params &P = ctx->P;
    if (!ctx->keys->have_bsk || !(ctx->keys->have_ksk || other_key))
        return fail(HELM_ERR_STATE, "bootstrapping / keyswitching key not loaded");
    const int64_t count = (int64_t)pbs.size();
    if (count == 0) return 0;
    if (ctx->d_small.cap < (size_t)count * ((size_t)P.n + 1)) {
        if (int rc = drain(ctx)) return rc; // growing the scratch frees the old one
        if (ctx->d_small.ensure((size_t)count * ((size_t)P.n + 1))) return fail(HELM_ERR_OOM, "small-LWE scratch");
    }
    if (int rc = luts_resident(ctx, luts_host, (size_t)n_luts * P.N)) return rc;
    helm_si_ctx::CallSlot *S = nullptr;
    if (int rc = slot_begin(ctx, ks.size() * sizeof(Ks64Job) + pbs.size() * sizeof(Pbs64Job), &S)) return rc;
    const Ks64Job *d_ks = slot_put(*S, ks.data(), ks.size());
    const Pbs64Job *d_pbs = slot_put(*S, pbs.data(), pbs.size());
    if (int rc = slot_flush(ctx, *S)) return rc;
    {
        Timed t(ctx, &ctx->ev_ks);
        if (other_key) HIP_TRY(launch_ks64_key(ctx, *other_key, d_ks, count, src, ctx->d_small.p));
        else HIP_TRY(launch_ks64(ctx, d_ks, count, src, ctx->d_small.p));
    }
    ctx->tacc.ks_launches++;
    ctx->tacc.ks_count += count;
    {
        Timed t(ctx, &ctx->ev_pbs);
        HIP_TRY(launch_pbs64(ctx, d_pbs, count, ctx->d_small.p, ctx->d_luts.p, dst));
    }
    if (int rc = slot_end(ctx, *S)) return rc;
    ctx->tacc.pbs_launches++;
    ctx->tacc.pbs_count += count;
    return 0;
}

// Order 0 (HELM_SI_CREATE_PBS_KS): one bootstrap launch, then one keyswitch.  The bootstraps read their n+1-word input rows
// in place - `src` is a wire table and Pbs64Job.in_row one of its rows - and write big rows into the stage buffer
// (`stage_rows` of them); the keyswitch takes stage rows (Ks64Job.in_row) to rows of `dst`: a wire table (dense < 0), or a
// rank's exchange slot of `dense` rows.  Every input row is read before any row of `dst` is written (kernel boundary), so an
// output row may be an input row of the same call.  Many-LUT callers leave the skipped outputs off `ks`.
int apply_luts_pbs_first(helm_si_ctx *ctx, const uint64_t *src, uint64_t *dst, const std::vector<Pbs64Job> &pbs,
                         int64_t stage_rows, const std::vector<Ks64Job> &ks, int64_t dense, const uint64_t *luts_host,
                         int64_t n_luts)
{
    const helm_si_params &P = ctx->P;
    if (!ctx->keys->have_bsk || !ctx->keys->have_ksk) return fail(HELM_ERR_STATE, "bootstrapping / keyswitching key not loaded");
    const int64_t count = (int64_t)pbs.size();
    if (count == 0) return 0;
    const size_t brow = (size_t)P.k * P.N + 1; // (a bootstrap's output row, not a wire row)
    if (ctx->d_stage.cap < (size_t)stage_rows * brow) {
        if (int rc = drain(ctx)) return rc; // growing the staging area frees the old one
        if (ctx->d_stage.ensure((size_t)stage_rows * brow)) return fail(HELM_ERR_OOM, "staging");
    }
    if (int rc = luts_resident(ctx, luts_host, (size_t)n_luts * P.N)) return rc;
    std::vector<int32_t> rows, none;
    if (dense < 0) {
        rows.resize(ks.size());
        none.assign(ks.size(), -1);
        for (size_t i = 0; i < ks.size(); i++) rows[i] = ks[i].out_row;
    }
    helm_si_ctx::CallSlot *S = nullptr;
    if (int rc = slot_begin(ctx, ks.size() * (sizeof(Ks64Job) + 2 * sizeof(int32_t)) + pbs.size() * sizeof(Pbs64Job) + 1024, &S))
        return rc;
    const Ks64Job *d_ks = slot_put(*S, ks.data(), ks.size());
    const Pbs64Job *d_pbs = slot_put(*S, pbs.data(), pbs.size());
    KsOutRows where;
    where.dense = dense;
    if (dense < 0) {
        where.rows = slot_put(*S, rows.data(), rows.size());
        where.none = slot_put(*S, none.data(), none.size());
    }
    if (int rc = slot_flush(ctx, *S)) return rc;
    {
        Timed t(ctx, &ctx->ev_pbs);
        HIP_TRY(launch_pbs64(ctx, d_pbs, count, src, ctx->d_luts.p, ctx->d_stage.p));
    }
    ctx->tacc.pbs_launches++;
    ctx->tacc.pbs_count += count;
    if (!ks.empty()) {
        Timed t(ctx, &ctx->ev_ks);
        HIP_TRY(launch_ks64(ctx, d_ks, (int64_t)ks.size(), ctx->d_stage.p, dst, &where));
        ctx->tacc.ks_launches++;
        ctx->tacc.ks_count += (int64_t)ks.size();
    }
    return slot_end(ctx, *S);
}

// Many-LUT: n functions share one blind rotation in M = the power of two >= n chunks of N/M coefficients (M <= t = message x
// carry, so that a chunk holds whole boxes).  -> M and the `pad` of the bootstrap jobs (Pbs64Job).
int many_lut_shape(const helm_si_ctx *ctx, int64_t n, int *M_out, int32_t *pad_out)
{
    const int t = ctx->P.message_modulus * ctx->P.carry_modulus;
    if (n < 1 || n > t) // (t is a power of two: the power of two >= n exceeds t exactly when n does)
        return fail(HELM_ERR_INVALID, "many-LUT: " + std::to_string(n) + " functions, this set holds 1 .. " + std::to_string(t));
    int logM = 0;
    while ((1 << logM) < n) logM++;
    if (M_out) *M_out = 1 << logM;
    if (pad_out) *pad_out = (int32_t)(n - 1) | (int32_t)(ctx->logN - logM) << 16;
    return 0;
}

// keyswitch + one blind rotation per job + n_out sample extracts into rows g n_out + x of the stage buffer
int apply_many_luts_stage(helm_si_ctx *ctx, const uint64_t *src, const int32_t *in_idx, const int32_t *lut_idx, int32_t n_out,
                          int32_t pad, int64_t count, const uint64_t *luts, int64_t n_luts)
{
    const size_t brow = (size_t)ctx->P.k * ctx->P.N + 1; // (a bootstrap's output row; order 1: also the wire row)
    std::vector<Ks64Job> ks((size_t)count);
    std::vector<Pbs64Job> pbs((size_t)count);
    for (int64_t g = 0; g < count; g++) {
        ks[(size_t)g] = Ks64Job{in_idx[g], (int32_t)g};
        pbs[(size_t)g] = Pbs64Job{(int32_t)g, lut_idx[g], (int32_t)(g * n_out), pad};
    }
    if (ctx->d_stage.cap < (size_t)count * n_out * brow) {
        if (int rc = drain(ctx)) return rc; // growing the staging area frees the old one
        if (ctx->d_stage.ensure((size_t)count * n_out * brow)) return fail(HELM_ERR_OOM, "staging");
    }
    return apply_luts_device(ctx, src, ctx->d_stage.p, ks, pbs, luts, n_luts);
}

// `polys` polynomials of K1 x K1 x l GGSW rows at `src` into k_pbs64s' half-transform order at `dst`, both fields of the 49-bit pair,
// scaled by n_inv per field (the split key of a context, and the probe below)
void launch_convert64s(helm_si_ctx *ctx, const uint64_t *src, double *dst, size_t polys, const double (&n_inv)[2], int K1, int l)
{
    const SiKeyState &K = *ctx->keys;
    with_logn<10, 11>(ctx->logN, false, [&](auto ln) {
        constexpr int LN = decltype(ln)::value;
        hipLaunchKernelGGL((k_bsk_convert64s<F0, LN>), dim3((unsigned)(polys * 2)), dim3(64), 0, ctx->stream, src, dst, K.tw[0],
                           K.tw_sub, n_inv[0], K.two32[0], K1, 0, l);
        hipLaunchKernelGGL((k_bsk_convert64s<F1, LN>), dim3((unsigned)(polys * 2)), dim3(64), 0, ctx->stream, src, dst, K.tw[1],
                           K.tw_sub + ctx->P.N, n_inv[1], K.two32[1], K1, 1, l);
        return true;
    });
}

// Multi-bit: which power of psi is the evaluation point of each spectrum position, in the order the key
// words (and the transform outputs of k_pbs64s) are held?  Transform the polynomial X through the key
// conversion kernel (one "key" of one polynomial) and look the values up among the powers of psi.
int probe_spectrum_positions(helm_si_ctx *ctx)
{
    SiKeyState &K = *ctx->keys;
    const int N = ctx->P.N, H = N / 2;
    std::vector<uint64_t> xpoly((size_t)N, 0);
    xpoly[1] = 1;
    // freed on every return path
    struct Tmp {
        void *p = nullptr;
        ~Tmp() { if (p) (void)hipFree(p); }
    } t_x, t_out;
    HIP_TRY(hipMalloc(&t_x.p, sizeof(uint64_t) * N));
    HIP_TRY(hipMalloc(&t_out.p, sizeof(double) * 4 * H));
    uint64_t *d_x = static_cast<uint64_t *>(t_x.p);
    double *d_out = static_cast<double *>(t_out.p);
    HIP_TRY(hipMemcpy(d_x, xpoly.data(), sizeof(uint64_t) * N, hipMemcpyHostToDevice));
    // one polynomial, K1 = 1: blocks (poly 0, half h) write d_out[(f * 2 + h) * N/2 ...] scaled by 1 (n_inv = 1)
    launch_convert64s(ctx, d_x, d_out, 1, {1.0, 1.0}, 1, 1);
    HIP_TRY(hipGetLastError());
    std::vector<double> val((size_t)4 * H), pw((size_t)4 * N);
    HIP_TRY(hipMemcpyAsync(val.data(), d_out, sizeof(double) * 4 * H, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(pw.data(), K.psi_pow, sizeof(double) * 4 * N, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::vector<uint16_t> expo((size_t)2 * H);
    for (int f = 0; f < 2; f++) {
        std::map<int64_t, int> where;
        for (int t = 0; t < 2 * N; t++) where[(int64_t)pw[(size_t)f * 2 * N + t]] = t;
        for (int q = 0; q < 2 * H; q++) {
            auto it = where.find((int64_t)val[(size_t)f * 2 * H + q]);
            if (it == where.end() || !(it->second & 1)) return fail(HELM_ERR_HIP, "multi-bit: spectrum position probe failed");
            if (f == 0) expo[(size_t)q] = (uint16_t)it->second;
            else if (expo[(size_t)q] != (uint16_t)it->second)
                return fail(HELM_ERR_HIP, "multi-bit: the two fields disagree on a spectrum position");
        }
    }
    { // the structure pbs64s_mb_body relies on: expo(h, lane, e) = expo(h, lane, 0) + (2N/EH) rev(e)  (mod 2N)
        const int EH = H / 64;
        int loge = 0;
        while ((1 << loge) < EH) loge++;
        for (int hh = 0; hh < 2; hh++)
            for (int e = 0; e < EH; e++)
                for (int lane = 0; lane < 64; lane++) {
                    const int v = expo[(size_t)hh * H + ((size_t)(e >> 1) * 64 + lane) * 2 + (e & 1)];
                    const int v0 = expo[(size_t)hh * H + (size_t)lane * 2];
                    if (v != ((v0 + (2 * N / EH) * bitrev_c(e, loge)) & (2 * N - 1)))
                        return fail(HELM_ERR_HIP, "multi-bit: unexpected order of the spectrum positions");
                }
    }
    if (const char *path = getenv("HELM_SI_DUMP_EXPO")) { // diagnostic: the probed table, [2 halves][N/2] u16
        if (FILE *fp = fopen(path, "wb")) {
            fwrite(expo.data(), sizeof(uint16_t), expo.size(), fp);
            fclose(fp);
        }
    }
    HIP_TRY(hipMalloc(&K.expo, expo.size() * sizeof(uint16_t)));
    HIP_TRY(hipMemcpy(K.expo, expo.data(), expo.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    return 0;
}

// all-gather of `rows` wire rows per rank into x_gather, on the context's stream
int si_exchange(helm_si_ctx *ctx, int64_t rows)
{
    if (ctx->x_comm)
        return helm_comm_all_gather(ctx->x_comm, ctx->x_slot(rows), ctx->x_gather,
                                    (size_t)rows * ctx->wire_row() * sizeof(uint64_t), ctx->stream);
    if (int rc = ctx->x_fn(ctx->x_user, rows))
        return fail(HELM_ERR_STATE, "exchange callback failed with " + std::to_string(rc));
    return 0;
}

// helm_si_apply_luts with the batch sharded over the ranks of helm_si_set_exchange(): identical
// ciphertexts to the unsharded call (every bootstrap is independent and deterministic)
int apply_luts_sharded(helm_si_ctx *ctx, helm_si_wires *w, const int32_t *in_idx, const int32_t *lut_idx,
                       const int32_t *out_idx, int64_t count, const uint64_t *luts, int64_t n_luts)
{
    const int dim = (int)ctx->wire_dim();
    const int64_t world = ctx->x_world;
    for (int64_t base = 0; base < count;) {
        const int64_t per = std::min(count - base, ctx->x_cap * world);
        const int64_t rows = (per + world - 1) / world;
        const int64_t lo = std::min(base + per, base + ctx->x_rank * rows), hi = std::min(base + per, lo + rows);
        std::vector<Ks64Job> ks((size_t)(hi - lo));
        std::vector<Pbs64Job> pbs((size_t)(hi - lo));
        for (int64_t g = lo; g < hi; g++) {
            // order 1: table row -> small row g - lo -> slot row g - lo; order 0: table row -> stage row g - lo -> slot row g - lo
            ks[(size_t)(g - lo)] = Ks64Job{ctx->order ? in_idx[g] : (int32_t)(g - lo), (int32_t)(g - lo)};
            pbs[(size_t)(g - lo)] = Pbs64Job{ctx->order ? (int32_t)(g - lo) : in_idx[g], lut_idx[g], (int32_t)(g - lo), 0};
        }
        if (ctx->order == 0) {
            if (int rc = apply_luts_pbs_first(ctx, w->d, ctx->x_slot(rows), pbs, hi - lo, ks, rows, luts, n_luts)) return rc;
        } else if (int rc = apply_luts_device(ctx, w->d, ctx->x_slot(rows), ks, pbs, luts, n_luts))
            return rc;
        // the collective (the library's ncclAllGather, or the caller's callback) on this context's stream: every
        // rank calls it, also one whose chunk is empty
        if (int rc = si_exchange(ctx, rows)) return rc;
        if (int rc = drain(ctx)) return rc;
        if (int rc = upload(ctx, ctx->d_idx2, out_idx + base, (size_t)per)) return rc;
        // gathered row q * rows + i is gate base + q * rows + i: the chunks are contiguous
        hipLaunchKernelGGL(k_rows64, dim3((unsigned)per), dim3(256), 0, ctx->stream, ctx->x_gather,
                           (const int32_t *)nullptr, w->d, ctx->d_idx2.p, dim);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        ctx->x_batches++;
        ctx->x_rows += rows * world;
        base += per;
    }
    return 0;
}

// helm_si_apply_many_luts with the batch sharded over the ranks of helm_si_set_exchange(): the ciphertexts are cut into
// contiguous chunks as apply_luts_sharded cuts them, a rank's slot of a round holds its chunk's n_out extracts per
// ciphertext (so a round takes x_cap / n_out ciphertexts per rank), and gathered row i n_out + x is output x of ciphertext
// base + i.  This rank keyswitches its share of EVERY round before the first round is scattered: an output row of an early
// ciphertext may be the input row of a later one, and the unsharded call reads every input before it writes any output.
int apply_many_luts_sharded(helm_si_ctx *ctx, helm_si_wires *w, const int32_t *in_idx, const int32_t *lut_idx,
                            const int32_t *out_idx, int32_t n_out, int32_t pad, int64_t count, const uint64_t *luts,
                            int64_t n_luts)
{
    const helm_si_params &P = ctx->P;
    const int dim = (int)ctx->wire_dim();
    const int64_t world = ctx->x_world, cts = ctx->x_cap / n_out;
    if (cts < 1)
        return fail(HELM_ERR_INVALID, "many-LUT: n_out = " + std::to_string(n_out) + " exceeds the exchange's capacity_rows = " +
                                          std::to_string(ctx->x_cap) + " (one ciphertext's outputs do not fit a rank's slot)");
    if (!ctx->keys->have_bsk || !ctx->keys->have_ksk) return fail(HELM_ERR_STATE, "bootstrapping / keyswitching key not loaded");
    struct Round {
        int64_t rows;         // ciphertexts per rank
        size_t first, mine;   // this rank's jobs: ks / pbs entries first .. first + mine
        size_t s_first, s_n;  // scatter list entries
        size_t k_first, k_n;  // order 0: this rank's keyswitch jobs of the round (one per output that is not skipped)
    };
    std::vector<Round> rounds;
    std::vector<Ks64Job> ks;
    std::vector<Pbs64Job> pbs;
    std::vector<int32_t> s_row, d_row;
    for (int64_t base = 0; base < count;) {
        const int64_t per = std::min(count - base, cts * world);
        const int64_t rows = (per + world - 1) / world;
        const int64_t lo = std::min(base + per, base + ctx->x_rank * rows), hi = std::min(base + per, lo + rows);
        Round R{rows, pbs.size(), (size_t)(hi - lo), s_row.size(), 0, ks.size(), 0};
        for (int64_t g = lo; g < hi; g++) {
            const int32_t q = (int32_t)pbs.size();
            if (ctx->order) {
                ks.push_back(Ks64Job{in_idx[g], q});
                pbs.push_back(Pbs64Job{q, lut_idx[g], (int32_t)((g - lo) * n_out), pad});
                continue;
            }
            // order 0: table row -> stage rows q n_out + x (every round's, before the first scatter) -> slot rows (g - lo) n_out + x
            pbs.push_back(Pbs64Job{in_idx[g], lut_idx[g], q * n_out, pad});
            for (int32_t x = 0; x < n_out; x++)
                if (out_idx[g * n_out + x] >= 0) ks.push_back(Ks64Job{q * n_out + x, (int32_t)((g - lo) * n_out + x)});
        }
        R.k_n = ks.size() - R.k_first;
        for (int64_t q = 0; q < per * n_out; q++) // the chunks are contiguous: gathered row q is output q % n_out of base + q / n_out
            if (out_idx[base * n_out + q] >= 0) {
                s_row.push_back((int32_t)q);
                d_row.push_back(out_idx[base * n_out + q]);
            }
        R.s_n = s_row.size() - R.s_first;
        rounds.push_back(R);
        base += per;
    }
    const size_t mine = pbs.size();
    if (ctx->order == 0) {
        const size_t need = mine * n_out * ((size_t)P.k * P.N + 1); // (bootstrap output rows)
        if (ctx->d_stage.cap < need) {
            if (int rc = drain(ctx)) return rc; // growing the staging area frees the old one
            if (ctx->d_stage.ensure(need)) return fail(HELM_ERR_OOM, "staging");
        }
    } else if (ctx->d_small.cap < mine * ((size_t)P.n + 1)) {
        if (int rc = drain(ctx)) return rc; // growing the scratch frees the old one
        if (ctx->d_small.ensure(mine * ((size_t)P.n + 1))) return fail(HELM_ERR_OOM, "small-LWE scratch");
    }
    if (int rc = luts_resident(ctx, luts, (size_t)n_luts * P.N)) return rc;
    helm_si_ctx::CallSlot *S = nullptr;
    if (int rc = slot_begin(ctx, ks.size() * sizeof(Ks64Job) + mine * sizeof(Pbs64Job) + 2 * s_row.size() * sizeof(int32_t) + 1024, &S))
        return rc;
    const Ks64Job *d_ks = slot_put(*S, ks.data(), ks.size());
    const Pbs64Job *d_pbs = slot_put(*S, pbs.data(), pbs.size());
    const int32_t *d_src = slot_put(*S, s_row.data(), s_row.size());
    const int32_t *d_dst = slot_put(*S, d_row.data(), d_row.size());
    if (int rc = slot_flush(ctx, *S)) return rc;
    if (mine && ctx->order == 0) { // this rank's share of every round, read from the table before the first scatter
        Timed t(ctx, &ctx->ev_pbs);
        HIP_TRY(launch_pbs64(ctx, d_pbs, (int64_t)mine, w->d, ctx->d_luts.p, ctx->d_stage.p));
        ctx->tacc.pbs_launches++;
        ctx->tacc.pbs_count += (int64_t)mine;
    } else if (mine) {
        Timed t(ctx, &ctx->ev_ks);
        HIP_TRY(launch_ks64(ctx, d_ks, (int64_t)mine, w->d, ctx->d_small.p));
        ctx->tacc.ks_launches++;
        ctx->tacc.ks_count += (int64_t)mine;
    }
    for (const Round &R : rounds) {
        const int64_t slot_rows = R.rows * n_out;
        if (ctx->order == 0) {
            if (R.k_n) {
                Timed t(ctx, &ctx->ev_ks);
                KsOutRows where;
                where.dense = slot_rows;
                HIP_TRY(launch_ks64(ctx, d_ks + R.k_first, (int64_t)R.k_n, ctx->d_stage.p, ctx->x_slot(slot_rows), &where));
                ctx->tacc.ks_launches++;
                ctx->tacc.ks_count += (int64_t)R.k_n;
            }
        } else if (R.mine) {
            Timed t(ctx, &ctx->ev_pbs);
            HIP_TRY(launch_pbs64(ctx, d_pbs + R.first, (int64_t)R.mine, ctx->d_small.p, ctx->d_luts.p, ctx->x_slot(slot_rows)));
            ctx->tacc.pbs_launches++;
            ctx->tacc.pbs_count += (int64_t)R.mine;
        }
        // the collective on this context's stream: every rank calls it, also one whose chunk is empty
        if (int rc = si_exchange(ctx, slot_rows)) return rc;
        if (int rc = drain(ctx)) return rc;
        if (R.s_n) {
            hipLaunchKernelGGL(k_rows64, dim3((unsigned)R.s_n), dim3(256), 0, ctx->stream, ctx->x_gather, d_src + R.s_first, w->d,
                               d_dst + R.s_first, dim);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipStreamSynchronize(ctx->stream)); // the next round overwrites the slot and the gather buffer
        ctx->x_batches++;
        ctx->x_rows += slot_rows * world;
    }
    return slot_end(ctx, *S);
}

uint64_t si_modulus(int pair, int f)
{
    if (pair == 2) return f ? L1::P_U64 : L0::P_U64;
    return pair ? (f ? J1::P_U64 : J0::P_U64) : (f ? F1::P_U64 : F0::P_U64);
}

// psi of field f of a pair: a primitive 2N-th root of unity.  pair 1 (the 46-bit fields): the one with psi^(N/4) = b - it is
// one of the primitive eighth roots b, b^3, -b, -b^3, and an odd power of psi puts it on b.  0: there is none.
uint64_t si_psi(int N, int pair, int f)
{
    const uint64_t p = si_modulus(pair, f);
    const uint64_t gen = pair == 2 ? (f ? L1::GEN : L0::GEN) : pair ? (f ? J1::GEN : J0::GEN) : (f ? F1::GEN : F0::GEN);
    const uint64_t psi = powmod_u64(gen, (p - 1) / (2 * (uint64_t)N), p);
    if (pair != 1) return psi;
    for (uint64_t t = 1; t < 8; t += 2)
        if (powmod_u64(powmod_u64(psi, t, p), (uint64_t)N / 4, p) == (uint64_t)(f ? J1::B1 : J0::B1)) return powmod_u64(psi, t, p);
    return 0;
}

// The forward twiddle tables (bit-reversed powers of psi), 1/N, 2^32 and the CRT constant of one pair of fields.  pair 1: with
// psi^(N/4) = b the first three table entries are b^2, b, b^3 - what the plain radix-4 top of a forward transform on digits
// multiplies by (fwd_top2_digits).
int setup_pair_tables(helm_si_ctx *ctx, int pair)
{
    SiKeyState &K = *ctx->keys;
    const uint64_t pm[2] = {si_modulus(pair, 0), si_modulus(pair, 1)};
    const double b1[2] = {J0::B1, J1::B1}, b2[2] = {J0::B2, J1::B2}, b3[2] = {J0::B3, J1::B3};
    const int N = ctx->P.N;
    for (int f = 0; f < 2; f++) {
        const uint64_t psi = si_psi(N, pair, f);
        if (!psi) return fail(HELM_ERR_STATE, "internal: no 2N-th root of unity with psi^(N/4) = b");
        std::vector<double> tf(N);
        power_table(tf.data(), psi, pm[f], N, ctx->logN);
        if (pair == 1 && (tf[1] != b2[f] || tf[2] != b1[f] || tf[3] != b3[f]))
            return fail(HELM_ERR_STATE, "internal: the first twiddles are not the constants the kernels assume");
        K.n_inv[f] = centred(powmod_u64((uint64_t)N, pm[f] - 2, pm[f]), pm[f]);
        K.two32[f] = centred((1ull << 32) % pm[f], pm[f]);
        if (!K.tw[f]) HIP_TRY(hipMalloc(&K.tw[f], sizeof(double) * N));
        HIP_TRY(hipMemcpy(K.tw[f], tf.data(), sizeof(double) * N, hipMemcpyHostToDevice));
    }
    K.p0inv_mod_p1 = centred(powmod_u64(pm[0] % pm[1], pm[1] - 2, pm[1]), pm[1]);
    K.pair = pair;
    return 0;
}

// A context whose launches run k_pbs64_generic: the inverse twiddle tables of the 49-bit pair, the kernel's LDS attribute and
// occupancy, and the digit batch D.  Refuses the shape cleanly if no workgroup of it fits a CU.
int setup_generic(helm_si_ctx *ctx)
{
#ifdef HELM_CHECK_BOUNDS
    // The -O0 counting build of k_pbs64_generic faulted on its first launch (a memory-aperture violation; the -O3 build of the
    // same source is bit-exact against the oracle on every shape tested), and the cause is not found yet:
    // until it is, this build refuses the generic class before anything is launched.
    (void)ctx;
    return fail(HELM_ERR_STATE, "the generic kernel is not available in the bound-checking build (libhelm_hip_check.so): "
                                "use the regular library for generic contexts");
#endif
    SiKeyState &K = *ctx->keys;
    const helm_si_params &P = ctx->P;
    const int N = P.N, logN = ctx->logN;
    for (int f = 0; f < 2; f++) {
        const uint64_t p = si_modulus(0, f);
        std::vector<double> ti(N);
        power_table(ti.data(), powmod_u64(si_psi(N, 0, f), p - 2, p), p, N, logN);
        if (!K.twi[f]) HIP_TRY(hipMalloc(&K.twi[f], sizeof(double) * N));
        HIP_TRY(hipMemcpy(K.twi[f], ti.data(), sizeof(double) * N, hipMemcpyHostToDevice));
    }
    const int group = P.grouping_factor > 1 ? P.grouping_factor : 1;
    const void *kern = pbs64_generic_kernel(logN, group);
    TwoPrimeFit fit;
    HIP_TRY(tp_fit<uint64_t>(kern, N, P.k, P.pbs_l, P.n, fit));
    if (fit.per_cu < 1)
        return fail(HELM_ERR_INVALID, "k_pbs64_generic: no workgroup of " + std::to_string(fit.lds) + " B LDS fits a CU for this shape");
    K.gen_d = fit.d;
    K.lds = fit.lds;
    K.per_cu = fit.per_cu;
    if (getenv("HELM_HIP_VERBOSE")) {
        hipFuncAttributes fa{};
        (void)hipFuncGetAttributes(&fa, kern);
        fprintf(stderr, "[helm_si] k_pbs64_generic N=%d k=%d l=%d g=%d D=%d: LDS %zu B, regs %d, scratch %zu B, %d workgroups/CU\n",
                N, P.k, P.pbs_l, group, K.gen_d, K.lds, fa.numRegs, (size_t)fa.localSizeBytes, K.per_cu);
    }
    return 0;
}

// the shapes k_pbs64_large takes (helm_si_ctx_create_ex with HELM_SI_CREATE_LARGE_N): k = 1, N = 4096, classical blind rotation
bool si_large_domain(const helm_si_params &P)
{
    return P.k == 1 && P.N == 4096 && P.pbs_l >= 1 && P.grouping_factor <= 1;
}

// the multi-bit shapes the two large-N kernels take under HELM_SI_CREATE_LARGE_MULTIBIT beside the bit of their N (4096:
// k_pbs64_large, 8192: k_pbs64_n8192): grouping_factor 2 or 3 (that it divides n is checked with n)
bool si_large_multibit_domain(const helm_si_params &P, int N)
{
    return P.k == 1 && P.N == N && P.pbs_l >= 1 && P.grouping_factor >= 2 && P.grouping_factor <= 3;
}

#ifndef HELM_CHECK_BOUNDS
// What a context of either large-N kernel sets up (name: the kernel's, shape: what its verbose line says beside it): the
// inverse twiddle tables of the pair FpG / FpI; the kernel's dynamic-LDS attribute, which is the kernel's and shared by every
// context of the process, so it is set once per device over the three instantiations (kernel(0), kernel(2), kernel(3)) at
// lds_max, the layout at the largest n; the workgroups per CU of this context's instantiation at its own layout of lds bytes.
int setup_large_class(helm_si_ctx *ctx, const char *name, const char *shape, const void *(*kernel)(int),
                      std::atomic<bool> (&attr_done)[64], size_t lds_max, size_t lds, int *per_cu)
{
    SiKeyState &K = *ctx->keys;
    const helm_si_params &P = ctx->P;
    const int N = P.N, logN = ctx->logN;
    for (int f = 0; f < 2; f++) {
        const uint64_t p = si_modulus(2, f);
        std::vector<double> ti(N);
        power_table(ti.data(), powmod_u64(si_psi(N, 2, f), p - 2, p), p, N, logN);
        if (!K.twi[f]) HIP_TRY(hipMalloc(&K.twi[f], sizeof(double) * N));
        HIP_TRY(hipMemcpy(K.twi[f], ti.data(), sizeof(double) * N, hipMemcpyHostToDevice));
    }
    const void *kern = kernel(P.grouping_factor);
    HIP_TRY(lds_attr_once(attr_done, ctx->device, {kernel(0), kernel(2), kernel(3)}, lds_max));
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, kern, L64_THREADS, lds));
    if (*per_cu < 1)
        return fail(HELM_ERR_INVALID, std::string(name) + ": no workgroup of " + std::to_string(lds) + " B LDS fits a CU");
    if (getenv("HELM_HIP_VERBOSE")) {
        hipFuncAttributes fa{};
        (void)hipFuncGetAttributes(&fa, kern);
        fprintf(stderr, "[helm_si] %s%s l=%d g=%d: LDS %zu B, regs %d, scratch %zu B, %d workgroups/CU\n", name, shape, P.pbs_l,
                P.grouping_factor > 1 ? P.grouping_factor : 1, lds, fa.numRegs, (size_t)fa.localSizeBytes, *per_cu);
    }
    return 0;
}
#endif

// A context whose launches run k_pbs64_large: setup_large_class and the dynamic-LDS limit of its key conversion.
int setup_large(helm_si_ctx *ctx)
{
#ifdef HELM_CHECK_BOUNDS
    // as setup_generic: the bound-checking build runs the tuned kernels only, and refuses before anything is launched
    (void)ctx;
    return fail(HELM_ERR_STATE, "the large-N kernel is not available in the bound-checking build (libhelm_hip_check.so): "
                                "use the regular library for HELM_SI_CREATE_LARGE_N contexts");
#else
    SiKeyState &K = *ctx->keys;
    const int N = ctx->P.N;
    static std::atomic<bool> attr_done[64], conv_done[64];
    K.lds = Large64Lds(N, ctx->P.n).bytes;
    if (int rc = setup_large_class(ctx, "k_pbs64_large", " N=4096", pbs64_large_kernel, attr_done, Large64Lds(N, 1024).bytes,
                                   K.lds, &K.per_cu))
        return rc;
    HIP_TRY(lds_attr_once(conv_done, ctx->device, {reinterpret_cast<const void *>(k_bsk_convert64_large<12>)},
                          sizeof(double) * 2 * (size_t)N));
    return 0;
#endif
}

// the shapes k_pbs64_n8192 takes (helm_si_ctx_create_ex with HELM_SI_CREATE_N8192): k = 1, N = 8192, classical blind rotation
bool si_n8192_domain(const helm_si_params &P)
{
    return P.k == 1 && P.N == 8192 && P.pbs_l >= 1 && P.grouping_factor <= 1;
}

// The accumulator rows of a context (primary or lane) whose launches run k_pbs64_n8192: one row of 2 N words per CU, the
// width of a launch chunk (launch_pbs64_n8192).  Made with the context, never resized.
int alloc_acc8192(helm_si_ctx *ctx)
{
    const size_t words = (size_t)std::max(ctx->n_cus, 1) * ((size_t)2 << N8192_LOGN);
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ctx->d_acc8192), words * sizeof(uint64_t)));
    return 0;
}

// A context whose launches run k_pbs64_n8192: setup_large_class, the dynamic-LDS limit of its key conversion and its
// accumulator rows.
int setup_n8192(helm_si_ctx *ctx)
{
#ifdef HELM_CHECK_BOUNDS
    // as setup_large: the bound-checking build runs the tuned kernels only, and refuses before anything is launched
    (void)ctx;
    return fail(HELM_ERR_STATE, "the N = 8192 kernel is not available in the bound-checking build (libhelm_hip_check.so): "
                                "use the regular library for HELM_SI_CREATE_N8192 contexts");
#else
    SiKeyState &K = *ctx->keys;
    static std::atomic<bool> attr_done[64], conv_done[64];
    K.lds = N8192Lds(ctx->P.n).bytes;
    if (int rc = setup_large_class(ctx, "k_pbs64_n8192", "", pbs64_n8192_kernel, attr_done, N8192Lds(1024).bytes, K.lds, &K.per_cu))
        return rc;
    K.per_cu = 1; // (whatever fits: a launch is one workgroup per CU, launch_pbs64_n8192)
    HIP_TRY(lds_attr_once(conv_done, ctx->device, {reinterpret_cast<const void *>(k_bsk_convert64_large<N8192_LOGN>)},
                          sizeof(double) * 2 * (size_t)ctx->P.N));
    return alloc_acc8192(ctx);
#endif
}

// What a new context sets up for its kernel: the tables of its pair and what its class adds to them (a tuned form: nothing)
int setup_class(helm_si_ctx *ctx, int pair)
{
    if (int rc = setup_pair_tables(ctx, pair)) return rc;
    switch (ctx->keys->run.cls) {
    case SI_GENERIC: return setup_generic(ctx);
    case SI_LARGE: return setup_large(ctx);
    case SI_N8192: return setup_n8192(ctx);
    case SI_TUNED: break;
    }
    return 0;
}

// The step bound of a bootstrapping key: the exact integer coefficient of one blind-rotation step is at most B/2 x the largest
// l1-norm over the key polynomials (taken as centred 64-bit words) that meet in one output column - or, transposed, in one row.
// A step sums `per_step` polynomials, laid out [...][r][c][N] (classical: the pbs_l (k+1)^2 of one GGSW; the generic multi-bit
// form: those of the 2^g subsets of a group, whose products it adds up before the CRT lift).  Exact for the key at hand and every
// input.
long double key_step_bound(const helm_si_params &P, const uint64_t *bsk_std, size_t steps, size_t per_step)
{
    const size_t K1 = P.k + 1;
    std::vector<long double> l1(per_step);
    long double worst = 0;
    for (size_t i = 0; i < steps; i++) {
        for (size_t q = 0; q < per_step; q++) {
            const uint64_t *poly = bsk_std + (i * per_step + q) * P.N;
            long double sum = 0;
            for (int j = 0; j < P.N; j++) {
                const int64_t v = (int64_t)poly[j];
                sum += v < 0 ? -(long double)v : (long double)v;
            }
            l1[q] = sum;
        }
        for (size_t c = 0; c < K1; c++) {
            long double by_col = 0, by_row = 0;
            for (size_t q = 0; q < per_step; q++) {
                if (q % K1 == c) by_col += l1[q];
                if ((q / K1) % K1 == c) by_row += l1[q];
            }
            worst = std::max(worst, std::max(by_col, by_row));
        }
    }
    return worst * (long double)(1ull << (P.pbs_logB - 1));
}

// What both key loaders begin with.  A lane refuses a key: the keys are its primary's.  On a primary, nothing in flight - on
// its own stream or on the stream of any of its lanes - may still read the tables and key buffers a load rewrites.
int begin_key_load(helm_si_ctx *ctx, const char *what)
{
    if (ctx->lane_of)
        return fail(HELM_ERR_INVALID, std::string(what) + ": this context is a lane; load keys into its primary (every lane sees them)");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (helm_si_ctx *lane : ctx->lanes) HIP_TRY(hipStreamSynchronize(lane->stream));
    return 0;
}

// A bootstrapping key in standard form (d_std: `polys` polynomials on the device, [i][lev][r][c][N]) into the layout(s) the
// context's kernel reads, in the fields of the pair its tables hold.  Buffers are allocated by the first key and refilled by
// every later one.
//
//   class     form      kernel               fills                      conversion kernel(s)                    pair
//   tuned     wide      k_pbs64              bsk                        k_bsk_convert64 per field               0
//   tuned     split     k_pbs64s<., false>   bsk and bsk_split          k_bsk_convert64, k_bsk_convert64s       0
//   tuned     split mb  k_pbs64s<., true>    bsk_split (expo: probed    k_bsk_convert64s                        0
//                                            once, after the first key)
//   tuned     k         k_pbs64k             bsk                        k_bsk_convert64 per field               0; N = 512: 0 or 1,
//                                                                                                               after the key at hand
//   generic             k_pbs64_generic      bsk, [i][r][c][lev][f][N]  k_bsk_convert64_generic, both fields    0
//   large-N             k_pbs64_large        bsk, the same layout       k_bsk_convert64_large<12>               2
//   N = 8192            k_pbs64_n8192        bsk, the same layout       k_bsk_convert64_large<13>               2
int convert_bootstrap_key(helm_si_ctx *ctx, const uint64_t *d_std, size_t n_words, size_t polys)
{
    SiKeyState &K = *ctx->keys;
    const helm_si_params &P = ctx->P;
    const int K1 = P.k + 1;
    // [i][r][c][lev][f][N], bit-reversed transform order, both fields in one launch
    const auto both_fields = [&](auto kern, unsigned threads, size_t lds) {
        hipLaunchKernelGGL(kern, dim3((unsigned)polys), dim3(threads), lds, ctx->stream, d_std, K.bsk, K.tw[0], K.tw[1],
                           K.n_inv[0], K.n_inv[1], K.two32[0], K.two32[1], K1, P.pbs_l);
    };
    if (!K.bsk && K.run.form != SI_SPLIT_MB) HIP_TRY(hipMalloc(&K.bsk, n_words * 2 * sizeof(double)));
    if (!K.bsk_split && K.run.split_key()) HIP_TRY(hipMalloc(&K.bsk_split, n_words * 2 * sizeof(double)));
    switch (K.run.cls) {
    case SI_N8192: both_fields(k_bsk_convert64_large<N8192_LOGN>, L64_THREADS, sizeof(double) * 2 * (size_t)P.N); break; // (the two-
    case SI_LARGE: both_fields(k_bsk_convert64_large<12>, L64_THREADS, sizeof(double) * 2 * (size_t)P.N); break; // field buffer in LDS)
    case SI_GENERIC:
        with_logn<8, 11>(ctx->logN, false, [&](auto ln) {
            both_fields(k_bsk_convert64_generic<decltype(ln)::value>, TP_THREADS, 0);
            return true;
        });
        break;
    case SI_TUNED: break; // by its form, below
    }
    // the lane order of k_pbs64 and k_pbs64k, one launch per field (pair 1 is built for N = 512 only)
    const auto wide = [&] {
        const auto fields = [&](auto kern0, auto kern1) {
            hipLaunchKernelGGL(kern0, dim3((unsigned)polys), dim3(64), 0, ctx->stream, d_std, K.bsk, K.tw[0], K.n_inv[0],
                               K.two32[0], K1, P.pbs_l, 0);
            hipLaunchKernelGGL(kern1, dim3((unsigned)polys), dim3(64), 0, ctx->stream, d_std, K.bsk, K.tw[1], K.n_inv[1],
                               K.two32[1], K1, P.pbs_l, 1);
            return true;
        };
        if (K.pair == 1) fields(k_bsk_convert64<J0, 9>, k_bsk_convert64<J1, 9>);
        else with_logn<9, 11>(ctx->logN, false, [&](auto ln) {
            return fields(k_bsk_convert64<F0, decltype(ln)::value>, k_bsk_convert64<F1, decltype(ln)::value>);
        });
    };
    // the half-transform order of k_pbs64s
    const auto split = [&] { launch_convert64s(ctx, d_std, K.bsk_split, polys, K.n_inv, K1, P.pbs_l); };
    switch (K.run.form) {
    case SI_WIDE:
    case SI_K: wide(); break;
    case SI_SPLIT: wide(), split(); break;
    case SI_SPLIT_MB: split(); break;
    case SI_NO_FORM: break;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// What a class has of its own beside its kernel, by SiClass: the CRT pair its context is created in (0: FpG / FpG2, 2:
// FpG / FpI; an SI_K context may move to pair 1 with a key, helm_si_load_bootstrap_key), the capacity p0 p1 / 2 of that pair
// (pair 2: 2^97.87), its name in the key-capacity error and in helm_wop_ctx_create's refusal.
struct SiClassFacts { int pair; long double half; const char *noun, *wop; };
constexpr long double SI_HALF_F = (long double)F0::P * F1::P / 2, SI_HALF_L = (long double)L0::P * L1::P / 2;
constexpr SiClassFacts SI_CLASS[4] = {
    {0, SI_HALF_F, "tuned", nullptr},
    {0, SI_HALF_F, "generic", "generic bootstrap kernel (helm_si_kernel_class 1)"},
    {2, SI_HALF_L, "large-N", "large-N bootstrap kernel (helm_si_kernel_class 2)"},
    {2, SI_HALF_L, "N = 8192", "N = 8192 bootstrap kernel (HELM_SI_CREATE_N8192, helm_si_kernel_class 3)"}};

// helm_si_ctx_create_ex, the half without a device: whether (params, flags) is admitted and, if so, what the context runs
// (*run), its order (helm_si_pbs_order) and its grouping factor (1: classical blind rotation)
int si_admit(const helm_si_params &P, int flags, SiKernelForm *run, int *order_out, int *group_out)
{
    // HELM_SI_CREATE_LARGE_N matters at N >= 4096 only: below, the call is the same call without the bit
    // HELM_SI_CREATE_N8192 matters at N >= 8192 only, in the same way; beside HELM_SI_CREATE_LARGE_N, N selects the kernel
    const bool n8192 = (flags & HELM_SI_CREATE_N8192) != 0 && P.N >= 8192;
    const bool large = (flags & HELM_SI_CREATE_LARGE_N) != 0 && P.N >= 4096 && !n8192;
    // HELM_SI_CREATE_PBS_KS changes no admission rule: the checks below see the flags without it
    const bool pbs_ks = (flags & HELM_SI_CREATE_PBS_KS) != 0;
    // HELM_SI_CREATE_LARGE_MULTIBIT matters for grouping_factor > 1 at N >= 4096 only, beside the bit of that N
    const bool large_mb_bit = (flags & HELM_SI_CREATE_LARGE_MULTIBIT) != 0;
    const bool large_mb = large_mb_bit && (large || n8192) && P.grouping_factor > 1;
    if (flags & ~(HELM_SI_CREATE_ALLOW_GENERIC | HELM_SI_CREATE_FORCE_GENERIC | HELM_SI_CREATE_GENERIC_MULTIBIT |
                  HELM_SI_CREATE_LARGE_N | HELM_SI_CREATE_PBS_KS | HELM_SI_CREATE_N8192 | HELM_SI_CREATE_LARGE_MULTIBIT))
        return fail(HELM_ERR_INVALID, "unknown bits in flags " + std::to_string(flags) +
                                          " (HELM_SI_CREATE_ALLOW_GENERIC = 1, HELM_SI_CREATE_FORCE_GENERIC = 2, "
                                          "HELM_SI_CREATE_GENERIC_MULTIBIT = 16" +
                                          ((flags & HELM_SI_CREATE_LARGE_N) ? ", HELM_SI_CREATE_LARGE_N = 32" : "") +
                                          (pbs_ks ? ", HELM_SI_CREATE_PBS_KS = 64" : "") +
                                          ((flags & HELM_SI_CREATE_N8192) ? ", HELM_SI_CREATE_N8192 = 256" : "") +
                                          (large_mb_bit ? ", HELM_SI_CREATE_LARGE_MULTIBIT = 1024" : "") +
                                          "; 4 and 8 are reserved)");
    if (large_mb_bit && !(flags & (HELM_SI_CREATE_LARGE_N | HELM_SI_CREATE_N8192)))
        return fail(HELM_ERR_INVALID, "flags " + std::to_string(flags) + ": HELM_SI_CREATE_LARGE_MULTIBIT goes with "
                                          "HELM_SI_CREATE_LARGE_N and/or HELM_SI_CREATE_N8192");
    flags &= ~(HELM_SI_CREATE_LARGE_N | HELM_SI_CREATE_PBS_KS | HELM_SI_CREATE_N8192 | HELM_SI_CREATE_LARGE_MULTIBIT);
    const bool force = (flags & HELM_SI_CREATE_FORCE_GENERIC) != 0;
    const bool multibit = (flags & HELM_SI_CREATE_GENERIC_MULTIBIT) != 0;
    if (multibit && !(flags & (HELM_SI_CREATE_ALLOW_GENERIC | HELM_SI_CREATE_FORCE_GENERIC)))
        return fail(HELM_ERR_INVALID, "flags " + std::to_string(flags) + ": HELM_SI_CREATE_GENERIC_MULTIBIT goes with "
                                          "HELM_SI_CREATE_ALLOW_GENERIC or HELM_SI_CREATE_FORCE_GENERIC");
    if (force && P.grouping_factor > 1 && !multibit)
        return fail(HELM_ERR_INVALID, "HELM_SI_CREATE_FORCE_GENERIC: the generic kernel has no multi-bit form (grouping_factor > 1)");
    // with HELM_SI_CREATE_GENERIC_MULTIBIT a multi-bit shape is tuned only where the tuned multi-bit build serves it
    if (large_mb && !si_large_multibit_domain(P, large ? 4096 : 8192))
        return fail(HELM_ERR_INVALID, "unsupported (k,N,pbs_l) for the multi-bit form of the large-N kernels: the domain under "
                                      "HELM_SI_CREATE_LARGE_MULTIBIT is k = 1, pbs_l >= 1, grouping_factor 2 or 3 dividing n, at "
                                      "N = 4096 beside HELM_SI_CREATE_LARGE_N and at N = 8192 beside HELM_SI_CREATE_N8192 (k > 1, "
                                      "grouping_factor >= 4 and N >= 16384 are out of scope)");
    if (large && !large_mb && !si_large_domain(P))
        return fail(HELM_ERR_INVALID, "unsupported (k,N,pbs_l) for the large-N kernel: its domain under HELM_SI_CREATE_LARGE_N is "
                                      "k = 1, N = 4096, pbs_l >= 1, grouping_factor <= 1 (k > 1 at N = 4096, multi-bit at "
                                      "N = 4096 and N = 8192 are out of scope)");
    if (n8192 && !large_mb && !si_n8192_domain(P))
        return fail(HELM_ERR_INVALID, "unsupported (k,N,pbs_l) for the N = 8192 kernel: its domain under HELM_SI_CREATE_N8192 is "
                                      "k = 1, N = 8192, pbs_l >= 1, grouping_factor <= 1 (k > 1 at N = 8192, multi-bit at "
                                      "N = 8192 and N >= 16384 are out of scope)");
    const bool tuned = large || n8192 || (si_supported(P) && !(multibit && P.grouping_factor > 1 && !si_tuned_multibit(P)));
    if (!tuned && flags == 0)
        return fail(HELM_ERR_INVALID, "unsupported (k,N,pbs_l): built variants are k = 1, N in {512,1024,2048}, pbs_l in {1,2}; k in {2,3}, N = 512, pbs_l = 1; k = 2, N = 1024, pbs_l = 1");
    if (!tuned && P.grouping_factor > 1 && !multibit)
        return fail(HELM_ERR_INVALID, "multi-bit blind rotation (grouping_factor > 1) runs on the tuned builds only: this shape "
                                      "(k,N,pbs_l) has none, and the generic kernel has no multi-bit form");
    const bool run_generic = !large && !n8192 && (force || !tuned); // (the large-N shapes have one kernel each, under every generic bit)
    const bool gen_mb = run_generic && multibit && P.grouping_factor > 1; // the generic kernel's multi-bit form
    if (gen_mb && (P.grouping_factor > 3 || P.n % P.grouping_factor))
        return fail(HELM_ERR_INVALID, "grouping_factor must be 0..3 and divide n");
    if ((!tuned || gen_mb) && !si_generic_domain(P, gen_mb))
        return fail(HELM_ERR_INVALID, std::string("unsupported (k,N,pbs_l) for the generic kernel: its domain is N in {256,512,1024,2048}, "
                                      "k >= 1 with (k+1) N <= 4096, pbs_l >= 1, ") +
                                          (gen_mb ? "grouping_factor <= 3 under HELM_SI_CREATE_GENERIC_MULTIBIT" : "grouping_factor <= 1"));
    if (P.n < 1 || P.n > 1024) return fail(HELM_ERR_INVALID, "n must be in [1,1024]");
    // (pbs_logB <= 24: the kernels multiply digits by the field's fourth root of unity, 25 bits, without a reduction)
    if (P.pbs_logB < 2 || P.pbs_logB > 24 || P.pbs_logB * P.pbs_l > 31)
        return fail(HELM_ERR_INVALID, "bad PBS decomposition (pbs_logB <= 24 and pbs_logB * pbs_l <= 31: every tfhe shortint set)");
    if (P.ks_logB < 1 || P.ks_logB > 7 || P.ks_l < 1 || P.ks_l > 8 || P.ks_logB * P.ks_l > 63)
        return fail(HELM_ERR_INVALID, "bad keyswitch decomposition (ks_logB <= 7, ks_l <= 8)");
    const int t = P.message_modulus * P.carry_modulus;
    if (P.message_modulus < 2 || P.carry_modulus < 1 || (t & (t - 1)) || t > P.N / 2)
        return fail(HELM_ERR_INVALID, "message_modulus * carry_modulus must be a power of two <= N/2");
    const int group = P.grouping_factor > 1 ? P.grouping_factor : 1;
    if (P.grouping_factor < 0 || group > 3 || P.n % group)
        return fail(HELM_ERR_INVALID, "grouping_factor must be 0..3 and divide n");
    if (group > 1 && !gen_mb && !large_mb && !(P.pbs_l == 1 && P.N >= 1024))
        return fail(HELM_ERR_INVALID, "multi-bit blind rotation is built for pbs_l = 1, N >= 1024 (every tfhe multi-bit set)");
    run->cls = n8192 ? SI_N8192 : large ? SI_LARGE : run_generic ? SI_GENERIC : SI_TUNED;
    // exactness: |sum| <= (k+1) * l * N * (B/2) * 2^63 must stay below p0 * p1 / 2 of the class's pair
    {
        const long double bound = (long double)(P.k + 1) * P.pbs_l * P.N * (long double)(1ull << (P.pbs_logB - 1)) *
                                  9223372036854775808.0L;
        if (bound * 1.001L >= SI_CLASS[run->cls].half) return fail(HELM_ERR_INVALID, "parameter set exceeds the two-prime NTT capacity");
        // per-field operands: digits must be far below p
        if ((double)(1ull << (P.pbs_logB - 1)) * 4 >= F1::P / 2) return fail(HELM_ERR_INVALID, "pbs_logB too large");
    }
    // The tuned form.  The eight-wave kernel (split transforms) where it exists: k = 1, N >= 1024, one level or two with
    // digits of at most 15 bits, unless HELM_SI_SPLIT=0; its multi-bit build for every tuned multi-bit shape (k = 1,
    // pbs_l = 1, N >= 1024: the checks above).
    const char *split_env = getenv("HELM_SI_SPLIT");
    const bool split = ((P.pbs_l == 1 && P.pbs_logB <= 24) || (P.pbs_l == 2 && P.pbs_logB <= 15)) && P.N >= 1024 && P.k == 1 &&
                       !(split_env && atoi(split_env) == 0);
    run->form = run->cls != SI_TUNED ? SI_NO_FORM : P.k >= 2 ? SI_K : group > 1 ? SI_SPLIT_MB : split ? SI_SPLIT : SI_WIDE;
    *order_out = pbs_ks ? 0 : 1;
    *group_out = group;
    return 0;
}

} // namespace

extern "C" {

int helm_si_ctx_create(int device_id, const helm_si_params *params, helm_si_ctx **out)
{
    return helm_si_ctx_create_ex(device_id, params, 0, out);
}

int helm_si_ctx_create_ex(int device_id, const helm_si_params *params, int flags, helm_si_ctx **out)
{
    if (!params || !out) return fail(HELM_ERR_INVALID, "null argument");
    *out = nullptr;
    const helm_si_params &P = *params;
    SiKernelForm run;
    int order = 1, group = 1;
    if (int rc = si_admit(P, flags, &run, &order, &group)) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(HELM_ERR_NO_DEVICE, "no HIP device visible (this engine has no CPU fallback)");
    if (device_id < 0 || device_id >= ndev) return fail(HELM_ERR_NO_DEVICE, "device_id out of range");
    HIP_TRY(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device_id));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(HELM_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
    helm_si_ctx *ctx = new (std::nothrow) helm_si_ctx();
    if (!ctx) return fail(HELM_ERR_OOM, "ctx");
    ctx->device = device_id;
    ctx->P = P;
    ctx->order = order;
    ctx->n_cus = prop.multiProcessorCount;
    while ((1 << ctx->logN) < P.N) ctx->logN++;
    ctx->delta = (1ull << 63) / (uint64_t)(P.message_modulus * P.carry_modulus);
    ctx->own_keys.reset(new (std::nothrow) SiKeyState());
    ctx->keys = ctx->own_keys.get();
    if (!ctx->keys) {
        delete ctx;
        return fail(HELM_ERR_OOM, "ctx");
    }
    SiKeyState &K = *ctx->keys;
    HIP_TRY(hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking));
    ctx->stream = ctx->own_stream;
    const int N = P.N, pair = SI_CLASS[run.cls].pair;
    K.run = run;
    K.group = group;
    if (int rc = setup_class(ctx, pair)) {
        (void)helm_si_ctx_destroy(ctx);
        return rc;
    }
    if (K.group > 1) { // the 2N powers of psi per field of the context's pair: monomial products in the transform domain
        std::vector<double> pw((size_t)4 * N);
        for (int f = 0; f < 2; f++) power_table(pw.data() + (size_t)f * 2 * N, si_psi(N, pair, f), si_modulus(pair, f), 2 * N, 0);
        HIP_TRY(hipMalloc(&K.psi_pow, pw.size() * sizeof(double)));
        HIP_TRY(hipMemcpy(K.psi_pow, pw.data(), pw.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    static_assert(Pbs64sCfg<11, 2>::BYTES <= 160 * 1024, "k_pbs64s<11, 2> must fit the LDS of a CU");
    if (const char *v = getenv("HELM_HIP_KS_MFMA")) K.ks_mfma = atoi(v);
    if (K.run.split_key()) { // the half-transform tables of k_pbs64s and its key conversion
        // half h of field f, stage with m' groups, group i': full table entry 2m' + h m' + i'
        std::vector<double> sub((size_t)4 * (N / 2), 0.0), full(N);
        for (int f = 0; f < 2; f++) {
            HIP_TRY(hipMemcpy(full.data(), K.tw[f], sizeof(double) * N, hipMemcpyDeviceToHost));
            for (int h = 0; h < 2; h++)
                for (int m = 1; m < N / 2; m <<= 1)
                    for (int i = 0; i < m; i++) sub[(size_t)(f * 2 + h) * (N / 2) + m + i] = full[2 * m + h * m + i];
        }
        HIP_TRY(hipMalloc(&K.tw_sub, sub.size() * sizeof(double)));
        HIP_TRY(hipMemcpy(K.tw_sub, sub.data(), sub.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    *out = ctx;
    return 0;
}

int helm_si_ctx_fork(helm_si_ctx *primary, helm_si_ctx **out)
{
    if (!primary || !out) return fail(HELM_ERR_INVALID, "null argument");
    *out = nullptr;
    if (primary->lane_of) return fail(HELM_ERR_INVALID, "fork the primary context, not one of its lanes");
    if (!primary->keys->have_bsk || !primary->keys->have_ksk) return fail(HELM_ERR_STATE, "load the keys before forking a lane");
    HIP_TRY(hipSetDevice(primary->device));
    helm_si_ctx *ctx = new (std::nothrow) helm_si_ctx();
    if (!ctx) return fail(HELM_ERR_OOM, "ctx");
    ctx->device = primary->device;
    ctx->lane_of = primary;
    ctx->keys = primary->keys; // keys, tables and what a later load makes of them: the primary's, not a copy
    ctx->P = primary->P;
    ctx->logN = primary->logN;
    ctx->order = primary->order;
    ctx->delta = primary->delta;
    ctx->n_cus = primary->n_cus;
    ctx->audit_fn = primary->audit_fn; // a lane is audited like its primary
    ctx->audit_user = primary->audit_user;
    ctx->level_many = primary->level_many; // ... and groups the gates of a level like it
    hipError_t e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete ctx;
        return fail(HELM_ERR_HIP, std::string("hipStreamCreateWithFlags: ") + hipGetErrorString(e));
    }
    ctx->stream = ctx->own_stream;
    if (primary->keys->run.cls == SI_N8192) { // a lane launches on its own stream: accumulator rows of its own
        if (int rc = alloc_acc8192(ctx)) {
            (void)hipStreamDestroy(ctx->own_stream);
            delete ctx;
            return rc;
        }
    }
    primary->lanes.push_back(ctx);
    *out = ctx;
    return 0;
}

int helm_si_ctx_destroy(helm_si_ctx *ctx)
{
    if (!ctx) return 0;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (auto *l : {&ctx->ev_pbs, &ctx->ev_ks, &ctx->ev_lin})
        for (auto &p : *l) {
            (void)hipEventDestroy(p.first);
            (void)hipEventDestroy(p.second);
        }
    for (auto *w : ctx->child_wires) {
        (void)hipFree(w->d);
        w->d = nullptr;
        w->owner = nullptr;
    }
    if (ctx->lane_of) {
        auto &ls = ctx->lane_of->lanes;
        ls.erase(std::remove(ls.begin(), ls.end(), ctx), ls.end());
    }
    (void)hipFree(ctx->x_own); // (helm_si_set_exchange_comm; a lane has none)
    for (auto &S : ctx->slots) {
        if (S.host) (void)hipHostFree(S.host);
        if (S.dev) (void)hipFree(S.dev);
        if (S.done) (void)hipEventDestroy(S.done);
    }
    ctx->d_ksdig.release();
    ctx->d_ksdsum.release();
    ctx->d_ksbody.release();
    ctx->d_pbs.release();
    ctx->d_ks.release();
    ctx->d_small.release();
    ctx->d_luts.release();
    ctx->d_stage.release();
    ctx->d_body.release();
    ctx->d_idx.release();
    ctx->d_idx2.release();
    ctx->d_coef.release();
    (void)hipFree(ctx->d_acc8192);
    (void)hipStreamDestroy(ctx->own_stream);
    delete ctx; // (a primary's key state goes with it: SiKeyState frees its device memory)
    return 0;
}

int helm_si_get_params(const helm_si_ctx *ctx, helm_si_params *out)
{
    if (!ctx || !out) return fail(HELM_ERR_INVALID, "null argument");
    *out = ctx->P;
    return 0;
}

int helm_si_field_bits(const helm_si_ctx *ctx)
{
    if (!ctx) return fail(HELM_ERR_INVALID, "null argument");
    return ctx->keys->pair == 2 ? 50 : ctx->keys->pair ? 46 : 49;
}

int helm_si_pbs_order(const helm_si_ctx *ctx)
{
    if (!ctx) return fail(HELM_ERR_INVALID, "null argument");
    return ctx->order;
}

int64_t helm_si_wire_words(const helm_si_ctx *ctx)
{
    if (!ctx) return fail(HELM_ERR_INVALID, "null argument");
    return (int64_t)ctx->wire_row();
}

int helm_si_kernel_class(const helm_si_ctx *ctx)
{
    if (!ctx) return fail(HELM_ERR_INVALID, "null argument");
    return ctx->keys->run.cls;
}

int helm_si_set_stream(helm_si_ctx *ctx, void *hip_stream)
{
    if (!ctx) return fail(HELM_ERR_INVALID, "null ctx");
    if (int rc = helm_hip_runtime_guard_("helm_si_set_stream")) return rc; // the handle was made by the caller's HIP runtime
    // NULL is HIP's null (legacy default) stream - what torch.cuda.current_stream() is unless the caller
    // switched streams - NOT "back to the context's own stream": collectives the caller orders on that
    // stream must see the engine's kernels on it
    ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
    return 0;
}

int helm_si_set_priority(helm_si_ctx *ctx, int high)
{
    if (!ctx) return fail(HELM_ERR_INVALID, "null ctx");
    if (ctx->stream != ctx->own_stream) return 0; // the caller's stream: its priority is the caller's business
    if ((high != 0) == ctx->high_priority) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    int least = 0, greatest = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIP_TRY(hipStreamSynchronize(ctx->own_stream));
    hipStream_t s = nullptr;
    HIP_TRY(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, high ? greatest : least));
    (void)hipStreamDestroy(ctx->own_stream);
    ctx->own_stream = ctx->stream = s;
    ctx->high_priority = high != 0;
    return 0;
}

int helm_si_sync(helm_si_ctx *ctx)
{
    if (!ctx) return fail(HELM_ERR_INVALID, "null ctx");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int helm_si_load_bootstrap_key(helm_si_ctx *ctx, const uint64_t *bsk_std, size_t n_words)
{
    if (!ctx || !bsk_std) return fail(HELM_ERR_INVALID, "null argument");
    SiKeyState &K = *ctx->keys;
    const helm_si_params &P = ctx->P;
    const size_t K1 = P.k + 1;
    const size_t n_ggsw = K.group > 1 ? (size_t)(P.n / K.group) << K.group : (size_t)P.n;
    const size_t per_ggsw = (size_t)P.pbs_l * K1 * K1, polys = n_ggsw * per_ggsw;
    if (n_words != polys * P.N)
        return fail(HELM_ERR_INVALID, "bootstrapping key: expected " + std::to_string(polys * P.N) + " words, got " +
                                          std::to_string(n_words));
    if (int rc = begin_key_load(ctx, "helm_si_load_bootstrap_key")) return rc;
    if (K.group > 1) {
        // Both multi-bit kernels (k_pbs64s<., true> and the generic kernel's multi-bit form) sum the 2^g subsets' products of a
        // group before the CRT lift, so a step is the 2^g GGSWs of a group (src is [t][S][lev][r][c][N]).  The creation-time
        // capacity check does not carry the factor 2^g (a worst case no honest key comes near: a uniformly random key of k = 1,
        // N = 2048, logB = 21, g = 3 stays at 0.71 of the limit); this one is sufficient for the key at hand and every input.
        // A key beyond it is refused before anything of the context is touched: the context keeps the key and state it had.
        const size_t subsets = (size_t)1 << K.group;
        const SiClassFacts &C = SI_CLASS[K.run.cls]; // (the capacity of the pair the class computes in)
        const long double key_bound = key_step_bound(P, bsk_std, n_ggsw / subsets, subsets * per_ggsw);
        if (key_bound * 1.001L >= C.half) {
            char ratio[32];
            snprintf(ratio, sizeof ratio, "%.3Lf", key_bound / C.half);
            return fail(HELM_ERR_INVALID, std::string("bootstrapping key exceeds the two-prime NTT capacity of the ") + C.noun +
                                              " multi-bit kernel: its largest group sum is " + ratio + " of p0 p1 / 2");
        }
    }
    struct Tmp {
        void *p = nullptr;
        ~Tmp() { if (p) (void)hipFree(p); }
    } t_std; // freed on every return path
    HIP_TRY(hipMalloc(&t_std.p, n_words * sizeof(uint64_t)));
    uint64_t *d_std = static_cast<uint64_t *>(t_std.p);
    if (K.run.form == SI_K && P.N == 512) {
        // k_pbs64k contexts at N = 512 (N = 1024 is built for the 49-bit pair only: its key converts as every k = 1 set's):
        // the CRT pair follows the key at hand, a step being one GGSW (src is [i][lev][r][c][N]).  With the
        // step bound below p p' / 2 of the 46-bit pair (and with digits of at most 17 bits, whose products with b^3 stay exact
        // doubles): FpJ / FpJ2, whose headroom drops stage 2's modular multiplications and most recentrings (ntt_fp64.h);
        // otherwise the 49-bit pair.  HELM_SI_FIELD=49 keeps the 49-bit pair.
        const long double key_bound = key_step_bound(P, bsk_std, (size_t)P.n, per_ggsw);
        // (margin 5 %: the CRT's quotient t = (r1 - r0) / p0 mod p1 comes out of mulmod within 0.512 p1, so the lifted value is
        // the exact integer as long as that stays below 0.488 p0 p1)
        int want = (key_bound * 1.05L < (long double)J0::P * (long double)J1::P / 2 && P.pbs_logB <= 18) ? 1 : 0;
        if (const char *v = getenv("HELM_SI_FIELD")) if (atoi(v) == 49) want = 0;
        if (want != K.pair) {
            K.have_bsk = false;
            if (int rc = setup_pair_tables(ctx, want)) return rc;
        }
    }
    HIP_TRY(hipMemcpyAsync(d_std, bsk_std, n_words * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    if (int rc = convert_bootstrap_key(ctx, d_std, n_words, polys)) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (K.run.form == SI_SPLIT_MB && !K.expo) { // once per context (the generic and large-N kernels derive their spectrum positions)
        if (int rc = probe_spectrum_positions(ctx)) return rc;
    }
    K.have_bsk = true;
    return 0;
}

int helm_si_load_keyswitch_key(helm_si_ctx *ctx, const uint64_t *ksk, size_t n_words)
{
    if (!ctx || !ksk) return fail(HELM_ERR_INVALID, "null argument");
    const helm_si_params &P = ctx->P;
    const size_t want = (size_t)P.k * P.N * P.ks_l * ((size_t)P.n + 1);
    if (n_words != want)
        return fail(HELM_ERR_INVALID, "keyswitching key: expected " + std::to_string(want) + " words, got " +
                                          std::to_string(n_words));
    if (int rc = begin_key_load(ctx, "helm_si_load_keyswitch_key")) return rc;
    SiKeyState &K = *ctx->keys;
    if (!K.ksk) HIP_TRY(hipMalloc(&K.ksk, want * sizeof(uint64_t)));
    HIP_TRY(hipMemcpyAsync(K.ksk, ksk, want * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    {
        // byte planes for the matrix-core keyswitch (levels padded to LP: the padding rows pair zero digits with -128)
        const helm_ks::Planes planes = helm_ks::build_planes(ksk, P.k * P.N, P.ks_l, ks64_padded_levels(P.ks_l), P.n);
        if (!planes.bytes.empty()) {
            if (!K.ksk_planes) HIP_TRY(hipMalloc(&K.ksk_planes, planes.bytes.size()));
            HIP_TRY(hipMemcpy(K.ksk_planes, planes.bytes.data(), planes.bytes.size(), hipMemcpyHostToDevice));
            K.ks_kchunks = planes.kchunks;
            K.ks_ctiles = planes.ctiles;
        }
    }
    K.have_ksk = true;
    return 0;
}

int helm_si_wires_alloc(helm_si_ctx *ctx, int64_t n_rows, helm_si_wires **out)
{
    if (!ctx || !out || n_rows <= 0) return fail(HELM_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(ctx->device));
    helm_si_wires *w = new (std::nothrow) helm_si_wires();
    if (!w) return fail(HELM_ERR_OOM, "wires");
    w->owner = ctx;
    w->n_rows = n_rows;
    const size_t bytes = (size_t)n_rows * ctx->wire_row() * sizeof(uint64_t);
    if (hipMalloc(&w->d, bytes) != hipSuccess) {
        delete w;
        return fail(HELM_ERR_OOM, "ciphertext table of " + std::to_string(bytes) + " bytes");
    }
    HIP_TRY(hipMemsetAsync(w->d, 0, bytes, ctx->stream));
    ctx->child_wires.push_back(w);
    *out = w;
    return 0;
}

int helm_si_wires_free(helm_si_ctx *ctx, helm_si_wires *w)
{
    if (!w) return 0;
    if (!w->owner) { // its context is gone and took the device memory with it
        delete w;
        return 0;
    }
    if (!ctx || w->owner != ctx) return fail(HELM_ERR_STATE, "table belongs to another context");
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(w->d);
    ctx->child_wires.erase(std::remove(ctx->child_wires.begin(), ctx->child_wires.end(), w), ctx->child_wires.end());
    delete w;
    return 0;
}

int helm_si_wires_upload(helm_si_ctx *ctx, helm_si_wires *w, const int32_t *idx, const uint64_t *lwe_host, int64_t count)
{
    if (!ctx || !w || !idx || !lwe_host || count < 0) return fail(HELM_ERR_INVALID, "bad argument");
    if (!owns(ctx, w)) return fail(HELM_ERR_STATE, "table belongs to another context");
    if (count == 0) return 0;
    if (int rc = check_rows(w, idx, count, false)) return rc;
    {
        std::vector<int32_t> sorted(idx, idx + count);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return fail(HELM_ERR_INVALID, "upload names the same row twice");
    }
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = drain(ctx)) return rc;
    const int dim = (int)ctx->wire_dim();
    if (int rc = upload(ctx, ctx->d_stage, lwe_host, (size_t)count * (dim + 1))) return rc;
    if (int rc = upload(ctx, ctx->d_idx, idx, (size_t)count)) return rc;
    hipLaunchKernelGGL(k_rows64, dim3((unsigned)count), dim3(256), 0, ctx->stream, ctx->d_stage.p, (const int32_t *)nullptr,
                       w->d, ctx->d_idx.p, dim);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int helm_si_wires_download(helm_si_ctx *ctx, helm_si_wires *w, const int32_t *idx, uint64_t *lwe_host, int64_t count)
{
    if (!ctx || !w || !idx || !lwe_host || count < 0) return fail(HELM_ERR_INVALID, "bad argument");
    if (!owns(ctx, w)) return fail(HELM_ERR_STATE, "table belongs to another context");
    if (count == 0) return 0;
    if (int rc = check_rows(w, idx, count, false)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = drain(ctx)) return rc;
    const int dim = (int)ctx->wire_dim();
    if (ctx->d_stage.ensure((size_t)count * (dim + 1))) return fail(HELM_ERR_OOM, "staging");
    if (int rc = upload(ctx, ctx->d_idx, idx, (size_t)count)) return rc;
    hipLaunchKernelGGL(k_rows64, dim3((unsigned)count), dim3(256), 0, ctx->stream, w->d, ctx->d_idx.p, ctx->d_stage.p,
                       (const int32_t *)nullptr, dim);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(lwe_host, ctx->d_stage.p, (size_t)count * (dim + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost,
                           ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int helm_si_wires_copy(helm_si_ctx *ctx, helm_si_wires *src, const int32_t *src_idx, helm_si_wires *dst,
                       const int32_t *dst_idx, int64_t count)
{
    if (!ctx || !src || !dst || !src_idx || !dst_idx || count < 0) return fail(HELM_ERR_INVALID, "bad argument");
    if (!owns(ctx, src) || !owns(ctx, dst)) return fail(HELM_ERR_STATE, "table belongs to another context");
    if (count == 0) return 0;
    if (int rc = check_rows(src, src_idx, count, false)) return rc;
    if (int rc = check_rows(dst, dst_idx, count, false)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = drain(ctx)) return rc;
    if (int rc = upload(ctx, ctx->d_idx, src_idx, (size_t)count)) return rc;
    if (int rc = upload(ctx, ctx->d_idx2, dst_idx, (size_t)count)) return rc;
    hipLaunchKernelGGL(k_rows64, dim3((unsigned)count), dim3(256), 0, ctx->stream, src->d, ctx->d_idx.p, dst->d,
                       ctx->d_idx2.p, (int)ctx->wire_dim());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int helm_si_wires_set_trivial(helm_si_ctx *ctx, helm_si_wires *w, const int32_t *idx, const uint64_t *value, int64_t count)
{
    if (!ctx || !w || !idx || !value || count < 0) return fail(HELM_ERR_INVALID, "bad argument");
    if (!owns(ctx, w)) return fail(HELM_ERR_STATE, "table belongs to another context");
    if (count == 0) return 0;
    if (int rc = check_rows(w, idx, count, false)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = drain(ctx)) return rc;
    std::vector<uint64_t> body((size_t)count);
    for (int64_t g = 0; g < count; g++) body[(size_t)g] = value[g] * ctx->delta;
    if (int rc = upload(ctx, ctx->d_body, body.data(), body.size())) return rc;
    if (int rc = upload(ctx, ctx->d_idx, idx, (size_t)count)) return rc;
    hipLaunchKernelGGL(k_set_trivial64, dim3((unsigned)count), dim3(256), 0, ctx->stream, ctx->d_idx.p, ctx->d_body.p, w->d,
                       (int)ctx->wire_dim());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int helm_si_bound_violations(helm_si_ctx *ctx, uint32_t counts[8], int reset)
{
    if (!ctx || !counts) return fail(HELM_ERR_INVALID, "null argument");
#ifdef HELM_CHECK_BOUNDS
    // this translation unit's own copy of the counters (ntt_fp64.h): every kernel of the 64-bit engine and of the WoP-PBS
    // path is compiled into it in the check build (one unit, no max-ILP split)
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpyFromSymbol(counts, HIP_SYMBOL(g_helm_bound_violations), 8 * sizeof(uint32_t)));
    if (reset) {
        const uint32_t zero[8] = {0};
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_helm_bound_violations), zero, sizeof(zero)));
    }
    return 0;
#else
    (void)reset;
    return fail(HELM_ERR_STATE, "this library was not built with -DHELM_CHECK_BOUNDS (make libhelm_hip_check.so, HELM_HIP_LIB)");
#endif
}

int helm_si_set_audit(helm_si_ctx *ctx, helm_si_audit_fn fn, void *user)
{
    if (!ctx) return fail(HELM_ERR_INVALID, "null context");
    ctx->audit_fn = fn;
    ctx->audit_user = fn ? user : nullptr;
    return 0;
}

// rows idx[0 .. count) of the table on the host (idx < 0: a zero row), for the audit
static int audit_fetch(helm_si_ctx *ctx, helm_si_wires *w, const int32_t *idx, int64_t count, std::vector<uint64_t> &rows)
{
    const size_t brow = ctx->wire_row();
    std::vector<int32_t> safe((size_t)count);
    for (int64_t g = 0; g < count; g++) safe[(size_t)g] = idx[g] < 0 ? 0 : idx[g];
    rows.assign((size_t)count * brow, 0);
    if (int rc = helm_si_wires_download(ctx, w, safe.data(), rows.data(), count)) return rc;
    for (int64_t g = 0; g < count; g++)
        if (idx[g] < 0) std::fill(rows.begin() + (size_t)g * brow, rows.begin() + (size_t)(g + 1) * brow, 0);
    return 0;
}

static int lincomb_impl(helm_si_ctx *ctx, helm_si_wires *w, const int32_t *in_idx, const int64_t *coef,
                        const int64_t *const_add, const int32_t *out_idx, int32_t terms, int64_t count);

int helm_si_lincomb(helm_si_ctx *ctx, helm_si_wires *w, const int32_t *in_idx, const int64_t *coef,
                    const int64_t *const_add, const int32_t *out_idx, int32_t terms, int64_t count)
{
    if (!ctx || !ctx->audit_fn || count <= 0) return lincomb_impl(ctx, w, in_idx, coef, const_add, out_idx, terms, count);
    if (!w || !in_idx || !coef || !out_idx || terms < 1) return fail(HELM_ERR_INVALID, "bad argument");
    if (!owns(ctx, w)) return fail(HELM_ERR_STATE, "table belongs to another context");
    if (int rc = check_rows(w, in_idx, count * terms, true)) return rc;
    std::vector<uint64_t> in_rows, out_rows;
    if (int rc = audit_fetch(ctx, w, in_idx, count * terms, in_rows)) return rc;
    if (int rc = lincomb_impl(ctx, w, in_idx, coef, const_add, out_idx, terms, count)) return rc;
    if (int rc = audit_fetch(ctx, w, out_idx, count, out_rows)) return rc;
    helm_si_audit_record rec{};
    rec.kind = 1;
    rec.count = count;
    rec.terms = terms;
    rec.in_rows = in_rows.data();
    rec.out_rows = out_rows.data();
    rec.in_idx = in_idx;
    rec.coef = coef;
    rec.const_add = const_add;
    if (int rc = ctx->audit_fn(ctx->audit_user, &rec))
        return fail(HELM_ERR_STATE, "helm_si_lincomb: the audit callback rejected the batch (" + std::to_string(rc) + ")");
    return 0;
}

static int lincomb_impl(helm_si_ctx *ctx, helm_si_wires *w, const int32_t *in_idx, const int64_t *coef,
                        const int64_t *const_add, const int32_t *out_idx, int32_t terms, int64_t count)
{
    if (!ctx || !w || !in_idx || !coef || !out_idx || terms < 1 || count < 0) return fail(HELM_ERR_INVALID, "bad argument");
    if (!owns(ctx, w)) return fail(HELM_ERR_STATE, "table belongs to another context");
    if (count == 0) return 0;
    if (int rc = check_rows(w, in_idx, count * terms, true)) return rc;
    if (int rc = check_rows(w, out_idx, count, false)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const int dim = (int)ctx->wire_dim();
    std::vector<uint64_t> body((size_t)count, 0);
    if (const_add)
        for (int64_t g = 0; g < count; g++) body[(size_t)g] = (uint64_t)const_add[g] * ctx->delta;
    // sums are staged (rows 0..count-1) and then scattered, so that a gate may overwrite a
    // row another gate of the same call still reads
    if (ctx->d_stage.cap < (size_t)count * (dim + 1)) {
        if (int rc = drain(ctx)) return rc; // growing the staging area frees the old one
        if (ctx->d_stage.ensure((size_t)count * (dim + 1))) return fail(HELM_ERR_OOM, "staging");
    }
    helm_si_ctx::CallSlot *S = nullptr;
    if (int rc = slot_begin(ctx, (size_t)count * (8 + 4) + (size_t)count * terms * (4 + 8), &S)) return rc;
    const uint64_t *d_body = slot_put(*S, body.data(), body.size());
    const int32_t *d_in = slot_put(*S, in_idx, (size_t)count * terms);
    const int32_t *d_out = slot_put(*S, out_idx, (size_t)count);
    const int64_t *d_coef = slot_put(*S, coef, (size_t)count * terms);
    if (int rc = slot_flush(ctx, *S)) return rc;
    {
        Timed t(ctx, &ctx->ev_lin);
        hipLaunchKernelGGL(k_lincomb64, dim3((unsigned)count), dim3(256), 0, ctx->stream, d_in, d_coef, d_body,
                           (const int32_t *)nullptr, w->d, ctx->d_stage.p, terms, dim);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_rows64, dim3((unsigned)count), dim3(256), 0, ctx->stream, ctx->d_stage.p,
                           (const int32_t *)nullptr, w->d, d_out, dim);
        HIP_TRY(hipGetLastError());
    }
    return slot_end(ctx, *S);
}

int helm_si_make_lut(const helm_si_ctx *ctx, const uint64_t *f_values, uint64_t *tv)
{
    if (!ctx || !f_values || !tv) return fail(HELM_ERR_INVALID, "null argument");
    const int N = ctx->P.N, t = ctx->P.message_modulus * ctx->P.carry_modulus;
    const int box = N / t, half = box / 2;
    std::vector<uint64_t> acc((size_t)N);
    for (int v = 0; v < t; v++)
        for (int j = 0; j < box; j++) acc[(size_t)v * box + j] = f_values[v] * ctx->delta;
    for (int j = 0; j < half; j++) acc[(size_t)j] = 0ull - acc[(size_t)j];
    for (int j = 0; j < N; j++) tv[j] = acc[(size_t)((j + half) % N)]; // rotate_left(half)
    return 0;
}

int helm_si_apply_luts(helm_si_ctx *ctx, helm_si_wires *w, const int32_t *in_idx, const int32_t *lut_idx,
                       const int32_t *out_idx, int64_t count, const uint64_t *luts, int64_t n_luts)
{
    if (!ctx || !w || !in_idx || !lut_idx || !out_idx || !luts || count < 0 || n_luts <= 0)
        return fail(HELM_ERR_INVALID, "bad argument");
    if (!owns(ctx, w)) return fail(HELM_ERR_STATE, "table belongs to another context");
    if (count == 0) return 0;
    if (int rc = check_rows(w, in_idx, count, false)) return rc;
    if (int rc = check_rows(w, out_idx, count, false)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<Ks64Job> ks((size_t)count);
    std::vector<Pbs64Job> pbs((size_t)count);
    for (int64_t g = 0; g < count; g++) {
        if (lut_idx[g] < 0 || lut_idx[g] >= n_luts) return fail(HELM_ERR_INVALID, "lut_idx out of range");
        ks[(size_t)g] = Ks64Job{in_idx[g], (int32_t)g};
        pbs[(size_t)g] = Pbs64Job{(int32_t)g, lut_idx[g], out_idx[g], 0};
    }
    std::vector<uint64_t> audit_in, audit_out;
    if (ctx->audit_fn)
        if (int rc = audit_fetch(ctx, w, in_idx, count, audit_in)) return rc;
    int rc = 0;
    if (ctx->x_on && count >= ctx->x_min)
        rc = apply_luts_sharded(ctx, w, in_idx, lut_idx, out_idx, count, luts, n_luts);
    else if (ctx->order == 0) { // every bootstrap finishes (kernel boundary) before any keyswitch writes its output row
        for (int64_t g = 0; g < count; g++) {
            pbs[(size_t)g] = Pbs64Job{in_idx[g], lut_idx[g], (int32_t)g, 0};
            ks[(size_t)g] = Ks64Job{(int32_t)g, out_idx[g]};
        }
        rc = apply_luts_pbs_first(ctx, w->d, w->d, pbs, count, ks, -1, luts, n_luts);
    } else // every keyswitch finishes (kernel boundary) before any bootstrap writes its output row
        rc = apply_luts_device(ctx, w->d, w->d, ks, pbs, luts, n_luts);
    if (rc || !ctx->audit_fn) return rc;
    if ((rc = audit_fetch(ctx, w, out_idx, count, audit_out))) return rc;
    helm_si_audit_record rec{};
    rec.kind = 0;
    rec.count = count;
    rec.n_luts = n_luts;
    rec.in_rows = audit_in.data();
    rec.out_rows = audit_out.data();
    rec.lut_idx = lut_idx;
    rec.luts = luts;
    if ((rc = ctx->audit_fn(ctx->audit_user, &rec)))
        return fail(HELM_ERR_STATE, "helm_si_apply_luts: the audit callback rejected the batch (" + std::to_string(rc) + ")");
    return 0;
}

int helm_si_make_many_lut(const helm_si_ctx *ctx, const uint64_t *f_values, int32_t n_funcs, uint64_t *tv)
{
    if (!ctx || !f_values || !tv) return fail(HELM_ERR_INVALID, "null argument");
    int M = 1;
    if (int rc = many_lut_shape(ctx, n_funcs, &M, nullptr)) return rc;
    const int N = ctx->P.N, t = ctx->P.message_modulus * ctx->P.carry_modulus;
    const int box = N / t, half = box / 2, per = t / M; // function i: boxes i per .. i per + per - 1, chunks >= n_funcs zero
    std::vector<uint64_t> acc((size_t)N, 0);
    for (int i = 0; i < n_funcs; i++)
        for (int v = 0; v < per; v++)
            for (int j = 0; j < box; j++) acc[((size_t)i * per + v) * box + j] = f_values[(size_t)i * per + v] * ctx->delta;
    for (int j = 0; j < half; j++) acc[(size_t)j] = 0ull - acc[(size_t)j];
    for (int j = 0; j < N; j++) tv[j] = acc[(size_t)((j + half) % N)]; // rotate_left(half)
    return 0;
}

int helm_si_apply_many_luts(helm_si_ctx *ctx, helm_si_wires *w, const int32_t *in_idx, const int32_t *lut_idx,
                            const int32_t *out_idx, int32_t n_out, int64_t count, const uint64_t *luts, int64_t n_luts)
{
    if (!ctx || !w || !in_idx || !lut_idx || !out_idx || !luts || count < 0 || n_luts <= 0)
        return fail(HELM_ERR_INVALID, "bad argument");
    if (!owns(ctx, w)) return fail(HELM_ERR_STATE, "table belongs to another context");
    int32_t pad = 0;
    if (int rc = many_lut_shape(ctx, n_out, nullptr, &pad)) return rc;
    if (count == 0) return 0;
    if (count * n_out > INT32_MAX) return fail(HELM_ERR_INVALID, "many-LUT: count * n_out exceeds the row index range");
    const int64_t n_rows = count * n_out;
    if (int rc = check_rows(w, in_idx, count, false)) return rc;
    if (int rc = check_rows(w, out_idx, n_rows, true)) return rc;
    for (int64_t g = 0; g < count; g++)
        if (lut_idx[g] < 0 || lut_idx[g] >= n_luts) return fail(HELM_ERR_INVALID, "lut_idx out of range");
    // the scatter list: stage row g n_out + x -> table row out_idx[g n_out + x]; skipped outputs (-1) are not on it
    std::vector<int32_t> s_row, d_row;
    for (int64_t q = 0; q < n_rows; q++)
        if (out_idx[q] >= 0) {
            s_row.push_back((int32_t)q);
            d_row.push_back(out_idx[q]);
        }
    {
        std::vector<int32_t> sorted(d_row);
        std::sort(sorted.begin(), sorted.end());
        const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
        if (dup != sorted.end())
            return fail(HELM_ERR_INVALID, "many-LUT: two outputs of the call name row " + std::to_string(*dup));
    }
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<uint64_t> audit_in, audit_out;
    if (ctx->audit_fn)
        if (int rc = audit_fetch(ctx, w, in_idx, count, audit_in)) return rc;
    if (ctx->x_on && count >= ctx->x_min) {
        if (int rc = apply_many_luts_sharded(ctx, w, in_idx, lut_idx, out_idx, n_out, pad, count, luts, n_luts)) return rc;
    } else if (ctx->order == 0) {
        // One rotation per ciphertext into stage rows g n_out + x, then one keyswitch job per output that is not skipped,
        // straight into its table row.
        std::vector<Pbs64Job> pbs((size_t)count);
        std::vector<Ks64Job> ks(s_row.size());
        for (int64_t g = 0; g < count; g++) pbs[(size_t)g] = Pbs64Job{in_idx[g], lut_idx[g], (int32_t)(g * n_out), pad};
        for (size_t i = 0; i < s_row.size(); i++) ks[i] = Ks64Job{s_row[i], d_row[i]};
        if (int rc = apply_luts_pbs_first(ctx, w->d, w->d, pbs, n_rows, ks, -1, luts, n_luts)) return rc;
    } else {
        // Every keyswitch finishes (kernel boundary) before the scatter writes an output row: the bootstraps write the stage
        // buffer only.
        if (int rc = apply_many_luts_stage(ctx, w->d, in_idx, lut_idx, n_out, pad, count, luts, n_luts)) return rc;
        if (!d_row.empty()) {
            helm_si_ctx::CallSlot *S = nullptr;
            if (int rc = slot_begin(ctx, 2 * d_row.size() * sizeof(int32_t), &S)) return rc;
            const int32_t *d_src = slot_put(*S, s_row.data(), s_row.size());
            const int32_t *d_dst = slot_put(*S, d_row.data(), d_row.size());
            if (int rc = slot_flush(ctx, *S)) return rc;
            {
                Timed t(ctx, &ctx->ev_lin);
                hipLaunchKernelGGL(k_rows64, dim3((unsigned)d_row.size()), dim3(256), 0, ctx->stream, ctx->d_stage.p, d_src, w->d,
                                   d_dst, (int)ctx->wire_dim());
                HIP_TRY(hipGetLastError());
            }
            if (int rc = slot_end(ctx, *S)) return rc;
        }
    }
    if (!ctx->audit_fn) return 0;
    if (int rc = audit_fetch(ctx, w, out_idx, n_rows, audit_out)) return rc;
    helm_si_audit_record rec{};
    rec.kind = 2;
    rec.terms = n_out;
    rec.count = count;
    rec.n_luts = n_luts;
    rec.in_rows = audit_in.data();
    rec.out_rows = audit_out.data();
    rec.lut_idx = lut_idx;
    rec.luts = luts;
    if (int rc = ctx->audit_fn(ctx->audit_user, &rec))
        return fail(HELM_ERR_STATE, "helm_si_apply_many_luts: the audit callback rejected the batch (" + std::to_string(rc) + ")");
    return 0;
}

int helm_si_set_level_many_lut(helm_si_ctx *ctx, int on)
{
    if (!ctx) return fail(HELM_ERR_INVALID, "null context");
    ctx->level_many = on != 0;
    return 0;
}

int helm_si_set_exchange(helm_si_ctx *ctx, int32_t rank, int32_t world, int64_t min_batch, void *stage_dev,
                         void *gather_dev, int64_t capacity_rows, helm_si_exchange_fn fn, void *user)
{
    if (!ctx) return fail(HELM_ERR_INVALID, "null context");
    if (fn)
        if (int rc = helm_hip_runtime_guard_("helm_si_set_exchange")) return rc; // the caller's buffers and collective
    if (ctx->x_own) {
        HIP_TRY(hipSetDevice(ctx->device));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        (void)hipFree(ctx->x_own);
        ctx->x_own = nullptr;
    }
    ctx->x_comm = nullptr;
    if (world < 1 || (world == 1 && !fn)) { // back to single-GPU evaluation
        ctx->x_world = 1;
        ctx->x_rank = 0;
        ctx->x_fn = nullptr;
        ctx->x_on = false;
        ctx->x_stage = ctx->x_gather = nullptr;
        return 0;
    }
    if (rank < 0 || rank >= world || min_batch < 1 || capacity_rows < 1 || !stage_dev || !gather_dev || !fn)
        return fail(HELM_ERR_INVALID, "helm_si_set_exchange: bad argument");
    ctx->x_on = true;
    ctx->x_rank = rank;
    ctx->x_world = world;
    ctx->x_min = min_batch;
    ctx->x_cap = capacity_rows;
    ctx->x_stage = static_cast<uint64_t *>(stage_dev);
    ctx->x_gather = static_cast<uint64_t *>(gather_dev);
    ctx->x_fn = fn;
    ctx->x_user = user;
    ctx->x_batches = ctx->x_rows = 0;
    return 0;
}

int helm_si_set_exchange_comm(helm_si_ctx *ctx, helm_comm *comm, int64_t min_batch, int64_t capacity_rows)
{
    if (!ctx) return fail(HELM_ERR_INVALID, "null context");
    if (!comm) return helm_si_set_exchange(ctx, 0, 1, 1, nullptr, nullptr, 1, nullptr, nullptr);
    if (min_batch < 1 || capacity_rows < 1) return fail(HELM_ERR_INVALID, "helm_si_set_exchange_comm: bad argument");
    int rank = 0, world = 0, dev = -1;
    if (int rc = helm_comm_info(comm, &rank, &world, &dev, nullptr)) return rc;
    if (dev != ctx->device) return fail(HELM_ERR_STATE, "helm_si_set_exchange_comm: the communicator lives on another device than the context");
    if (int rc = helm_si_set_exchange(ctx, 0, 1, 1, nullptr, nullptr, 1, nullptr, nullptr)) return rc; // releases an earlier buffer
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t brow = ctx->wire_row();
    HIP_TRY(hipMalloc(&ctx->x_own, (size_t)capacity_rows * (size_t)world * brow * sizeof(uint64_t)));
    ctx->x_comm = comm;
    ctx->x_gather = ctx->x_own;
    ctx->x_stage = nullptr; // chunks go straight into the gather buffer (x_slot)
    ctx->x_rank = rank;
    ctx->x_world = world;
    ctx->x_min = min_batch;
    ctx->x_cap = capacity_rows;
    ctx->x_fn = nullptr;
    ctx->x_user = nullptr;
    ctx->x_on = true;
    ctx->x_batches = ctx->x_rows = 0;
    return 0;
}

int helm_si_exchange_world(const helm_si_ctx *ctx) { return ctx ? ctx->x_world : 1; }

int64_t helm_si_round_capacity(helm_si_ctx *ctx)
{
    if (!ctx) return fail(HELM_ERR_INVALID, "null context");
    if (ctx->round_capacity <= 0) {
        HIP_TRY(hipSetDevice(ctx->device));
        int per_cu = 0;
        HIP_TRY(launch_pbs64(ctx, nullptr, 0, nullptr, nullptr, nullptr, &per_cu));
        ctx->round_capacity = (int64_t)std::max(per_cu, 1) * ctx->n_cus;
    }
    return ctx->round_capacity;
}

int helm_si_exchange_stats(const helm_si_ctx *ctx, int64_t *batches, int64_t *rows)
{
    if (!ctx) return fail(HELM_ERR_INVALID, "null context");
    if (batches) *batches = ctx->x_batches;
    if (rows) *rows = ctx->x_rows;
    return 0;
}

int helm_si_eval_lut_level(helm_si_ctx *ctx, helm_si_wires *w, const int32_t *arity, const int32_t *in_idx,
                           int32_t max_in, const uint64_t *table, const int32_t *out_idx, int64_t count)
{
    if (!ctx || !w || !arity || !in_idx || !table || !out_idx || max_in < 1 || count < 0)
        return fail(HELM_ERR_INVALID, "bad argument");
    if (!owns(ctx, w)) return fail(HELM_ERR_STATE, "table belongs to another context");
    if (count == 0) return 0;
    if (int rc = check_rows(w, out_idx, count, false)) return rc;
    // The gates of a level run concurrently (circuit.rs:1057: par_iter over the level; the reference's guarantee comes from
    // compute_levels, circuit.rs:174-239): a level in which a gate reads a row ANOTHER gate of the level writes, or in which
    // two gates write one row, is refused instead of evaluated in an unspecified order.  A gate may rewrite its own input row.
    {
        std::vector<std::pair<int32_t, int64_t>> writer((size_t)count);
        for (int64_t g = 0; g < count; g++) writer[(size_t)g] = {out_idx[g], g};
        std::sort(writer.begin(), writer.end());
        for (int64_t g = 1; g < count; g++)
            if (writer[(size_t)g].first == writer[(size_t)g - 1].first)
                return fail(HELM_ERR_INVALID, "gates " + std::to_string(writer[(size_t)g - 1].second) + " and " +
                                                  std::to_string(writer[(size_t)g].second) + " both write row " +
                                                  std::to_string(writer[(size_t)g].first) + " (write-after-write inside a level)");
        for (int64_t g = 0; g < count; g++) {
            const int ar = arity[g] < 0 ? 0 : (arity[g] > max_in ? max_in : arity[g]);
            for (int q = 0; q < std::max(ar, 1); q++) {
                const int32_t r = in_idx[(size_t)g * max_in + q];
                auto it = std::lower_bound(writer.begin(), writer.end(), std::make_pair(r, (int64_t)-1));
                if (it != writer.end() && it->first == r && it->second != g)
                    return fail(HELM_ERR_INVALID, "gate " + std::to_string(g) + " reads row " + std::to_string(r) + ", which gate " +
                                                      std::to_string(it->second) + " of the same level writes (read-after-write inside a level)");
            }
        }
    }
    const helm_si_params &P = ctx->P;
    const int t = P.message_modulus * P.carry_modulus;
    // ---- linear part of every gate: packed operand (LUT gates), copy or negation ---------
    std::vector<int32_t> lin_in((size_t)count * max_in, -1);
    std::vector<int64_t> lin_coef((size_t)count * max_in, 0);
    std::vector<int32_t> pbs_gate; // gates that bootstrap
    std::map<std::pair<int, uint64_t>, int32_t> lut_of;
    std::vector<uint64_t> luts;
    std::vector<int32_t> lut_idx;
    for (int64_t g = 0; g < count; g++) {
        const int ar = arity[g];
        if (ar < 0 || ar > max_in) return fail(HELM_ERR_INVALID, "gate " + std::to_string(g) + ": bad arity");
        const int32_t *in = in_idx + (size_t)g * max_in;
        for (int q = 0; q < std::max(ar, 1); q++)
            if (in[q] < 0 || in[q] >= w->n_rows)
                return fail(HELM_ERR_INVALID, "gate " + std::to_string(g) + ": operand row out of range");
        if (ar == 0) { // DFF / copy (circuit.rs:1063-1069)
            lin_in[(size_t)g * max_in] = in[0];
            lin_coef[(size_t)g * max_in] = 1;
        } else if (ar == 1) { // gates.rs:765-770
            lin_in[(size_t)g * max_in] = in[0];
            lin_coef[(size_t)g * max_in] = table[g] == 0 ? 1 : -1;
        } else {
            if ((1 << ar) > t)
                return fail(HELM_ERR_INVALID, "gate " + std::to_string(g) + ": " + std::to_string(ar) +
                                                  " inputs do not fit the plaintext space of " + std::to_string(t));
            for (int q = 0; q < ar; q++) { // gates.rs:773-778 (ar = 2: x * 2 + y)
                lin_in[(size_t)g * max_in + q] = in[q];
                lin_coef[(size_t)g * max_in + q] = (int64_t)1 << (ar - 1 - q);
            }
            if (ctx->level_many) { // tables per group of gates, below
                pbs_gate.push_back((int32_t)g);
                continue;
            }
            const std::pair<int, uint64_t> key(ar, table[g]);
            auto it = lut_of.find(key);
            if (it == lut_of.end()) {
                std::vector<uint64_t> f((size_t)t, 0);
                for (int v = 0; v < t; v++) {
                    // arity 2: table[(x&1)*2 + (y&1)] with v = 2x + y (gates.rs:750-752); else table[v] & 1
                    const int idx = ar == 2 ? (((v >> 1) & 1) * 2 + (v & 1)) : (v & ((1 << ar) - 1));
                    f[(size_t)v] = (table[g] >> idx) & 1ull;
                }
                const int32_t id = (int32_t)(luts.size() / P.N);
                luts.resize(luts.size() + P.N);
                helm_si_make_lut(ctx, f.data(), luts.data() + (size_t)id * P.N);
                it = lut_of.emplace(key, id).first;
            }
            pbs_gate.push_back((int32_t)g);
            lut_idx.push_back(it->second);
        }
    }
    // bootstrapped gates first (pack, then KS + PBS in place), copies / negations after them:
    // the order the boolean engine uses, which only matters for a DFF that latches a wire
    // produced in its own (last) level
    std::vector<int32_t> sub_in, sub_out;
    std::vector<int64_t> sub_coef;
    auto gather = [&](bool want_pbs) {
        sub_in.clear();
        sub_out.clear();
        sub_coef.clear();
        for (int64_t g = 0; g < count; g++) {
            if ((arity[g] >= 2) != want_pbs) continue;
            sub_in.insert(sub_in.end(), lin_in.begin() + g * max_in, lin_in.begin() + (g + 1) * max_in);
            sub_coef.insert(sub_coef.end(), lin_coef.begin() + g * max_in, lin_coef.begin() + (g + 1) * max_in);
            sub_out.push_back(out_idx[g]);
        }
    };
    if (ctx->level_many && !pbs_gate.empty()) {
        // helm_si_set_level_many_lut: gates with the same inputs in the same order pack the same index, so up to
        // helm_many_lut::group_max of them are the functions of one many-LUT table and one blind rotation.  A group's index is
        // packed into its first gate's output row; a group of n gates has a table of M_g = the power of two >= n chunks
        // (n = 1: helm_si_make_lut's polynomial) and the level is ONE dispatch of n_out = M_d = the largest M_g: gate i of a
        // group is output i M_d / M_g (the extract at coefficient i N / M_g), every other output is skipped.
        struct Group {
            std::vector<int32_t> gates;
            int32_t lut = 0;
            int M = 1;
        };
        std::vector<Group> groups;
        std::map<std::pair<int, std::vector<int32_t>>, size_t> open; // (arity, inputs) -> the group that still has room
        for (int32_t g : pbs_gate) {
            const int ar = arity[g];
            std::pair<int, std::vector<int32_t>> key(ar, std::vector<int32_t>(in_idx + (size_t)g * max_in, in_idx + (size_t)g * max_in + ar));
            auto it = open.find(key);
            if (it == open.end() || (int)groups[it->second].gates.size() >= helm_many_lut::group_max(ar, t)) {
                open[key] = groups.size();
                groups.push_back(Group());
                groups.back().gates.push_back(g);
            } else
                groups[it->second].gates.push_back(g);
        }
        std::map<std::pair<int, std::vector<uint64_t>>, int32_t> tables_of; // one test polynomial per distinct function tuple
        int Md = 1;
        for (Group &G : groups) {
            const int ar = arity[G.gates[0]], n = (int)G.gates.size();
            while (G.M < n) G.M *= 2;
            Md = std::max(Md, G.M);
            std::pair<int, std::vector<uint64_t>> key(ar, std::vector<uint64_t>());
            for (int32_t g : G.gates) key.second.push_back(table[g]);
            auto it = tables_of.find(key);
            if (it == tables_of.end()) {
                const int per = t / G.M; // 2^ar <= per (helm_many_lut::group_max): the packed index is below it
                std::vector<uint64_t> f((size_t)n * per, 0);
                for (int i = 0; i < n; i++)
                    for (int v = 0; v < per; v++) {
                        const int idx = ar == 2 ? (((v >> 1) & 1) * 2 + (v & 1)) : (v & ((1 << ar) - 1));
                        f[(size_t)i * per + v] = (key.second[(size_t)i] >> idx) & 1ull;
                    }
                const int32_t id = (int32_t)(luts.size() / P.N);
                luts.resize(luts.size() + P.N);
                if (int rc = n == 1 ? helm_si_make_lut(ctx, f.data(), luts.data() + (size_t)id * P.N)
                                    : helm_si_make_many_lut(ctx, f.data(), n, luts.data() + (size_t)id * P.N))
                    return rc;
                it = tables_of.emplace(key, id).first;
            }
            G.lut = it->second;
        }
        std::vector<int32_t> g_in, g_row, g_out;
        std::vector<int64_t> g_coef;
        for (const Group &G : groups) {
            const int32_t g0 = G.gates[0];
            g_in.insert(g_in.end(), lin_in.begin() + (size_t)g0 * max_in, lin_in.begin() + (size_t)(g0 + 1) * max_in);
            g_coef.insert(g_coef.end(), lin_coef.begin() + (size_t)g0 * max_in, lin_coef.begin() + (size_t)(g0 + 1) * max_in);
            g_row.push_back(out_idx[g0]);
            lut_idx.push_back(G.lut);
            const size_t at = g_out.size();
            g_out.resize(at + (size_t)Md, -1);
            for (size_t i = 0; i < G.gates.size(); i++) g_out[at + i * (size_t)(Md / G.M)] = out_idx[G.gates[i]];
        }
        if (int rc = helm_si_lincomb(ctx, w, g_in.data(), g_coef.data(), nullptr, g_row.data(), max_in, (int64_t)g_row.size()))
            return rc;
        const int rc = Md == 1 ? helm_si_apply_luts(ctx, w, g_row.data(), lut_idx.data(), g_row.data(), (int64_t)g_row.size(),
                                                    luts.data(), (int64_t)(luts.size() / P.N))
                               : helm_si_apply_many_luts(ctx, w, g_row.data(), lut_idx.data(), g_out.data(), Md, (int64_t)g_row.size(),
                                                         luts.data(), (int64_t)(luts.size() / P.N));
        if (rc) return rc;
    } else if (!pbs_gate.empty()) {
        gather(true);
        if (int rc = helm_si_lincomb(ctx, w, sub_in.data(), sub_coef.data(), nullptr, sub_out.data(), max_in,
                                     (int64_t)sub_out.size()))
            return rc;
        if (int rc = helm_si_apply_luts(ctx, w, sub_out.data(), lut_idx.data(), sub_out.data(), (int64_t)sub_out.size(),
                                        luts.data(), (int64_t)(luts.size() / P.N)))
            return rc;
    }
    gather(false);
    if (!sub_out.empty())
        if (int rc = helm_si_lincomb(ctx, w, sub_in.data(), sub_coef.data(), nullptr, sub_out.data(), max_in,
                                     (int64_t)sub_out.size()))
            return rc;
    return 0;
}

int helm_si_keyswitch_batch(helm_si_ctx *ctx, const uint64_t *in_big, uint64_t *out_small, int64_t count)
{
    if (!ctx || !in_big || !out_small || count < 0) return fail(HELM_ERR_INVALID, "bad argument");
    if (!ctx->keys->have_ksk) return fail(HELM_ERR_STATE, "keyswitching key not loaded");
    if (count == 0) return 0;
    const helm_si_params &P = ctx->P;
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = drain(ctx)) return rc;
    const size_t row = (size_t)P.n + 1, brow = (size_t)P.k * P.N + 1;
    std::vector<Ks64Job> jobs((size_t)count);
    for (int64_t g = 0; g < count; g++) jobs[(size_t)g] = Ks64Job{(int32_t)g, (int32_t)g};
    if (int rc = upload(ctx, ctx->d_stage, in_big, (size_t)count * brow)) return rc;
    if (int rc = upload(ctx, ctx->d_ks, jobs.data(), jobs.size())) return rc;
    if (ctx->d_small.ensure((size_t)count * row)) return fail(HELM_ERR_OOM, "small-LWE scratch");
    {
        Timed t(ctx, &ctx->ev_ks);
        HIP_TRY(launch_ks64(ctx, ctx->d_ks.p, count, ctx->d_stage.p, ctx->d_small.p));
    }
    HIP_TRY(hipMemcpyAsync(out_small, ctx->d_small.p, (size_t)count * row * sizeof(uint64_t), hipMemcpyDeviceToHost,
                           ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int helm_si_pbs_batch(helm_si_ctx *ctx, const uint64_t *in_small, const uint64_t *luts, int64_t n_luts,
                      const int32_t *lut_idx, uint64_t *out_big, int64_t count)
{
    if (!ctx || !in_small || !luts || !lut_idx || !out_big || count < 0 || n_luts <= 0)
        return fail(HELM_ERR_INVALID, "bad argument");
    if (!ctx->keys->have_bsk) return fail(HELM_ERR_STATE, "bootstrapping key not loaded");
    if (count == 0) return 0;
    const helm_si_params &P = ctx->P;
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = drain(ctx)) return rc;
    const size_t row = (size_t)P.n + 1, brow = (size_t)P.k * P.N + 1;
    std::vector<Pbs64Job> jobs((size_t)count);
    for (int64_t g = 0; g < count; g++) {
        if (lut_idx[g] < 0 || lut_idx[g] >= n_luts) return fail(HELM_ERR_INVALID, "lut_idx out of range");
        jobs[(size_t)g] = Pbs64Job{(int32_t)g, lut_idx[g], (int32_t)g, 0};
    }
    if (int rc = upload(ctx, ctx->d_small, in_small, (size_t)count * row)) return rc;
    ctx->luts_words = 0; // the resident tables of the call slots are overwritten
    if (int rc = upload(ctx, ctx->d_luts, luts, (size_t)n_luts * P.N)) return rc;
    if (int rc = upload(ctx, ctx->d_pbs, jobs.data(), jobs.size())) return rc;
    if (ctx->d_stage.ensure((size_t)count * brow)) return fail(HELM_ERR_OOM, "staging");
    {
        Timed t(ctx, &ctx->ev_pbs);
        HIP_TRY(launch_pbs64(ctx, ctx->d_pbs.p, count, ctx->d_small.p, ctx->d_luts.p, ctx->d_stage.p));
    }
    ctx->tacc.pbs_launches++;
    ctx->tacc.pbs_count += count;
    HIP_TRY(hipMemcpyAsync(out_big, ctx->d_stage.p, (size_t)count * brow * sizeof(uint64_t), hipMemcpyDeviceToHost,
                           ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int helm_si_pbs_many_batch(helm_si_ctx *ctx, const uint64_t *in_small, const uint64_t *luts, int64_t n_luts,
                           const int32_t *lut_idx, int32_t n_out, uint64_t *out_big, int64_t count)
{
    if (!ctx || !in_small || !luts || !lut_idx || !out_big || count < 0 || n_luts <= 0)
        return fail(HELM_ERR_INVALID, "bad argument");
    int32_t pad = 0;
    if (int rc = many_lut_shape(ctx, n_out, nullptr, &pad)) return rc;
    if (!ctx->keys->have_bsk) return fail(HELM_ERR_STATE, "bootstrapping key not loaded");
    if (count == 0) return 0;
    if (count * n_out > INT32_MAX) return fail(HELM_ERR_INVALID, "many-LUT: count * n_out exceeds the row index range");
    const helm_si_params &P = ctx->P;
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = drain(ctx)) return rc;
    const size_t row = (size_t)P.n + 1, brow = (size_t)P.k * P.N + 1, n_rows = (size_t)count * n_out;
    std::vector<Pbs64Job> jobs((size_t)count);
    for (int64_t g = 0; g < count; g++) {
        if (lut_idx[g] < 0 || lut_idx[g] >= n_luts) return fail(HELM_ERR_INVALID, "lut_idx out of range");
        jobs[(size_t)g] = Pbs64Job{(int32_t)g, lut_idx[g], (int32_t)(g * n_out), pad};
    }
    if (int rc = upload(ctx, ctx->d_small, in_small, (size_t)count * row)) return rc;
    ctx->luts_words = 0; // the resident tables of the call slots are overwritten
    if (int rc = upload(ctx, ctx->d_luts, luts, (size_t)n_luts * P.N)) return rc;
    if (int rc = upload(ctx, ctx->d_pbs, jobs.data(), jobs.size())) return rc;
    if (ctx->d_stage.ensure(n_rows * brow)) return fail(HELM_ERR_OOM, "staging");
    {
        Timed t(ctx, &ctx->ev_pbs);
        HIP_TRY(launch_pbs64(ctx, ctx->d_pbs.p, count, ctx->d_small.p, ctx->d_luts.p, ctx->d_stage.p));
    }
    ctx->tacc.pbs_launches++;
    ctx->tacc.pbs_count += count;
    HIP_TRY(hipMemcpyAsync(out_big, ctx->d_stage.p, n_rows * brow * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int helm_si_timing_enable(helm_si_ctx *ctx, int enable)
{
    if (!ctx) return fail(HELM_ERR_INVALID, "null ctx");
    ctx->timing = enable != 0;
    return 0;
}

int helm_si_get_timing(helm_si_ctx *ctx, helm_si_timing *out, int reset)
{
    if (!ctx || !out) return fail(HELM_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    auto drain = [](std::vector<std::pair<hipEvent_t, hipEvent_t>> &l, double &acc) {
        for (auto &p : l) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) acc += ms;
            (void)hipEventDestroy(p.first);
            (void)hipEventDestroy(p.second);
        }
        l.clear();
    };
    drain(ctx->ev_pbs, ctx->tacc.pbs_ms);
    drain(ctx->ev_ks, ctx->tacc.ks_ms);
    drain(ctx->ev_lin, ctx->tacc.linear_ms);
    *out = ctx->tacc;
    if (reset) ctx->tacc = helm_si_timing{};
    return 0;
}

} // extern "C"

// the WoP-PBS wide-LUT path (include/helm_wopbs.h): same translation unit, it is built from the kernels and launch
// helpers above
#include "helm_wopbs.inc"
#endif // HELM_SI_TU == 0
