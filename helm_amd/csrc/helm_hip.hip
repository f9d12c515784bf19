// helm_hip.hip — gfx950 kernels + C ABI (include/helm_hip.h) of the gate-bootstrap
// engine.  Replaces the tfhe::boolean::ServerKey calls HELM issues per gate
// (reference src/gates.rs:254-275) with level-batched device kernels:
//
//   k_linear        NOT / BUF / DFF / constants (no bootstrap)    gates.rs:256,268,272-274
//   k_pbs           gate linear step + modulus switch + blind rotate (CMUX chain over
//                   the NTT-domain bootstrapping key) + sample extract, one workgroup
//                   of (k+1) waves per bootstrap
//   k_keyswitch     big-key LWE -> small-key LWE, MUX recombination fused in
//   k_bsk_convert   standard-domain BSK -> NTT domain (once per key)
//   k_scatter_rows  multi-GPU: all-gathered level outputs -> wire table
//
// There is no CPU fallback in this file.
#include "../../include/helm_hip.h"
#include "../../include/helm_comm.h"
#include "ntt_fp64.h"
#include "shard_rule.h"
#include "keyswitch.h"
#include "pbs_frame.h"
#include "with_logn.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#ifndef HELM_HIP_TU
#define HELM_HIP_TU 0 // 1: the translation unit that holds k_pbs_wide alone (default scheduling strategy, Makefile)
#endif
#ifndef HELM_HIP_SPLIT_TU
#define HELM_HIP_SPLIT_TU 0
#endif
using namespace helm;
struct helm_hip_wires;
struct helm_hip_program;

// ------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------
static thread_local std::string g_err;
static int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}
// shared with helm_shortint.hip (same library, same helm_hip_last_error())
#if HELM_HIP_TU == 0
int helm_hip_fail_(int code, const std::string &msg) { return fail(code, msg); }
#endif
int helm_hip_runtime_guard_(const char *where); // helm_comm.cpp: one HIP runtime per process, or HELM_ERR_STATE naming the copies
#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t e__ = (expr);                                                                    \
        if (e__ != hipSuccess)                                                                      \
            return fail(HELM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));          \
    } while (0)

// ------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------
struct KsJob {
    int32_t big0, big1; // rows of the big-LWE buffer to add (big1 = -1: single)
    int32_t out;        // destination row (wire index, or staging row)
    uint32_t add_body;  // constant added to the body before switching (MUX: +1/8)
};

struct LinJob {
    int32_t op, in0, out;
};

// Signed gadget decomposition, closest representable + balanced digits (tfhe's SignedDecomposer:
//   d = state & (B-1); state >>= logB; carry = (((d-1) | state) & d) >> (logB-1); state += carry;
//   digit = d - carry*B), least significant level first.
// The carry is set when d > B/2, or d == B/2 and bit logB-1 of the remaining state is set, i.e. when
// d - 1 + sb >= B/2 with sb = bit 2 logB - 1 of the state before the shift; adding B/2 - 1 + sb to the
// whole state carries into the upper part exactly then:
//   next = (state + B/2 - 1 + sb) >> logB;  digit = state - next * B
// - five instructions per digit with the conversion (bit-field extract, three-operand add, shift,
// 24-bit multiply-add, convert) instead of eight.  Needs state + B/2 < 2^32 (logB * L <= 31) and
// next < 2^23 (the 24-bit multiply).  next after the least significant level is at most 2^(logB (L-1)), so the second
// needs logB (L-1) <= 22: for the five tuned shapes the capacity bound checked in helm_hip_ctx_create caps logB (L-1) at
// 16 ((512,1,3), logB <= 8).  The generic kernel's domain does not (e.g. L = 5, logB = 6): it uses gen_decompose_step
// (helm_pbs_generic.inc), the same recurrence with a full 32-bit multiply.
// `last`: the most significant level.  There the state is at most B = 2^logB (it starts below 2^(L logB) and loses logB
// bits per level, the rounding carry included), so its tie bit - bit 2 logB - 1 - is zero for logB >= 2, and for logB = 1
// (s = 2: tie bit set) (s + tie) >> 1 == s >> 1: the bit never changes the digit and is not extracted.
__device__ __forceinline__ int decompose_step(uint32_t &state, int logB, uint32_t half_m1, int neg_B, bool last = false)
{
    const uint32_t s = state;
    const uint32_t next = last ? (s + half_m1) >> logB : (s + half_m1 + __builtin_amdgcn_ubfe(s, 2 * logB - 1, 1)) >> logB;
    state = next;
    return __mul24((int)next, neg_B) + (int)s;
}

// dig[0] is the most significant level.  L and logB are compile-time / uniform.
template <int L>
__device__ __forceinline__ void decompose(uint32_t x, int logB, int (&dig)[L])
{
    const int rep = logB * L;
    const uint32_t half_m1 = (1u << (logB - 1)) - 1u;
    if (L >= 2 && rep == 32) {
        // every bit is representable (the keyswitch admits ks_l * ks_logB == 32; uniform branch): the word as it is, no
        // rounding term (a shift by 31 - rep = -1 would be undefined; the hardware masks it to 31 and adds 2^31).  The
        // state then fills the word: the addition of the least significant level can carry out of it (the carry is bit
        // 32 - logB of `next`), and `next` outgrows decompose_step's 24-bit multiply - shifts and a subtraction instead.
        uint32_t state = x;
#pragma unroll
        for (int lev = L - 1; lev >= 0; lev--) {
            const uint32_t sum = state + half_m1 + __builtin_amdgcn_ubfe(state, 2 * logB - 1, 1);
            uint32_t next = sum >> logB;
            if (lev == L - 1) next |= (uint32_t)(sum < state) << (32 - logB);
            dig[lev] = (int)(state - (next << logB));
            state = next;
        }
        return;
    }
    uint32_t state = (x + (1u << (31 - rep))) >> (32 - rep);
    const int neg_B = -(1 << logB);
#pragma unroll
    for (int lev = L - 1; lev >= 0; lev--) dig[lev] = decompose_step(state, logB, half_m1, neg_B, lev == 0);
}

// Diagnostic clock stamps (HELM_HIP_CLOCK_PROBE=1): workgroup 0 records s_memtime (shader
// clock) and s_memrealtime (100 MHz) around its blind rotation; the ratio is the clock the
// chip actually holds under this kernel's load.  Written to a buffer nothing else reads.
static __device__ unsigned long long g_clock_probe[4];
#ifdef HELM_WIDE_STAMPS
// per-phase cycle totals (diagnostic build only): [workgroup 0 | last workgroup][wave][phase]
static __device__ unsigned long long g_wide_stamps[2 * 16 * 6];
#define STAMP_DECL unsigned long long ph[6] = {0, 0, 0, 0, 0, 0}, t0 = 0, t1;
#define STAMP_BEGIN                        \
    t0 = __builtin_amdgcn_s_memtime();     \
    __builtin_amdgcn_s_waitcnt(0xC07F);
#define STAMP(k)                           \
    t1 = __builtin_amdgcn_s_memtime();     \
    __builtin_amdgcn_s_waitcnt(0xC07F);    \
    ph[k] += t1 - t0;                      \
    t0 = t1;
#define STAMP_END(wave)                                                                          \
    if ((blockIdx.x == 0 || blockIdx.x == gridDim.x - 1) && lane == 0)                           \
        for (int q = 0; q < 6; q++) g_wide_stamps[((blockIdx.x ? 1 : 0) * 16 + (wave)) * 6 + q] = ph[q];
#else
#define STAMP_DECL
#define STAMP_BEGIN
#define STAMP(k)
#define STAMP_END(wave)
#endif

// ------------------------------------------------------------------------------------
// k_pbs: one workgroup = one bootstrap; wave p owns accumulator polynomial p.
//
// Per CMUX step, wave p: rotates/subtracts its polynomial (LDS), decomposes it into L
// digit polynomials, transforms them (M at a time, wave-private LDS transposes),
// multiplies by its (k+1)*L key polynomials, hands the K partial sums that belong to
// other waves over through LDS (the only two workgroup barriers of the step),
// inverse-transforms its own sum and accumulates.
//
// One build (struct PbsCfg): LOCKSTEP - one level at a time (digits produced in the order the signed decomposition generates
// them), that level's key words fetched around its transform, only two partial sums in registers (the third accumulates in
// LDS), twiddles from the LDS lane table (the forward direction's per-lane twiddles copied into registers once), NB = 4
// bootstraps per workgroup, one bootstrap per SIMD (see NB below), issue priorities that fall as a wave advances through the
// step; 168 registers, 138 KB LDS at N = 512 -> one workgroup per CU, three waves on every SIMD doing the same work at the same
// time.  The full rounds of every wide launch: the dominant kernel of the benchmark.  (Rounds 1-5 also carried a latency, a
// balanced and a throughput build of this kernel - all levels transformed together, key words prefetched a step ahead,
// twiddles in registers - and k_pbs_sym; the size dispatch stopped selecting them in round 4 and they were removed in
// round 6: profiles/README.md "retired builds".)
// ------------------------------------------------------------------------------------
enum { TW_LANE = 1 /* lane-major LDS table of forward twiddles, inverse reads it mirrored */,
       TW_LANE_FREG = 2 /* the same, the forward direction's per-lane twiddles copied into registers once */ };

template <typename F_, int LOGN_, int K_, int L_, int TW_, int NB_ = 4>
struct PbsCfg {
    using F = F_;
    static constexpr int LOGN = LOGN_, K = K_, L = L_, TW = TW_;
    // bootstraps per workgroup.  NB = 4: wave w serves bootstrap w % 4 as polynomial w / 4; the
    // hardware deals the waves of a workgroup round the four SIMDs (tools/ubench_placement.hip), so
    // the k+1 waves of a bootstrap share one SIMD, every SIMD carries the same work, and the
    // workgroup barriers couple waves that progress alike
    static constexpr int NB = NB_;
    // level-at-a-time path: key columns fetched before the level's transform (the rest after it)
    // (2 of k+1 = 3: fetching the third one early as well measured the same in the lockstep build)
    static constexpr int EARLY_COLS = 2;
    using G = Geo<LOGN>;
    static constexpr int K1 = K + 1;
    static constexpr int SLOTS = K > 1 ? K : 1; // exchange slots per wave (also carry the hand-over)
    static constexpr int MAX_SMALL_N = 1024;
    // slot 0 is the (padded) transform scratch; the other slots only carry the hand-over and need no padding
    static constexpr int SLOT_STRIDE = G::N;
    // the u32 copy of a wave's accumulator polynomial lives in the wave's (then idle) exchange
    // slots, unrolled negacyclically over 3N - 64 entries (+acc, -acc, +acc) so that the rotated
    // read of slot e is one address register + 256 e bytes, sign included
    static constexpr int ACC3 = 3 * G::N - 64;
    static constexpr int WAVE_STRIDE_X = G::XPAD + (SLOTS - 1) * SLOT_STRIDE;
    static constexpr int WAVE_STRIDE = WAVE_STRIDE_X > (ACC3 + 1) / 2 ? WAVE_STRIDE_X : (ACC3 + 1) / 2;
    static constexpr int slot_off(int s) { return s == 0 ? 0 : G::XPAD + (s - 1) * SLOT_STRIDE; }
    static constexpr int TW_ROWS = G::TWB + G::TWC;
    // the 8-point block form of the N = 512 transforms (ntt_fp64.h fwd_blk8 / inv_blk8; profiles/r07/ab_gates_blk8.txt)
    static constexpr bool BLK8 = blk8_field<F>::value && LOGN == 9 && TW == TW_LANE_FREG;
    static_assert(!BLK8 || TW_ROWS == 14, "the table holds the 2 x 7 block-form twiddles of the inverse");
    static constexpr size_t X_OFF = 0;                                                // double [K1][WAVE_STRIDE]
    static constexpr size_t TW_OFF = X_OFF + sizeof(double) * K1 * WAVE_STRIDE;       // double [TW_ROWS][64]
    static constexpr size_t MS_OFF = TW_OFF + sizeof(double) * TW_ROWS * 64;          // u16 [n+1]
    static constexpr size_t BOOT_BYTES = (MS_OFF + sizeof(uint16_t) * (MAX_SMALL_N + 1) + 15) / 16 * 16;
    static constexpr size_t BYTES = BOOT_BYTES * NB;
};

template <typename C>
__global__ __launch_bounds__(64 * (C::K + 1) * C::NB, 1) void k_pbs(const PbsJob *__restrict__ jobs,
                                                                  const uint32_t *__restrict__ wires,  // rows of n+1
                                                                  const uint32_t *__restrict__ raw_in, // rows of n+1
                                                                  const uint32_t *__restrict__ tvs,    // rows of N
                                                                  const double *__restrict__ bsk,      // NTT domain
                                                                  const double *__restrict__ tw_fwd,
                                                                  const double *__restrict__ tw_inv,
                                                                  uint32_t *__restrict__ out_big, // rows of K*N+1
                                                                  int n, int logB, int probe, int count)
{
    constexpr int LOGN = C::LOGN, K = C::K, L = C::L, NB = C::NB;
    using F = typename C::F;
    using G = Geo<LOGN>;
    constexpr int N = G::N, E = G::E, K1 = K + 1;
    extern __shared__ __align__(16) unsigned char smem_wg[];

    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int p = wv / NB;                       // this wave's polynomial
    const int tid = p * 64 + lane;               // thread index within the bootstrap's k+1 waves
    const int jix = (int)blockIdx.x * NB + wv % NB; // this wave's bootstrap
    // a wave without a bootstrap leaves; the hardware barrier counts the surviving waves only
    if (NB > 1 && jix >= count) return;
    unsigned char *smem = smem_wg + (size_t)(wv % NB) * C::BOOT_BYTES;
    double *X = reinterpret_cast<double *>(smem + C::X_OFF);
    uint16_t *MS = reinterpret_cast<uint16_t *>(smem + C::MS_OFF);
    const PbsJob job = jobs[jix];
    const size_t row = (size_t)n + 1;

    // ---- gate linear step + modulus switch (whole workgroup) ------------------------
    switch_row(MS, GateRows(job, wires, raw_in, row), n, tid, 64 * K1, LOGN + 1);
    // ---- twiddles: the lane-major LDS table (block A: lane-uniform scalars) ---------------
    // C::BLK8 (N = 512 in FpG): blocks B and C of both transforms in the 8-point block form - the lane's seven powers w^t of
    // its group root per block in registers (forward), the w^-t in the LDS table (inverse), the same 14 rows
    using TwF0 = TwLane<LOGN, false>;
    using TwF = typename std::conditional<C::BLK8, TwBlk8Fwd<LOGN>,
                                          typename std::conditional<C::TW == TW_LANE_FREG, TwLaneFwdReg<LOGN>, TwF0>::type>::type;
    using TwI = typename std::conditional<C::BLK8, TwBlk8Inv<LOGN>, TwLane<LOGN, true>>::type;
    TwF0 twf0;
    TwF twf;
    TwI twi;
    {
        double *TW = reinterpret_cast<double *>(smem + C::TW_OFF);
        if constexpr (C::BLK8) {
            for (int r = p; r < C::TW_ROWS; r += K1) TW[r * 64 + lane] = tw_blk8_row<LOGN, -1>(tw_fwd, r, lane);
        } else tw_lane_fill<LOGN>(TW, tw_fwd, p, K1, C::TW_ROWS, lane);
        tw_lane_views(twf0, twi, TW, tw_fwd, lane);
        if constexpr (C::BLK8) {
            twi.row = TW + lane;
            twf.load(tw_fwd, lane);
        } else if constexpr (C::TW == TW_LANE) twf = twf0;
    }
    __syncthreads();
    if constexpr (!C::BLK8 && C::TW == TW_LANE_FREG) twf.load(twf0); // the table is complete: this lane's forward twiddles into registers

    // ---- accumulator init: (0,...,0, X^{-b~} * tv) ------------------------------------
    double *xb = X + (size_t)p * C::WAVE_STRIDE; // this wave's exchange slots
    uint32_t *acc_p = reinterpret_cast<uint32_t *>(xb);
    // the wave's accumulator coefficients in registers, NEGATED: the rotated difference of a step is then one three-operand
    // addition (rotated + (-acc) + rounding offset) instead of a subtraction and an addition
    uint32_t nacc[E];
    {
        const int bt = (int)MS[n];
        const uint32_t *tv = tvs + (size_t)job.tv * N;
#pragma unroll
        for (int e = 0; e < E; e++) {
            const uint32_t v = p == K ? lut_rotated(tv, G::jA(lane, e), bt, N) : 0u;
            nacc[e] = 0u - v;
        }
    }
    auto acc_store = [&]() { acc3_store<N, E, true, true>(acc_p + lane, nacc); };
    acc_store();
    lds_wave_sync();

    // key words of step i for this wave: [i][p][c][lev][e/2][lane] as double2, byte offsets
    const unsigned poly_bytes = (unsigned)(N / 2) * 16u;                 // one key polynomial
    const unsigned step_bytes = (unsigned)(K1 * K1 * L) * poly_bytes;    // one LWE coefficient
    const unsigned row_off = (unsigned)(p * K1 * L) * poly_bytes;        // this wave's GGSW row
    KeyBuf kb;
    kb.init(bsk, (size_t)n * step_bytes, lane);
    // (a zero rotation is not skipped - one step in 2N, its external product is exactly zero - so that the bootstraps that
    // share a workgroup meet at the same barriers)

    // four scalar clock reads per launch that fills the chip (probe bit 1, set by the host), taken by the LAST
    // workgroup - it runs in the launch's last round, when the chip has been under this load for the whole launch
    // (helm_hip_get_clock); HELM_HIP_CLOCK_PROBE=1 (bit 0) stamps every launch
    const bool stamp = (probe & 3) && blockIdx.x == gridDim.x - 1 && tid == 0;
    if (stamp) {
        g_clock_probe[0] = __builtin_amdgcn_s_memtime();
        g_clock_probe[1] = __builtin_amdgcn_s_memrealtime();
    }
    // ---- blind rotation: acc += BSK_i (x) (X^{a_i} acc - acc) -------------------------
    int i = 0;
    // Lockstep build: the waves of a bootstrap share a SIMD, which issues oldest-first, so the youngest
    // would run the end of every step alone (and a lone wave cannot hide its own latencies).  Each wave
    // lowers its priority as it advances through the step - 3 from the second barrier through the
    // inverse transform and the first level, 2 for the second level, 1 for the last level's digits and
    // transform, 0 for its products - so whoever is behind goes first and the three reach the first
    // barrier within one short stage of each other (finer stages towards the end, where it matters).  Plain oldest-first
    // issue measured 109 k instead of 116 k gates/s.
    constexpr bool PRIO = NB > 1;
    if constexpr (PRIO) __builtin_amdgcn_s_setprio(3);
    STAMP_DECL
    while (i < n) {
        STAMP_BEGIN
        const int a = __builtin_amdgcn_readfirstlane((int)MS[i]);
        const unsigned so_i = (unsigned)i * step_bytes + row_off;

        double mine[E];
        {
            // ---- one level at a time, least significant first (throughput build): the
            //      decomposition state is carried in registers, digits are produced in the
            //      order the signed decomposition generates them ---------------------------
            uint32_t state[E];
            {
                const int rep = logB * L;
                const uint32_t *ar = acc_p + ((lane - a) & (2 * N - 1)); // (X^a acc)[jA(lane, e)] = ar[64 e]
#pragma unroll
                for (int e = 0; e < E; e++) state[e] = (ar[64 * e] + nacc[e] + (1u << (31 - rep))) >> (32 - rep);
            }
            // Key column (p + d) % K1 is handled at distance d: d = 0 is this wave's own sum
            // (registers), d = 1 stays in registers and is written to the transform scratch
            // once the last transform is done, d >= 2 is accumulated level by level in its
            // hand-over slot with ds_add_f64 (exact: integers below 2^53) - three partial
            // sums never live in registers together.
            double keep[E];
            const uint32_t half_m1 = (1u << (logB - 1)) - 1u;
            const int neg_B = -(1 << logB);
            int cd[K1]; // wave-uniform column of each distance
#pragma unroll
            for (int d = 0; d < K1; d++) cd[d] = p + d >= K1 ? p + d - K1 : p + d;
#pragma unroll
            for (int lev = L - 1; lev >= 0; lev--) {
                double x[1][E];
#pragma unroll
                for (int e = 0; e < E; e++) x[0][e] = (double)decompose_step(state[e], logB, half_m1, neg_B, lev == 0);
                // this level's key words: issued before the transform that hides their latency
                // (the last column is fetched after the transform: during it the transform's own
                // temporaries need the registers, and the first two products cover its latency)
                double2 bwl[K1][E / 2];
                constexpr int EARLY = C::EARLY_COLS < K1 ? C::EARLY_COLS : K1;
#pragma unroll
                for (int d = 0; d < EARLY; d++)
#pragma unroll
                    for (int e2 = 0; e2 < E / 2; e2++) bwl[d][e2] = kb.load(so_i + (unsigned)(cd[d] * L + lev) * poly_bytes, e2 * 1024);
                __builtin_amdgcn_sched_barrier(0);
                ntt_forward_digits<F, LOGN, 1>(x, xb, twf, lane);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int d = EARLY; d < K1; d++)
#pragma unroll
                    for (int e2 = 0; e2 < E / 2; e2++) bwl[d][e2] = kb.load(so_i + (unsigned)(cd[d] * L + lev) * poly_bytes, e2 * 1024);
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (PRIO)
                    if (lev == 0) __builtin_amdgcn_s_setprio(0);
#pragma unroll
                for (int d = 0; d < K1; d++)
#pragma unroll
                    for (int e2 = 0; e2 < E / 2; e2++) {
                        const double2 w = bwl[d][e2];
                        const double t0 = mulmod<F>(x[0][2 * e2], w.x), t1 = mulmod<F>(x[0][2 * e2 + 1], w.y);
                        if (d == 0) {
                            mine[2 * e2] = lev == L - 1 ? t0 : mine[2 * e2] + t0;
                            mine[2 * e2 + 1] = lev == L - 1 ? t1 : mine[2 * e2 + 1] + t1;
                        } else if (d == 1) {
                            keep[2 * e2] = lev == L - 1 ? t0 : keep[2 * e2] + t0;
                            keep[2 * e2 + 1] = lev == L - 1 ? t1 : keep[2 * e2 + 1] + t1;
                        } else {
                            double *dst = xb + C::slot_off(d - 1) + lane;
                            if (lev == L - 1) {
                                dst[(2 * e2) * 64] = t0;
                                dst[(2 * e2 + 1) * 64] = t1;
                            } else {
                                lds_add(dst + (2 * e2) * 64, t0);
                                lds_add(dst + (2 * e2 + 1) * 64, t1);
                            }
                        }
                    }
                if constexpr (PRIO) {
                    if (lev == L - 1) __builtin_amdgcn_s_setprio(2);
                    else if (lev == 1) __builtin_amdgcn_s_setprio(1);
                }
            }
            {
                double *dst = xb + C::slot_off(0) + lane;
#pragma unroll
                for (int e = 0; e < E; e++) dst[e * 64] = keep[e];
            }
        }
        STAMP(0) // rotation, decomposition, forward transforms, products, hand-over written

        lds_block_sync();
        STAMP(1) // barrier 1
        {
            // the sum for this wave computed at distance d sits in wave (p - d) mod K1, slot d - 1
            if constexpr (!F::LAZY) {
#pragma unroll
                for (int e = 0; e < E; e++) mine[e] = reduce<F>(mine[e]);
            }
#pragma unroll
            for (int d = 1; d < K1; d++) {
                const int q = p - d < 0 ? p - d + K1 : p - d;
                const double *src = X + (size_t)q * C::WAVE_STRIDE + C::slot_off(d - 1);
#pragma unroll
                for (int e = 0; e < E; e++) mine[e] += reduce_unless_lazy<F>(src[e * 64 + lane]);
            }
        }
#pragma unroll
        for (int e = 0; e < E; e++) mine[e] = reduce<F>(mine[e]);
        STAMP(2) // hand-over read and summed
        lds_block_sync(); // every hand-over slot has been read: the slots are free again
        STAMP(3) // barrier 2
        if constexpr (PRIO) __builtin_amdgcn_s_setprio(3);

        ntt_inverse<F, LOGN>(mine, xb, twi, lane);
        STAMP(4) // inverse transform
#pragma unroll
        for (int e = 0; e < E; e++) nacc[e] -= to_torus32(mine[e]);
        acc_store();
        lds_wave_sync();
        STAMP(5) // lift, accumulate, publish
        i++;
    }
    STAMP_END(p)

    if (stamp) {
        g_clock_probe[2] = __builtin_amdgcn_s_memtime();
        g_clock_probe[3] = __builtin_amdgcn_s_memrealtime();
    }
    // ---- sample extract (coefficient 0): wave p writes its own polynomial -------------
    sample_extract0<K, N, -1>(out_big, jix, p, lane == 0, nacc, lane); // nacc[e] = -A_p[jA(lane, e)]
}

// ------------------------------------------------------------------------------------
// k_pbs_wide: one workgroup of (k+1)*L waves per bootstrap - one wave per (polynomial, level).
// For launches that leave CUs partly empty (<= one bootstrap per CU: a single netlist's levels)
// the chain of n CMUX steps is the whole cost, so the step is spread over every SIMD of the CU:
// wave (r, lev) rotates / subtracts polynomial r, keeps digit `lev` of the decomposition,
// transforms it (one NTT instead of L), multiplies by its k+1 key polynomials and adds the
// products into per-column accumulators in LDS (ds_add_f64: exact integer sums, any order);
// the lev = 0 wave of polynomial c then recentres column c, inverse-transforms, lifts and
// updates the accumulator copy every wave of the polynomial reads in the next step.
// ------------------------------------------------------------------------------------
template <typename F_, int LOGN_, int K_, int L_>
struct WideCfg {
    using F = F_;
    static constexpr int LOGN = LOGN_, K = K_, L = L_, K1 = K_ + 1, NW = (K_ + 1) * L_;
    using G = Geo<LOGN>;
    static constexpr int MAX_SMALL_N = 1024;
    static constexpr int ACC3 = (3 * G::N - 64 + 1) / 2 * 2; // u32 entries per polynomial (see PbsCfg)
    static constexpr int TW_ROWS = G::TWB + G::TWC;
    static constexpr size_t X_OFF = 0;                                              // double [NW][XPAD]
    static constexpr size_t COL_OFF = X_OFF + sizeof(double) * NW * G::XPAD;        // double [K1][N]
    static constexpr size_t TW_OFF = COL_OFF + sizeof(double) * K1 * G::N;          // double [TW_ROWS][64]
    static constexpr size_t ACC_OFF = TW_OFF + sizeof(double) * TW_ROWS * 64;       // u32 [K1][ACC3]
    static constexpr size_t MS_OFF = ACC_OFF + sizeof(uint32_t) * K1 * ACC3;        // u16 [n+1]
    static constexpr size_t BYTES = (MS_OFF + sizeof(uint16_t) * (MAX_SMALL_N + 1) + 15) / 16 * 16;
};

template <typename C>
__global__ __launch_bounds__(64 * C::NW, 1) void k_pbs_wide(const PbsJob *__restrict__ jobs,
                                                            const uint32_t *__restrict__ wires,
                                                            const uint32_t *__restrict__ raw_in,
                                                            const uint32_t *__restrict__ tvs,
                                                            const double *__restrict__ bsk,
                                                            const double *__restrict__ tw_fwd,
                                                            uint32_t *__restrict__ out_big, int n, int logB)
{
    constexpr int LOGN = C::LOGN, K = C::K, L = C::L, K1 = C::K1, NW = C::NW;
    using F = typename C::F;
    using G = Geo<LOGN>;
    constexpr int N = G::N, E = G::E;
    extern __shared__ __align__(16) unsigned char smem[];
    double *X = reinterpret_cast<double *>(smem + C::X_OFF);
    double *COL = reinterpret_cast<double *>(smem + C::COL_OFF);
    double *TW = reinterpret_cast<double *>(smem + C::TW_OFF);
    uint32_t *ACC = reinterpret_cast<uint32_t *>(smem + C::ACC_OFF);
    uint16_t *MS = reinterpret_cast<uint16_t *>(smem + C::MS_OFF);

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    // polynomial (GGSW row) and decomposition level of this wave.  The hardware deals the waves of a workgroup
    // round the four SIMDs (wave w -> SIMD w % 4, tools/ubench_placement.hip), so with nine waves SIMD 0 hosts
    // three of them and bounds the forward phase.  A unit's cost grows with the depth of its digit (the carry
    // chain runs from the last level down to the wave's own): the three cheapest units - the last level of each
    // polynomial - go to SIMD 0, and the three level-0 waves, which also run the inverse transforms, to three
    // different SIMDs (the plain (polynomial, level) order measured 3.6 - 4.6 % slower,
    // profiles/r02/wide_kernel_experiments.txt).
    int r = w / L, lev = w - r * L;
    if constexpr (K1 == 3 && L == 3) {
        // w:  0  1  2  3  4  5  6  7  8      (two bits per wave, packed: a table indexed by w would live in scratch)
        // r:  0  0  1  2  1  0  1  2  2      lev:  2  0  0  0  2  1  1  1  2
        constexpr unsigned RR = 0u | 0u << 2 | 1u << 4 | 2u << 6 | 1u << 8 | 0u << 10 | 1u << 12 | 2u << 14 | 2u << 16;
        constexpr unsigned LL = 2u | 0u << 2 | 0u << 4 | 0u << 6 | 2u << 8 | 1u << 10 | 1u << 12 | 1u << 14 | 2u << 16;
        r = (int)((RR >> (2 * w)) & 3u);
        lev = (int)((LL >> (2 * w)) & 3u);
    } else if constexpr (K1 == 2 && L == 3) {
        // six waves sit 2 / 2 / 1 / 1 on the SIMDs: the two inverse waves (level 0) alone on SIMDs 2 and 3, the
        // last-level units on SIMD 0, the level-1 units on SIMD 1.  The polynomial stays r = w / L; only the levels are
        // permuted (a table for r as well costs 9 - 10 more registers at the same occupancy)
        // w:  0  1  2  3  4  5        r:  0  0  0  1  1  1        lev:  2  1  0  0  2  1
        constexpr unsigned LL = 2u | 1u << 2 | 0u << 4 | 0u << 6 | 2u << 8 | 1u << 10;
        lev = (int)((LL >> (2 * w)) & 3u);
    }
    const PbsJob job = jobs[blockIdx.x];
    const size_t row = (size_t)n + 1;
    switch_row(MS, GateRows(job, wires, raw_in, row), n, tid, 64 * NW, LOGN + 1);
    tw_lane_fill<LOGN>(TW, tw_fwd, w, NW, C::TW_ROWS, lane);
    for (int j = tid; j < K1 * N; j += 64 * NW) COL[j] = 0.0;
    // Round 4: at N = 512 the lane's block-B / block-C twiddles of BOTH directions are copied into registers once per
    // kernel (2 x 14 doubles: 110 -> 166 registers, the limit for the three waves of SIMD 0 is 168) instead of read from the
    // LDS lane table in every transform - the reads sat on the latency chain of a step: 3.5 % faster (64 bootstraps: 3.136
    // -> 3.024 ms, 256: 3.444 -> 3.324 ms, same box, alternating, identical ciphertexts; forward direction alone: 1.4 %).
    // N = 1024 keeps the table (2 x 28 doubles spill).
    constexpr int TWR = LOGN == 9 ? 3 : 0; // bit 0: forward twiddles in registers, bit 1: inverse
    TwLane<LOGN, false> twf0;
    TwLane<LOGN, true> twi0;
    tw_lane_views(twf0, twi0, TW, tw_fwd, lane);
    __syncthreads();
    typename std::conditional<(TWR & 1) != 0, TwLaneReg<LOGN, false>, TwLane<LOGN, false>>::type twf;
    typename std::conditional<(TWR & 2) != 0, TwLaneReg<LOGN, true>, TwLane<LOGN, true>>::type twi;
    if constexpr ((TWR & 1) != 0) twf.load(twf0);
    else twf = twf0;
    if constexpr ((TWR & 2) != 0) twi.load(twi0);
    else twi = twi0;

    // accumulator (0, ..., 0, X^{-b~} tv): the lev = 0 wave of polynomial r owns it (registers)
    // and publishes the negacyclically unrolled u32 copy every wave of the polynomial reads
    uint32_t *acc_r = ACC + (size_t)r * C::ACC3;
    uint32_t accr[E];
    auto acc_store = [&]() { acc3_store<N, E, false, true>(acc_r + lane, accr); };
    if (lev == 0) {
        const int bt = (int)MS[n];
        const uint32_t *tv = tvs + (size_t)job.tv * N;
#pragma unroll
        for (int e = 0; e < E; e++) accr[e] = r == K ? lut_rotated(tv, G::jA(lane, e), bt, N) : 0u;
        acc_store();
    }
    __syncthreads();

    double *xb = X + (size_t)w * G::XPAD;
    const unsigned poly_bytes = (unsigned)(N / 2) * 16u;
    const unsigned step_bytes = (unsigned)(K1 * K1 * L) * poly_bytes;
    const unsigned wave_off = (unsigned)(r * K1 * L + lev) * poly_bytes; // + c * L * poly_bytes per column
    KeyBuf kb;
    kb.init(bsk, (size_t)n * step_bytes, lane);
    const uint32_t half_m1 = (1u << (logB - 1)) - 1u;
    const int neg_B = -(1 << logB);
    const int rep = logB * L;

    STAMP_DECL
    __builtin_amdgcn_s_setprio(3);
    // Key words (k+1 polynomials of this wave's row and level).  Nine waves x 12 loads of 1 KiB per step keep the CU's
    // vector-memory path busy for ~1.7 k cycles, and a wave cannot start its arithmetic until its loads are accepted:
    // finer per-phase stamps showed the load issue alone taking 0.3 k (oldest wave) to 1.6 k cycles (youngest) at the
    // top of a step.  The six waves that idle during the inverse transforms therefore fetch the NEXT step's words
    // right after barrier 1, into the registers their products have just released; only the three inverse waves
    // still load at the top of the step (every wave loading there measured 5 % slower,
    // profiles/r02/wide_kernel_experiments.txt).
    double2 kw[K1][E / 2];
    auto load_keys = [&](int ii) {
        const unsigned so = (unsigned)ii * step_bytes + wave_off;
#pragma unroll
        for (int c = 0; c < K1; c++)
#pragma unroll
            for (int e2 = 0; e2 < E / 2; e2++) kw[c][e2] = kb.load(so + (unsigned)(c * L) * poly_bytes, e2 * 1024);
    };
    const bool ahead = lev != 0;
    int i = 0, a = 0;
    while (i < n && (a = __builtin_amdgcn_readfirstlane((int)MS[i])) == 0) i++; // a zero rotation adds nothing
    if (i < n && ahead) load_keys(i);
    while (i < n) {
        STAMP_BEGIN
        if (!ahead) load_keys(i);
        // rotate / subtract, run the signed decomposition down to this wave's level
        double x[1][E];
        {
            const uint32_t *ar = acc_r + ((lane - a) & (2 * N - 1));
            const uint32_t *ac = acc_r + lane;
            uint32_t st[E];
            int dig[E];
#pragma unroll
            for (int e = 0; e < E; e++) st[e] = ((ar[64 * e] - ac[64 * e]) + (1u << (31 - rep))) >> (32 - rep);
            // the carry chain runs from the least significant level down to this wave's own
#pragma unroll
            for (int l = L - 1; l >= 0; l--) {
                if (l >= lev) {
#pragma unroll
                    for (int e = 0; e < E; e++) dig[e] = decompose_step(st[e], logB, half_m1, neg_B, l == 0);
                }
            }
#pragma unroll
            for (int e = 0; e < E; e++) x[0][e] = (double)dig[e];
        }
        STAMP(0) // loads issued, rotation, decomposition
        // the SIMD that hosts three of the nine waves bounds this phase: stepping the issue priority down
        // block by block keeps its waves abreast instead of letting the youngest finish alone
        ntt_forward_digits<F, LOGN, 1, 3>(x, xb, twf, lane);
        __builtin_amdgcn_s_setprio(0);
        STAMP(1) // forward transform
#pragma unroll
        for (int c = 0; c < K1; c++) {
            double *col = COL + (size_t)c * N + lane;
#pragma unroll
            for (int e2 = 0; e2 < E / 2; e2++) {
                // (k+1) L products meet in a column: <= 11.3 p in the lazy field (2^53 = 14.2 p); the
                // 51-bit field recentres each first (<= 4.5 p of its 5.3 p)
                lds_add_wg(col + (2 * e2) * 64, reduce_unless_lazy<F>(mulmod<F>(x[0][2 * e2], kw[c][e2].x)));
                lds_add_wg(col + (2 * e2 + 1) * 64, reduce_unless_lazy<F>(mulmod<F>(x[0][2 * e2 + 1], kw[c][e2].y)));
            }
        }
        STAMP(2) // products
        int inext = i + 1, anext = 0;
        while (inext < n && (anext = __builtin_amdgcn_readfirstlane((int)MS[inext])) == 0) inext++; // uniform over the workgroup
        lds_block_sync(); // every product of the step is in its column
        STAMP(3) // barrier 1
        if (ahead && inext < n) load_keys(inext);
        if (lev == 0) {
            double mine[E];
            double *col = COL + (size_t)r * N + lane;
#pragma unroll
            for (int e = 0; e < E; e++) {
                mine[e] = reduce<F>(col[e * 64]);
                col[e * 64] = 0.0;
            }
            ntt_inverse<F, LOGN>(mine, xb, twi, lane);
#pragma unroll
            for (int e = 0; e < E; e++) accr[e] += to_torus32(mine[e]);
            acc_store();
        }
        STAMP(4) // inverse side (lev = 0) or nothing
        lds_block_sync(); // accumulator copies published, columns cleared
        STAMP(5) // barrier 2
        __builtin_amdgcn_s_setprio(3);
        i = inext;
        a = anext;
    }
    STAMP_END(w)

    if (lev == 0) sample_extract0<K, N, 1>(out_big, blockIdx.x, r, lane == 0, accr, lane);
}

// ------------------------------------------------------------------------------------
// k_pbs_duo: the build for launches of MORE than one and at most TWO bootstraps per CU.
// Round 3 had nothing between the wide build (one bootstrap per CU on all four SIMDs, 3.2 - 3.6 ms per round) and a
// lockstep round (four per CU, one SIMD each, 8.5 ms): 257 - 512 bootstraps cost 7.4 ms on the throughput build, which is
// what a rank's chunk of a sharded launch looks like at 8 GPUs (circuit.rs:531: the level is the sharded unit).
//
// Two bootstraps per workgroup, 2 (k+1) waves per bootstrap = (polynomial r, part g): 12 waves, three per SIMD.
//   g = 0 ("A")  the digits of levels 0 .. L-2 of polynomial r: per level one forward transform and k+1 products, added to
//                the per-column accumulators in LDS (ds_add_f64: exact integer sums, any order)
//   g = 1 ("B")  the digit of level L-1 (first out of the carry chain), its transform and products; after the barrier the
//                inverse transform of column r, the lift and the accumulator update of polynomial r, whose negacyclically
//                unrolled u32 copy both waves of the polynomial rotate and decompose in the next step.
// A step of a bootstrap is two intervals between workgroup barriers: the forward interval (rotation, digits, transforms,
// products: issue-bound, 4.8 k wave-instructions) and the inverse interval (k+1 inverse transforms on k+1 waves: a
// dependent chain of nine butterfly stages and four LDS round trips, 3.5 k cycles for a wave that runs alone while the
// other waves of the bootstrap have nothing to do).
//   STAG = false  both bootstraps in the same interval, bootstrap b on SIMDs 2b and 2b + 1 as (A0, A1, B2 | B0, B1, A2):
//                 per-phase stamps (profiles/r04) show 11.4 k cycles of forward interval and 5.5 k of inverse interval in
//                 which nine of twelve waves wait.
//   STAG = true   bootstrap 1 runs ONE INTERVAL BEHIND bootstrap 0 and the two share all four SIMDs: while one bootstrap's
//                 three inverse waves walk their latency chain, the other's six waves fill the issue slots with its forward
//                 interval.  The priorities decide it: with the inverse waves ABOVE the forward waves the forward interval
//                 stretches from 5.7 k to 9 k cycles (5 % slower than in step); BELOW them (they only have to be done by the
//                 end of the interval) and the forward waves at one flat priority: 4 % FASTER than in step - the default.
//                 Same barriers per step, same arithmetic: identical ciphertexts.
// Issue priorities (profiles/r04/duo_experiments.txt, profiles/r05/ab_duo1024_fpi.jsonl): at N = 512 as just described, in
// either build; at N = 1024 the forward waves step down 3 -> 2 -> 1 and the inverse waves go first, in either build (flat
// priorities and none measured 5 % slower there).
// ------------------------------------------------------------------------------------
template <typename F_, int LOGN_, int K_, int L_, bool STAG_>
struct DuoCfg {
    using F = F_;
    static constexpr int LOGN = LOGN_, K = K_, L = L_, K1 = K_ + 1, NB = 2, NWB = 2 * (K_ + 1), NW = 4 * (K_ + 1);
    static constexpr bool STAG = STAG_;
    using G = Geo<LOGN>;
    static constexpr int MAX_SMALL_N = 1024;
    // COMPACT (N = 1024, round 5): two bootstraps of the N = 512 layout scaled up would need 2 x 91.5 KB.  The lane twiddle
    // table is shared by the workgroup's two bootstraps (it is the same table) and the accumulator copy holds the polynomial
    // and its negation only (2 N entries; the third, wrap-free part of the N = 512 layout becomes an index mask per read):
    // 2 x 69.6 KB + 14.3 KB = 153.6 KB.
    static constexpr bool COMPACT = LOGN >= 10;
    static constexpr int ACC3 = COMPACT ? 2 * G::N : (3 * G::N - 64 + 1) / 2 * 2; // u32 entries per polynomial (see PbsCfg)
    static constexpr int TW_ROWS = G::TWB + G::TWC;
    static_assert(L >= 2, "part A needs at least one level");
    static_assert(K1 == 2 || K1 == 3, "wave maps are written for k = 1 and k = 2");
    static constexpr bool FLAT = LOGN < 10;            // forward waves at one priority (2) instead of stepping 3 -> 2 -> 1
    static constexpr bool INV_LOW = STAG && LOGN < 10; // inverse waves below the other bootstrap's forward waves
    static constexpr size_t TW_SHARED = COMPACT ? sizeof(double) * TW_ROWS * 64 : 0; // at the workgroup's base, before the bootstraps
    // per bootstrap
    static constexpr size_t X_OFF = 0;                                              // double [NWB][XPAD]
    static constexpr size_t COL_OFF = X_OFF + sizeof(double) * NWB * G::XPAD;       // double [K1][N]
    static constexpr size_t TW_OFF = COL_OFF + sizeof(double) * K1 * G::N;          // double [TW_ROWS][64] (not COMPACT)
    static constexpr size_t ACC_OFF = TW_OFF + (COMPACT ? 0 : sizeof(double) * TW_ROWS * 64); // u32 [K1][ACC3]
    static constexpr size_t MS_OFF = ACC_OFF + sizeof(uint32_t) * K1 * ACC3;        // u16 [n+1]
    static constexpr size_t BOOT_BYTES = (MS_OFF + sizeof(uint16_t) * (MAX_SMALL_N + 1) + 15) / 16 * 16;
    static constexpr size_t BYTES = TW_SHARED + BOOT_BYTES * NB;
};

template <typename C>
__global__ __launch_bounds__(64 * C::NW, C::NW / 4) void k_pbs_duo(const PbsJob *__restrict__ jobs, const uint32_t *__restrict__ wires,
                                                           const uint32_t *__restrict__ raw_in, const uint32_t *__restrict__ tvs,
                                                           const double *__restrict__ bsk, const double *__restrict__ tw_fwd,
                                                           uint32_t *__restrict__ out_big, int n, int logB, int count)
{
    constexpr int LOGN = C::LOGN, K = C::K, L = C::L, K1 = C::K1, NB = C::NB, NWB = C::NWB;
    using F = typename C::F;
    using G = Geo<LOGN>;
    constexpr int N = G::N, E = G::E;
    extern __shared__ __align__(16) unsigned char smem_wg[];

    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // wave -> (bootstrap of the workgroup, polynomial, part); wave w sits on SIMD w % 4
    int b, r, g;
    if constexpr (!C::STAG) {
        const int s = w & 1, q = w >> 2; // SIMD of the bootstrap's pair, wave of that SIMD
        b = (w & 3) >> 1;
        r = q;
        g = ((q == K1 - 1) ? 1 : 0) ^ s;
    } else if constexpr (K1 == 3) {
        // SIMD 0: A0 a0 B0   SIMD 1: A1 a1 B1   SIMD 2: A2 a2 b0   SIMD 3: B2 b1 b2   (capitals: bootstrap 0): in either kind of
        // interval every SIMD carries close to a quarter of (forward interval of one bootstrap + inverses of the other)
        // w:     0  1  2  3  4  5  6  7  8  9 10 11
        // b:     0  0  0  0  1  1  1  1  0  0  1  1      r:  0 1 2 2 0 1 2 1 0 1 0 2      g:  0 0 0 1 0 0 0 1 1 1 1 1
        constexpr unsigned BB = 0xCF0u, GG = 0xF88u;
        constexpr unsigned RR = 0u | 1u << 2 | 2u << 4 | 2u << 6 | 0u << 8 | 1u << 10 | 2u << 12 | 1u << 14 | 0u << 16 | 1u << 18 | 0u << 20 | 2u << 22;
        b = (int)((BB >> w) & 1u);
        g = (int)((GG >> w) & 1u);
        r = (int)((RR >> (2 * w)) & 3u);
    } else {
        // eight waves, two per SIMD: SIMD 0: A0 a0   SIMD 1: A1 a1   SIMD 2: B0 b0   SIMD 3: B1 b1
        b = w >> 2;
        r = w & 1;
        g = (w >> 1) & 1;
    }
    const int jix = (int)blockIdx.x * NB + b;
    if (jix >= count) return; // the hardware barrier counts the surviving waves only
    unsigned char *smem = smem_wg + C::TW_SHARED + (size_t)b * C::BOOT_BYTES;
    double *X = reinterpret_cast<double *>(smem + C::X_OFF);
    double *COL = reinterpret_cast<double *>(smem + C::COL_OFF);
    // COMPACT: one table for the workgroup; each bootstrap's waves fill ALL of it (the same values: the other bootstrap's
    // waves may have left already, and nobody reads before the barrier below)
    double *TW = C::COMPACT ? reinterpret_cast<double *>(smem_wg) : reinterpret_cast<double *>(smem + C::TW_OFF);
    uint32_t *ACC = reinterpret_cast<uint32_t *>(smem + C::ACC_OFF);
    uint16_t *MS = reinterpret_cast<uint16_t *>(smem + C::MS_OFF);
    const int wb = r * 2 + g;            // wave index within the bootstrap
    const int tid = wb * 64 + lane;      // thread index within the bootstrap
    const PbsJob job = jobs[jix];
    const size_t row = (size_t)n + 1;
    switch_row(MS, GateRows(job, wires, raw_in, row), n, tid, 64 * NWB, LOGN + 1);
    tw_lane_fill<LOGN>(TW, tw_fwd, wb, NWB, C::TW_ROWS, lane);
    for (int j = tid; j < K1 * N; j += 64 * NWB) COL[j] = 0.0;
    // the forward direction's per-lane twiddles in registers (123 -> 151): 1.5 % (same-box A/B with the wide kernel's)
    TwLane<LOGN, false> twf0;
    TwLane<LOGN, true> twi;
    tw_lane_views(twf0, twi, TW, tw_fwd, lane);
    __syncthreads();
    TwLaneReg<LOGN, false> twf;
    twf.load(twf0);

    // accumulator (0, ..., 0, X^{-b~} tv): part B of polynomial r owns it (registers) and publishes the unrolled u32 copy
    uint32_t *acc_r = ACC + (size_t)r * C::ACC3;
    uint32_t accr[E];
    auto acc_store = [&]() { acc3_store<N, E, false, !C::COMPACT>(acc_r + lane, accr); };
    if (g == 1) {
        const int bt = (int)MS[n];
        const uint32_t *tv = tvs + (size_t)job.tv * N;
#pragma unroll
        for (int e = 0; e < E; e++) accr[e] = r == K ? lut_rotated(tv, G::jA(lane, e), bt, N) : 0u;
        acc_store();
    }
    __syncthreads();

    double *xb = X + (size_t)wb * G::XPAD;
    const unsigned poly_bytes = (unsigned)(N / 2) * 16u;
    const unsigned step_bytes = (unsigned)(K1 * K1 * L) * poly_bytes;
    const unsigned row_off = (unsigned)(r * K1 * L) * poly_bytes; // + (c * L + lev) * poly_bytes
    KeyBuf kb;
    kb.init(bsk, (size_t)n * step_bytes, lane);
    const uint32_t half_m1 = (1u << (logB - 1)) - 1u;
    const int neg_B = -(1 << logB);
    const int rep = logB * L;

    // key words of one level of this wave's row: k+1 polynomials
    double2 kw[K1][E / 2];
    auto load_keys = [&](int ii, int lev) {
        const unsigned so = (unsigned)ii * step_bytes + row_off + (unsigned)lev * poly_bytes;
#pragma unroll
        for (int c = 0; c < K1; c++)
#pragma unroll
            for (int e2 = 0; e2 < E / 2; e2++) kw[c][e2] = kb.load(so + (unsigned)(c * L) * poly_bytes, e2 * 1024);
    };
    // the level a wave transforms first in a step: its key words are fetched in the inverse interval before - by part A
    // while it has nothing else to do, by part B right after its accumulator update
    const int first_lev = g == 1 ? L - 1 : L - 2;
    // a zero rotation is not skipped: the two bootstraps of a workgroup meet at the same barriers (one step in 2N; its
    // external product is exactly zero)
    load_keys(0, first_lev);
    const int lag = C::STAG ? b : 0;          // intervals this bootstrap runs behind bootstrap 0
    const int T = 2 * n + (C::STAG ? 1 : 0);  // intervals of the workgroup
    STAMP_DECL
    for (int t = 0; t < T; t++) {
        STAMP_BEGIN
        const int tt = t - lag;
        const int i = tt >> 1;
        if (tt >= 0 && tt < 2 * n && !(tt & 1)) {
            // ---- forward interval of step i --------------------------------------------------------------------------
            __builtin_amdgcn_s_setprio(C::FLAT ? 2 : 3);
            const int a = __builtin_amdgcn_readfirstlane((int)MS[i]);
            uint32_t st[E];
            {
                const uint32_t *ac = acc_r + lane;
                if constexpr (C::COMPACT) { // [acc, -acc]: the rotated index wraps at 2 N
                    const int base = lane - a;
#pragma unroll
                    for (int e = 0; e < E; e++)
                        st[e] = ((acc_r[(base + 64 * e) & (2 * N - 1)] - ac[64 * e]) + (1u << (31 - rep))) >> (32 - rep);
                } else {
                    const uint32_t *ar = acc_r + ((lane - a) & (2 * N - 1));
#pragma unroll
                    for (int e = 0; e < E; e++) st[e] = ((ar[64 * e] - ac[64 * e]) + (1u << (31 - rep))) >> (32 - rep);
                }
            }
            double x[1][E];
            if (g == 1) {
#pragma unroll
                for (int e = 0; e < E; e++) x[0][e] = (double)decompose_step(st[e], logB, half_m1, neg_B);
                ntt_forward_digits<F, LOGN, 1>(x, xb, twf, lane);
                if constexpr (!C::FLAT) __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int c = 0; c < K1; c++) {
                    double *col = COL + (size_t)c * N + lane;
#pragma unroll
                    for (int e2 = 0; e2 < E / 2; e2++) {
                        lds_add_wg(col + (2 * e2) * 64, reduce_unless_lazy<F>(mulmod<F>(x[0][2 * e2], kw[c][e2].x)));
                        lds_add_wg(col + (2 * e2 + 1) * 64, reduce_unless_lazy<F>(mulmod<F>(x[0][2 * e2 + 1], kw[c][e2].y)));
                    }
                }
            } else {
                // the carry chain starts at the least significant level, which part B transforms
#pragma unroll
                for (int e = 0; e < E; e++) (void)decompose_step(st[e], logB, half_m1, neg_B);
                // (summing the levels' products in registers first would halve the LDS additions, but (k+1) E more doubles
                // next to the key words and the transform's temporaries do not fit three waves per SIMD: 49 spilled registers)
#pragma unroll
                for (int lev = L - 2; lev >= 0; lev--) {
#pragma unroll
                    for (int e = 0; e < E; e++) x[0][e] = (double)decompose_step(st[e], logB, half_m1, neg_B, lev == 0);
                    if (lev != L - 2) load_keys(i, lev); // (the first level's words came an interval ahead)
                    ntt_forward_digits<F, LOGN, 1>(x, xb, twf, lane);
                    if constexpr (!C::FLAT) { // a wave steps its priority down as it advances: whoever is behind goes first (see k_pbs)
                        if (lev) __builtin_amdgcn_s_setprio(2);
                        else __builtin_amdgcn_s_setprio(1);
                    }
#pragma unroll
                    for (int c = 0; c < K1; c++) {
                        double *col = COL + (size_t)c * N + lane;
#pragma unroll
                        for (int e2 = 0; e2 < E / 2; e2++) {
                            lds_add_wg(col + (2 * e2) * 64, reduce_unless_lazy<F>(mulmod<F>(x[0][2 * e2], kw[c][e2].x)));
                            lds_add_wg(col + (2 * e2 + 1) * 64, reduce_unless_lazy<F>(mulmod<F>(x[0][2 * e2 + 1], kw[c][e2].y)));
                        }
                    }
                }
            }
            STAMP(0) // rotation, digits, forward transforms, products
        } else if (tt >= 0 && tt < 2 * n) {
            // ---- inverse interval of step i: every product of the step is in its column ------------------------------
            // in step: everybody waits for the inverse waves, they go first.  INV_LOW puts the inverse chain BELOW the other
            // bootstrap's forward waves instead (it only has to be done by the end of their interval)
            __builtin_amdgcn_s_setprio(C::INV_LOW ? 0 : 3);
            if (g == 1) {
                double mine[E];
                double *col = COL + (size_t)r * N + lane;
#pragma unroll
                for (int e = 0; e < E; e++) {
                    mine[e] = reduce<F>(col[e * 64]);
                    col[e * 64] = 0.0;
                }
                ntt_inverse<F, LOGN>(mine, xb, twi, lane);
#pragma unroll
                for (int e = 0; e < E; e++) accr[e] += to_torus32(mine[e]);
                acc_store();
            }
            if (i + 1 < n) load_keys(i + 1, first_lev);
            STAMP(2) // part B: inverse transform, lift, accumulator update; key words of the next step issued
        }
        lds_block_sync(); // forward interval: products in their columns; inverse interval: accumulator copies published
        STAMP(1) // barrier
    }
    STAMP_END(w)

    if (g == 1) sample_extract0<K, N, 1>(out_big, jix, r, lane == 0, accr, lane);
}

// ------------------------------------------------------------------------------------
// k_pbs_trio: THREE bootstraps per workgroup of 12 waves, four waves per bootstrap - for the remainders of a launch that
// hold between two and three bootstraps per CU (round 4: a lockstep round with one SIMD empty costs as much as a full one).
// The (k+1) L = 9 forward transforms, 27 products and k+1 = 3 inverse transforms of a step are cut into four wave-roles of
// three transforms each:
//   polynomial wave p (k+1 of them)  rotates / subtracts polynomial p, produces the first digit of the signed decomposition
//                                    (level L-1) and hands it to the helper, transforms levels L-2 .. 0 itself (level at a
//                                    time, as the lockstep build), multiplies with their key rows, and after the hand-over of
//                                    the column sums inverse-transforms column p and updates the accumulator;
//   helper wave                      transforms the level-(L-1) digits of ALL k+1 polynomials and multiplies them with their
//                                    key rows (k+1 transforms, (k+1)^2 products); idle during the inverse transforms.
// Wave w serves bootstrap w % 3 in role w / 3: every SIMD carries three waves of about the same instruction count.  Three
// workgroup barriers per step (digits published | column sums published | column sums consumed).  Ciphertexts identical
// to every other build (exact integer sums in any order).  Issue priorities step down as a
// wave advances, as in k_pbs (without them 7 % slower, profiles/r04/trio_experiments.txt).
// ------------------------------------------------------------------------------------
template <typename F_, int LOGN_, int K_, int L_>
struct TrioCfg {
    using F = F_;
    static constexpr int LOGN = LOGN_, K = K_, L = L_, K1 = K_ + 1, NB = 3, NWB = K_ + 2, NW = NWB * NB;
    using G = Geo<LOGN>;
    static_assert(K == 2 && L >= 2, "three column distances; the polynomial waves keep L - 1 levels");
    static constexpr int HL = L - 1;                       // the helper's level: the first digit produced
    static constexpr int ACC3 = 3 * G::N - 64;             // accumulator copy, unrolled negacyclically (see PbsCfg)
    static constexpr int PW = G::XPAD + G::N;              // polynomial wave: transform scratch (= slot 0) + slot 1, doubles
    static_assert(PW >= (ACC3 + 1) / 2, "the accumulator copy lives in the wave's slots between steps");
    static constexpr int HW = G::XPAD + K * G::N + K1 * G::N / 2; // helper: scratch (= slot 0) + slots 1..K + the int32 digits
    static constexpr int slot_off(int s) { return s == 0 ? 0 : G::XPAD + (s - 1) * G::N; }
    static constexpr int DIG_OFF = G::XPAD + K * G::N;     // (doubles) int32 digits [K1][N] behind the helper's slots
    static constexpr int TW_ROWS = G::TWB + G::TWC;
    static constexpr int MAX_SMALL_N = 1024;
    static constexpr size_t TW_BYTES = sizeof(double) * TW_ROWS * 64; // one lane table for the workgroup
    static constexpr size_t MS_OFF = sizeof(double) * (K1 * PW + HW);
    static constexpr size_t BOOT_BYTES = (MS_OFF + sizeof(uint16_t) * (MAX_SMALL_N + 1) + 15) / 16 * 16;
    static constexpr size_t BYTES = TW_BYTES + BOOT_BYTES * NB;
};

template <typename C>
__global__ __launch_bounds__(64 * C::NW, 1) void k_pbs_trio(const PbsJob *__restrict__ jobs, const uint32_t *__restrict__ wires,
                                                            const uint32_t *__restrict__ raw_in, const uint32_t *__restrict__ tvs,
                                                            const double *__restrict__ bsk, const double *__restrict__ tw_fwd,
                                                            uint32_t *__restrict__ out_big, int n, int logB, int count)
{
    constexpr int LOGN = C::LOGN, K = C::K, L = C::L, NB = C::NB, K1 = C::K1, HL = C::HL;
    using F = typename C::F;
    using G = Geo<LOGN>;
    constexpr int N = G::N, E = G::E;
    extern __shared__ __align__(16) unsigned char smem_wg[];

    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int role = wv / NB;                          // 0..K: polynomial, K1: helper
    const int jix = (int)blockIdx.x * NB + wv % NB;    // this wave's bootstrap
    const bool helper = role == K1;
    const int p = role;
    double *TW = reinterpret_cast<double *>(smem_wg);
    // the lane table of the forward twiddles, one for the workgroup: filled by every wave BEFORE the waves without a
    // bootstrap leave (the hardware barrier counts the surviving waves only)
    tw_lane_fill<LOGN>(TW, tw_fwd, wv, C::NW, C::TW_ROWS, lane);
    __syncthreads();
    if (jix >= count) return;
    unsigned char *smem = smem_wg + C::TW_BYTES + (size_t)(wv % NB) * C::BOOT_BYTES;
    double *X = reinterpret_cast<double *>(smem);
    double *HX = X + (size_t)K1 * C::PW;               // the helper's slots
    int *DIG = reinterpret_cast<int *>(HX + C::DIG_OFF);
    uint16_t *MS = reinterpret_cast<uint16_t *>(smem + C::MS_OFF);
    const PbsJob job = jobs[jix];
    const size_t row = (size_t)n + 1;
    const int tid = role * 64 + lane;

    // ---- gate linear step + modulus switch (the bootstrap's four waves) ----------------
    switch_row(MS, GateRows(job, wires, raw_in, row), n, tid, 64 * C::NWB, LOGN + 1);
    TwLane<LOGN, false> twf0;
    TwLane<LOGN, true> twi;
    TwLaneFwdReg<LOGN> twf;
    tw_lane_views(twf0, twi, TW, tw_fwd, lane);
    twf.load(twf0); // this lane's forward twiddles of blocks B and C in registers (as the lockstep build)
    __syncthreads(); // MS complete

    const unsigned poly_bytes = (unsigned)(N / 2) * 16u;
    const unsigned step_bytes = (unsigned)(K1 * K1 * L) * poly_bytes;
    KeyBuf kb;
    kb.init(bsk, (size_t)n * step_bytes, lane);
    const uint32_t half_m1 = (1u << (logB - 1)) - 1u;
    const int neg_B = -(1 << logB);
    STAMP_DECL

    if (helper) {
        // ================= helper wave: level HL of every polynomial ======================================
        for (int i = 0; i < n; i++) {
            STAMP_BEGIN
            lds_block_sync(); // A: the digits of this step are published
            STAMP(1)
            __builtin_amdgcn_s_setprio(2);
            double s0[E], s1[E];
#pragma unroll
            for (int q = 0; q < K1; q++) {
                const unsigned so = (unsigned)i * step_bytes + (unsigned)(q * K1 * L + HL) * poly_bytes;
                double x[1][E];
                {
                    const int *dq = DIG + q * N + lane;
#pragma unroll
                    for (int e = 0; e < E; e++) x[0][e] = (double)dq[64 * e];
                }
                double2 bwl[K1][E / 2];
#pragma unroll
                for (int c = 0; c < 2; c++)
#pragma unroll
                    for (int e2 = 0; e2 < E / 2; e2++) bwl[c][e2] = kb.load(so + (unsigned)(c * L) * poly_bytes, e2 * 1024);
                __builtin_amdgcn_sched_barrier(0);
                ntt_forward_digits<F, LOGN, 1>(x, HX, twf, lane);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int c = 2; c < K1; c++)
#pragma unroll
                    for (int e2 = 0; e2 < E / 2; e2++) bwl[c][e2] = kb.load(so + (unsigned)(c * L) * poly_bytes, e2 * 1024);
                __builtin_amdgcn_sched_barrier(0);
                if (q == K1 - 1) __builtin_amdgcn_s_setprio(0);
#pragma unroll
                for (int c = 0; c < K1; c++)
#pragma unroll
                    for (int e2 = 0; e2 < E / 2; e2++) {
                        const double2 w = bwl[c][e2];
                        const double t0 = mulmod<F>(x[0][2 * e2], w.x), t1 = mulmod<F>(x[0][2 * e2 + 1], w.y);
                        if (c == 0) {
                            s0[2 * e2] = q == 0 ? t0 : s0[2 * e2] + t0;
                            s0[2 * e2 + 1] = q == 0 ? t1 : s0[2 * e2 + 1] + t1;
                        } else if (c == 1) {
                            s1[2 * e2] = q == 0 ? t0 : s1[2 * e2] + t0;
                            s1[2 * e2 + 1] = q == 0 ? t1 : s1[2 * e2 + 1] + t1;
                        } else {
                            double *dst = HX + C::slot_off(c) + lane;
                            if (q == 0) {
                                dst[(2 * e2) * 64] = t0;
                                dst[(2 * e2 + 1) * 64] = t1;
                            } else {
                                lds_add(dst + (2 * e2) * 64, t0);
                                lds_add(dst + (2 * e2 + 1) * 64, t1);
                            }
                        }
                    }
                if (q == 0) __builtin_amdgcn_s_setprio(1);
            }
            lds_wave_sync(); // the last transform's reads of the scratch (= slot 0) are done
            {
                double *d0 = HX + C::slot_off(0) + lane, *d1 = HX + C::slot_off(1) + lane;
#pragma unroll
                for (int e = 0; e < E; e++) {
                    d0[e * 64] = s0[e];
                    d1[e * 64] = s1[e];
                }
            }
            STAMP(2)
            lds_block_sync(); // B: column sums published
            lds_block_sync(); // C: column sums consumed
            STAMP(3)
        }
        STAMP_END(wv)
        return;
    }

    // ================= polynomial wave p ==================================================================
    double *xb = X + (size_t)p * C::PW;
    uint32_t *acc_p = reinterpret_cast<uint32_t *>(xb);
    uint32_t accr[E];
    {
        const int bt = (int)MS[n];
        const uint32_t *tv = tvs + (size_t)job.tv * N;
#pragma unroll
        for (int e = 0; e < E; e++) accr[e] = p == K ? lut_rotated(tv, G::jA(lane, e), bt, N) : 0u;
    }
    auto acc_store = [&]() { acc3_store<N, E, false, true>(acc_p + lane, accr); };
    acc_store();
    lds_wave_sync();
    const unsigned row_off = (unsigned)(p * K1 * L) * poly_bytes;
    int cd[K1]; // wave-uniform column of each distance
#pragma unroll
    for (int d = 0; d < K1; d++) cd[d] = p + d >= K1 ? p + d - K1 : p + d;
    __builtin_amdgcn_s_setprio(3);

    for (int i = 0; i < n; i++) {
        STAMP_BEGIN
        const int a = __builtin_amdgcn_readfirstlane((int)MS[i]);
        const unsigned so_i = (unsigned)i * step_bytes + row_off;
        uint32_t state[E];
        {
            const int rep = logB * L;
            const uint32_t *ar = acc_p + ((lane - a) & (2 * N - 1)); // (X^a acc)[jA(lane, e)] = ar[64 e]
#pragma unroll
            for (int e = 0; e < E; e++) state[e] = ((ar[64 * e] - accr[e]) + (1u << (31 - rep))) >> (32 - rep);
            int *dq = DIG + p * N + lane;
#pragma unroll
            for (int e = 0; e < E; e++) dq[64 * e] = decompose_step(state[e], logB, half_m1, neg_B); // level L-1: the helper's
        }
        STAMP(0)
        lds_block_sync(); // A: digits published (the accumulator copy in this wave's slots has been read)
        STAMP(1)
        __builtin_amdgcn_s_setprio(2);
        double mine[E], keep[E];
#pragma unroll
        for (int lev = L - 2; lev >= 0; lev--) {
            double x[1][E];
#pragma unroll
            for (int e = 0; e < E; e++) x[0][e] = (double)decompose_step(state[e], logB, half_m1, neg_B, lev == 0);
            double2 bwl[K1][E / 2];
#pragma unroll
            for (int d = 0; d < 2; d++)
#pragma unroll
                for (int e2 = 0; e2 < E / 2; e2++) bwl[d][e2] = kb.load(so_i + (unsigned)(cd[d] * L + lev) * poly_bytes, e2 * 1024);
            __builtin_amdgcn_sched_barrier(0);
            ntt_forward_digits<F, LOGN, 1>(x, xb, twf, lane);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int d = 2; d < K1; d++)
#pragma unroll
                for (int e2 = 0; e2 < E / 2; e2++) bwl[d][e2] = kb.load(so_i + (unsigned)(cd[d] * L + lev) * poly_bytes, e2 * 1024);
            __builtin_amdgcn_sched_barrier(0);
            if (lev == 0) __builtin_amdgcn_s_setprio(0);
#pragma unroll
            for (int d = 0; d < K1; d++)
#pragma unroll
                for (int e2 = 0; e2 < E / 2; e2++) {
                    const double2 w = bwl[d][e2];
                    const double t0 = mulmod<F>(x[0][2 * e2], w.x), t1 = mulmod<F>(x[0][2 * e2 + 1], w.y);
                    if (d == 0) {
                        mine[2 * e2] = lev == L - 2 ? t0 : mine[2 * e2] + t0;
                        mine[2 * e2 + 1] = lev == L - 2 ? t1 : mine[2 * e2 + 1] + t1;
                    } else if (d == 1) {
                        keep[2 * e2] = lev == L - 2 ? t0 : keep[2 * e2] + t0;
                        keep[2 * e2 + 1] = lev == L - 2 ? t1 : keep[2 * e2 + 1] + t1;
                    } else {
                        double *dst = xb + C::slot_off(d - 1) + lane;
                        if (lev == L - 2) {
                            dst[(2 * e2) * 64] = t0;
                            dst[(2 * e2 + 1) * 64] = t1;
                        } else {
                            lds_add(dst + (2 * e2) * 64, t0);
                            lds_add(dst + (2 * e2 + 1) * 64, t1);
                        }
                    }
                }
            if (lev == L - 2 && lev != 0) __builtin_amdgcn_s_setprio(1);
        }
        {
            double *dst = xb + C::slot_off(0) + lane;
#pragma unroll
            for (int e = 0; e < E; e++) dst[e * 64] = keep[e];
        }
        STAMP(2)
        lds_block_sync(); // B
        STAMP(3)
        if constexpr (!F::LAZY) {
#pragma unroll
            for (int e = 0; e < E; e++) mine[e] = reduce<F>(mine[e]);
        }
        // the sum for column p computed at distance d sits in wave (p - d) mod K1, slot d - 1; the helper's in its slot p
#pragma unroll
        for (int d = 1; d < K1; d++) {
            const int q = p - d < 0 ? p - d + K1 : p - d;
            const double *src = X + (size_t)q * C::PW + C::slot_off(d - 1);
#pragma unroll
            for (int e = 0; e < E; e++) mine[e] += reduce_unless_lazy<F>(src[e * 64 + lane]);
        }
        {
            const double *src = HX + C::slot_off(p);
#pragma unroll
            for (int e = 0; e < E; e++) mine[e] += reduce_unless_lazy<F>(src[e * 64 + lane]);
        }
#pragma unroll
        for (int e = 0; e < E; e++) mine[e] = reduce<F>(mine[e]);
        lds_block_sync(); // C: every hand-over slot has been read
        STAMP(4)
        __builtin_amdgcn_s_setprio(3);
        ntt_inverse<F, LOGN>(mine, xb, twi, lane);
#pragma unroll
        for (int e = 0; e < E; e++) accr[e] += to_torus32(mine[e]);
        acc_store();
        lds_wave_sync();
        STAMP(5)
    }
    STAMP_END(wv)

    // ---- sample extract (coefficient 0): wave p writes its own polynomial -------------
    sample_extract0<K, N, 1>(out_big, jix, p, lane == 0, accr, lane);
}

// ------------------------------------------------------------------------------------
// k_pbs_tri10 (round 6): THREE bootstraps per workgroup at N = 1024 (k = 1: reference src/bin/helm.rs:141-146's set) - for the
// remainders of a launch that hold between two and three bootstraps per CU, which until now cost a lockstep round with one
// SIMD in four empty (0.93 - 0.97 of a full round).  Two-wave bootstraps cannot fill four SIMDs three at a time, and four
// waves of the duo form (248 registers' worth of 16-value transforms) do not fit three times; so every wave here is
// (polynomial r, TRANSFORM HALF h) with EIGHT values per lane: after its first stage (stride 512) a 1,024-point negacyclic
// transform is two independent 512-point transforms on the position halves, whose butterflies and twiddles are the full
// transform's stages 8 .. 0 restricted to positions with top bit h -
//   twiddle of the butterfly on stride bit sb for half position q:  table[(1024 >> (sb+1)) + (((h << 9) | q) >> (sb+1))]
// - so the bootstrapping key needs no second layout (spectrum position (h << 9) | q).  Wave (r, h), per step:
//   - rotates / subtracts / decomposes polynomial r (all 16 values of a lane: both waves of a polynomial do) level by level,
//     least significant first; per level the split stage and the half's first stage on the digits are the plain radix-4
//     butterfly of the b^4 + 1 fields restricted to its two outputs (fwd_top2_digits: 5 operations per two values), then the
//     512-point transform continues (ntt_forward<F, 9, ..., DIGITS = 3>) and the k + 1 = 2 products with its half of row r
//     follow: column r stays in registers, the other column's sum is handed to wave (1 - r, h) through LDS;
//   - barrier 1; adds the sum it receives, inverse-transforms its half of column r, publishes it;
//   - barrier 2; does its half of the joining stage (h = 0: z0 + z1 -> coefficients j; h = 1: (z0 - z1) psi^-(N/2) ->
//     coefficients j + N/2), lifts, updates its half of the accumulator copy both waves of the polynomial read next;
//   - barrier 3.
// Twelve identical waves, three per SIMD (wave w = 4 b + 2 r + h sits on SIMD w % 4: the four waves of a bootstrap on four
// SIMDs).  LDS: one lane-twiddle table per transform half for the workgroup (the inverse of half h reads the FORWARD table of
// half 1 - h mirrored: psi^-i = -psi^(2N - i) lands in the other half's index range), per wave the transform scratch and a
// hand-over slot, per polynomial ONE copy of the accumulator (N words: the negacyclic sign of a rotated read is arithmetic -
// the [acc | -acc] form of the other builds does not fit three times), 149.6 KB in all.
// Same exact integers as every other build: identical ciphertexts.
// ------------------------------------------------------------------------------------
template <typename F_, int L_, int NB_ = 3>
struct Tri10Cfg {
    using F = F_;
    static constexpr int LOGN = 10, K = 1, K1 = 2, L = L_, NB = NB_, NWB = 4, NW = NWB * NB_; // NB = 2: the same waves, two per SIMD
    using G = Geo<10>;
    using GH = Geo<9>; // the half transforms: 512 points, eight values per lane
    static constexpr int MAX_SMALL_N = 1024;
    static constexpr int TWH_ROWS = GH::TWB + GH::TWC;                               // rows of one half's lane table
    static constexpr size_t TW_SHARED = sizeof(double) * 2 * TWH_ROWS * 64;          // at the workgroup's base: double [2][TWH_ROWS][64]
    static constexpr int HO_OFF = GH::XPAD;                                          // the hand-over slot behind the transform scratch
    static constexpr int WAVE_DOUBLES = GH::XPAD + GH::N;
    // per bootstrap
    static constexpr size_t X_OFF = 0;                                               // double [NWB][WAVE_DOUBLES]
    static constexpr size_t ACC_OFF = X_OFF + sizeof(double) * NWB * WAVE_DOUBLES;   // u32 [K1][N]
    static constexpr size_t MS_OFF = ACC_OFF + sizeof(uint32_t) * K1 * G::N;         // u16 [n+1]
    static constexpr size_t BOOT_BYTES = (MS_OFF + sizeof(uint16_t) * (MAX_SMALL_N + 1) + 15) / 16 * 16;
    static constexpr size_t BYTES = TW_SHARED + BOOT_BYTES * NB;
    static_assert(BYTES <= 160 * 1024, "three bootstraps per workgroup must fit the CU's LDS");
};

// index into the 1,024-point forward table of lane-table row s (0 .. TWB + TWC - 1 of Geo<9>) of transform half hh
__device__ inline int tw_lane_index_half10(int s, int lane, int hh)
{
    using G = Geo<9>;
    int slot = 0;
    for (int sb = G::BC + G::BB - 1; sb >= G::BC; sb--) {
        const int eb = sb - G::BC, cnt = G::E >> (eb + 1);
        if (s < slot + cnt) {
            const int jh = (hh << 9) | G::jB(lane, 0) | ((s - slot) << (eb + 1 + G::BC));
            return (1024 >> (sb + 1)) + (jh >> (sb + 1));
        }
        slot += cnt;
    }
    for (int sb = G::BC - 1; sb >= 0; sb--) {
        const int cnt = G::E >> (sb + 1);
        if (s < slot + cnt) {
            const int jh = (hh << 9) | G::jC(lane, 0) | ((s - slot) << (sb + 1));
            return (1024 >> (sb + 1)) + (jh >> (sb + 1));
        }
        slot += cnt;
    }
    return 0;
}

template <typename C>
__global__ __launch_bounds__(64 * C::NW, 1) void k_pbs_tri10(const PbsJob *__restrict__ jobs, const uint32_t *__restrict__ wires,
                                                             const uint32_t *__restrict__ raw_in, const uint32_t *__restrict__ tvs,
                                                             const double *__restrict__ bsk, const double *__restrict__ tw_fwd,
                                                             const double *__restrict__ tw_inv, uint32_t *__restrict__ out_big, int n,
                                                             int logB, int count)
{
    constexpr int L = C::L, K = 1, K1 = 2, NB = C::NB, NWB = C::NWB, N = 1024, EH = 8;
    using F = typename C::F;
    extern __shared__ __align__(16) unsigned char smem_wg[];

    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = w >> 2, wb = w & 3;  // bootstrap of the workgroup, wave of the bootstrap
    const int r = wb >> 1, h = wb & 1; // polynomial, transform half
    const int jix = (int)blockIdx.x * NB + b;
    if (jix >= count) return; // the hardware barrier counts the surviving waves only
    unsigned char *smem = smem_wg + C::TW_SHARED + (size_t)b * C::BOOT_BYTES;
    double *X = reinterpret_cast<double *>(smem + C::X_OFF);
    double *TWS = reinterpret_cast<double *>(smem_wg);
    uint32_t *ACC = reinterpret_cast<uint32_t *>(smem + C::ACC_OFF);
    uint16_t *MS = reinterpret_cast<uint16_t *>(smem + C::MS_OFF);
    const int tid = wb * 64 + lane;
    const PbsJob job = jobs[jix];
    const size_t row = (size_t)n + 1;
    { // (this kernel keeps its own prologue, initialisation and extract: profiles/README.md r27)
        const uint32_t *a0 = nullptr, *a1 = nullptr, *a2 = nullptr;
        if (job.op < 0) a0 = raw_in + row * (size_t)job.in0;
        else {
            if (job.in0 >= 0) a0 = wires + row * (size_t)job.in0;
            if (job.in1 >= 0) a1 = wires + row * (size_t)job.in1;
            if (job.in2 >= 0) a2 = wires + row * (size_t)job.in2;
        }
        for (int i = tid; i <= n; i += 64 * NWB) {
            uint32_t v;
            if (job.op < 0) v = a0[i];
            else v = gate_lincomb(job.op, job.which, a0 ? a0[i] : 0u, a1 ? a1[i] : 0u, a2 ? a2[i] : 0u, i == n);
            MS[i] = (uint16_t)modswitch(v, 11);
        }
    }
    // one table for the workgroup; each bootstrap's waves fill ALL of it (the same values: another bootstrap's waves may have
    // left already, and nobody reads before the barrier below)
    for (int q = wb; q < 2 * C::TWH_ROWS; q += NWB) {
        const int hh = q / C::TWH_ROWS, s = q - hh * C::TWH_ROWS;
        TWS[q * 64 + lane] = tw_fwd[tw_lane_index_half10(s, lane, hh)];
    }
    TwLane<9, false> twf0;
    TwLane<9, true> twi;
    twf0.base = TWS + h * C::TWH_ROWS * 64 + lane;
    twi.base = TWS + (1 - h) * C::TWH_ROWS * 64 + (63 - lane);
    {
        // block A's lane-uniform twiddles (stride bits 8, 7, 6 of the half): forward those of half h, inverse those of half
        // 1 - h (read mirrored by TwLane<., true>)
        int slot = 0;
#pragma unroll
        for (int sb = 8; sb >= 6; sb--) {
#pragma unroll
            for (int hi = 0; hi < (EH >> (sb - 6 + 1)); hi++) {
                twf0.ua[slot] = tw_fwd[(1024 >> (sb + 1)) + h * (512 >> (sb + 1)) + hi];
                twi.ua[slot] = tw_fwd[(1024 >> (sb + 1)) + (1 - h) * (512 >> (sb + 1)) + hi];
                slot++;
            }
        }
    }
    const double w9i = tw_inv[1]; // the joining stage (stride bit 9): psi^-(N/2)
    // the split stage and the half's first stage on digits: x(q) = (d0 +- b^2 d4) + (c1 d2 + c2 d6), x(q + 256) = ... - ...
    const double cA = h ? -F::B2 : F::B2, c1 = h ? F::B3 : F::B1, c2 = h ? F::B1 : F::B3;
    __syncthreads();
    TwLaneReg<9, false> twf;
    twf.load(twf0);

    // accumulator (0, X^{-b~} tv): wave (r, h) owns the coefficients j = 512 h + 64 e + lane of polynomial r
    uint32_t *acc_r = ACC + (size_t)r * N;
    uint32_t accr[EH];
    auto acc_store = [&]() {
        uint32_t *aw = acc_r + 512 * h + lane;
#pragma unroll
        for (int e = 0; e < EH; e++) aw[64 * e] = accr[e];
    };
    {
        const int bt = (int)MS[n];
        const uint32_t *tv = tvs + (size_t)job.tv * N;
#pragma unroll
        for (int e = 0; e < EH; e++) {
            uint32_t v = 0;
            if (r == K) {
                const int idx = (512 * h + 64 * e + lane + bt) & (2 * N - 1);
                v = tv[idx & (N - 1)];
                if (idx >= N) v = 0u - v;
            }
            accr[e] = v;
        }
        acc_store();
    }
    __syncthreads();

    double *xb = X + (size_t)wb * C::WAVE_DOUBLES;
    const unsigned poly_bytes = (unsigned)(N / 2) * 16u;
    const unsigned step_bytes = (unsigned)(K1 * K1 * L) * poly_bytes;
    const unsigned row_off = (unsigned)(r * K1 * L) * poly_bytes; // + (c * L + lev) * poly_bytes
    KeyBuf kb;
    kb.init(bsk, (size_t)n * step_bytes, lane);
    // this wave's eight spectrum positions (h << 9) | (lane << 3 | e) sit in the full-transform layout [e_f / 2][lane_f][2] at
    // lane_f = 32 h + (lane >> 1), e_f = 8 (lane & 1) + e: double2 number 4 (lane & 1) + e / 2 of that lane
    kb.lane16 = (lane & 1) * 4096 + (h * 32 + (lane >> 1)) * 16;
    const uint32_t half_m1 = (1u << (logB - 1)) - 1u;
    const int neg_B = -(1 << logB);
    const int rep = logB * L;
    const uint32_t rnd = 1u << (31 - rep);

    // issue priorities stepping down through the step (off: 6.61 against 6.18 ms per 768, profiles/r06/ab_tri10.jsonl)
    __builtin_amdgcn_s_setprio(3);
    STAMP_DECL
    for (int i = 0; i < n; i++) {
        STAMP_BEGIN
        // a zero rotation is not skipped: the bootstraps of a workgroup meet at the same barriers (its product is exactly zero)
        const int a = __builtin_amdgcn_readfirstlane((int)MS[i]);
        const unsigned so_i = (unsigned)i * step_bytes + row_off;
        // ---- rotation and difference: st[e] = round((X^a acc - acc)[64 e + lane]) >> (32 - rep) -------------------------------
        uint32_t st[16];
        {
            // rotated index (64 e + lane - a) mod 2N: bits 0-9 address the one copy, bit 10 is the negacyclic sign
            const int base = (lane - a) & (2 * N - 1);
            const uint32_t *own = acc_r + lane;
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int t = base + 64 * e;
                const uint32_t raw = acc_r[t & (N - 1)];
                const uint32_t m = 0u - ((uint32_t)(t >> 10) & 1u);
                // (all sixteen unrotated values from the copy too: picking the own half out of registers by h costs a select each)
                st[e] = (((raw ^ m) - m) - own[64 * e] + rnd) >> (32 - rep);
            }
        }
        double mine[EH], keep[EH];
#pragma unroll
        for (int lev = L - 1; lev >= 0; lev--) {
            // this level's key words of both columns (0: column r, this wave's own; 1: the other one): issued before the
            // transform that hides their latency
            double2 kw[K1][EH / 2];
#pragma unroll
            for (int c = 0; c < K1; c++)
#pragma unroll
                for (int e2 = 0; e2 < EH / 2; e2++)
                    kw[c][e2] = kb.load(so_i + (unsigned)((c ? 1 - r : r) * L + lev) * poly_bytes, e2 * 1024);
            double x[1][EH];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const double d0 = (double)decompose_step(st[e], logB, half_m1, neg_B, lev == 0);
                const double d2 = (double)decompose_step(st[e + 4], logB, half_m1, neg_B, lev == 0);
                const double d4 = (double)decompose_step(st[e + 8], logB, half_m1, neg_B, lev == 0);
                const double d6 = (double)decompose_step(st[e + 12], logB, half_m1, neg_B, lev == 0);
                const double s0 = __builtin_fma(d4, cA, d0);
                const double u = __builtin_fma(d6, c2, d2 * c1);
                x[0][e] = s0 + u;
                x[0][e + 4] = s0 - u;
                HELM_BOUND(__builtin_fabs(x[0][e]) < F::P * 0.5 && __builtin_fabs(x[0][e + 4]) < F::P * 0.5, 2);
            }
            __builtin_amdgcn_sched_barrier(0);
            ntt_forward<F, 9, 1, decltype(twf), 0, NoHook, 3>(x, xb, twf, lane);
            __builtin_amdgcn_sched_barrier(0);
            if (lev == 0) __builtin_amdgcn_s_setprio(0);
#pragma unroll
            for (int e2 = 0; e2 < EH / 2; e2++) {
                const double2 wr = kw[0][e2], wo = kw[1][e2];
                const double t0 = mulmod<F>(x[0][2 * e2], wr.x), t1 = mulmod<F>(x[0][2 * e2 + 1], wr.y);
                const double u0 = mulmod<F>(x[0][2 * e2], wo.x), u1 = mulmod<F>(x[0][2 * e2 + 1], wo.y);
                mine[2 * e2] = lev == L - 1 ? t0 : mine[2 * e2] + t0;
                mine[2 * e2 + 1] = lev == L - 1 ? t1 : mine[2 * e2 + 1] + t1;
                keep[2 * e2] = lev == L - 1 ? u0 : keep[2 * e2] + u0;
                keep[2 * e2 + 1] = lev == L - 1 ? u1 : keep[2 * e2 + 1] + u1;
            }
            if (lev == L - 1) __builtin_amdgcn_s_setprio(2);
            else if (lev == 1) __builtin_amdgcn_s_setprio(1);
        }
        {
            double *dst = xb + C::HO_OFF + lane;
#pragma unroll
            for (int e = 0; e < EH; e++) dst[64 * e] = keep[e];
        }
        STAMP(0) // rotation, digits, forward half transforms, products, hand-over written
        lds_block_sync();
        STAMP(1) // barrier 1
        __builtin_amdgcn_s_setprio(3);
        {
            const double *src = X + (size_t)(2 * (1 - r) + h) * C::WAVE_DOUBLES + C::HO_OFF + lane;
            if constexpr (!F::LAZY) {
#pragma unroll
                for (int e = 0; e < EH; e++) mine[e] = reduce<F>(mine[e]);
            }
#pragma unroll
            for (int e = 0; e < EH; e++) mine[e] = reduce<F>(mine[e] + reduce_unless_lazy<F>(src[64 * e]));
        }
        ntt_inverse<F, 9>(mine, xb, twi, lane);
        {
            double *zx = xb + lane;
#pragma unroll
            for (int e = 0; e < EH; e++) zx[64 * e] = mine[e];
        }
        STAMP(2) // hand-over summed, inverse half transform, published
        lds_block_sync();
        STAMP(3) // barrier 2
        {
            const double *zp = X + (size_t)(2 * r + (1 - h)) * C::WAVE_DOUBLES + lane;
#pragma unroll
            for (int e = 0; e < EH; e++) {
                const double o = zp[64 * e];
                // h = 0: z0 + z1 -> coefficient j;  h = 1: (z0 - z1) psi^-(N/2) -> coefficient j + N / 2 (own = z1, other = z0)
                const double v = h ? mulmod<F>(o - mine[e], w9i) : mine[e] + o;
                accr[e] += to_torus32(reduce<F>(v));
            }
        }
        acc_store();
        STAMP(4) // joining stage, lift, accumulator update
        lds_block_sync();
        STAMP(5) // barrier 3
    }
    STAMP_END(w)

    // ---- sample extract (coefficient 0): every wave writes its half of its polynomial -------------------------------
    uint32_t *ob = out_big + (size_t)jix * ((size_t)K * N + 1);
    if (r < K) {
#pragma unroll
        for (int e = 0; e < EH; e++) {
            const int j = 512 * h + 64 * e + lane;
            if (j == 0) ob[r * N] = accr[e];
            else ob[r * N + (N - j)] = 0u - accr[e];
        }
    } else if (h == 0 && lane == 0) {
        ob[K * N] = accr[0];
    }
}

#if HELM_HIP_TU == 0 // the keyswitch, linear and table kernels: main translation unit only (see launch_pbs_wide)
// ------------------------------------------------------------------------------------
// The keyswitch kernels: wrappers over the bodies of keyswitch.h, one set per row policy.
//   k_keyswitch / k_keyswitch_gate      vector-ALU form, ks_l in 1..6, 8
//   k_ks_digits / k_ks_gate_digits      matrix-core form (ks_l in {1, 2, 4, 8}): digits in A-fragment order ...
//   k_ks_mfma                           ... times the key's four byte planes, two column tiles per wave
//                                       (int32 accumulators: |sum| <= 4096 * 64 * 128 < 2^25)
// ------------------------------------------------------------------------------------
// KsJob rows: one row of the big-LWE buffer or the sum of two (MUX recombination: two bootstrap outputs + 1/8 on the body)
struct KsRows {
    using Job = KsJob;
    using Word = uint32_t;
    const KsJob &job;
    const uint32_t *big;
    size_t row;
    __device__ __forceinline__ KsRows(const KsJob &job, const uint32_t *big, size_t row) : job(job), big(big), row(row) {}
    __device__ __forceinline__ uint32_t word(int t) const
    {
        uint32_t v = big[row * (size_t)job.big0 + t];
        if (job.big1 >= 0) v += big[row * (size_t)job.big1 + t];
        return v;
    }
    __device__ __forceinline__ uint32_t body(int kN) const { return word(kN) + job.add_body; }
    static __device__ __forceinline__ int out_row(const KsJob &job, int) { return job.out; }
};

template <int KSL>
__global__ __launch_bounds__(256) void k_keyswitch(const KsJob *__restrict__ jobs, const uint32_t *__restrict__ big,
                                                   const uint32_t *__restrict__ ksk, uint32_t *__restrict__ out,
                                                   int n, int kN, int logB, int count, int t_chunk)
{
    helm_ks::vector_body<KSL, KsRows>(jobs, big, ksk, out, n, kN, logB, count, t_chunk);
}

template <int KSL>
__global__ __launch_bounds__(256) void k_ks_digits(const KsJob *__restrict__ jobs, const uint32_t *__restrict__ big,
                                                   int8_t *__restrict__ dig, int32_t *__restrict__ dsum,
                                                   uint32_t *__restrict__ body, int kN, int logB, int count, int kchunks)
{
    helm_ks::digits_body<KSL, KSL, KsRows>(jobs, big, dig, dsum, body, kN, logB, count, kchunks);
}

__global__ __launch_bounds__(64) void k_ks_mfma(const KsJob *__restrict__ jobs, const int8_t *__restrict__ dig,
                                                const int32_t *__restrict__ dsum, const uint32_t *__restrict__ body,
                                                const int8_t *__restrict__ kplanes, uint32_t *__restrict__ out, int n,
                                                int count, int kchunks, int ctiles)
{
    helm_ks::product_body<2, KsRows>(jobs, dig, dsum, body, kplanes, out, n, count, kchunks, ctiles);
}

// rows named by the keyswitch jobs <- 0 (before a row-split keyswitch accumulates into them)
__global__ __launch_bounds__(256) void k_ks_zero(const KsJob *__restrict__ jobs, uint32_t *__restrict__ out, int n)
{
    uint32_t *dst = out + ((size_t)n + 1) * (size_t)jobs[blockIdx.x].out;
    for (int i = threadIdx.x; i <= n; i += 256) dst[i] = 0u;
}

// ------------------------------------------------------------------------------------
// Keyswitch-first levels (pbs_order = 1: wires are big LWE rows of k*N + 1 words under the GLWE key).  A gate is linear
// combination -> keyswitch -> bootstrap, so the keyswitch is the front of the level: k_keyswitch_gate and k_ks_gate_digits
// are the keyswitch bodies fed by the level's PbsJob list - they form gate_lincomb() of up to three wire rows as they read
// them (the +-1/8 on the body word, index k*N); k_ks_mfma runs behind k_ks_gate_digits with the identity job list.  The small
// row of job i is row i of the context's staging buffer (`out`); the blind-rotate kernels then take those rows as raw LWEs.
// ------------------------------------------------------------------------------------
// PbsJob rows: the gate's linear combination of its wire rows (GateRows, pbs_frame.h); job g writes row g
struct GateKsRows {
    using Job = PbsJob;
    using Word = uint32_t;
    const GateRows rows;
    __device__ __forceinline__ GateKsRows(const PbsJob &job, const uint32_t *wires, size_t row) : rows(job, wires, row) {}
    __device__ __forceinline__ uint32_t word(int t) const { return rows.word(t, false); }
    __device__ __forceinline__ uint32_t body(int kN) const { return rows.word(kN, true); }
    static __device__ __forceinline__ int out_row(const PbsJob &, int g) { return g; }
};

template <int KSL>
__global__ __launch_bounds__(256) void k_keyswitch_gate(const PbsJob *__restrict__ jobs, const uint32_t *__restrict__ wires,
                                                        const uint32_t *__restrict__ ksk, uint32_t *__restrict__ out,
                                                        int n, int kN, int logB, int count, int t_chunk)
{
    helm_ks::vector_body<KSL, GateKsRows>(jobs, wires, ksk, out, n, kN, logB, count, t_chunk);
}

template <int KSL>
__global__ __launch_bounds__(256) void k_ks_gate_digits(const PbsJob *__restrict__ jobs, const uint32_t *__restrict__ wires,
                                                        int8_t *__restrict__ dig, int32_t *__restrict__ dsum,
                                                        uint32_t *__restrict__ body, int kN, int logB, int count, int kchunks)
{
    helm_ks::digits_body<KSL, KSL, GateKsRows>(jobs, wires, dig, dsum, body, kN, logB, count, kchunks);
}

// raw[i] = {op -1, in0 = i, tv 0} (the bootstrap of staging row i), ident[i] = {out = i} (k_ks_mfma's and k_ks_zero's
// destination of job i): the two job lists of a keyswitch-first level that do not depend on the level
__global__ __launch_bounds__(256) void k_iota_jobs(PbsJob *__restrict__ raw, KsJob *__restrict__ ident, int count)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    raw[i] = PbsJob{-1, 0, i, -1, -1, 0};
    ident[i] = KsJob{i, -1, i, 0u};
}

// k_big_out: dst[out] = big[big0] (+ big[big1]) over k*N + 1 words, add_body on the body word - the scatter of the extracted
// rows into the wire table (or a shard's staging chunk) and the MUX recombination of a keyswitch-first level.
__global__ __launch_bounds__(256) void k_big_out(const KsJob *__restrict__ jobs, const uint32_t *__restrict__ big,
                                                 uint32_t *__restrict__ dst, int kN)
{
    const KsJob job = jobs[blockIdx.x];
    const size_t row = (size_t)kN + 1;
    const uint32_t *b0 = big + row * (size_t)job.big0, *b1 = job.big1 >= 0 ? big + row * (size_t)job.big1 : nullptr;
    uint32_t *d = dst + row * (size_t)job.out;
    for (int i = threadIdx.x; i <= kN; i += 256) {
        uint32_t v = b0[i];
        if (b1) v += b1[i];
        if (i == kN) v += job.add_body;
        d[i] = v;
    }
}

// ------------------------------------------------------------------------------------
// k_linear: NOT / BUF / DFF / constants.  One workgroup per gate.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_linear(const LinJob *__restrict__ jobs, const uint32_t *__restrict__ wires,
                                                uint32_t *__restrict__ out, int n)
{
    const LinJob job = jobs[blockIdx.x];
    const size_t row = (size_t)n + 1;
    const uint32_t *src = job.in0 >= 0 ? wires + row * (size_t)job.in0 : nullptr;
    uint32_t *dst = out + row * (size_t)job.out;
    for (int i = threadIdx.x; i <= n; i += 256) {
        uint32_t v;
        switch (job.op) {
        case HELM_GATE_NOT: v = 0u - src[i]; break;
        case HELM_GATE_BUF:
        case HELM_GATE_DFF: v = src[i]; break;
        case HELM_GATE_CONST_ONE: v = (i == n) ? PT_TRUE : 0u; break;
        case HELM_GATE_CONST_ZERO: v = (i == n) ? PT_FALSE : 0u; break;
        default: v = 0u; break;
        }
        dst[i] = v;
    }
}

// rows gathered[r] -> wires[dst_row[r]] (dst_row < 0: padding, skipped)
__global__ __launch_bounds__(256) void k_scatter_rows(const uint32_t *__restrict__ gathered,
                                                      const int32_t *__restrict__ dst_row,
                                                      uint32_t *__restrict__ wires, int n)
{
    const int d = dst_row[blockIdx.x];
    if (d < 0) return;
    const size_t row = (size_t)n + 1;
    for (int i = threadIdx.x; i <= n; i += 256) wires[row * (size_t)d + i] = gathered[row * (size_t)blockIdx.x + i];
}

__global__ __launch_bounds__(256) void k_gather_rows(const uint32_t *__restrict__ wires,
                                                     const int32_t *__restrict__ src_row,
                                                     uint32_t *__restrict__ packed, int n)
{
    const int s = src_row[blockIdx.x];
    const size_t row = (size_t)n + 1;
    for (int i = threadIdx.x; i <= n; i += 256)
        packed[row * (size_t)blockIdx.x + i] = s < 0 ? 0u : wires[row * (size_t)s + i];
}

// wire dst_row[r] of `dst` <- wire src_row[r] of `src` (Ciphertext::clone of whole rows)
__global__ __launch_bounds__(256) void k_copy_rows(const uint32_t *__restrict__ src, const int32_t *__restrict__ src_row,
                                                   uint32_t *__restrict__ dst, const int32_t *__restrict__ dst_row, int n)
{
    const size_t row = (size_t)n + 1;
    const uint32_t *s = src + row * (size_t)src_row[blockIdx.x];
    uint32_t *d = dst + row * (size_t)dst_row[blockIdx.x];
    for (int i = threadIdx.x; i <= n; i += 256) d[i] = s[i];
}

__global__ __launch_bounds__(256) void k_set_trivial(const int32_t *__restrict__ idx, const uint8_t *__restrict__ val,
                                                     uint32_t *__restrict__ wires, int n)
{
    const size_t row = (size_t)n + 1;
    uint32_t *dst = wires + row * (size_t)idx[blockIdx.x];
    const uint32_t body = val[blockIdx.x] ? PT_TRUE : PT_FALSE;
    for (int i = threadIdx.x; i <= n; i += 256) dst[i] = (i == n) ? body : 0u;
}

// ------------------------------------------------------------------------------------
// k_bsk_convert: one wave per BSK polynomial.  Standard-domain u32 coefficients (taken
// as signed) -> forward NTT -> * N^{-1} -> centred doubles in the lane-order k_pbs reads:
//   dst[i][r][c][lev][e/2][lane][e&1]      (src is [i][lev][r][c][N])
// ------------------------------------------------------------------------------------
template <typename F, int LOGN>
__global__ __launch_bounds__(64) void k_bsk_convert(const uint32_t *__restrict__ src, double *__restrict__ dst,
                                                    const double *__restrict__ tw_fwd, double n_inv, int K1, int L)
{
    using G = Geo<LOGN>;
    constexpr int N = G::N, E = G::E;
    __shared__ double xbuf[G::XPAD];
    const int lane = threadIdx.x;
    const size_t poly = blockIdx.x; // index in src order
    const int c = poly % K1;
    const int r = (poly / K1) % K1;
    const int lev = (poly / ((size_t)K1 * K1)) % L;
    const size_t i = poly / ((size_t)K1 * K1 * L);
    double x[1][E];
#pragma unroll
    for (int e = 0; e < E; e++) x[0][e] = (double)(int32_t)src[poly * N + G::jA(lane, e)];
    // |x| <= 2^31: far below p/2, so the digit-sized input bound of ntt_forward holds
    ntt_forward<F, LOGN, 1>(x, xbuf, TwMem{tw_fwd}, lane);
    const size_t dpoly = ((i * K1 + r) * K1 + c) * L + lev;
    double *d = dst + dpoly * N;
#pragma unroll
    for (int e = 0; e < E; e++) d[((e >> 1) * 64 + lane) * 2 + (e & 1)] = reduce<F>(mulmod<F>(x[0][e], n_inv));
}

// NTT self-test: forward, scale, inverse; must reproduce the input exactly.
template <typename F, int LOGN>
__global__ __launch_bounds__(64) void k_ntt_roundtrip(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst,
                                                      const double *__restrict__ tw_fwd,
                                                      const double *__restrict__ tw_inv, double n_inv)
{
    using G = Geo<LOGN>;
    constexpr int N = G::N, E = G::E;
    __shared__ double xbuf[G::XPAD];
    const int lane = threadIdx.x;
    double x[1][E];
#pragma unroll
    for (int e = 0; e < E; e++) x[0][e] = (double)(int32_t)src[(size_t)blockIdx.x * N + G::jA(lane, e)];
    ntt_forward<F, LOGN, 1>(x, xbuf, TwMem{tw_fwd}, lane);
#pragma unroll
    for (int e = 0; e < E; e++) x[0][e] = reduce<F>(mulmod<F>(x[0][e], n_inv));
    ntt_inverse<F, LOGN>(x[0], xbuf, TwMem{tw_inv}, lane);
#pragma unroll
    for (int e = 0; e < E; e++) dst[(size_t)blockIdx.x * N + G::jA(lane, e)] = to_torus32(x[0][e]);
}

// k_pbs_generic: k and pbs_l at run time, every admitted shape the tuned builds do not cover (and HELM_HIP_PBS_VARIANT=10)
#include "helm_pbs_generic.inc"
// k_pbs_crt: the same in the CRT pair FpG x FpG2, for shapes beyond the single-prime capacity bound (helm_hip_ctx_create_ex);
// pbs_twoprime.h: what it shares with the 64-bit engine's k_pbs64_generic
#include "pbs_twoprime.h"
#include "helm_pbs_crt.inc"

#endif // HELM_HIP_TU == 0

// ------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------
namespace {

template <typename T> struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    int ensure(size_t n)
    {
        if (n <= cap) return 0;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = std::max(n, (size_t)64);
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

// device temporary of one call: freed on every return path
template <typename T> struct Scratch {
    T *p = nullptr;
    Scratch() = default;
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch()
    {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t n) { return hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)); }
};

struct LevelPlan {
    std::vector<PbsJob> pbs;
    std::vector<KsJob> ks;
    std::vector<LinJob> lin;
};

} // namespace

// The tuned builds (kernel class 0), listed once for both translation units: the shapes, and per shape the lazy field that
// may serve it besides the 51-bit FpH (49: FpG at N = 512, chosen from the parameter set; 50: FpI at N = 1024, chosen per
// loaded key) - ten (field, LOGN, K, L) forms, the only ones a tuned kernel is instantiated for.
struct TunedShape {
    int N, k, pbs_l, lazy;
    bool trio; // a build with three bootstraps per workgroup exists: k_pbs_trio | k_pbs_tri10
};
constexpr TunedShape TUNED[] = {{512, 2, 3, 49, true},   {512, 1, 3, 49, false},  {512, 1, 2, 49, false},
                                {1024, 1, 3, 50, true},  {1024, 1, 2, 50, true}};
constexpr int N_TUNED = (int)(sizeof(TUNED) / sizeof(TUNED[0]));
// index of a shape in TUNED, or -1: the shape has no tuned build
static inline int tuned_shape(const helm_hip_params &P)
{
    for (int i = 0; i < N_TUNED; i++)
        if (P.N == TUNED[i].N && P.k == TUNED[i].k && P.pbs_l == TUNED[i].pbs_l) return i;
    return -1;
}
// field id of the engine context -> field type of the boolean kernels
template <int ID> struct BoolField;
template <> struct BoolField<49> { using type = FpG; };
template <> struct BoolField<50> { using type = FpI; };
template <> struct BoolField<51> { using type = FpH; };
template <typename F_, int LOGN_, int K_, int L_> struct TunedForm {
    using F = F_;
    static constexpr int LOGN = LOGN_, K = K_, L = L_;
};
// f(TunedForm<F, LOGN, K, L>) for row `shape` of TUNED in `field` (the row's lazy field, or 51), `outside` for anything else:
// a call site instantiates what it names for the ten forms and no other.
template <int I = 0, class R, class Fn>
R with_tuned(int shape, int field, R outside, Fn &&f)
{
    if constexpr (I < N_TUNED) {
        constexpr TunedShape S = TUNED[I];
        constexpr int LOGN = S.N == 512 ? 9 : 10;
        static_assert(S.N == 1 << LOGN, "tuned builds exist at N = 512 and N = 1024");
        if (shape == I) {
            if (field == S.lazy) return f(TunedForm<typename BoolField<S.lazy>::type, LOGN, S.k, S.pbs_l>{});
            if (field == 51) return f(TunedForm<FpH, LOGN, S.k, S.pbs_l>{});
            return outside;
        }
        return with_tuned<I + 1>(shape, field, outside, f);
    } else return outside;
}

// Which bootstrap kernel a context runs and how: decided once, by bool_admit() from (params, flags, environment), and only
// read afterwards.  The class's setup step fills (d, lds, per_cu) once the device is chosen; helm_hip_load_bootstrap_key
// moves `field` between 50 and 51 for a tuned N = 1024 context; nothing else writes the record.
enum BoolClass { BOOL_TUNED = 0, BOOL_GENERIC = 1, BOOL_CRT = 2 }; // the values helm_hip_kernel_class returns
enum BoolBuild { // the builds of the tuned class, by their HELM_HIP_PBS_VARIANT numbers
    BUILD_WIDE = 4,     // k_pbs_wide
    BUILD_LOCKSTEP = 5, // k_pbs
    BUILD_DUO = 6,      // k_pbs_duo, the two bootstraps of a workgroup in step
    BUILD_DUO_STAG = 7, // k_pbs_duo staggered by half a step
    BUILD_TRI10_2 = 8,  // (N = 1024) k_pbs_tri10's waves, two bootstraps per workgroup
    BUILD_TRIO = 9      // k_pbs_trio (N = 512, k = 2) | k_pbs_tri10 (N = 1024)
};
struct BoolForm {
    BoolClass cls = BOOL_TUNED; // of the shape: 1 no tuned build covers it, 2 beyond the single-prime capacity bound
    BoolClass run = BOOL_TUNED; // what runs every launch: cls, or k_pbs_generic under HELM_HIP_PBS_VARIANT=10 (FpH, its own
                                // key layout), or k_pbs_crt under HELM_HIP_CREATE_FORCE_CRT (FpG x FpG2, its own key layout)
    int shape = -1;             // row of TUNED, when the shape has a tuned build
    int field = 51;             // 51: FpH, 49: FpG, 50: FpI (both lazy) - all with short eighth roots of unity -, 98: the CRT pair
    int variant = 0;            // HELM_HIP_PBS_VARIANT: 0 = by launch size, or one BoolBuild for every launch (10: see `run`)
    // the builds launch_pbs_f's size dispatch gives a remainder of <= 1, <= 2 and <= 3 bootstraps per CU (BUILD_LOCKSTEP: no
    // build of that size, or switched off):
    //   [1] N = 512 (HELM_HIP_DUO): 2 k_pbs_duo staggered, 1 in step, 0 none.  N = 1024 (HELM_HIP_DUO1024): 3 k_pbs_tri10's waves,
    //       two bootstraps per workgroup (round 6: 512 bootstraps of helm_cuda 5.11 -> 4.41 ms, profiles/r06/ab_tri10.jsonl);
    //       1 / 2 k_pbs_duo's compact layout in step / staggered (round 5: 5.50 - 5.55 / 5.75 ms in the 51-bit field, the
    //       two-wave build of rounds 1-4 6.04); 0 none
    //   [2] k_pbs_trio / k_pbs_tri10 where the shape has one (HELM_HIP_TRIO=0: a partial lockstep round, round 3's choice)
    int rem[3] = {BUILD_WIDE, BUILD_LOCKSTEP, BUILD_LOCKSTEP};
    // classes 1 and 2 (setup_generic, setup_crt): the launch sizing of the class's kernel
    int d = 1;      // digit polynomials per batch (gen_batch | tp_batch, tp_fit)
    size_t lds = 0; // LDS bytes per workgroup (GenLds | TwoPrimeLds<uint32_t>)
    int per_cu = 1; // resident workgroups per CU at lds
};

struct helm_hip_wires {
    helm_hip_ctx *owner;
    uint32_t *d;
    int64_t n_wires;
};

struct helm_hip_ctx {
    int device = 0;
    helm_hip_params P{};
    int logN = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipStream_t xchg_stream = nullptr; // overlapped exchange: all-gather + scatter of a launch run here (created at first use)
    double *tw_fwd = nullptr, *tw_inv = nullptr;
    double n_inv = 0;
    double *bsk = nullptr;
    uint32_t *ksk = nullptr;
    int8_t *ksk_planes = nullptr; // matrix-core keyswitch: the key's four byte planes as signed bytes, B-fragment order
    int ks_kchunks = 0, ks_ctiles = 0;
    int ks_mfma = 1;             // HELM_HIP_KS_MFMA=0: the vector-ALU keyswitch for every launch
    DevBuf<int8_t> d_ksdig;
    DevBuf<int32_t> d_ksdsum;
    DevBuf<uint32_t> d_ksbody;
    uint32_t *tv_bool = nullptr; // one row: all +1/8
    bool have_bsk = false, have_ksk = false;
    BoolForm form;           // which kernel runs the launches, and how: bool_admit's answer
    int n_cus = 256;
    int clock_probe = 0;     // HELM_HIP_CLOCK_PROBE: print the in-kernel clock of every k_pbs launch
    double *crt_tw[4] = {nullptr, nullptr, nullptr, nullptr}; // k_pbs_crt: forward tables of FpG, FpG2, then the inverse ones
    double crt_n_inv[2] = {0, 0}, crt_p0inv = 0;              // 1/N in each field, p0^-1 mod p1
    // per-call scratch
    DevBuf<PbsJob> d_pbs;
    DevBuf<KsJob> d_ks;
    DevBuf<LinJob> d_lin;
    DevBuf<uint32_t> d_big;
    // keyswitch-first levels (pbs_order = 1): the small rows between the gate keyswitch and the bootstrap, and the two job
    // lists that do not depend on the level (k_iota_jobs), filled up to iota_filled
    DevBuf<uint32_t> d_small;
    DevBuf<PbsJob> d_raw;
    DevBuf<KsJob> d_ident;
    size_t iota_filled = 0;
    // timing
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pbs, ev_pbs_main, ev_ks, ev_lin, ev_xchg;
    helm_hip_timing tacc{};
    // wire tables and programs created from this context: released with it, so that a handle
    // freed after its context (host-language destructors run in any order) is harmless
    std::vector<helm_hip_wires *> child_wires;
    std::vector<helm_hip_program *> child_progs;
};

struct helm_hip_program {
    helm_hip_ctx *owner;
    int64_t n_levels;
    std::vector<int64_t> off;
    std::vector<int32_t> op, in0, in1, in2, out;
    int64_t max_row = -1; // largest wire index any gate reads or writes
    // device copies of the full job lists, with per-level offsets
    PbsJob *d_pbs = nullptr;
    KsJob *d_ks = nullptr;
    LinJob *d_lin = nullptr;
    std::vector<int64_t> pbs_off, ks_off, lin_off;
    std::vector<LevelPlan> plans; // host copies (used for sharding)
    // shard tables of (sh_rank, sh_world), built once (shard_prepare): per level the job lists of this rank's
    // chunk (destination rows = rows of the staging chunk) and the scatter rows of the gathered level
    int sh_rank = -1, sh_world = 0;
    DevBuf<PbsJob> s_pbs;
    DevBuf<KsJob> s_ks;
    DevBuf<LinJob> s_lin;
    DevBuf<int32_t> s_rows;
    std::vector<int64_t> sh_pbs_off, sh_ks_off, sh_lin_off, sh_rows_off;
    DevBuf<uint32_t> x_gather; // helm_hip_program_run_sharded_comm: the launches' gather buffer (chunk rows x world)
    // chunk boundaries of (sh_world): level l's rank r owns gates [sh_bounds[l (world+1) + r], sh_bounds[l (world+1) + r + 1]),
    // cut by bootstrap weight (shard_rule.h); sh_rows[l] = the largest chunk = rows of one rank's slot in the all-gather
    std::vector<int64_t> sh_bounds, sh_rows;
    // overlapped exchange (run_sharded_comm, overlap = 1): for every launch the last EARLIER launch that writes one of
    // its input rows (-1: none), whether every row is written at most once per pass (otherwise the overlapped schedule
    // does not apply), a ring of gather buffers and one event per sharded launch recorded behind its scatter
    std::vector<int64_t> dep;
    int dep_state = 0; // 0 not computed, 1 usable, -1 a row is written twice per pass
    DevBuf<uint32_t> x_ring[3];
    std::vector<hipEvent_t> x_done, x_comp; // per sharded launch: recorded behind its scatter / behind its chunk's kernels
};

static void release_overlap(helm_hip_program *pr)
{
    for (auto &b : pr->x_ring) b.release();
    for (auto *v : {&pr->x_done, &pr->x_comp}) {
        for (hipEvent_t e : *v) (void)hipEventDestroy(e);
        v->clear();
    }
}

// Words of the mask of a wire row: n in order 0 (wires under the small key), k N in order 1 (under the GLWE key)
static int wire_dim(const helm_hip_ctx *ctx) { return ctx->P.pbs_order == 1 ? ctx->P.k * ctx->P.N : ctx->P.n; }

static bool needs_pbs(int op)
{
    switch (op) {
    case HELM_GATE_AND: case HELM_GATE_NAND: case HELM_GATE_OR: case HELM_GATE_NOR:
    case HELM_GATE_XOR: case HELM_GATE_XNOR: case HELM_GATE_MUX:
    case HELM_GATE_MAJ3: case HELM_GATE_XOR3: case HELM_GATE_XNOR3: return true;
    default: return false;
    }
}
// gates whose third operand is required (the others read in0 and in1 alone)
static bool needs_in2(int op)
{
    return op == HELM_GATE_MUX || op == HELM_GATE_MAJ3 || op == HELM_GATE_XOR3 || op == HELM_GATE_XNOR3;
}
static bool is_linear(int op)
{
    switch (op) {
    case HELM_GATE_NOT: case HELM_GATE_BUF: case HELM_GATE_DFF:
    case HELM_GATE_CONST_ONE: case HELM_GATE_CONST_ZERO: return true;
    default: return false;
    }
}

// Build the job lists of one level.  `out_row(g)` maps gate g to its destination row.
template <typename F>
static int plan_level(const int32_t *op, const int32_t *in0, const int32_t *in1, const int32_t *in2, int64_t count,
                      F out_row, LevelPlan &pl)
{
    pl.pbs.clear();
    pl.ks.clear();
    pl.lin.clear();
    for (int64_t g = 0; g < count; g++) {
        const int o = op[g];
        if (needs_pbs(o)) {
            if (in0[g] < 0 || in1[g] < 0 || (needs_in2(o) && in2[g] < 0))
                return fail(HELM_ERR_INVALID, "gate " + std::to_string(g) + ": missing operand");
            KsJob k;
            k.big0 = (int32_t)pl.pbs.size();
            k.big1 = -1;
            k.out = out_row(g);
            k.add_body = 0;
            pl.pbs.push_back(PbsJob{o, 0, in0[g], in1[g], in2[g], 0});
            if (o == HELM_GATE_MUX) {
                k.big1 = (int32_t)pl.pbs.size();
                k.add_body = PT_TRUE;
                pl.pbs.push_back(PbsJob{o, 1, in0[g], in1[g], in2[g], 0});
            }
            pl.ks.push_back(k);
        } else if (is_linear(o)) {
            if ((o == HELM_GATE_NOT || o == HELM_GATE_BUF || o == HELM_GATE_DFF) && in0[g] < 0)
                return fail(HELM_ERR_INVALID, "gate " + std::to_string(g) + ": missing operand");
            pl.lin.push_back(LinJob{o, in0[g], out_row(g)});
        } else {
            // gates.rs:257-264: LUT / arithmetic gates panic in boolean mode
            return fail(HELM_ERR_INVALID, "gate " + std::to_string(g) + ": op " + std::to_string(o) +
                                              " can't be mixed with Boolean gates");
        }
    }
    return 0;
}

// The gates of a level run concurrently (circuit.rs:531: par_iter over the level), and the reference gets its guarantee that
// none of them reads what another one writes from Circuit::compute_levels (circuit.rs:174-239).  A host with a wrong level
// map must not get silently non-deterministic ciphertexts: a level in which a gate reads a row ANOTHER gate of the level
// writes (RAW), or in which two gates write one row (WAW), is refused.  A gate may update its own row in place (the READY
// latch of circuit.rs:482-504: out = mux(READY, new, out)): every kernel reads a gate's operands before it writes its
// result.  `owner` has one entry per row, -1 at the start; `base` = index of the level's first gate among all gates checked
// with this `owner` (stale entries of earlier levels are below it, so nothing is cleared between levels).
static int check_level_hazards(const int32_t *in0, const int32_t *in1, const int32_t *in2, const int32_t *out, int64_t count,
                               int64_t base, std::vector<int64_t> &owner, int64_t level)
{
    for (int64_t g = 0; g < count; g++) {
        int64_t &o = owner[(size_t)out[g]];
        if (o >= base)
            return fail(HELM_ERR_INVALID, "level " + std::to_string(level) + ": gates " + std::to_string(o - base) + " and " +
                                              std::to_string(g) + " both write wire " + std::to_string(out[g]) +
                                              " (write-after-write inside a level)");
        o = base + g;
    }
    const int32_t *ins[3] = {in0, in1, in2};
    for (int64_t g = 0; g < count; g++)
        for (int q = 0; q < 3; q++) {
            const int32_t r = ins[q][g];
            if (r < 0) continue;
            const int64_t o = owner[(size_t)r];
            if (o >= base && o != base + g)
                return fail(HELM_ERR_INVALID, "level " + std::to_string(level) + ": gate " + std::to_string(g) + " reads wire " +
                                                  std::to_string(r) + ", which gate " + std::to_string(o - base) +
                                                  " of the same level writes (read-after-write inside a level)");
        }
    return 0;
}

struct TimedScope {
    helm_hip_ctx *ctx;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> *list;
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t on;
    TimedScope(helm_hip_ctx *c, std::vector<std::pair<hipEvent_t, hipEvent_t>> *l) : TimedScope(c, l, c->stream) {}
    TimedScope(helm_hip_ctx *c, std::vector<std::pair<hipEvent_t, hipEvent_t>> *l, hipStream_t s) : ctx(c), list(l), on(s)
    {
        if (ctx->timing) {
            (void)hipEventCreate(&a);
            (void)hipEventCreate(&b);
            (void)hipEventRecord(a, on);
        }
    }
    ~TimedScope()
    {
        if (ctx->timing) {
            (void)hipEventRecord(b, on);
            list->push_back({a, b});
        }
    }
};

static void print_stamps(helm_hip_ctx *ctx, int waves, const char *what)
{
#ifdef HELM_WIDE_STAMPS
    unsigned long long v[2 * 16 * 6];
    (void)hipStreamSynchronize(ctx->stream);
    if (hipMemcpyFromSymbol(v, HIP_SYMBOL(g_wide_stamps), sizeof(v)) != hipSuccess) return;
    for (int b = 0; b < 2; b++)
        for (int w = 0; w < waves; w++) {
            const unsigned long long *q = v + (b * 16 + w) * 6;
            fprintf(stderr, "[stamps %s] %s workgroup, wave %d: %llu %llu %llu %llu %llu %llu cycles/step\n", what,
                    b ? "last" : "first", w, q[0] / ctx->P.n, q[1] / ctx->P.n, q[2] / ctx->P.n, q[3] / ctx->P.n, q[4] / ctx->P.n,
                    q[5] / ctx->P.n);
        }
#else
    (void)ctx;
    (void)waves;
    (void)what;
#endif
}

// One launch of a tuned kernel, C its configuration (one type per kernel instantiation): the dynamic-LDS attribute once per
// kernel and device with the HELM_HIP_VERBOSE line, the launch with C::BYTES of LDS on the context's stream, the stamps.
template <typename C, typename Kern, typename... Args>
static hipError_t launch_tuned(helm_hip_ctx *ctx, Kern kern, const char *name, dim3 grid, dim3 block, int stamp_waves,
                               const char *legend, Args... args)
{
    static std::atomic<bool> attr_done[64]; // (rank threads of one process launch concurrently)
    if (!attr_done[ctx->device & 63]) {
        const void *fn = reinterpret_cast<const void *>(kern);
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)C::BYTES);
        if (e != hipSuccess) return e;
        attr_done[ctx->device & 63] = true;
        if (getenv("HELM_HIP_VERBOSE")) {
            int nb = -1;
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, (int)block.x, C::BYTES);
            hipFuncAttributes fa{};
            (void)hipFuncGetAttributes(&fa, fn);
            fprintf(stderr, "[helm_hip] %s: %u waves, LDS %zu B, regs %d, scratch %zu B, max %d workgroups/CU\n", name, block.x / 64,
                    (size_t)C::BYTES, fa.numRegs, (size_t)fa.localSizeBytes, nb);
        }
    }
    hipLaunchKernelGGL(kern, grid, block, C::BYTES, ctx->stream, args...);
    const hipError_t e = hipGetLastError();
    print_stamps(ctx, stamp_waves, legend);
    return e;
}

template <typename C>
static hipError_t launch_pbs_v(helm_hip_ctx *ctx, const PbsJob *jobs, int64_t count, const uint32_t *wires,
                               const uint32_t *raw, const uint32_t *tvs, uint32_t *out_big)
{
    hipError_t e = launch_tuned<C>(ctx, k_pbs<C>, "k_pbs (lockstep)", dim3((unsigned)((count + C::NB - 1) / C::NB)),
                                   dim3(64 * (C::K + 1) * C::NB), C::K + 1, "k_pbs: work | bar1 | sum | bar2 | inverse | publish", jobs,
                                   wires, raw, tvs, ctx->bsk, ctx->tw_fwd, ctx->tw_inv, out_big, ctx->P.n, ctx->P.pbs_logB,
                                   ctx->clock_probe | (count >= (int64_t)C::NB * ctx->n_cus ? 2 : 0), (int)count);
    if (e == hipSuccess && (ctx->clock_probe & 1)) {
        unsigned long long v[4];
        (void)hipStreamSynchronize(ctx->stream);
        if (hipMemcpyFromSymbol(v, HIP_SYMBOL(g_clock_probe), sizeof(v)) == hipSuccess && v[3] > v[1])
            fprintf(stderr, "[helm_hip] k_pbs x%lld: in-kernel clock %.3f GHz (%.3f ms of blind rotation)\n",
                    (long long)count, (double)(v[2] - v[0]) / (double)(v[3] - v[1]) * 0.1, (double)(v[3] - v[1]) * 1e-5);
    }
    return e;
}

template <typename C>
static hipError_t launch_pbs_wide(helm_hip_ctx *ctx, const PbsJob *jobs, int64_t count, const uint32_t *wires,
                                  const uint32_t *raw, const uint32_t *tvs, uint32_t *out_big)
{
    return launch_tuned<C>(ctx, k_pbs_wide<C>, "k_pbs_wide", dim3((unsigned)count), dim3(64 * C::NW), C::NW,
                           "wide: prep | fwd | products | bar1 | inverse | bar2", jobs, wires, raw, tvs, ctx->bsk, ctx->tw_fwd,
                           out_big, ctx->P.n, ctx->P.pbs_logB);
}

template <typename C>
static hipError_t launch_pbs_duo(helm_hip_ctx *ctx, const PbsJob *jobs, int64_t count, const uint32_t *wires,
                                 const uint32_t *raw, const uint32_t *tvs, uint32_t *out_big)
{
    return launch_tuned<C>(ctx, k_pbs_duo<C>, C::STAG ? "k_pbs_duo (staggered)" : "k_pbs_duo",
                           dim3((unsigned)((count + C::NB - 1) / C::NB)), dim3(64 * C::NW), C::NW,
                           "duo: forward | barriers | inverse | - | - | -", jobs, wires, raw, tvs, ctx->bsk, ctx->tw_fwd, out_big,
                           ctx->P.n, ctx->P.pbs_logB, (int)count);
}

template <typename C>
static hipError_t launch_pbs_trio(helm_hip_ctx *ctx, const PbsJob *jobs, int64_t count, const uint32_t *wires,
                                  const uint32_t *raw, const uint32_t *tvs, uint32_t *out_big)
{
    return launch_tuned<C>(ctx, k_pbs_trio<C>, "k_pbs_trio", dim3((unsigned)((count + C::NB - 1) / C::NB)), dim3(64 * C::NW), C::NW,
                           "trio: rotate+publish | bar A | forward work | bar B (helper: B+C) | sums + bar C | inverse + lift", jobs,
                           wires, raw, tvs, ctx->bsk, ctx->tw_fwd, out_big, ctx->P.n, ctx->P.pbs_logB, (int)count);
}

template <typename C>
static hipError_t launch_pbs_tri10(helm_hip_ctx *ctx, const PbsJob *jobs, int64_t count, const uint32_t *wires,
                                   const uint32_t *raw, const uint32_t *tvs, uint32_t *out_big)
{
    return launch_tuned<C>(ctx, k_pbs_tri10<C>, "k_pbs_tri10", dim3((unsigned)((count + C::NB - 1) / C::NB)), dim3(64 * C::NW), C::NW,
                           "tri10: forward work | bar 1 | sum + inverse half | bar 2 | join + lift | bar 3", jobs, wires, raw, tvs,
                           ctx->bsk, ctx->tw_fwd, ctx->tw_inv, out_big, ctx->P.n, ctx->P.pbs_logB, (int)count);
}

// Two translation units from this one source (Makefile): the whole file is compiled under the compiler's max-ILP scheduling
// strategy (-mllvm -amdgpu-sched-strategy=max-ilp: +1.9 % on the lockstep k_pbs, same box, alternating, identical
// ciphertexts), except k_pbs_wide, which that strategy slows down by 0.9 % and which is therefore compiled a second time
// with -DHELM_HIP_TU=1 under the default strategy - that unit holds this launcher and nothing else of the host side.
// build: BUILD_WIDE, BUILD_DUO or BUILD_DUO_STAG (at N = 1024 k_pbs_duo has its compact LDS layout, DuoCfg::COMPACT), of the
// context's tuned form
__attribute__((visibility("hidden"))) hipError_t helm_hip_tu1_launch_wide(helm_hip_ctx *ctx, int build, const PbsJob *jobs,
                                                                        int64_t count, const uint32_t *wires, const uint32_t *raw,
                                                                        const uint32_t *tvs, uint32_t *out_big);
#if !HELM_HIP_SPLIT_TU // (that unit, and a build of the file as a single unit)
hipError_t helm_hip_tu1_launch_wide(helm_hip_ctx *ctx, int build, const PbsJob *jobs, int64_t count, const uint32_t *wires,
                                    const uint32_t *raw, const uint32_t *tvs, uint32_t *out_big)
{
    return with_tuned(ctx->form.shape, ctx->form.field, hipErrorInvalidValue, [&](auto t) {
        using T = decltype(t);
        if (build == BUILD_DUO)
            return launch_pbs_duo<DuoCfg<typename T::F, T::LOGN, T::K, T::L, false>>(ctx, jobs, count, wires, raw, tvs, out_big);
        if (build == BUILD_DUO_STAG)
            return launch_pbs_duo<DuoCfg<typename T::F, T::LOGN, T::K, T::L, true>>(ctx, jobs, count, wires, raw, tvs, out_big);
        if (build != BUILD_WIDE) return hipErrorInvalidValue;
        return launch_pbs_wide<WideCfg<typename T::F, T::LOGN, T::K, T::L>>(ctx, jobs, count, wires, raw, tvs, out_big);
    });
}
#endif
#if HELM_HIP_TU == 0 // ==== everything below: the main unit only ===============================================

// Build choice by launch size (measured: profiles/r04/microbench.jsonl, profiles/r05/microbench*.jsonl; relative costs in
// helm_hip_launch_costs).  A launch runs its full rounds of 4 bootstraps per CU on the lockstep k_pbs and the remainder by size:
//   <= 1 per CU   k_pbs_wide   (k+1) L waves per bootstrap: the latency of ONE chain (a single netlist's levels)
//   <= 2 per CU   k_pbs_duo    two bootstraps per workgroup, staggered by half a step (N = 1024: k_pbs_tri10's waves, two
//                              bootstraps per workgroup - 14 % faster there than k_pbs_duo's compact layout)
//   <= 3 per CU   k_pbs_trio   three bootstraps per workgroup, four waves each (k = 2, N = 512); k_pbs_tri10 (N = 1024: twelve
//                              (polynomial, transform half) waves); other sets: a lockstep round
//   more          another lockstep round
// HELM_HIP_PBS_VARIANT=4|5|6|7|9 forces wide | lockstep | duo in step | duo staggered | trio for the whole launch, 8 (N = 1024)
// k_pbs_tri10 with two bootstraps per workgroup (parity tests and same-box A/B runs); every other value is refused by
// helm_hip_ctx_create.
template <typename F, int LOGN, int K, int L>
static hipError_t launch_pbs_f(helm_hip_ctx *ctx, const PbsJob *jobs, int64_t count, const uint32_t *wires,
                               const uint32_t *raw, const uint32_t *tvs, uint32_t *out_big)
{
    // Round 4 (N = 512): the lane's block-B / block-C twiddles of the FORWARD direction sit in registers (TW_LANE_FREG: 28 of
    // them, 140 -> 162 registers, still three waves per SIMD) instead of being read from the LDS lane table in every one of the
    // three forward transforms of a step: +1.9 % (profiles/r04/lockstep_twiddle_registers.txt).  N = 1024 (two waves per
    // bootstrap on one SIMD, 248 registers) reads the table.
    using Lock = PbsCfg<F, LOGN, K, L, LOGN == 9 ? TW_LANE_FREG : TW_LANE>;
    const BoolForm &form = ctx->form;
    const int64_t cus = ctx->n_cus;
    int v = form.variant;
    if (v == 0) {
        const int64_t round = 4 * cus;
        int64_t full = count / round * round;
        // a remainder of more than three per CU (two where there is no three-per-CU build) is another lockstep round
        const bool trio = form.rem[2] == BUILD_TRIO;
        if (count - full > (trio ? 3 : 2) * cus) full = count;
        if (full) {
            hipError_t e;
            {
                TimedScope t(ctx, &ctx->ev_pbs_main);
                e = launch_pbs_v<Lock>(ctx, jobs, full, wires, raw, tvs, out_big);
            }
            ctx->tacc.pbs_main_launches++;
            ctx->tacc.pbs_main_count += full;
            if (e != hipSuccess || full == count) return e;
            jobs += full;
            out_big += (size_t)full * ((size_t)K * (1 << LOGN) + 1);
            count -= full;
        }
        v = form.rem[count <= cus ? 0 : count <= 2 * cus ? 1 : 2]; // (BUILD_LOCKSTEP: no build of that size - a lockstep round instead)
    }
    if (v == BUILD_WIDE || v == BUILD_DUO || v == BUILD_DUO_STAG) // (the other translation unit's builds, of this same form)
        return helm_hip_tu1_launch_wide(ctx, v, jobs, count, wires, raw, tvs, out_big);
    if (v == BUILD_TRIO) {
        if constexpr (LOGN == 9 && K == 2) return launch_pbs_trio<TrioCfg<F, LOGN, K, L>>(ctx, jobs, count, wires, raw, tvs, out_big);
        else if constexpr (LOGN == 10 && K == 1) return launch_pbs_tri10<Tri10Cfg<F, L>>(ctx, jobs, count, wires, raw, tvs, out_big);
    }
    if (v == BUILD_TRI10_2) { // (N = 1024: HELM_HIP_DUO1024=3) k_pbs_tri10's waves, two bootstraps per workgroup
        if constexpr (LOGN == 10 && K == 1) return launch_pbs_tri10<Tri10Cfg<F, L, 2>>(ctx, jobs, count, wires, raw, tvs, out_big);
    }
    return launch_pbs_v<Lock>(ctx, jobs, count, wires, raw, tvs, out_big);
}

// the shapes k_pbs_generic takes (a superset of the tuned ones): its LDS budget is (k+1) N <= 8192 (helm_pbs_generic.inc)
static bool pbs_admitted(const helm_hip_params &P)
{
    return (P.N == 256 || P.N == 512 || P.N == 1024 || P.N == 2048) && P.k >= 1 && (int64_t)(P.k + 1) * P.N <= 8192 &&
           P.pbs_l >= 1;
}


// the CRT domain, whole (helm_hip_ctx_create_ex under HELM_HIP_CREATE_ALLOW_CRT / FORCE_CRT, as include/helm_hip.h states
// it): N stops at 2048 because FpG2 has 2-adicity 2^12; (k+1) N <= 4096 is the kernel's LDS budget (helm_pbs_crt.inc);
// n <= 1024 is what tp_fit sizes the kernel's LDS attribute for; pbs_logB pbs_l <= 31 is what gen_decompose_step's 32-bit
// recurrence and the static_assert below rest on.  helm_hip_ctx_create_ex checks n, the decomposition, pbs_order and
// grouping_factor on their own as well (with helm_hip_ctx_create's messages, before this function is asked): they are
// repeated here so that this function alone is the domain.
static bool crt_admitted(const helm_hip_params &P)
{
    return (P.N == 256 || P.N == 512 || P.N == 1024 || P.N == 2048) && P.k >= 1 && (int64_t)(P.k + 1) * P.N <= 4096 &&
           P.pbs_l >= 1 && P.pbs_logB >= 1 && (int64_t)P.pbs_logB * P.pbs_l <= 31 && P.n >= 1 && P.n <= 1024 &&
           (P.pbs_order == 0 || P.pbs_order == 1) && P.grouping_factor == 1; // (order 1: only under HELM_HIP_CREATE_KS_PBS,
                                                                              // which helm_hip_ctx_create_ex has checked)
}
// The CRT domain needs no capacity check: the largest exact product over it, (k+1) N <= 4096 times l 2^(logB-1) <= 31 x 2^30
// (logB l <= 31) times 2^31, is 4096 x 31 x 2^61 = 2^77.96 < 2^78, and p0 p1 / 2 = 2^97.5.
static_assert(((unsigned __int128)4096 * 31 << 61) < ((unsigned __int128)1 << 78) &&
                  ((unsigned __int128)1 << 78) < (unsigned __int128)FpG::P_U64 * FpG2::P_U64 / 2,
              "the CRT domain's largest exact product is below p0 p1 / 2");

// k_pbs_generic / k_pbs_crt of a logN, as the occupancy and attribute calls take them (setup_generic, setup_crt)
static const void *class_kernel(BoolClass run, int logN)
{
    return with_logn<8, 11>(logN, (const void *)nullptr, [&](auto ln) {
        constexpr int LOGN = decltype(ln)::value;
        return run == BOOL_CRT ? reinterpret_cast<const void *>(k_pbs_crt<LOGN>) : reinterpret_cast<const void *>(k_pbs_generic<LOGN>);
    });
}

// Every bootstrap launch of the engine: the context's record says which kernel runs it (one workgroup per bootstrap at the
// setup step's (d, lds) for classes 1 and 2, whose dynamic-LDS attribute that step has set; launch_pbs_f's size dispatch for
// a tuned form).
static hipError_t launch_pbs(helm_hip_ctx *ctx, const PbsJob *jobs, int64_t count, const uint32_t *wires,
                             const uint32_t *raw, const uint32_t *tvs, uint32_t *out_big)
{
    const helm_hip_params &P = ctx->P;
    const BoolForm &form = ctx->form;
    switch (form.run) {
    case BOOL_CRT:
        return with_logn<8, 11>(ctx->logN, hipErrorInvalidValue, [&](auto ln) {
            hipLaunchKernelGGL(k_pbs_crt<decltype(ln)::value>, dim3((unsigned)count), dim3(TP_THREADS), form.lds, ctx->stream, jobs,
                               wires, raw, tvs, ctx->bsk, ctx->crt_tw[0], ctx->crt_tw[1], ctx->crt_tw[2], ctx->crt_tw[3], out_big, P.n,
                               P.k, P.pbs_l, P.pbs_logB, form.d, ctx->crt_p0inv);
            return hipGetLastError();
        });
    case BOOL_GENERIC:
        return with_logn<8, 11>(ctx->logN, hipErrorInvalidValue, [&](auto ln) {
            hipLaunchKernelGGL(k_pbs_generic<decltype(ln)::value>, dim3((unsigned)count), dim3(GEN_THREADS), form.lds, ctx->stream,
                               jobs, wires, raw, tvs, ctx->bsk, ctx->tw_fwd, ctx->tw_inv, out_big, P.n, P.k, P.pbs_l, P.pbs_logB,
                               form.d);
            return hipGetLastError();
        });
    case BOOL_TUNED:
        return with_tuned(form.shape, form.field, hipErrorInvalidValue, [&](auto t) {
            using T = decltype(t);
            return launch_pbs_f<typename T::F, T::LOGN, T::K, T::L>(ctx, jobs, count, wires, raw, tvs, out_big);
        });
    }
    return hipErrorInvalidValue;
}

// What the boolean engine's keyswitch launches have of their own (helm_ks::launch): the matrix-core form whenever the key
// has byte planes (ks_l in {1, 2, 4, 8}), two column tiles per product wave, no level padding, no ks_l = 7, the default
// dynamic-LDS limit, and k_ks_zero over the product kernel's job list before a sliced launch.
struct KsEngine32 {
    using Word = uint32_t;
    using Ctx = helm_hip_ctx;
    using OutJob = KsJob;
    using Where = std::nullptr_t;
    using VectorLevels = std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 8>;
    using DigitLevels = std::integer_sequence<int, 1, 2, 4, 8>;
    static constexpr int CT = 2;
    static constexpr int padded_levels(int ks_l) { return ks_l; }
    static auto product_kernel() { return k_ks_mfma; }
    static bool matrix_path(const Ctx *ctx, const helm_ks::Key<uint32_t> &K, int64_t) { return K.planes && ctx->ks_mfma; }
    static hipError_t zero_rows(Ctx *ctx, const KsJob *out_jobs, Where, uint32_t *out, int64_t count, int n)
    {
        hipLaunchKernelGGL(k_ks_zero, dim3((unsigned)count), dim3(256), 0, ctx->stream, out_jobs, out, n);
        return hipGetLastError();
    }
    template <typename> static hipError_t allow_lds(Ctx *, const void *) { return hipSuccess; }
};

static helm_ks::Key<uint32_t> ks_key(const helm_hip_ctx *ctx)
{
    const helm_hip_params &P = ctx->P;
    helm_ks::Key<uint32_t> K;
    K.key = ctx->ksk;
    K.planes = ctx->ksk_planes;
    K.in_dim = P.k * P.N;
    K.out_dim = P.n;
    K.l = P.ks_l;
    K.logB = P.ks_logB;
    K.kchunks = ctx->ks_kchunks;
    K.ctiles = ctx->ks_ctiles;
    return K;
}

static hipError_t launch_ks(helm_hip_ctx *ctx, const KsJob *jobs, int64_t count, const uint32_t *big, uint32_t *out)
{
    return helm_ks::launch<KsEngine32>(
        ctx, ks_key(ctx), jobs, jobs, count, big, out, nullptr, [](auto lv) { return k_ks_digits<decltype(lv)::value>; },
        [](auto lv) { return k_keyswitch<decltype(lv)::value>; });
}

// pbs_order = 1: the level-independent job lists of `count` rows (grown on demand, filled on the context's stream)
static hipError_t ensure_iota_jobs(helm_hip_ctx *ctx, int64_t count)
{
    if ((size_t)count <= ctx->iota_filled) return hipSuccess;
    ctx->iota_filled = 0;
    if (ctx->d_raw.ensure((size_t)count) || ctx->d_ident.ensure((size_t)count)) return hipErrorOutOfMemory;
    const size_t fill = std::min(ctx->d_raw.cap, ctx->d_ident.cap);
    hipLaunchKernelGGL(k_iota_jobs, dim3((unsigned)((fill + 255) / 256)), dim3(256), 0, ctx->stream, ctx->d_raw.p, ctx->d_ident.p,
                       (int)fill);
    hipError_t e = hipGetLastError();
    // the lists outlive this launch and helm_hip_set_stream may move the context to another stream before the next one:
    // wait once, where the buffers grew (the allocation above has synchronised the device already) - never in a round
    // that finds them large enough
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) ctx->iota_filled = fill;
    return e;
}

// The front of a keyswitch-first level: job i of the level's PbsJob list, over the big wire rows, to row i of `out` (the
// identity job list names those rows to k_ks_mfma and k_ks_zero).
static hipError_t launch_ks_gate(helm_hip_ctx *ctx, const PbsJob *jobs, int64_t count, const uint32_t *wires, uint32_t *out)
{
    return helm_ks::launch<KsEngine32>(
        ctx, ks_key(ctx), jobs, ctx->d_ident.p, count, wires, out, nullptr,
        [](auto lv) { return k_ks_gate_digits<decltype(lv)::value>; }, [](auto lv) { return k_keyswitch_gate<decltype(lv)::value>; });
}

// A keyswitch-first level (pbs_order = 1): gate keyswitch from the big wire rows to the small staging, bootstrap of the
// staging rows as raw LWEs, k_big_out from the extracted rows to `dst` (MUX: the sum of its two halves + 1/8), k_linear at
// dimension k N.  k_big_out writes only after every keyswitch of the level has read, so a gate may update its row in place.
static int run_level_device_ks_first(helm_hip_ctx *ctx, const PbsJob *d_pbs, int64_t n_pbs, const KsJob *d_ks, int64_t n_ks,
                                     const LinJob *d_lin, int64_t n_lin, const uint32_t *wires_in, uint32_t *dst)
{
    const helm_hip_params &P = ctx->P;
    const int kN = P.k * P.N;
    if (n_pbs > 0) {
        if (!ctx->have_bsk || !ctx->have_ksk) return fail(HELM_ERR_STATE, "bootstrapping / keyswitching key not loaded");
        if (ctx->d_big.ensure((size_t)n_pbs * ((size_t)kN + 1))) return fail(HELM_ERR_OOM, "big-LWE scratch");
        if (ctx->d_small.ensure((size_t)n_pbs * ((size_t)P.n + 1))) return fail(HELM_ERR_OOM, "small-LWE staging");
        HIP_TRY(ensure_iota_jobs(ctx, n_pbs));
        {
            TimedScope t(ctx, &ctx->ev_ks);
            HIP_TRY(launch_ks_gate(ctx, d_pbs, n_pbs, wires_in, ctx->d_small.p));
        }
        ctx->tacc.ks_launches++;
        ctx->tacc.ks_count += n_pbs;
        {
            TimedScope t(ctx, &ctx->ev_pbs);
            HIP_TRY(launch_pbs(ctx, ctx->d_raw.p, n_pbs, nullptr, ctx->d_small.p, ctx->tv_bool, ctx->d_big.p));
        }
        ctx->tacc.pbs_launches++;
        ctx->tacc.pbs_count += n_pbs;
        {
            TimedScope t(ctx, &ctx->ev_ks);
            hipLaunchKernelGGL(k_big_out, dim3((unsigned)n_ks), dim3(256), 0, ctx->stream, d_ks, ctx->d_big.p, dst, kN);
            HIP_TRY(hipGetLastError());
        }
    }
    if (n_lin > 0) {
        TimedScope t(ctx, &ctx->ev_lin);
        hipLaunchKernelGGL(k_linear, dim3((unsigned)n_lin), dim3(256), 0, ctx->stream, d_lin, wires_in, dst, kN);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// Run one planned level whose job arrays are already on the device.
static int run_level_device(helm_hip_ctx *ctx, const PbsJob *d_pbs, int64_t n_pbs, const KsJob *d_ks, int64_t n_ks,
                            const LinJob *d_lin, int64_t n_lin, const uint32_t *wires_in, uint32_t *dst)
{
    const helm_hip_params &P = ctx->P;
    if (P.pbs_order == 1) return run_level_device_ks_first(ctx, d_pbs, n_pbs, d_ks, n_ks, d_lin, n_lin, wires_in, dst);
    if (n_pbs > 0) {
        if (!ctx->have_bsk || !ctx->have_ksk) return fail(HELM_ERR_STATE, "bootstrapping / keyswitching key not loaded");
        if (ctx->d_big.ensure((size_t)n_pbs * ((size_t)P.k * P.N + 1))) return fail(HELM_ERR_OOM, "big-LWE scratch");
        {
            TimedScope t(ctx, &ctx->ev_pbs);
            HIP_TRY(launch_pbs(ctx, d_pbs, n_pbs, wires_in, nullptr, ctx->tv_bool, ctx->d_big.p));
        }
        ctx->tacc.pbs_launches++;
        ctx->tacc.pbs_count += n_pbs;
        {
            TimedScope t(ctx, &ctx->ev_ks);
            HIP_TRY(launch_ks(ctx, d_ks, n_ks, ctx->d_big.p, dst));
        }
        ctx->tacc.ks_launches++;
        ctx->tacc.ks_count += n_ks;
    }
    if (n_lin > 0) {
        TimedScope t(ctx, &ctx->ev_lin);
        hipLaunchKernelGGL(k_linear, dim3((unsigned)n_lin), dim3(256), 0, ctx->stream, d_lin, wires_in, dst, P.n);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// The tables of the single-prime field F the context computes in: bit-reversed powers of psi and psi^-1, 1/N.
template <typename F> static int setup_field_tables_of(helm_hip_ctx *ctx)
{
    // twiddle tables: bit-reversed powers of psi (primitive 2N-th root) and of psi^-1
    const int N = ctx->P.N, logN = ctx->logN;
    const uint64_t pm = F::P_U64;
    uint64_t psi = powmod_u64(F::GEN, (pm - 1) / (2 * (uint64_t)N), pm);
    const double b1 = F::B1, b2 = F::B2, b3 = F::B3;
    {
        // the kernels' first two forward stages assume psi^(N/4) = b (then psi^(N/2) = b^2, psi^(3N/4) = b^3): psi^(N/4) is
        // one of the four primitive eighth roots b, b^3, -b, -b^3 - an odd power of psi puts it on b
        uint64_t pick = 0;
        for (uint64_t t = 1; t < 8 && !pick; t += 2)
            if (powmod_u64(powmod_u64(psi, t, pm), (uint64_t)N / 4, pm) == (uint64_t)b1) pick = t;
        if (!pick) return fail(HELM_ERR_STATE, "internal: no 2N-th root of unity with psi^(N/4) = b");
        psi = powmod_u64(psi, pick, pm);
    }
    std::vector<double> tf(N), ti(N);
    power_table(tf.data(), psi, pm, N, logN);
    power_table(ti.data(), powmod_u64(psi, pm - 2, pm), pm, N, logN);
    if (tf[1] != b2 || tf[2] != b1 || tf[3] != b3)
        return fail(HELM_ERR_STATE, "internal: the first twiddles are not the constants the kernels assume");
    ctx->n_inv = centred(powmod_u64((uint64_t)N, pm - 2, pm), pm);
    if (!ctx->tw_fwd) HIP_TRY(hipMalloc(&ctx->tw_fwd, sizeof(double) * N));
    if (!ctx->tw_inv) HIP_TRY(hipMalloc(&ctx->tw_inv, sizeof(double) * N));
    HIP_TRY(hipMemcpy(ctx->tw_fwd, tf.data(), sizeof(double) * N, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ctx->tw_inv, ti.data(), sizeof(double) * N, hipMemcpyHostToDevice));
    return 0;
}

// ------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------
extern "C" {

const char *helm_hip_last_error(void) { return g_err.c_str(); }

int helm_hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// The tables of form.field (49 FpG, 50 FpI, 51 FpH: setup_field_tables_of).  Called by helm_hip_ctx_create and again by helm_hip_load_bootstrap_key when
// the key moves an N = 1024 set into or out of the lazy field.
static int setup_field_tables(helm_hip_ctx *ctx)
{
    switch (ctx->form.field) {
    case 49: return setup_field_tables_of<FpG>(ctx);
    case 50: return setup_field_tables_of<FpI>(ctx);
    case 51: return setup_field_tables_of<FpH>(ctx);
    default: return fail(HELM_ERR_STATE, "internal: no single-prime tables for field " + std::to_string(ctx->form.field));
    }
}

// A context whose launches run k_pbs_crt: the four twiddle tables of the pair FpG / FpG2 (any primitive 2N-th root serves:
// no stage of this kernel assumes a short root), 1/N in each field and p0^-1 mod p1, the kernel's LDS attribute, its occupancy
// and the digit batch D.
static int setup_crt(helm_hip_ctx *ctx)
{
#ifdef HELM_CHECK_BOUNDS
    // k_pbs_crt is built like the 64-bit engine's k_pbs64_generic, whose -O0 counting build faulted on its first launch for a
    // cause that was never found: until it is, this build refuses the CRT class before anything is launched.
    (void)ctx;
    return fail(HELM_ERR_STATE, "the two-prime CRT kernel is not available in the bound-checking build (libhelm_hip_check.so): "
                                "use the regular library for CRT contexts");
#else
    const helm_hip_params &P = ctx->P;
    const int N = P.N, logN = ctx->logN;
    const uint64_t pm[2] = {FpG::P_U64, FpG2::P_U64}, gen[2] = {FpG::GEN, FpG2::GEN};
    for (int f = 0; f < 2; f++) {
        const uint64_t psi = powmod_u64(gen[f], (pm[f] - 1) / (2 * (uint64_t)N), pm[f]);
        if (powmod_u64(psi, (uint64_t)N, pm[f]) != pm[f] - 1) return fail(HELM_ERR_STATE, "internal: no primitive 2N-th root of unity");
        std::vector<double> tf(N), ti(N);
        power_table(tf.data(), psi, pm[f], N, logN);
        power_table(ti.data(), powmod_u64(psi, pm[f] - 2, pm[f]), pm[f], N, logN);
        ctx->crt_n_inv[f] = centred(powmod_u64((uint64_t)N, pm[f] - 2, pm[f]), pm[f]);
        HIP_TRY(hipMalloc(&ctx->crt_tw[f], sizeof(double) * N));
        HIP_TRY(hipMalloc(&ctx->crt_tw[2 + f], sizeof(double) * N));
        HIP_TRY(hipMemcpy(ctx->crt_tw[f], tf.data(), sizeof(double) * N, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(ctx->crt_tw[2 + f], ti.data(), sizeof(double) * N, hipMemcpyHostToDevice));
    }
    ctx->crt_p0inv = centred(powmod_u64(pm[0] % pm[1], pm[1] - 2, pm[1]), pm[1]);
    const void *kern = class_kernel(BOOL_CRT, logN);
    TwoPrimeFit fit;
    HIP_TRY(tp_fit<uint32_t>(kern, N, P.k, P.pbs_l, P.n, fit));
    if (fit.per_cu < 1) return fail(HELM_ERR_STATE, "k_pbs_crt: no workgroup of " + std::to_string(fit.lds) + " B LDS fits a CU");
    ctx->form.d = fit.d;
    ctx->form.lds = fit.lds;
    ctx->form.per_cu = fit.per_cu;
    return 0;
#endif
}

// A context whose launches run k_pbs_generic (a shape no tuned build covers, or HELM_HIP_PBS_VARIANT=10): one workgroup of
// GEN_THREADS per bootstrap; the kernel's LDS attribute, its occupancy - the launch quantum follows it - and the digit batch D.
static int setup_generic(helm_hip_ctx *ctx)
{
    const helm_hip_params &P = ctx->P;
    const int N = P.N;
    const void *kern = class_kernel(BOOL_GENERIC, ctx->logN);
    // the attribute is the kernel's, shared by every context of the process: the largest layout of this N, so that a
    // context created later with a smaller one cannot lower it under an earlier context's launches
    const int K1max = 8192 / N;
    const size_t lds_max = GenLds(N, K1max, gen_batch(N, K1max - 1, 31), 1024).bytes;
    HIP_TRY(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
    // digit polynomials per batch: the most (<= gen_batch) that cost no resident workgroup against one per batch - a
    // launch of more bootstraps than fit at once runs a partial second round (boolean_default's shape: D = 4 leaves
    // 3 workgroups per CU, 2 leave 4, 1 leaves 5 - 51.9 against 44.7 ms for 1,024 bootstraps)
    auto occupancy = [&](int d, int &nb) -> int {
        nb = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, GEN_THREADS, GenLds(N, P.k + 1, d, P.n).bytes));
        return 0;
    };
    int nb1 = 0;
    if (int rc = occupancy(1, nb1)) return rc;
    if (nb1 < 1) return fail(HELM_ERR_STATE, "k_pbs_generic: no workgroup of " + std::to_string(GenLds(N, P.k + 1, 1, P.n).bytes) +
                                                 " B LDS fits a CU");
    ctx->form.d = 1;
    for (int d = gen_batch(N, P.k, P.pbs_l); d > 1; d--) {
        int nb = 0;
        if (int rc = occupancy(d, nb)) return rc;
        if (nb == nb1) {
            ctx->form.d = d;
            break;
        }
    }
    ctx->form.lds = GenLds(N, P.k + 1, ctx->form.d, P.n).bytes;
    ctx->form.per_cu = nb1;
    return 0;
}

// The setup step of the class that runs the launches, once the device is chosen: tables, and for classes 1 and 2 the
// occupancy-dependent (d, lds, per_cu) of the record with the HELM_HIP_VERBOSE line.
static int setup_class(helm_hip_ctx *ctx)
{
    const BoolForm &form = ctx->form;
    if (form.run == BOOL_TUNED) return setup_field_tables(ctx);
    if (int rc = form.run == BOOL_CRT ? setup_crt(ctx) : setup_generic(ctx)) return rc;
    if (getenv("HELM_HIP_VERBOSE")) {
        hipFuncAttributes fa{};
        (void)hipFuncGetAttributes(&fa, class_kernel(form.run, ctx->logN));
        fprintf(stderr, "[helm_hip] %s N=%d k=%d l=%d D=%d: LDS %zu B, regs %d, scratch %zu B, %d workgroups/CU\n",
                form.run == BOOL_CRT ? "k_pbs_crt" : "k_pbs_generic", ctx->P.N, ctx->P.k, ctx->P.pbs_l, form.d, form.lds, fa.numRegs,
                (size_t)fa.localSizeBytes, form.per_cu);
    }
    return form.run == BOOL_GENERIC ? setup_field_tables(ctx) : 0;
}

int helm_hip_ctx_create(int device_id, const helm_hip_params *params, helm_hip_ctx **out)
{
    return helm_hip_ctx_create_ex(device_id, params, 0, out);
}

// What helm_hip_ctx_create_ex decides before it touches a device: the record of (params, flags) and of the environment's
// switches, or the refusal - parameters and flags first, then HELM_HIP_PBS_VARIANT.
static int bool_admit(const helm_hip_params &P, uint32_t flags, BoolForm *out)
{
    // HELM_HIP_CREATE_KS_PBS admits pbs_order = 1 and changes nothing else: the CRT flags are judged on the remaining bits
    const bool ks_pbs = (flags & HELM_HIP_CREATE_KS_PBS) != 0;
    const uint32_t crt_flags = flags & ~(uint32_t)HELM_HIP_CREATE_KS_PBS;
    if (crt_flags & ~(uint32_t)(HELM_HIP_CREATE_ALLOW_CRT | HELM_HIP_CREATE_FORCE_CRT))
        return fail(HELM_ERR_INVALID, "unknown bits in flags " + std::to_string(flags) +
                                          " (HELM_HIP_CREATE_ALLOW_CRT = 1, HELM_HIP_CREATE_FORCE_CRT = 2" +
                                          (ks_pbs ? ", HELM_HIP_CREATE_KS_PBS = 16)" : ")"));
    if (crt_flags == (HELM_HIP_CREATE_ALLOW_CRT | HELM_HIP_CREATE_FORCE_CRT))
        return fail(HELM_ERR_INVALID, "flags " + std::to_string(flags) +
                                          ": HELM_HIP_CREATE_ALLOW_CRT and HELM_HIP_CREATE_FORCE_CRT exclude each other");
    const bool allow_crt = crt_flags == HELM_HIP_CREATE_ALLOW_CRT, force_crt = crt_flags == HELM_HIP_CREATE_FORCE_CRT;
    static const char *const crt_domain = "the CRT domain (HELM_HIP_CREATE_ALLOW_CRT / HELM_HIP_CREATE_FORCE_CRT) is N in {256, 512, 1024, "
                                          "2048}, k >= 1 with (k+1) N <= 4096, pbs_l >= 1 with pbs_logB pbs_l <= 31, n in [1,1024], "
                                          "pbs_order 0, grouping_factor 1";
    if (P.torus_bits != 32) return fail(HELM_ERR_INVALID, "only torus_bits = 32 is implemented");
    if (P.pbs_order != 0 && !ks_pbs) return fail(HELM_ERR_INVALID, "only pbs_order = 0 (bootstrap then keyswitch)");
    if (P.pbs_order != 0 && P.pbs_order != 1)
        return fail(HELM_ERR_INVALID, "pbs_order must be 0 (bootstrap then keyswitch) or 1 (keyswitch then bootstrap)");
    if (P.grouping_factor != 1) return fail(HELM_ERR_INVALID, "multi-bit PBS (grouping_factor > 1) not implemented");
    if (force_crt && !crt_admitted(P))
        return fail(HELM_ERR_INVALID, std::string("HELM_HIP_CREATE_FORCE_CRT: unsupported (N,k,pbs_l): ") + crt_domain);
    if (!pbs_admitted(P))
        return fail(HELM_ERR_INVALID, "unsupported (N,k,pbs_l): N must be 256, 512, 1024 or 2048, k >= 1 with (k+1) N <= 8192, "
                                      "pbs_l >= 1 (tuned builds: (512,2,3) (512,1,3) (512,1,2) (1024,1,3) (1024,1,2); "
                                      "every other shape runs the generic kernel)");
    if (P.n < 1 || P.n > 1024) return fail(HELM_ERR_INVALID, "n must be in [1,1024]");
    if (P.pbs_logB < 1 || P.pbs_logB * P.pbs_l > 31) return fail(HELM_ERR_INVALID, "bad PBS decomposition");
    if (P.ks_logB < 1 || P.ks_logB > 7 || P.ks_logB * P.ks_l > 32 ||
        !(P.ks_l >= 1 && (P.ks_l <= 6 || P.ks_l == 8)))
        return fail(HELM_ERR_INVALID, "bad keyswitch decomposition (ks_logB <= 7, ks_l in {1..6,8})");
    // exactness: |sum| <= (k+1) * l * N * (B/2) * 2^31 must stay below p/2
    const double bound = (double)(P.k + 1) * P.pbs_l * P.N * (double)(1u << (P.pbs_logB - 1)) * 2147483648.0;
    bool crt_class = false; // beyond the single prime, inside the CRT domain, and the caller allows the two-prime kernel
    if (bound * 1.0001 >= FpH::P / 2) {
        if (!allow_crt && !force_crt) return fail(HELM_ERR_INVALID, "parameter set exceeds the single-prime NTT capacity");
        if (!crt_admitted(P))
            return fail(HELM_ERR_INVALID, std::string("parameter set exceeds the single-prime NTT capacity and lies outside the "
                                                      "two-prime kernel's LDS budget: ") + crt_domain);
        crt_class = true; // (no capacity check of its own: see the static_assert at crt_admitted)
    }
    BoolForm form;
    form.shape = tuned_shape(P);
    form.cls = crt_class ? BOOL_CRT : form.shape < 0 ? BOOL_GENERIC : BOOL_TUNED;
    if (const char *v = getenv("HELM_HIP_PBS_VARIANT")) {
        const int pv = form.variant = atoi(v);
        if (!(pv == 0 || pv == 4 || pv == 5 || pv == 6 || pv == 7 || pv == 9 || pv == 10 || (pv == 8 && P.N == 1024)))
            return fail(HELM_ERR_INVALID, std::string("HELM_HIP_PBS_VARIANT=") + v + ": builds are 4 wide, 5 lockstep, 6 / 7 duo in step / "
                                          "staggered, 9 trio, 10 generic (1 latency, 2 balanced, 3 throughput, 8 sym were retired in round 6)");
    }
    // the CRT class (a shape beyond the single-prime bound under HELM_HIP_CREATE_ALLOW_CRT, or every launch of a shape of the
    // CRT domain under HELM_HIP_CREATE_FORCE_CRT): FpG x FpG2, its own key layout and tables, no single-prime table.  The
    // generic class (a shape no tuned build covers, or every launch under HELM_HIP_PBS_VARIANT=10): always FpH, its own key
    // layout.
    form.run = crt_class || force_crt ? BOOL_CRT : form.cls == BOOL_GENERIC || form.variant == 10 ? BOOL_GENERIC : BOOL_TUNED;
    if (form.run == BOOL_CRT && form.variant != 0)
        return fail(HELM_ERR_INVALID, "HELM_HIP_PBS_VARIANT=" + std::to_string(form.variant) +
                                          " names a single-prime build: a CRT context runs the two-prime kernel only "
                                          "(leave the variable unset, or 0)");
    if (form.cls == BOOL_GENERIC && form.variant != 0 && form.variant != 10)
        return fail(HELM_ERR_INVALID, "HELM_HIP_PBS_VARIANT=" + std::to_string(form.variant) +
                                          " names a tuned build, which this shape (N,k,pbs_l) has not: it runs the generic kernel "
                                          "(variant 10, or leave the variable unset)");
    // the 49-bit prime (no recentring inside transforms) when the set's exact products fit
    // below its half and a lazy build exists (N = 512); HELM_HIP_FIELD=51 forces the other
    // ("49": the lazy field of the boolean kernels is FpG, p = 5072^4 + 1 = 2^49.23, ntt_fp64.h; its first two forward stages
    // on digits need 2^(logB-1) b^3 far below p/2: any logB <= 12).  N = 1024 starts in the 51-bit field; the key decides
    // whether the lazy FpI serves (helm_hip_load_bootstrap_key)
    form.field = (P.N == 512 && bound * 1.002 < FpG::P / 2 && P.pbs_logB <= 12) ? 49 : 51;
    if (const char *v = getenv("HELM_HIP_FIELD")) if (atoi(v) == 51) form.field = 51;
    if (form.run != BOOL_TUNED) form.field = form.run == BOOL_CRT ? 98 : 51;
    // the remainder builds of a tuned shape (HELM_HIP_DUO at N = 512, HELM_HIP_DUO1024 at N = 1024: 0 or a build's number - 5;
    // HELM_HIP_TRIO=0).  A value outside a switch's range: the default at N = 512, none at N = 1024
    int duo = P.N == 512 ? 2 : 3;
    if (const char *v = getenv(P.N == 512 ? "HELM_HIP_DUO" : "HELM_HIP_DUO1024")) {
        duo = atoi(v);
        if (P.N == 512 ? duo < 0 || duo > 2 : duo < 1 || duo > 3) duo = P.N == 512 ? 2 : 0;
    }
    const char *trio = getenv("HELM_HIP_TRIO");
    const bool has_trio = form.shape >= 0 && TUNED[form.shape].trio;
    form.rem[1] = duo ? BUILD_LOCKSTEP + duo : BUILD_LOCKSTEP;
    form.rem[2] = has_trio && (!trio || atoi(trio) != 0) ? BUILD_TRIO : BUILD_LOCKSTEP;
    *out = form;
    return 0;
}

int helm_hip_ctx_create_ex(int device_id, const helm_hip_params *params, uint32_t flags, helm_hip_ctx **out)
{
    if (!params || !out) return fail(HELM_ERR_INVALID, "null argument");
    *out = nullptr;
    const helm_hip_params &P = *params;
    BoolForm form;
    if (int rc = bool_admit(P, flags, &form)) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(HELM_ERR_NO_DEVICE, "no HIP device visible (this engine has no CPU fallback)");
    if (device_id < 0 || device_id >= ndev) return fail(HELM_ERR_NO_DEVICE, "device_id out of range");
    HIP_TRY(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device_id));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(HELM_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");

    helm_hip_ctx *ctx = new (std::nothrow) helm_hip_ctx();
    if (!ctx) return fail(HELM_ERR_OOM, "ctx");
    // everything below may fail half-way: the partially built context is destroyed on every error path
    const int rc = [&]() -> int {
        ctx->device = device_id;
        ctx->P = P;
        ctx->form = form;
        ctx->n_cus = prop.multiProcessorCount;
        if (const char *v = getenv("HELM_HIP_CLOCK_PROBE")) ctx->clock_probe = atoi(v);
        if (const char *v = getenv("HELM_HIP_KS_MFMA")) ctx->ks_mfma = atoi(v);
        while ((1 << ctx->logN) < P.N) ctx->logN++;
        HIP_TRY(hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking));
        ctx->stream = ctx->own_stream;
        if (int rc = setup_class(ctx)) return rc;
        const int N = P.N;
        std::vector<uint32_t> tv(N, PT_TRUE);
        HIP_TRY(hipMalloc(&ctx->tv_bool, sizeof(uint32_t) * N));
        HIP_TRY(hipMemcpy(ctx->tv_bool, tv.data(), sizeof(uint32_t) * N, hipMemcpyHostToDevice));
        return 0;
    }();
    if (rc) {
        const std::string msg = g_err;
        (void)helm_hip_ctx_destroy(ctx);
        return fail(rc, msg);
    }
    *out = ctx;
    return 0;
}

int helm_hip_ctx_destroy(helm_hip_ctx *ctx)
{
    if (!ctx) return 0;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream || !ctx->own_stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->xchg_stream) (void)hipStreamSynchronize(ctx->xchg_stream);
    for (auto *l : {&ctx->ev_pbs, &ctx->ev_pbs_main, &ctx->ev_ks, &ctx->ev_lin, &ctx->ev_xchg})
        for (auto &p : *l) {
            (void)hipEventDestroy(p.first);
            (void)hipEventDestroy(p.second);
        }
    for (auto *w : ctx->child_wires) {
        (void)hipFree(w->d);
        w->d = nullptr;
        w->owner = nullptr;
    }
    for (auto *pr : ctx->child_progs) {
        (void)hipFree(pr->d_pbs);
        (void)hipFree(pr->d_ks);
        (void)hipFree(pr->d_lin);
        pr->d_pbs = nullptr;
        pr->d_ks = nullptr;
        pr->d_lin = nullptr;
        pr->s_pbs.release();
        pr->s_ks.release();
        pr->s_lin.release();
        pr->s_rows.release();
        pr->x_gather.release();
        release_overlap(pr);
        pr->owner = nullptr;
    }
    (void)hipFree(ctx->tw_fwd);
    (void)hipFree(ctx->tw_inv);
    for (double *t : ctx->crt_tw) (void)hipFree(t);
    (void)hipFree(ctx->bsk);
    (void)hipFree(ctx->ksk);
    (void)hipFree(ctx->ksk_planes);
    ctx->d_ksdig.release();
    ctx->d_ksdsum.release();
    ctx->d_ksbody.release();
    (void)hipFree(ctx->tv_bool);
    ctx->d_pbs.release();
    ctx->d_ks.release();
    ctx->d_lin.release();
    ctx->d_big.release();
    ctx->d_small.release();
    ctx->d_raw.release();
    ctx->d_ident.release();
    if (ctx->xchg_stream) (void)hipStreamDestroy(ctx->xchg_stream);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
    return 0;
}

int helm_hip_get_params(const helm_hip_ctx *ctx, helm_hip_params *out)
{
    if (!ctx || !out) return fail(HELM_ERR_INVALID, "null argument");
    *out = ctx->P;
    return 0;
}

int helm_hip_set_stream(helm_hip_ctx *ctx, void *hip_stream)
{
    if (!ctx) return fail(HELM_ERR_INVALID, "null ctx");
    // the handle was made by the caller's HIP runtime: it must be the one this library runs on
    if (int rc = helm_hip_runtime_guard_("helm_hip_set_stream")) return rc;
    // NULL is HIP's null (legacy default) stream - what torch.cuda.current_stream() is unless the caller
    // switched streams - NOT "back to the context's own stream": collectives the caller orders on that
    // stream must see the engine's kernels on it
    ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
    return 0;
}

int helm_hip_sync(helm_hip_ctx *ctx)
{
    if (!ctx) return fail(HELM_ERR_INVALID, "null ctx");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int64_t helm_hip_launch_quantum(const helm_hip_ctx *ctx)
{
    if (!ctx) return fail(HELM_ERR_INVALID, "null ctx");
    // k_pbs_generic, k_pbs_crt: one bootstrap per workgroup, all resident
    if (ctx->form.run != BOOL_TUNED) return (int64_t)ctx->form.per_cu * ctx->n_cus;
    return 4 * (int64_t)ctx->n_cus; // PbsCfg::NB bootstraps per workgroup, one workgroup per CU
}

int helm_hip_kernel_class(const helm_hip_ctx *ctx)
{
    if (!ctx) return fail(HELM_ERR_INVALID, "null argument");
    return ctx->form.cls;
}

int64_t helm_hip_wire_words(const helm_hip_ctx *ctx)
{
    if (!ctx) return fail(HELM_ERR_INVALID, "null argument");
    return (int64_t)wire_dim(ctx) + 1;
}

int helm_hip_digit_batch(const helm_hip_ctx *ctx)
{
    if (!ctx) return fail(HELM_ERR_INVALID, "null argument");
    return ctx->form.run != BOOL_TUNED ? ctx->form.d : 0;
}

int helm_hip_field_bits(const helm_hip_ctx *ctx)
{
    if (!ctx) return fail(HELM_ERR_INVALID, "null argument");
    return ctx->form.field;
}

#ifdef HELM_CHECK_BOUNDS
// the check build's self-test: one contract broken on purpose (mulmod with |a| = 2^53), so that a test can see the counter move
__global__ void k_bounds_selftest(double *out)
{
    out[threadIdx.x] = mulmod<FpG>(threadIdx.x == 0 ? 0x1p53 : 3.0, 5.0);
}
#endif

int helm_hip_bound_violations(helm_hip_ctx *ctx, uint32_t counts[8], int reset, int selftest)
{
    if (!ctx || !counts) return fail(HELM_ERR_INVALID, "null argument");
#ifdef HELM_CHECK_BOUNDS
    HIP_TRY(hipSetDevice(ctx->device));
    if (selftest) {
        Scratch<double> d;
        HIP_TRY(d.alloc(64));
        hipLaunchKernelGGL(k_bounds_selftest, dim3(1), dim3(64), 0, ctx->stream, d.p);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpyFromSymbol(counts, HIP_SYMBOL(g_helm_bound_violations), 8 * sizeof(uint32_t)));
    if (reset) {
        const uint32_t zero[8] = {0};
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_helm_bound_violations), zero, sizeof(zero)));
    }
    return 0;
#else
    (void)reset;
    (void)selftest;
    return fail(HELM_ERR_STATE, "this library was not built with -DHELM_CHECK_BOUNDS (make libhelm_hip_check.so, HELM_HIP_LIB)");
#endif
}

int helm_hip_short_root_stages(const helm_hip_ctx *ctx)
{
    if (!ctx) return fail(HELM_ERR_INVALID, "null argument");
    if (ctx->form.run != BOOL_TUNED) return 0; // k_pbs_generic, k_pbs_crt: plain radix-2 stages throughout
    return 2; // both fields of this engine (5072^4 + 1, 6432^4 + 1) have short eighth roots
}

int helm_hip_launch_costs(const helm_hip_ctx *ctx, double cost[4])
{
    if (!ctx || !cost) return fail(HELM_ERR_INVALID, "null argument");
    const BoolForm &form = ctx->form;
    if (form.run != BOOL_TUNED) {
        // k_pbs_generic / k_pbs_crt, from its occupancy W (workgroups per CU, one wave of each on every SIMD): a launch of at most q/4 of
        // the quantum puts w = ceil(q W / 4) workgroups on a CU.  One wave per SIMD leaves the step's latencies (LDS round
        // trips, key loads, barriers) exposed; from two on, the SIMD's time grows with its waves.  Model: time ~ max(1, w / 2),
        // relative to the full round - non-decreasing, cost[3] = 1 (not measured; DESIGN.md "The generic kernel class")
        const int W = form.per_cu;
        const double full = std::max(1.0, W / 2.0);
        for (int q = 1; q <= 4; q++) cost[q - 1] = std::max(1.0, ((q * W + 3) / 4) / 2.0) / full;
        return 0;
    }
    // launch_pbs_f's dispatch, measured (profiles/r04/microbench.jsonl and the other boxes of the round; boolean_default:
    // 3.2 - 3.3 / 5.0 - 5.3 / 6.6 - 6.7 / 7.6 - 8.0 ms for <= 256 / 512 / 768 / 1,024 bootstraps - wide, duo, trio and a full
    // lockstep round, final build of round 4; without k_pbs_duo (A/B switch) a launch of <= 512 is a lockstep round, without
    // k_pbs_trio a lockstep round of three per CU 0.89 - 0.90 for <= 768)
    if (ctx->P.N == 512) {
        cost[0] = 0.42;
        cost[1] = form.rem[1] != BUILD_LOCKSTEP ? 0.66 : 1.0;
        cost[2] = form.rem[2] == BUILD_TRIO ? 0.86 : 0.89;
    } else { // N = 1024 (helm_cuda, round 5: 3.9 / 5.5 / 8.0 / 8.6 ms - wide, k_pbs_duo's compact layout (two-wave build: 6.05), lockstep rounds;
             // in the lazy field FpI: 3.41 / 5.11 / 7.55 / 7.76 ms, profiles/r05/ab_field1024.jsonl)
        const bool lazy = form.field == 50;
        cost[0] = lazy ? 0.44 : 0.45;
        // round 6 (profiles/r06/ab_tri10.jsonl, same process, alternating): k_pbs_tri10 with two / three bootstraps per workgroup -
        // FpI 4.41 / 6.19 of 7.80 ms, FpH 4.65 / 6.49 of 8.32 ms (k_pbs_duo: 5.11 of 7.80; a partial lockstep round: 7.49 / 7.94)
        cost[1] = form.rem[1] == BUILD_TRI10_2 ? 0.57 : form.rem[1] != BUILD_LOCKSTEP ? (lazy ? 0.66 : 0.64) : 1.0;
        cost[2] = form.rem[2] == BUILD_TRIO ? (lazy ? 0.80 : 0.78) : (lazy ? 0.97 : 0.93);
    }
    cost[3] = 1.0;
    return 0;
}

int helm_hip_load_bootstrap_key(helm_hip_ctx *ctx, const uint32_t *bsk_std, size_t n_words)
{
    if (!ctx || !bsk_std) return fail(HELM_ERR_INVALID, "null argument");
    const helm_hip_params &P = ctx->P;
    const size_t K1 = P.k + 1;
    const size_t polys = (size_t)P.n * P.pbs_l * K1 * K1;
    if (n_words != polys * P.N)
        return fail(HELM_ERR_INVALID, "bootstrapping key: expected " + std::to_string(polys * P.N) + " words, got " +
                                          std::to_string(n_words));
    HIP_TRY(hipSetDevice(ctx->device));
    BoolForm &form = ctx->form;
    if (P.N == 1024 && form.run == BOOL_TUNED) {
        // Round 5: which field serves THIS key.  The exact sum an external product can reach is at most B/2 x the l1-norm of
        // the key coefficients that meet in one output coefficient: the (k+1) l polynomials of one key column of one step (a
        // negacyclic product's output coefficient is a signed sum over ALL coefficients of each factor).  Both groupings of
        // the (k+1)^2 polynomials of a level are taken (row-wise and column-wise), so the bound does not depend on the
        // container's order.  Below FpI's half (2^48.64; a key of uniform masks gives 2^48.58 under helm.rs:141-146's set)
        // the lazy field is exact for every input under this key; otherwise the 51-bit field stays (worst case 2^49.58).
        double worst = 0.0;
        const size_t per_step = (size_t)P.pbs_l * K1 * K1;
        std::vector<double> l1(per_step);
        for (size_t i = 0; i < (size_t)P.n; i++) {
            for (size_t q = 0; q < per_step; q++) {
                const uint32_t *w = bsk_std + (i * per_step + q) * (size_t)P.N;
                uint64_t acc = 0;
                for (int j = 0; j < P.N; j++) {
                    const int32_t v = (int32_t)w[j];
                    acc += (uint64_t)(v < 0 ? -(int64_t)v : (int64_t)v);
                }
                l1[q] = (double)acc;
            }
            for (size_t c = 0; c < K1; c++) {
                double by_col = 0.0, by_row = 0.0;
                for (size_t q = 0; q < per_step; q++) {
                    if (q % K1 == c) by_col += l1[q];
                    if ((q / K1) % K1 == c) by_row += l1[q];
                }
                worst = std::max(worst, std::max(by_col, by_row));
            }
        }
        const double key_bound = worst * (double)(1u << (P.pbs_logB - 1));
        // logB <= 7: the envelope tests/test_lazy_bounds.py recomputes for this field (forward outputs <= 6.9 p, column sums
        // <= 9.1 p of the 10.28 p a double holds exactly; SKIP_T1's premise on block A); top-2 outputs grow with the digit
        // size, so a small-norm key with larger digits keeps the recentring 51-bit field
        int want = (key_bound * 1.002 < FpI::P / 2 && P.pbs_logB <= 7) ? 50 : 51;
        if (const char *v = getenv("HELM_HIP_FIELD")) if (atoi(v) == 51) want = 51;
        if (want != form.field) {
            HIP_TRY(hipStreamSynchronize(ctx->stream)); // nothing in flight may still read the other field's tables
            if (ctx->xchg_stream) HIP_TRY(hipStreamSynchronize(ctx->xchg_stream));
            form.field = want; // (the one write of the record after creation)
            ctx->have_bsk = false;
            if (int rc = setup_field_tables(ctx)) return rc;
        }
    }
    Scratch<uint32_t> d_std;
    HIP_TRY(d_std.alloc(n_words));
    // (a CRT context keeps every key word in both fields: 16 bytes per word)
    if (!ctx->bsk) HIP_TRY(hipMalloc(&ctx->bsk, n_words * sizeof(double) * (form.run == BOOL_CRT ? 2 : 1)));
    HIP_TRY(hipMemcpyAsync(d_std.p, bsk_std, n_words * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    hipError_t e = hipErrorInvalidValue;
    switch (form.run) {
    case BOOL_CRT: // the CRT class's layout: [i][r][c][lev][f][N], bit-reversed transform order (k_bsk_convert_crt)
        e = with_logn<8, 11>(ctx->logN, e, [&](auto ln) {
            hipLaunchKernelGGL(k_bsk_convert_crt<decltype(ln)::value>, dim3((unsigned)polys), dim3(TP_THREADS), 0, ctx->stream,
                               d_std.p, ctx->bsk, ctx->crt_tw[0], ctx->crt_tw[1], ctx->crt_n_inv[0], ctx->crt_n_inv[1], (int)K1,
                               P.pbs_l);
            return hipGetLastError();
        });
        break;
    case BOOL_GENERIC: // the generic class's layout: [i][r][c][lev][N], bit-reversed transform order (k_bsk_convert_generic)
        e = with_logn<8, 11>(ctx->logN, e, [&](auto ln) {
            hipLaunchKernelGGL(k_bsk_convert_generic<decltype(ln)::value>, dim3((unsigned)polys), dim3(GEN_THREADS), 0, ctx->stream,
                               d_std.p, ctx->bsk, ctx->tw_fwd, ctx->n_inv, (int)K1, P.pbs_l);
            return hipGetLastError();
        });
        break;
    case BOOL_TUNED:
        e = with_tuned(form.shape, form.field, e, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL((k_bsk_convert<typename T::F, T::LOGN>), dim3((unsigned)polys), dim3(64), 0, ctx->stream, d_std.p,
                               ctx->bsk, ctx->tw_fwd, ctx->n_inv, (int)K1, P.pbs_l);
            return hipGetLastError();
        });
        break;
    }
    HIP_TRY(e);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->have_bsk = true;
    return 0;
}

int helm_hip_load_keyswitch_key(helm_hip_ctx *ctx, const uint32_t *ksk, size_t n_words)
{
    if (!ctx || !ksk) return fail(HELM_ERR_INVALID, "null argument");
    const helm_hip_params &P = ctx->P;
    const size_t want = (size_t)P.k * P.N * P.ks_l * ((size_t)P.n + 1);
    if (n_words != want)
        return fail(HELM_ERR_INVALID, "keyswitching key: expected " + std::to_string(want) + " words, got " +
                                          std::to_string(n_words));
    HIP_TRY(hipSetDevice(ctx->device));
    if (!ctx->ksk) HIP_TRY(hipMalloc(&ctx->ksk, want * sizeof(uint32_t)));
    HIP_TRY(hipMemcpyAsync(ctx->ksk, ksk, want * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    // byte planes for the matrix-core keyswitch: ks_l must divide 16 (a lane's 16 fragment bytes hold whole words'
    // digits), the rows must fill 64-row chunks, digits must fit a signed byte (ks_logB <= 7: checked at ctx_create)
    if (P.ks_l == 1 || P.ks_l == 2 || P.ks_l == 4 || P.ks_l == 8) {
        const helm_ks::Planes planes = helm_ks::build_planes(ksk, P.k * P.N, P.ks_l, P.ks_l, P.n);
        if (!planes.bytes.empty()) {
            if (!ctx->ksk_planes) HIP_TRY(hipMalloc(&ctx->ksk_planes, planes.bytes.size()));
            HIP_TRY(hipMemcpy(ctx->ksk_planes, planes.bytes.data(), planes.bytes.size(), hipMemcpyHostToDevice));
            ctx->ks_kchunks = planes.kchunks;
            ctx->ks_ctiles = planes.ctiles;
        }
    }
    ctx->have_ksk = true;
    return 0;
}

int helm_hip_wires_alloc(helm_hip_ctx *ctx, int64_t n_wires, helm_hip_wires **out)
{
    if (!ctx || !out || n_wires <= 0) return fail(HELM_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(ctx->device));
    helm_hip_wires *w = new (std::nothrow) helm_hip_wires();
    if (!w) return fail(HELM_ERR_OOM, "wires");
    w->owner = ctx;
    w->n_wires = n_wires;
    const size_t bytes = (size_t)n_wires * ((size_t)wire_dim(ctx) + 1) * sizeof(uint32_t);
    if (hipMalloc(&w->d, bytes) != hipSuccess) {
        delete w;
        return fail(HELM_ERR_OOM, "wire table of " + std::to_string(bytes) + " bytes");
    }
    HIP_TRY(hipMemsetAsync(w->d, 0, bytes, ctx->stream));
    ctx->child_wires.push_back(w);
    *out = w;
    return 0;
}

int helm_hip_wires_free(helm_hip_ctx *ctx, helm_hip_wires *w)
{
    if (!w) return 0;
    if (!w->owner) { // its context is gone and took the device memory with it
        delete w;
        return 0;
    }
    if (!ctx || w->owner != ctx) return fail(HELM_ERR_STATE, "wire table belongs to another context");
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(w->d);
    ctx->child_wires.erase(std::remove(ctx->child_wires.begin(), ctx->child_wires.end(), w), ctx->child_wires.end());
    delete w;
    return 0;
}

static int check_idx(const helm_hip_wires *w, const int32_t *idx, int64_t count, bool allow_neg)
{
    for (int64_t i = 0; i < count; i++)
        if (idx[i] >= w->n_wires || (idx[i] < 0 && !(allow_neg && idx[i] == -1)))
            return fail(HELM_ERR_INVALID, "wire index " + std::to_string(idx[i]) + " out of range at position " +
                                              std::to_string(i));
    return 0;
}

int helm_hip_wires_upload(helm_hip_ctx *ctx, helm_hip_wires *w, const int32_t *idx, const uint32_t *lwe_host,
                          int64_t count)
{
    if (!ctx || !w || !idx || !lwe_host || count < 0) return fail(HELM_ERR_INVALID, "bad argument");
    if (w->owner != ctx) return fail(HELM_ERR_STATE, "wire table belongs to another context");
    if (count == 0) return 0;
    if (int rc = check_idx(w, idx, count, false)) return rc;
    {
        std::vector<int32_t> sorted(idx, idx + count);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return fail(HELM_ERR_INVALID, "upload names the same wire twice");
    }
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t row = (size_t)wire_dim(ctx) + 1;
    Scratch<uint32_t> d_rows;
    Scratch<int32_t> d_idx;
    HIP_TRY(d_rows.alloc((size_t)count * row));
    HIP_TRY(d_idx.alloc((size_t)count));
    HIP_TRY(hipMemcpyAsync(d_rows.p, lwe_host, (size_t)count * row * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_idx.p, idx, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_scatter_rows, dim3((unsigned)count), dim3(256), 0, ctx->stream, d_rows.p, d_idx.p, w->d, wire_dim(ctx));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int helm_hip_wires_download(helm_hip_ctx *ctx, helm_hip_wires *w, const int32_t *idx, uint32_t *lwe_host, int64_t count)
{
    if (!ctx || !w || !idx || !lwe_host || count < 0) return fail(HELM_ERR_INVALID, "bad argument");
    if (w->owner != ctx) return fail(HELM_ERR_STATE, "wire table belongs to another context");
    if (count == 0) return 0;
    if (int rc = check_idx(w, idx, count, false)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t row = (size_t)wire_dim(ctx) + 1;
    Scratch<uint32_t> d_rows;
    Scratch<int32_t> d_idx;
    HIP_TRY(d_rows.alloc((size_t)count * row));
    HIP_TRY(d_idx.alloc((size_t)count));
    HIP_TRY(hipMemcpyAsync(d_idx.p, idx, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)count), dim3(256), 0, ctx->stream, w->d, d_idx.p, d_rows.p, wire_dim(ctx));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(lwe_host, d_rows.p, (size_t)count * row * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int helm_hip_wires_copy(helm_hip_ctx *ctx, helm_hip_wires *src, const int32_t *src_idx, helm_hip_wires *dst,
                        const int32_t *dst_idx, int64_t count)
{
    if (!ctx || !src || !dst || !src_idx || !dst_idx || count < 0) return fail(HELM_ERR_INVALID, "bad argument");
    if (src->owner != ctx || dst->owner != ctx) return fail(HELM_ERR_STATE, "wire table belongs to another context");
    if (count == 0) return 0;
    if (int rc = check_idx(src, src_idx, count, false)) return rc;
    if (int rc = check_idx(dst, dst_idx, count, false)) return rc;
    {
        std::vector<int32_t> sorted(dst_idx, dst_idx + count);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return fail(HELM_ERR_INVALID, "copy names the same destination wire twice");
        if (src == dst)
            for (int64_t r = 0; r < count; r++)
                if (std::binary_search(sorted.begin(), sorted.end(), src_idx[r]) && src_idx[r] != dst_idx[r])
                    return fail(HELM_ERR_INVALID, "copy within one table: source and destination rows overlap");
    }
    HIP_TRY(hipSetDevice(ctx->device));
    Scratch<int32_t> d_src, d_dst;
    HIP_TRY(d_src.alloc((size_t)count));
    HIP_TRY(d_dst.alloc((size_t)count));
    HIP_TRY(hipMemcpyAsync(d_src.p, src_idx, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_dst.p, dst_idx, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_copy_rows, dim3((unsigned)count), dim3(256), 0, ctx->stream, src->d, d_src.p, dst->d, d_dst.p, wire_dim(ctx));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int helm_hip_wires_set_trivial(helm_hip_ctx *ctx, helm_hip_wires *w, const int32_t *idx, const uint8_t *value,
                               int64_t count)
{
    if (!ctx || !w || !idx || !value || count < 0) return fail(HELM_ERR_INVALID, "bad argument");
    if (w->owner != ctx) return fail(HELM_ERR_STATE, "wire table belongs to another context");
    if (count == 0) return 0;
    if (int rc = check_idx(w, idx, count, false)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    Scratch<int32_t> d_idx;
    Scratch<uint8_t> d_val;
    HIP_TRY(d_idx.alloc((size_t)count));
    HIP_TRY(d_val.alloc((size_t)count));
    HIP_TRY(hipMemcpyAsync(d_idx.p, idx, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_val.p, value, (size_t)count, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_set_trivial, dim3((unsigned)count), dim3(256), 0, ctx->stream, d_idx.p, d_val.p, w->d, wire_dim(ctx));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int helm_hip_wires_device_ptr(helm_hip_ctx *ctx, helm_hip_wires *w, void **dev_ptr, int64_t *n_wires)
{
    if (!ctx || !w || !dev_ptr) return fail(HELM_ERR_INVALID, "bad argument");
    if (w->owner != ctx) return fail(HELM_ERR_STATE, "wire table belongs to another context");
    if (int rc = helm_hip_runtime_guard_("helm_hip_wires_device_ptr")) return rc; // the pointer leaves for the caller's runtime
    *dev_ptr = w->d;
    if (n_wires) *n_wires = w->n_wires;
    return 0;
}

int helm_hip_eval_gate_level(helm_hip_ctx *ctx, helm_hip_wires *w, const int32_t *opcode, const int32_t *in0,
                             const int32_t *in1, const int32_t *in2, const int32_t *out, int64_t count)
{
    if (!ctx || !w || !opcode || !in0 || !in1 || !in2 || !out || count < 0) return fail(HELM_ERR_INVALID, "bad argument");
    if (w->owner != ctx) return fail(HELM_ERR_STATE, "wire table belongs to another context");
    if (count == 0) return 0;
    if (int rc = check_idx(w, in0, count, true)) return rc;
    if (int rc = check_idx(w, in1, count, true)) return rc;
    if (int rc = check_idx(w, in2, count, true)) return rc;
    if (int rc = check_idx(w, out, count, false)) return rc;
    if ((int64_t)count * 16 >= w->n_wires) {
        std::vector<int64_t> owner((size_t)w->n_wires, -1);
        if (int rc = check_level_hazards(in0, in1, in2, out, count, 0, owner, 0)) return rc;
    } else { // a narrow level on a large table: the same check over a compacted row numbering, O(count log count)
        std::vector<int32_t> rows(out, out + count);
        std::sort(rows.begin(), rows.end());
        rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
        if ((int64_t)rows.size() != count)
            return fail(HELM_ERR_INVALID, "two gates of the level write the same wire (write-after-write inside a level)");
        auto compact = [&](const int32_t *src, std::vector<int32_t> &dst) {
            dst.resize((size_t)count);
            for (int64_t g = 0; g < count; g++) {
                auto it = src[g] < 0 ? rows.end() : std::lower_bound(rows.begin(), rows.end(), src[g]);
                dst[(size_t)g] = it != rows.end() && *it == src[g] ? (int32_t)(it - rows.begin()) : -1; // rows nobody writes: no hazard
            }
        };
        std::vector<int32_t> c0, c1, c2, co;
        compact(in0, c0); compact(in1, c1); compact(in2, c2); compact(out, co);
        std::vector<int64_t> owner(rows.size(), -1);
        if (int rc = check_level_hazards(c0.data(), c1.data(), c2.data(), co.data(), count, 0, owner, 0)) {
            // name the caller's wire in the message, not the compacted index
            for (int64_t g = 0; g < count; g++) {
                const int32_t *ins[3] = {c0.data(), c1.data(), c2.data()};
                const int32_t *raw[3] = {in0, in1, in2};
                for (int q = 0; q < 3; q++)
                    if (ins[q][g] >= 0 && owner[(size_t)ins[q][g]] >= 0 && owner[(size_t)ins[q][g]] != g)
                        return fail(HELM_ERR_INVALID, "gate " + std::to_string(g) + " reads wire " + std::to_string(raw[q][g]) +
                                                          ", which gate " + std::to_string(owner[(size_t)ins[q][g]]) +
                                                          " of the same level writes (read-after-write inside a level)");
            }
            return rc;
        }
    }
    LevelPlan pl;
    if (int rc = plan_level(opcode, in0, in1, in2, count, [&](int64_t g) { return out[g]; }, pl)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->d_pbs.ensure(pl.pbs.size()) || ctx->d_ks.ensure(pl.ks.size()) || ctx->d_lin.ensure(pl.lin.size()))
        return fail(HELM_ERR_OOM, "job buffers");
    // the previous level may still be reading the job buffers, and a host-to-device copy from
    // pageable memory is not guaranteed to queue behind it: drain the stream first
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (!pl.pbs.empty())
        HIP_TRY(hipMemcpyAsync(ctx->d_pbs.p, pl.pbs.data(), pl.pbs.size() * sizeof(PbsJob), hipMemcpyHostToDevice, ctx->stream));
    if (!pl.ks.empty())
        HIP_TRY(hipMemcpyAsync(ctx->d_ks.p, pl.ks.data(), pl.ks.size() * sizeof(KsJob), hipMemcpyHostToDevice, ctx->stream));
    if (!pl.lin.empty())
        HIP_TRY(hipMemcpyAsync(ctx->d_lin.p, pl.lin.data(), pl.lin.size() * sizeof(LinJob), hipMemcpyHostToDevice, ctx->stream));
    // pageable-memory async copies return after staging, so `pl` may go out of scope
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return run_level_device(ctx, ctx->d_pbs.p, (int64_t)pl.pbs.size(), ctx->d_ks.p, (int64_t)pl.ks.size(), ctx->d_lin.p,
                            (int64_t)pl.lin.size(), w->d, w->d);
}

int helm_hip_program_create(helm_hip_ctx *ctx, const int32_t *opcode, const int32_t *in0, const int32_t *in1,
                            const int32_t *in2, const int32_t *out, const int64_t *level_offsets, int64_t n_levels,
                            helm_hip_program **prog)
{
    if (!ctx || !opcode || !in0 || !in1 || !in2 || !out || !level_offsets || !prog || n_levels < 0)
        return fail(HELM_ERR_INVALID, "bad argument");
    *prog = nullptr;
    for (int64_t l = 0; l < n_levels; l++)
        if (level_offsets[l + 1] < level_offsets[l]) return fail(HELM_ERR_INVALID, "level_offsets must be non-decreasing");
    if (n_levels > 0 && level_offsets[0] != 0) return fail(HELM_ERR_INVALID, "level_offsets[0] must be 0");
    helm_hip_program *pr = new (std::nothrow) helm_hip_program();
    if (!pr) return fail(HELM_ERR_OOM, "program");
    pr->owner = ctx;
    pr->n_levels = n_levels;
    pr->off.assign(level_offsets, level_offsets + n_levels + 1);
    const int64_t total = n_levels ? level_offsets[n_levels] : 0;
    pr->op.assign(opcode, opcode + total);
    pr->in0.assign(in0, in0 + total);
    pr->in1.assign(in1, in1 + total);
    pr->in2.assign(in2, in2 + total);
    pr->out.assign(out, out + total);
    for (int64_t i = 0; i < total; i++) {
        const int32_t v[4] = {in0[i], in1[i], in2[i], out[i]};
        for (int q = 0; q < 4; q++) {
            if (v[q] < -1 || (q == 3 && v[q] < 0)) {
                delete pr;
                return fail(HELM_ERR_INVALID, "gate " + std::to_string(i) + ": bad wire index " + std::to_string(v[q]));
            }
            pr->max_row = std::max<int64_t>(pr->max_row, v[q]);
        }
    }
    {
        std::vector<int64_t> owner((size_t)(pr->max_row + 1), -1);
        for (int64_t l = 0; l < n_levels; l++) {
            const int64_t b = pr->off[l], cnt = pr->off[l + 1] - b;
            if (int rc = check_level_hazards(in0 + b, in1 + b, in2 + b, out + b, cnt, b, owner, l)) {
                delete pr;
                return rc;
            }
        }
    }
    pr->plans.resize(n_levels);
    std::vector<PbsJob> all_pbs;
    std::vector<KsJob> all_ks;
    std::vector<LinJob> all_lin;
    pr->pbs_off.push_back(0);
    pr->ks_off.push_back(0);
    pr->lin_off.push_back(0);
    for (int64_t l = 0; l < n_levels; l++) {
        const int64_t b = pr->off[l], cnt = pr->off[l + 1] - b;
        const int32_t *o = pr->out.data() + b;
        int rc = plan_level(pr->op.data() + b, pr->in0.data() + b, pr->in1.data() + b, pr->in2.data() + b, cnt,
                            [&](int64_t g) { return o[g]; }, pr->plans[l]);
        if (rc) {
            delete pr;
            return rc;
        }
        all_pbs.insert(all_pbs.end(), pr->plans[l].pbs.begin(), pr->plans[l].pbs.end());
        all_ks.insert(all_ks.end(), pr->plans[l].ks.begin(), pr->plans[l].ks.end());
        all_lin.insert(all_lin.end(), pr->plans[l].lin.begin(), pr->plans[l].lin.end());
        pr->pbs_off.push_back((int64_t)all_pbs.size());
        pr->ks_off.push_back((int64_t)all_ks.size());
        pr->lin_off.push_back((int64_t)all_lin.size());
    }
    const int up = [&]() -> int {
        HIP_TRY(hipSetDevice(ctx->device));
        if (!all_pbs.empty()) {
            HIP_TRY(hipMalloc(&pr->d_pbs, all_pbs.size() * sizeof(PbsJob)));
            HIP_TRY(hipMemcpy(pr->d_pbs, all_pbs.data(), all_pbs.size() * sizeof(PbsJob), hipMemcpyHostToDevice));
            HIP_TRY(hipMalloc(&pr->d_ks, all_ks.size() * sizeof(KsJob)));
            HIP_TRY(hipMemcpy(pr->d_ks, all_ks.data(), all_ks.size() * sizeof(KsJob), hipMemcpyHostToDevice));
        }
        if (!all_lin.empty()) {
            HIP_TRY(hipMalloc(&pr->d_lin, all_lin.size() * sizeof(LinJob)));
            HIP_TRY(hipMemcpy(pr->d_lin, all_lin.data(), all_lin.size() * sizeof(LinJob), hipMemcpyHostToDevice));
        }
        return 0;
    }();
    if (up) { // a half-uploaded program: release what was allocated
        (void)hipFree(pr->d_pbs);
        (void)hipFree(pr->d_ks);
        (void)hipFree(pr->d_lin);
        delete pr;
        return up;
    }
    ctx->child_progs.push_back(pr);
    *prog = pr;
    return 0;
}

int helm_hip_program_destroy(helm_hip_ctx *ctx, helm_hip_program *prog)
{
    if (!prog) return 0;
    if (!prog->owner) {
        delete prog;
        return 0;
    }
    if (!ctx || prog->owner != ctx) return fail(HELM_ERR_STATE, "program belongs to another context");
    ctx->child_progs.erase(std::remove(ctx->child_progs.begin(), ctx->child_progs.end(), prog), ctx->child_progs.end());
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->xchg_stream) (void)hipStreamSynchronize(ctx->xchg_stream);
    (void)hipFree(prog->d_pbs);
    (void)hipFree(prog->d_ks);
    (void)hipFree(prog->d_lin);
    prog->s_pbs.release();
    prog->s_ks.release();
    prog->s_lin.release();
    prog->s_rows.release();
    prog->x_gather.release();
    release_overlap(prog);
    delete prog;
    return 0;
}

// O(1): the index range of a program is established once, at creation (a level call must not
// cost a pass over the whole netlist: 207 levels x millions of gates on a multi-GPU batch)
static int check_program(helm_hip_ctx *ctx, helm_hip_program *prog, helm_hip_wires *w)
{
    if (!ctx || !prog || !w) return fail(HELM_ERR_INVALID, "null argument");
    if (prog->owner != ctx || w->owner != ctx) return fail(HELM_ERR_STATE, "handle belongs to another context");
    if (prog->max_row >= w->n_wires)
        return fail(HELM_ERR_INVALID, "program references wire " + std::to_string(prog->max_row) + " outside the table");
    return 0;
}

int helm_hip_program_run(helm_hip_ctx *ctx, helm_hip_program *prog, helm_hip_wires *w, int64_t level_begin,
                         int64_t level_end)
{
    if (int rc = check_program(ctx, prog, w)) return rc;
    if (level_begin < 0 || level_end > prog->n_levels || level_begin > level_end)
        return fail(HELM_ERR_INVALID, "level range out of bounds");
    HIP_TRY(hipSetDevice(ctx->device));
    for (int64_t l = level_begin; l < level_end; l++) {
        int rc = run_level_device(ctx, prog->d_pbs + prog->pbs_off[l], prog->pbs_off[l + 1] - prog->pbs_off[l],
                                  prog->d_ks + prog->ks_off[l], prog->ks_off[l + 1] - prog->ks_off[l],
                                  prog->d_lin + prog->lin_off[l], prog->lin_off[l + 1] - prog->lin_off[l], w->d, w->d);
        if (rc) return rc;
    }
    return 0;
}

// The cut of a level for `world` ranks: shard_rule.h (by bootstrap weight).
int64_t helm_hip_program_chunk_rows(helm_hip_program *prog, int64_t level, int world)
{
    if (!prog || level < 0 || level >= prog->n_levels || world <= 0) return -1;
    if (prog->sh_world == world && !prog->sh_rows.empty()) return prog->sh_rows[(size_t)level];
    std::vector<int64_t> b((size_t)world + 1);
    return helm_shard::chunk_bounds(prog->op.data() + prog->off[level], prog->off[level + 1] - prog->off[level], world, b.data());
}

int helm_hip_program_chunk_bounds(helm_hip_program *prog, int64_t level, int world, int64_t *bounds)
{
    if (!prog || !bounds || level < 0 || level >= prog->n_levels || world <= 0) return fail(HELM_ERR_INVALID, "bad chunk_bounds arguments");
    helm_shard::chunk_bounds(prog->op.data() + prog->off[level], prog->off[level + 1] - prog->off[level], world, bounds);
    return 0;
}

int64_t helm_hip_program_level_pbs(helm_hip_program *prog, int64_t level)
{
    if (!prog || level < 0 || level >= prog->n_levels) return -1;
    return prog->pbs_off[level + 1] - prog->pbs_off[level];
}

// Per-(rank, world) shard tables: every level's chunk planned and uploaded ONCE, so that the per-level
// calls below only launch kernels (no host planning, no host-device copies, no stream synchronisation
// inside the level loop - the exchange is latency-bound).
static int shard_prepare(helm_hip_ctx *ctx, helm_hip_program *prog, int rank, int world)
{
    if (prog->sh_rank == rank && prog->sh_world == world) return 0;
    if (prog->sh_world != world) {
        prog->sh_rows.clear();
        prog->sh_world = 0;
    }
    std::vector<PbsJob> all_pbs;
    std::vector<KsJob> all_ks;
    std::vector<LinJob> all_lin;
    std::vector<int32_t> all_rows;
    std::vector<int64_t> po{0}, ko{0}, lo{0}, ro{0};
    std::vector<int64_t> bounds((size_t)prog->n_levels * (world + 1)), rows_of((size_t)prog->n_levels);
    LevelPlan pl;
    for (int64_t level = 0; level < prog->n_levels; level++) {
        const int64_t b = prog->off[level], cnt = prog->off[level + 1] - b;
        int64_t *bd = bounds.data() + (size_t)level * (world + 1);
        const int64_t chunk = helm_shard::chunk_bounds(prog->op.data() + b, cnt, world, bd);
        rows_of[(size_t)level] = chunk;
        const int64_t g0 = bd[rank], g1 = bd[rank + 1];
        if (g1 > g0) {
            if (int rc = plan_level(prog->op.data() + b + g0, prog->in0.data() + b + g0, prog->in1.data() + b + g0,
                                    prog->in2.data() + b + g0, g1 - g0, [&](int64_t g) { return (int32_t)g; }, pl))
                return rc;
            all_pbs.insert(all_pbs.end(), pl.pbs.begin(), pl.pbs.end());
            all_ks.insert(all_ks.end(), pl.ks.begin(), pl.ks.end());
            all_lin.insert(all_lin.end(), pl.lin.begin(), pl.lin.end());
        }
        // rank r's slot of the gathered launch holds its chunk's outputs in gate order, then padding rows (skipped)
        for (int r = 0; r < world; r++)
            for (int64_t j = 0; j < chunk; j++)
                all_rows.push_back(bd[r] + j < bd[r + 1] ? prog->out[(size_t)(b + bd[r] + j)] : -1);
        po.push_back((int64_t)all_pbs.size());
        ko.push_back((int64_t)all_ks.size());
        lo.push_back((int64_t)all_lin.size());
        ro.push_back((int64_t)all_rows.size());
    }
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream)); // an earlier (rank, world) table may still be in use
    if (ctx->xchg_stream) HIP_TRY(hipStreamSynchronize(ctx->xchg_stream));
    if (prog->s_pbs.ensure(all_pbs.size()) || prog->s_ks.ensure(all_ks.size()) || prog->s_lin.ensure(all_lin.size()) ||
        prog->s_rows.ensure(all_rows.size()))
        return fail(HELM_ERR_OOM, "shard tables");
    if (!all_pbs.empty()) HIP_TRY(hipMemcpy(prog->s_pbs.p, all_pbs.data(), all_pbs.size() * sizeof(PbsJob), hipMemcpyHostToDevice));
    if (!all_ks.empty()) HIP_TRY(hipMemcpy(prog->s_ks.p, all_ks.data(), all_ks.size() * sizeof(KsJob), hipMemcpyHostToDevice));
    if (!all_lin.empty()) HIP_TRY(hipMemcpy(prog->s_lin.p, all_lin.data(), all_lin.size() * sizeof(LinJob), hipMemcpyHostToDevice));
    if (!all_rows.empty()) HIP_TRY(hipMemcpy(prog->s_rows.p, all_rows.data(), all_rows.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    prog->sh_pbs_off.swap(po);
    prog->sh_ks_off.swap(ko);
    prog->sh_lin_off.swap(lo);
    prog->sh_rows_off.swap(ro);
    prog->sh_bounds.swap(bounds);
    prog->sh_rows.swap(rows_of);
    prog->sh_rank = rank;
    prog->sh_world = world;
    return 0;
}

int helm_hip_program_shard_prepare(helm_hip_ctx *ctx, helm_hip_program *prog, int rank, int world)
{
    if (!ctx || !prog) return fail(HELM_ERR_INVALID, "null argument");
    if (prog->owner != ctx) return fail(HELM_ERR_STATE, "program belongs to another context");
    if (world <= 0 || rank < 0 || rank >= world) return fail(HELM_ERR_INVALID, "bad shard arguments");
    return shard_prepare(ctx, prog, rank, world);
}

int helm_hip_program_run_level_shard(helm_hip_ctx *ctx, helm_hip_program *prog, helm_hip_wires *w, int64_t level,
                                     int rank, int world, void *staging_dev)
{
    if (int rc = check_program(ctx, prog, w)) return rc;
    if (level < 0 || level >= prog->n_levels || world <= 0 || rank < 0 || rank >= world || !staging_dev)
        return fail(HELM_ERR_INVALID, "bad shard arguments");
    if (int rc = shard_prepare(ctx, prog, rank, world)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const int64_t *bd = prog->sh_bounds.data() + (size_t)level * (world + 1);
    const int64_t chunk = prog->sh_rows[(size_t)level], mine = bd[rank + 1] - bd[rank];
    const size_t row = (size_t)wire_dim(ctx) + 1;
    // padding rows of the staging chunk must be defined (they travel through the all-gather)
    if (mine < chunk)
        HIP_TRY(hipMemsetAsync(static_cast<uint32_t *>(staging_dev) + row * (size_t)mine, 0,
                               row * (size_t)(chunk - mine) * sizeof(uint32_t), ctx->stream));
    if (mine == 0) return 0;
    const int64_t pb = prog->sh_pbs_off[level], kb = prog->sh_ks_off[level], lb = prog->sh_lin_off[level];
    return run_level_device(ctx, prog->s_pbs.p + pb, prog->sh_pbs_off[level + 1] - pb, prog->s_ks.p + kb,
                            prog->sh_ks_off[level + 1] - kb, prog->s_lin.p + lb, prog->sh_lin_off[level + 1] - lb, w->d,
                            static_cast<uint32_t *>(staging_dev));
}

static int scatter_level_on(helm_hip_ctx *ctx, helm_hip_program *prog, helm_hip_wires *w, int64_t level, const void *gathered_dev,
                            hipStream_t stream)
{
    const int64_t rb = prog->sh_rows_off[level], rows = prog->sh_rows_off[level + 1] - rb;
    if (rows == 0) return 0;
    hipLaunchKernelGGL(k_scatter_rows, dim3((unsigned)rows), dim3(256), 0, stream, static_cast<const uint32_t *>(gathered_dev),
                       prog->s_rows.p + rb, w->d, wire_dim(ctx));
    HIP_TRY(hipGetLastError());
    return 0;
}

int helm_hip_program_scatter_level(helm_hip_ctx *ctx, helm_hip_program *prog, helm_hip_wires *w, int64_t level,
                                   int world, const void *gathered_dev)
{
    if (int rc = check_program(ctx, prog, w)) return rc;
    if (level < 0 || level >= prog->n_levels || world <= 0 || !gathered_dev)
        return fail(HELM_ERR_INVALID, "bad scatter arguments");
    if (prog->sh_world != world)
        return fail(HELM_ERR_STATE, "scatter_level: run_level_shard / shard_prepare with this world size first");
    HIP_TRY(hipSetDevice(ctx->device));
    return scatter_level_on(ctx, prog, w, level, gathered_dev, ctx->stream);
}

int helm_hip_program_run_sharded(helm_hip_ctx *ctx, helm_hip_program *prog, helm_hip_wires *w, int rank, int world,
                                 int64_t replicate_below, void *stage_dev, void *gather_dev, int64_t capacity_rows,
                                 helm_hip_exchange_fn fn, void *user)
{
    if (int rc = check_program(ctx, prog, w)) return rc;
    if (world <= 0 || rank < 0 || rank >= world) return fail(HELM_ERR_INVALID, "bad shard arguments");
    if ((world > 1 || fn) && (!stage_dev || !gather_dev || !fn || capacity_rows <= 0))
        return fail(HELM_ERR_INVALID, "run_sharded: staging buffers and the exchange callback are needed for world > 1");
    if (fn)
        if (int rc = helm_hip_runtime_guard_("helm_hip_program_run_sharded")) return rc; // the caller's buffers and collective
    if (world > 1 || fn)
        if (int rc = shard_prepare(ctx, prog, rank, world)) return rc;
    for (int64_t l = 0; l < prog->n_levels; l++) {
        if ((world == 1 && !fn) || helm_hip_program_level_pbs(prog, l) <= replicate_below) { // one wave of workgroups absorbs it
            if (int rc = helm_hip_program_run(ctx, prog, w, l, l + 1)) return rc;
            continue;
        }
        const int64_t rows = prog->sh_rows[(size_t)l];
        if (rows > capacity_rows)
            return fail(HELM_ERR_INVALID, "run_sharded: a launch's chunk has " + std::to_string(rows) + " rows, the staging buffer " +
                                              std::to_string(capacity_rows));
        if (int rc = helm_hip_program_run_level_shard(ctx, prog, w, l, rank, world, stage_dev)) return rc;
        if (int rc = fn(user, stage_dev, gather_dev, rows))
            return fail(HELM_ERR_STATE, "run_sharded: the exchange callback failed (" + std::to_string(rc) + ")");
        if (int rc = helm_hip_program_scatter_level(ctx, prog, w, l, world, gather_dev)) return rc;
    }
    return 0;
}

// For every launch the last EARLIER launch that writes one of its input rows (-1: none): what the overlapped exchange
// waits for.  The overlapped schedule needs every row written at most once per pass (a second writer could overtake the
// first one's scatter); netlists with state-writing gates fall back to the in-order exchange.
static void launch_dependencies(helm_hip_program *prog)
{
    if (prog->dep_state != 0) return;
    std::vector<int64_t> producer((size_t)prog->max_row + 1, -1);
    prog->dep.assign((size_t)prog->n_levels, -1);
    prog->dep_state = 1;
    const std::vector<int32_t> *ins[3] = {&prog->in0, &prog->in1, &prog->in2};
    for (int64_t l = 0; l < prog->n_levels; l++) {
        int64_t d = -1;
        for (int64_t g = prog->off[l]; g < prog->off[l + 1]; g++)
            for (auto *in : ins) {
                const int32_t r = (*in)[(size_t)g];
                if (r >= 0) d = std::max(d, producer[(size_t)r]);
            }
        prog->dep[(size_t)l] = d;
        for (int64_t g = prog->off[l]; g < prog->off[l + 1]; g++) {
            int64_t &pr = producer[(size_t)prog->out[(size_t)g]];
            if (pr >= 0) prog->dep_state = -1;
            pr = l;
        }
    }
}

int helm_hip_program_overlap_applies(helm_hip_program *prog)
{
    if (!prog) return fail(HELM_ERR_INVALID, "null program");
    launch_dependencies(prog);
    return prog->dep_state == 1 ? 1 : 0;
}

// The overlapped form of the pass below: launch l's chunk is computed on the context's stream into a gather buffer of a
// ring of three; its all-gather and the scatter into the wire table follow on the context's exchange stream while the
// main stream goes on with launch l + 1.  A launch waits only for the scatter of the launch it depends on (the exchange
// stream runs in order, so everything before that one is in the table too); a ring buffer is reused once the exchange
// stream is through with it.  Replicated launches run on the main stream as before.  Every rank issues the same
// collectives in the same order (the schedule depends on the program alone).
static int run_sharded_comm_overlapped(helm_hip_ctx *ctx, helm_hip_program *prog, helm_hip_wires *w, helm_comm *comm, int rank,
                                       int world, int64_t replicate_below, int64_t cap)
{
    const size_t row = (size_t)wire_dim(ctx) + 1;
    if (!ctx->xchg_stream) HIP_TRY(hipStreamCreateWithFlags(&ctx->xchg_stream, hipStreamNonBlocking));
    for (auto &b : prog->x_ring)
        if (b.ensure((size_t)cap * world * row)) return fail(HELM_ERR_OOM, "gather ring");
    hipStream_t main = ctx->stream, side = ctx->xchg_stream;
    std::vector<int64_t> sharded; // launches exchanged so far, in order; x_done[i] is recorded behind the scatter of sharded[i]
    auto event_of = [&](std::vector<hipEvent_t> &v, size_t i, hipEvent_t *e) -> int {
        while (v.size() <= i) {
            hipEvent_t ev;
            HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            v.push_back(ev);
        }
        *e = v[i];
        return 0;
    };
    int rc = 0;
    size_t waited = 0; // the main stream has already waited for x_done[0 .. waited)
    for (int64_t l = 0; l < prog->n_levels && !rc; l++) {
        const int64_t d = prog->dep[(size_t)l];
        if (d >= 0 && !sharded.empty()) {
            // the latest exchanged launch at or before d
            const size_t i = (size_t)(std::upper_bound(sharded.begin(), sharded.end(), d) - sharded.begin());
            if (i > waited) {
                if (hipStreamWaitEvent(main, prog->x_done[i - 1], 0) != hipSuccess) rc = fail(HELM_ERR_HIP, "hipStreamWaitEvent");
                waited = i;
            }
        }
        if (rc) break;
        if (helm_hip_program_level_pbs(prog, l) <= replicate_below) {
            rc = helm_hip_program_run(ctx, prog, w, l, l + 1);
            continue;
        }
        const size_t k = sharded.size();
        if (k >= 3 && k - 3 >= waited) { // the exchange stream must be through with this ring buffer
            if (hipStreamWaitEvent(main, prog->x_done[k - 3], 0) != hipSuccess) rc = fail(HELM_ERR_HIP, "hipStreamWaitEvent");
            waited = k - 2;
        }
        if (rc) break;
        uint32_t *gather = prog->x_ring[k % 3].p;
        const int64_t rows = prog->sh_rows[(size_t)l];
        uint32_t *slot = gather + (size_t)rank * rows * row;
        if ((rc = helm_hip_program_run_level_shard(ctx, prog, w, l, rank, world, slot))) break;
        hipEvent_t computed, ev;
        if ((rc = event_of(prog->x_comp, k, &computed)) || (rc = event_of(prog->x_done, k, &ev))) break;
        if (hipEventRecord(computed, main) != hipSuccess || hipStreamWaitEvent(side, computed, 0) != hipSuccess) {
            rc = fail(HELM_ERR_HIP, "overlapped exchange: event hand-over");
            break;
        }
        {
            TimedScope t(ctx, &ctx->ev_xchg, side);
            rc = helm_comm_all_gather(comm, slot, gather, (size_t)rows * row * sizeof(uint32_t), side);
        }
        if (rc) break;
        ctx->tacc.exchange_count++;
        ctx->tacc.exchange_bytes += rows * (int64_t)(row * sizeof(uint32_t));
        if ((rc = scatter_level_on(ctx, prog, w, l, gather, side))) break;
        if (hipEventRecord(ev, side) != hipSuccess) rc = fail(HELM_ERR_HIP, "hipEventRecord");
        sharded.push_back(l);
    }
    // whatever follows on the context's stream sees the whole table; on an error nothing is left in flight either
    if (!sharded.empty() && sharded.size() > waited) (void)hipStreamWaitEvent(main, prog->x_done[sharded.size() - 1], 0);
    if (rc) (void)hipStreamSynchronize(side);
    return rc;
}

int helm_hip_program_run_sharded_comm(helm_hip_ctx *ctx, helm_hip_program *prog, helm_hip_wires *w, helm_comm *comm,
                                      int64_t replicate_below, int overlap)
{
    if (int rc = check_program(ctx, prog, w)) return rc;
    if (!comm) return fail(HELM_ERR_INVALID, "run_sharded_comm: null communicator");
    int rank = 0, world = 0, dev = -1;
    if (int rc = helm_comm_info(comm, &rank, &world, &dev, nullptr)) return rc;
    if (dev != ctx->device) return fail(HELM_ERR_STATE, "run_sharded_comm: the communicator lives on another device than the context");
    HIP_TRY(hipSetDevice(ctx->device)); // the gather buffers and the exchange stream below belong to the context's device
    if (int rc = shard_prepare(ctx, prog, rank, world)) return rc;
    const size_t row = (size_t)wire_dim(ctx) + 1;
    int64_t cap = 0;
    for (int64_t l = 0; l < prog->n_levels; l++)
        if (helm_hip_program_level_pbs(prog, l) > replicate_below) cap = std::max(cap, prog->sh_rows[(size_t)l]);
    if (overlap && cap > 0) {
        launch_dependencies(prog);
        if (prog->dep_state == 1) return run_sharded_comm_overlapped(ctx, prog, w, comm, rank, world, replicate_below, cap);
        // a row written twice per pass (state-writing gates): the in-order exchange below
    }
    if (cap > 0 && prog->x_gather.ensure((size_t)cap * world * row)) return fail(HELM_ERR_OOM, "gather buffer");
    for (int64_t l = 0; l < prog->n_levels; l++) {
        if (helm_hip_program_level_pbs(prog, l) <= replicate_below) {
            if (int rc = helm_hip_program_run(ctx, prog, w, l, l + 1)) return rc;
            continue;
        }
        // this rank's chunk goes straight into its slot of the gather buffer: ncclAllGather in place
        const int64_t rows = prog->sh_rows[(size_t)l];
        uint32_t *slot = prog->x_gather.p + (size_t)rank * rows * row;
        if (int rc = helm_hip_program_run_level_shard(ctx, prog, w, l, rank, world, slot)) return rc;
        {
            TimedScope t(ctx, &ctx->ev_xchg);
            if (int rc = helm_comm_all_gather(comm, slot, prog->x_gather.p, (size_t)rows * row * sizeof(uint32_t), ctx->stream)) return rc;
        }
        ctx->tacc.exchange_count++;
        ctx->tacc.exchange_bytes += rows * (int64_t)(row * sizeof(uint32_t));
        if (int rc = helm_hip_program_scatter_level(ctx, prog, w, l, world, prog->x_gather.p)) return rc;
    }
    return 0;
}

int helm_hip_pbs_batch(helm_hip_ctx *ctx, const uint32_t *lwe_in, const uint32_t *test_vectors, int64_t n_tv,
                       const int32_t *tv_index, uint32_t *out_big, int64_t count)
{
    if (!ctx || !lwe_in || !test_vectors || !tv_index || !out_big || count < 0 || n_tv <= 0)
        return fail(HELM_ERR_INVALID, "bad argument");
    if (!ctx->have_bsk) return fail(HELM_ERR_STATE, "bootstrapping key not loaded");
    if (count == 0) return 0;
    const helm_hip_params &P = ctx->P;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t row = (size_t)P.n + 1, brow = (size_t)P.k * P.N + 1;
    std::vector<PbsJob> jobs((size_t)count);
    for (int64_t g = 0; g < count; g++) {
        if (tv_index[g] < 0 || tv_index[g] >= n_tv) return fail(HELM_ERR_INVALID, "tv_index out of range");
        jobs[(size_t)g] = PbsJob{-1, 0, (int32_t)g, -1, -1, tv_index[g]};
    }
    Scratch<uint32_t> d_in, d_tv, d_out;
    Scratch<PbsJob> d_jobs;
    HIP_TRY(d_in.alloc((size_t)count * row));
    HIP_TRY(d_tv.alloc((size_t)n_tv * P.N));
    HIP_TRY(d_out.alloc((size_t)count * brow));
    HIP_TRY(d_jobs.alloc((size_t)count));
    HIP_TRY(hipMemcpyAsync(d_in.p, lwe_in, (size_t)count * row * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_tv.p, test_vectors, (size_t)n_tv * P.N * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_jobs.p, jobs.data(), (size_t)count * sizeof(PbsJob), hipMemcpyHostToDevice, ctx->stream));
    {
        TimedScope t(ctx, &ctx->ev_pbs);
        HIP_TRY(launch_pbs(ctx, d_jobs.p, count, nullptr, d_in.p, d_tv.p, d_out.p));
    }
    ctx->tacc.pbs_launches++;
    ctx->tacc.pbs_count += count;
    HIP_TRY(hipMemcpyAsync(out_big, d_out.p, (size_t)count * brow * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int helm_hip_keyswitch_batch(helm_hip_ctx *ctx, const uint32_t *in_big, uint32_t *out, int64_t count)
{
    if (!ctx || !in_big || !out || count < 0) return fail(HELM_ERR_INVALID, "bad argument");
    if (!ctx->have_ksk) return fail(HELM_ERR_STATE, "keyswitching key not loaded");
    if (count == 0) return 0;
    const helm_hip_params &P = ctx->P;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t row = (size_t)P.n + 1, brow = (size_t)P.k * P.N + 1;
    std::vector<KsJob> jobs((size_t)count);
    for (int64_t g = 0; g < count; g++) jobs[(size_t)g] = KsJob{(int32_t)g, -1, (int32_t)g, 0u};
    Scratch<uint32_t> d_in, d_out;
    Scratch<KsJob> d_jobs;
    HIP_TRY(d_in.alloc((size_t)count * brow));
    HIP_TRY(d_out.alloc((size_t)count * row));
    HIP_TRY(d_jobs.alloc((size_t)count));
    HIP_TRY(hipMemcpyAsync(d_in.p, in_big, (size_t)count * brow * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_jobs.p, jobs.data(), (size_t)count * sizeof(KsJob), hipMemcpyHostToDevice, ctx->stream));
    {
        TimedScope t(ctx, &ctx->ev_ks);
        HIP_TRY(launch_ks(ctx, d_jobs.p, count, d_in.p, d_out.p));
    }
    ctx->tacc.ks_launches++;
    ctx->tacc.ks_count += count;
    HIP_TRY(hipMemcpyAsync(out, d_out.p, (size_t)count * row * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int helm_hip_ntt_roundtrip(helm_hip_ctx *ctx, const uint32_t *poly_in, uint32_t *poly_out, int64_t count)
{
    if (!ctx || !poly_in || !poly_out || count < 0) return fail(HELM_ERR_INVALID, "bad argument");
    if (count == 0) return 0;
    const int N = ctx->P.N;
    HIP_TRY(hipSetDevice(ctx->device));
    Scratch<uint32_t> d_in, d_out;
    HIP_TRY(d_in.alloc((size_t)count * N));
    HIP_TRY(d_out.alloc((size_t)count * N));
    HIP_TRY(hipMemcpyAsync(d_in.p, poly_in, (size_t)count * N * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    const BoolForm &form = ctx->form;
    hipError_t e = hipErrorInvalidValue;
    switch (form.run) {
    case BOOL_CRT:
        e = with_logn<8, 11>(ctx->logN, e, [&](auto ln) {
            hipLaunchKernelGGL(k_ntt_roundtrip_crt<decltype(ln)::value>, dim3((unsigned)count), dim3(TP_THREADS), 0, ctx->stream,
                               d_in.p, d_out.p, ctx->crt_tw[0], ctx->crt_tw[1], ctx->crt_tw[2], ctx->crt_tw[3], ctx->crt_n_inv[0],
                               ctx->crt_n_inv[1], ctx->crt_p0inv);
            return hipGetLastError();
        });
        break;
    case BOOL_GENERIC:
        e = with_logn<8, 11>(ctx->logN, e, [&](auto ln) {
            hipLaunchKernelGGL(k_ntt_roundtrip_generic<decltype(ln)::value>, dim3((unsigned)count), dim3(GEN_THREADS), 0,
                               ctx->stream, d_in.p, d_out.p, ctx->tw_fwd, ctx->tw_inv, ctx->n_inv);
            return hipGetLastError();
        });
        break;
    case BOOL_TUNED:
        e = with_tuned(form.shape, form.field, e, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL((k_ntt_roundtrip<typename T::F, T::LOGN>), dim3((unsigned)count), dim3(64), 0, ctx->stream, d_in.p,
                               d_out.p, ctx->tw_fwd, ctx->tw_inv, ctx->n_inv);
            return hipGetLastError();
        });
        break;
    }
    HIP_TRY(e);
    HIP_TRY(hipMemcpyAsync(poly_out, d_out.p, (size_t)count * N * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int helm_hip_get_clock(helm_hip_ctx *ctx, double *shader_ghz, double *blind_rotation_ms)
{
    if (!ctx || !shader_ghz) return fail(HELM_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    unsigned long long v[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyFromSymbol(v, HIP_SYMBOL(g_clock_probe), sizeof(v)));
    if (v[3] <= v[1] || v[2] <= v[0]) return fail(HELM_ERR_STATE, "no k_pbs launch has run on this device yet");
    *shader_ghz = (double)(v[2] - v[0]) / (double)(v[3] - v[1]) * 0.1; // s_memrealtime ticks at 100 MHz
    if (blind_rotation_ms) *blind_rotation_ms = (double)(v[3] - v[1]) * 1e-5;
    return 0;
}

int helm_hip_timing_enable(helm_hip_ctx *ctx, int enable)
{
    if (!ctx) return fail(HELM_ERR_INVALID, "null ctx");
    ctx->timing = enable != 0;
    return 0;
}

int helm_hip_get_timing(helm_hip_ctx *ctx, helm_hip_timing *out, int reset)
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
    drain(ctx->ev_pbs_main, ctx->tacc.pbs_main_ms);
    drain(ctx->ev_ks, ctx->tacc.ks_ms);
    drain(ctx->ev_lin, ctx->tacc.linear_ms);
    drain(ctx->ev_xchg, ctx->tacc.exchange_ms);
    *out = ctx->tacc;
    if (reset) ctx->tacc = helm_hip_timing{};
    return 0;
}

} // extern "C"
#endif // HELM_HIP_TU == 0
