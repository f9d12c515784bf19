// pbs_frame.h — the frame of a bootstrap kernel, one copy for both engines (helm_hip.hip: 32-bit words, helm_shortint.hip:
// 64-bit words): what stands around the blind-rotation loop of every blind-rotate kernel.
//   modswitch          a torus word -> Z_2N, half-up
//   GateRows, PlainRow where a job's input row comes from (ROW POLICY: Word word(int i, bool is_body) const)
//   switch_row         MS[0..n] <- modswitch of the policy's words, strided
//   lut_rotated        (X^{-b~} lut)[j]: the initial accumulator's body polynomial
//   extract_put, big_row, sample_extract_lds, sample_extract0
//                      the sample extract, from registers or from LDS
//   acc3_store         the negacyclically unrolled u32 copy of an accumulator polynomial (+v, -v, +v)
//   tw_lane_fill, tw_lane_views
//                      the boolean kernels' lane-major LDS twiddle table and its two views
// Everything is __device__ __forceinline__ and holds no barrier: WHO owns which coefficient, WHERE a value lands (register,
// LDS, an accumulator view) and WHEN the workgroup meets stay in the kernel.
#pragma once
#include "../../include/helm_hip.h"
#include "ntt_fp64.h"

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

// ------------------------------------------------------------------------------------
// modulus switch: the closest multiple of 1/2N, ties upwards
// ------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t modswitch(uint32_t x, int log2_2N)
{
    uint32_t r = (x >> (32 - log2_2N - 1)) + 1u;
    return (r >> 1) & ((1u << log2_2N) - 1u);
}
__device__ __forceinline__ uint32_t modswitch(uint64_t x, int log2_2N)
{
    uint32_t r = (uint32_t)(x >> (64 - log2_2N - 1)) + 1u;
    return (r >> 1) & ((1u << log2_2N) - 1u);
}

// ------------------------------------------------------------------------------------
// the boolean engine's job and its input row (PbsJob, gate_lincomb, GateRows, PT_TRUE / PT_FALSE: used by helm_hip.hip
// alone; they stand here because GateRows is the boolean instance of the row policy below and calls gate_lincomb for
// every kernel but k_pbs_tri10, which keeps its own copy - the 64-bit engine's units see them and use none)
// ------------------------------------------------------------------------------------
#define PT_TRUE 0x20000000u  // +1/8, reference src/circuit.rs:29
#define PT_FALSE 0xE0000000u // -1/8, reference src/circuit.rs:33

struct PbsJob {
    int32_t op;    // helm_gate_op, or -1: raw LWE taken from `raw_in`
    int32_t which; // MUX: 0 -> AND(sel, in0) half, 1 -> AND(!sel, in1) half
    int32_t in0, in1, in2;
    int32_t tv;    // test-vector row
};

// Gate linear step, tfhe boolean engine formulas (see oracle/tfhe_oracle.c header).
__device__ __forceinline__ uint32_t gate_lincomb(int op, int which, uint32_t l, uint32_t r, uint32_t c, bool body)
{
    const uint32_t t = body ? PT_TRUE : 0u, f = body ? PT_FALSE : 0u;
    switch (op) {
    case HELM_GATE_AND: return l + r + f;
    case HELM_GATE_OR: return l + r + t;
    case HELM_GATE_NAND: return 0u - (l + r) + t;
    case HELM_GATE_NOR: return 0u - (l + r) + f;
    case HELM_GATE_XOR: return 2u * (l + r + t);
    case HELM_GATE_XNOR: return 2u * (0u - (l + r + t));
    case HELM_GATE_MUX: return which == 0 ? (c + l + f) : (0u - c + r + f);
    // the three-input extensions (helm_hip.h): the sum of three +-1/8 is +-1/8 or +-3/8, its sign their majority; twice
    // the sum is +-2/8 and carries their parity (-6/8 = +2/8).  No constant: the phase is never 0 or 1/2.
    case HELM_GATE_MAJ3: return l + r + c;
    case HELM_GATE_XOR3: return 0u - 2u * (l + r + c);
    case HELM_GATE_XNOR3: return 2u * (l + r + c);
    default: return 0u;
    }
}

// The input row of a PbsJob: the gate's linear combination of up to three wire rows (rows of `row` words), or - the
// constructor that is given `raw_in` - for job.op < 0 row job.in0 of `raw_in` as it is.  Holds a reference: the job must
// outlive the policy object (the kernels' local copy of the job does; the object is a temporary of the switch_row call).
struct GateRows {
    const PbsJob &job;
    const bool raw;
    const uint32_t *a0 = nullptr, *a1 = nullptr, *a2 = nullptr;
    __device__ __forceinline__ GateRows(const PbsJob &job, const uint32_t *wires, size_t row) : job(job), raw(false)
    {
        set_wires(wires, row);
    }
    __device__ __forceinline__ GateRows(const PbsJob &job, const uint32_t *wires, const uint32_t *raw_in, size_t row)
        : job(job), raw(job.op < 0)
    {
        if (raw) a0 = raw_in + row * (size_t)job.in0;
        else set_wires(wires, row);
    }
    __device__ __forceinline__ uint32_t word(int i, bool is_body) const
    {
        uint32_t v;
        if (raw) v = a0[i];
        else v = gate_lincomb(job.op, job.which, a0 ? a0[i] : 0u, a1 ? a1[i] : 0u, a2 ? a2[i] : 0u, is_body);
        return v;
    }

private:
    __device__ __forceinline__ void set_wires(const uint32_t *wires, size_t row)
    {
        if (job.in0 >= 0) a0 = wires + row * (size_t)job.in0;
        if (job.in1 >= 0) a1 = wires + row * (size_t)job.in1;
        if (job.in2 >= 0) a2 = wires + row * (size_t)job.in2;
    }
};

// row `r` of a table of rows of n + 1 words, as it is (the 64-bit engine's small LWE rows)
template <typename W>
struct PlainRow {
    const W *p;
    __device__ __forceinline__ PlainRow(const W *table, int r, int n) : p(table + (size_t)r * ((size_t)n + 1)) {}
    __device__ __forceinline__ W word(int i, bool) const { return p[i]; }
};

// MS[i] <- modswitch(word i of the row), i = first, first + stride, ... <= n (word n is the body)
template <typename Rows>
__device__ __forceinline__ void switch_row(uint16_t *MS, const Rows &rows, int n, int first, int stride, int log2_2N)
{
    for (int i = first; i <= n; i += stride) MS[i] = (uint16_t)modswitch(rows.word(i, i == n), log2_2N);
}

// ------------------------------------------------------------------------------------
// initial accumulator (0, ..., 0, X^{-b~} tv): coefficient j of the body polynomial, bt = b~ in [0, 2N)
// ------------------------------------------------------------------------------------
template <typename W>
__device__ __forceinline__ W lut_rotated(const W *tv, int j, int bt, int N)
{
    const int idx = (j + bt) & (2 * N - 1);
    W v = tv[idx & (N - 1)];
    if (idx >= N) v = (W)0 - v;
    return v;
}

// ------------------------------------------------------------------------------------
// sample extract
// ------------------------------------------------------------------------------------
// Sample extract at coefficient h of the accumulator (A_0 .. A_{k-1}, B): mask word r N + u is A_r[h - u] for u <= h and
// -A_r[N + h - u] for u > h, the body is B[h].  Seen from accumulator coefficient j of polynomial r: it goes to word
// u = (h - j) mod N, with its own sign for j <= h and negated for j > h - a permutation of the row's words for every h, so a
// wave that holds a set of coefficients writes as many words for any h (h = 0: word 0 is A_r[0], word N - j is -A_r[j]).
template <typename W>
__device__ __forceinline__ void extract_put(W *__restrict__ row_r, int N, int h, int j, W v)
{
    row_r[(h - j) & (N - 1)] = j <= h ? v : (W)0 - v;
}

// row `r` of a table of big LWE rows (K N + 1 words)
template <typename W>
__device__ __forceinline__ W *big_row(W *out, size_t r, int K, int N)
{
    return out + r * ((size_t)K * N + 1);
}

// The accumulator lies in LDS, acc[r N + j]: the extract at coefficient h into the row `ob`; threads first, first + stride, ...
template <int LOGN, typename W>
__device__ __forceinline__ void sample_extract_lds(W *ob, const W *acc, int K, int h, int first, int stride)
{
    constexpr int N = 1 << LOGN;
    for (int idx = first; idx < K * N; idx += stride) {
        const int r = idx >> LOGN, j = idx & (N - 1);
        extract_put(ob + (size_t)r * N, N, h, j, acc[idx]);
    }
    if (first == 0) ob[(size_t)K * N] = acc[(size_t)K * N + h]; // body = B[h]
}

// The boolean engine's extract (coefficient 0) into row jix of out_big from registers: this wave holds CNT coefficients of
// polynomial r with sign SGN, regs[e] = SGN * A_r[j0 + 64 e]; the lane `body` of the wave r = K (whose regs[0] is
// coefficient 0) writes the body.  (Own copies: k_pbs_tri10 keeps its extract - profiles/README.md r27 - and k_pbs_generic
// and k_pbs_crt, whose accumulator lies in LDS, keep a loop that walks the output words, so a wave's stores are consecutive.)
template <int K, int N, int SGN, int CNT>
__device__ __forceinline__ void sample_extract0(uint32_t *out_big, size_t jix, int r, bool body,
                                                const uint32_t (&regs)[CNT], int j0)
{
    static_assert(SGN == 1 || SGN == -1, "a sign");
    uint32_t *ob = big_row(out_big, jix, K, N);
    if (r < K) {
#pragma unroll
        for (int e = 0; e < CNT; e++) extract_put(ob + r * N, N, 0, j0 + 64 * e, SGN < 0 ? 0u - regs[e] : regs[e]);
    } else if (body) {
        ob[K * N] = SGN < 0 ? 0u - regs[0] : regs[0]; // body = B[0]
    }
}

// ------------------------------------------------------------------------------------
// The u32 copy of an accumulator polynomial, unrolled negacyclically over 3N - 64 entries so that the rotated read of slot e
// is one address register + 256 e bytes, sign included: aw[j] = v, aw[j + N] = -v, aw[j + 2N] = v (j < N - 64; THIRD = false:
// the compact form, 2N entries), from this lane's E coefficients regs[e] = +-A[j = 64 e + lane] (NEG: the registers hold
// -A); aw = the copy + lane.
// ------------------------------------------------------------------------------------
template <int N, int E, bool NEG, bool THIRD>
__device__ __forceinline__ void acc3_store(uint32_t *aw, const uint32_t (&regs)[E])
{
#pragma unroll
    for (int e = 0; e < E; e++) {
        const uint32_t v = NEG ? 0u - regs[e] : regs[e], nv = NEG ? regs[e] : 0u - regs[e];
        aw[64 * e] = v;
        aw[64 * e + N] = nv;
        if (THIRD && e < E - 1) aw[64 * e + 2 * N] = v;
    }
}

// ------------------------------------------------------------------------------------
// the lane-major LDS table of forward twiddles (ntt_fp64.h tw_lane_index) and its views
// ------------------------------------------------------------------------------------
// rows first, first + stride, ... < rows of the table, one lane each
template <int LOGN>
__device__ __forceinline__ void tw_lane_fill(double *TW, const double *tw_fwd, int first, int stride, int rows, int lane)
{
    for (int r = first; r < rows; r += stride) TW[r * 64 + lane] = tw_fwd[helm::tw_lane_index<LOGN>(r, lane)];
}

// the forward view reads the table at its lane, the inverse view mirrored; block A's lane-uniform twiddles of both
template <typename TWF, typename TWI>
__device__ __forceinline__ void tw_lane_views(TWF &twf0, TWI &twi, const double *TW, const double *tw_fwd, int lane)
{
    twf0.base = TW + lane;
    twi.base = TW + (63 - lane);
    twf0.fill_uniform(tw_fwd);
    twi.fill_uniform(tw_fwd);
}
// (The two-field table of k_pbs64 and k_pbs64k is filled in those kernels: a shared helper with the same text moved the
// allocation of k_pbs64<Pbs64Cfg<10, 3>, 2> - 256 registers, AGPRs 30 -> 32 - profiles/README.md r27.)
