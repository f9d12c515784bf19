// keyswitch.h — the LWE keyswitch, one copy for both engines (helm_hip.hip: 32-bit words, helm_shortint.hip: 64-bit words):
//   out[c] = (c == n ? body : 0) - sum_t sum_j digit_j(in[t]) * KSK[t][j][c]          (mod 2^32 / 2^64)
// Two forms.  The vector-ALU form (vector_body) decomposes the rows of four jobs once into LDS and walks the key column by
// column; the matrix-core form decomposes once per job into A fragments (digits_body) and multiplies them with the key's
// byte planes (product_body; build_planes lays them out at key load).  Both are integer arithmetic and bit-identical.
//
// A kernel is a thin __global__ wrapper over a body, instantiated for a ROW POLICY - where a job's input words come from
// and where its result goes:
//   struct Rows {
//       using Job = ...; using Word = uint32_t or uint64_t;
//       Rows(const Job &, const Word *src, size_t row);   // the job's view of the input rows of `row` = kN + 1 words
//       Word word(int t) const;                           // input word t < kN
//       Word body(int kN) const;                          // the body word
//       static int out_row(const Job &, int g);           // the output row of job g
//   };
// Three exist: the boolean engine's KsRows (KsJob: one big row or the sum of two, a constant on the body) and GateKsRows
// (PbsJob: the gate's linear combination of up to three wire rows, job g to row g), the 64-bit engine's Ks64Rows (Ks64Job).
// The host side (launch) is one launcher over an ENGINE TRAIT, which states what really differs between the engines - see
// KsEngine32 in helm_hip.hip and KsEngine64 in helm_shortint.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>
#include <utility>
#include <vector>

// the 32-bit signed decomposition (helm_hip.hip, shared with its blind-rotate kernels' decompose_step)
template <int L> __device__ __forceinline__ void decompose(uint32_t x, int logB, int (&dig)[L]);

namespace helm_ks {

typedef int v4i __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------
// Signed gadget decomposition of the closest representable value (tfhe's SignedDecomposer), dig[0] the most significant
// level.  L and logB are compile-time / uniform.
template <int L> __device__ __forceinline__ void ks_decompose(uint32_t x, int logB, int (&dig)[L]) { decompose<L>(x, logB, dig); }

template <int L> __device__ __forceinline__ void ks_decompose(uint64_t x, int logB, int (&dig)[L])
{
    const int rep = logB * L;
    const uint64_t mask = (1ull << logB) - 1ull;
    uint64_t state = (x + (1ull << (63 - rep))) >> (64 - rep);
#pragma unroll
    for (int lev = L - 1; lev >= 0; lev--) {
        const uint64_t d = state & mask;
        state >>= logB;
        const uint64_t carry = (((d - 1ull) | state) & d) >> (logB - 1);
        state += carry;
        dig[lev] = (int)(uint32_t)d - (int)((uint32_t)carry << logB);
    }
}

__device__ __forceinline__ void ks_atomic_add(uint32_t *dst, uint32_t v) { atomicAdd(dst, v); }
__device__ __forceinline__ void ks_atomic_add(uint64_t *dst, uint64_t v)
{
    atomicAdd(reinterpret_cast<unsigned long long *>(dst), (unsigned long long)v);
}

// Vector-ALU form.  Grid (ceil(jobs / 4), column chunks of 256, slices); 256 threads; one output column per thread, FOUR
// jobs per workgroup so that every key word fetched (from L2 / Infinity Cache: the key is shared by all jobs) feeds four
// multiply-adds.  The digits of the four jobs are decomposed once into LDS, packed as 4 x int8 per word (one broadcast
// ds_read_b32 per key word).  blockIdx.z selects a slice of t_chunk input coefficients (narrow launches: the kN * KSL key
// rows are split over several workgroups whose partial sums meet in `out` by atomic add - wrapping integer adds, any
// order; the rows are zeroed beforehand).  gridDim.z == 1: plain stores.
template <int KSL, typename R>
__device__ __forceinline__ void vector_body(const typename R::Job *jobs, const typename R::Word *src,
                                            const typename R::Word *ksk, typename R::Word *out, int n, int kN, int logB,
                                            int count, int t_chunk)
{
    using W = typename R::Word;
    using SW = typename std::make_signed<W>::type;
    constexpr int G = 4;
    constexpr int UNROLL = sizeof(W) == 4 ? 8 : 4;
    extern __shared__ __align__(16) unsigned char smem[];
    uint32_t *DIG = reinterpret_cast<uint32_t *>(smem); // [t_chunk * KSL] words, byte g = digit of job g
    const int g0 = blockIdx.x * G;
    const int ng = min(G, count - g0);
    const int t0 = blockIdx.z * t_chunk, t1 = min(kN, t0 + t_chunk);
    typename R::Job job[G];
#pragma unroll
    for (int g = 0; g < G; g++) job[g] = jobs[g0 + (g < ng ? g : 0)];
    const size_t brow = (size_t)kN + 1;
    for (int t = t0 + threadIdx.x; t < t1; t += 256) {
        uint32_t packed[KSL];
#pragma unroll
        for (int j = 0; j < KSL; j++) packed[j] = 0;
#pragma unroll
        for (int g = 0; g < G; g++) {
            if (g < ng) {
                int dig[KSL];
                ks_decompose<KSL>(R(job[g], src, brow).word(t), logB, dig);
#pragma unroll
                for (int j = 0; j < KSL; j++) packed[j] |= ((uint32_t)dig[j] & 0xFFu) << (8 * g);
            }
        }
#pragma unroll
        for (int j = 0; j < KSL; j++) DIG[(t - t0) * KSL + j] = packed[j];
    }
    __syncthreads();
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c > n) return;
    const size_t krow = (size_t)n + 1;
    W acc[G] = {0, 0, 0, 0};
    const W *kp = ksk + (size_t)t0 * KSL * krow + c;
    const int rows = (t1 - t0) * KSL;
#pragma unroll UNROLL
    for (int r = 0; r < rows; r++) {
        const W w = kp[(size_t)r * krow];
        const uint32_t pk = DIG[r];
#pragma unroll
        for (int g = 0; g < G; g++) acc[g] += (W)(SW)(int32_t)__builtin_amdgcn_sbfe(pk, 8 * g, 8) * w;
    }
    const bool with_body = c == n && blockIdx.z == 0, one_slice = gridDim.z == 1;
#pragma unroll
    for (int g = 0; g < G; g++) {
        if (g < ng) {
            const W body = with_body ? R(job[g], src, brow).body(kN) : (W)0;
            W *dst = out + krow * (size_t)R::out_row(job[g], g0 + g) + c;
            if (one_slice) *dst = body - acc[g];
            else ks_atomic_add(dst, body - acc[g]);
        }
    }
}

// Matrix-core form: the keyswitch of a batch is a GEMM
//   out[g][c] = body_g [c == n] - sum_r D[g][r] * K[r][c],  r = t * LP + level
// with D the signed digits (|d| <= 2^(logB-1) <= 64: int8) of the jobs' input words and K the key.  K is split into its
// sizeof(Word) bytes, each recentred to a signed byte K_b - 128 (v_mfma_i32_16x16x64_i8 is signed x signed):
//   sum_r d K = sum_b 2^(8b) sum_r d (K_b - 128)  +  0x80..80 * sum_r d
// - one int8 GEMM per byte plane with exact int32 accumulators and a per-job correction.  The level count is padded to
// LP in {1, 2, 4, 8} (a lane's 16 fragment bytes hold whole words' digits; padded levels carry zero digits).
//
// digits_body: one workgroup per padded job index (g >= count: an all-zero row) decomposes its row once and writes D in
// A-fragment order, the digit sum and the body word.
// fragment (tile, kc): 64 lanes x 16 bytes; lane = (k-quarter << 4 | row or column), byte j: k = 64 kc + 16 kq + j
template <int KSL, int LP, typename R>
__device__ __forceinline__ void digits_body(const typename R::Job *jobs, const typename R::Word *src, int8_t *dig,
                                            int32_t *dsum, typename R::Word *body, int kN, int logB, int count, int kchunks)
{
    using W = typename R::Word;
    const int g = blockIdx.x;
    __shared__ int red[256];
    int local = 0;
    const size_t brow = (size_t)kN + 1;
    const bool live = g < count;
    typename R::Job job{};
    if (live) job = jobs[g];
    const R rows(job, src, brow);
    int8_t *tile = dig + (size_t)(g >> 4) * kchunks * 1024;
    for (int t = threadIdx.x; t < kN; t += 256) {
        int d[LP];
#pragma unroll
        for (int j = 0; j < LP; j++) d[j] = 0;
        if (live) {
            int lv[KSL];
            ks_decompose<KSL>(rows.word(t), logB, lv);
#pragma unroll
            for (int j = 0; j < KSL; j++) d[j] = lv[j];
        }
        const int r0 = t * LP, kc = r0 >> 6, kq = (r0 & 63) >> 4, j0 = r0 & 15;
        int8_t *dst = tile + ((size_t)kc * 64 + (kq << 4 | (g & 15))) * 16 + j0;
#pragma unroll
        for (int j = 0; j < LP; j++) {
            dst[j] = (int8_t)d[j];
            local += d[j];
        }
    }
    red[threadIdx.x] = local;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        dsum[g] = red[0];
        body[g] = live ? rows.body(kN) : (W)0;
    }
}

// product_body: one wave = 64 jobs (four tiles of 16) x CT column tiles of 16 x sizeof(Word) byte planes; the job tiles of
// a wave reuse every B fragment (1 KiB, coalesced) four times.  With CT > 1 a wave past the last column tile repeats it
// and discards the result.
template <int CT, typename R>
__device__ __forceinline__ void product_body(const typename R::Job *jobs, const int8_t *dig, const int32_t *dsum,
                                             const typename R::Word *body, const int8_t *kplanes, typename R::Word *out,
                                             int n, int count, int kchunks, int ctiles)
{
    using W = typename R::Word;
    using SW = typename std::make_signed<W>::type;
    constexpr int GT = 4, NB = sizeof(W);
    const int lane = threadIdx.x;
    const int gt0 = blockIdx.x * GT, ct0 = blockIdx.y * CT;
    const v4i *A = reinterpret_cast<const v4i *>(dig) + (size_t)gt0 * kchunks * 64 + lane;
    const v4i *B = reinterpret_cast<const v4i *>(kplanes) + lane;
    const size_t plane = (size_t)ctiles * kchunks * 64; // fragments of one byte plane, in v4i units
    v4i acc[GT][CT][NB];
#pragma unroll
    for (int a = 0; a < GT; a++)
#pragma unroll
        for (int c = 0; c < CT; c++)
#pragma unroll
            for (int b = 0; b < NB; b++) acc[a][c][b] = v4i{0, 0, 0, 0};
    for (int kc = 0; kc < kchunks; kc++) {
        v4i fa[GT], fb[CT][NB];
#pragma unroll
        for (int a = 0; a < GT; a++) fa[a] = A[((size_t)a * kchunks + kc) * 64];
#pragma unroll
        for (int c = 0; c < CT; c++)
#pragma unroll
            for (int b = 0; b < NB; b++) {
                const int ct = (CT == 1 || ct0 + c < ctiles) ? ct0 + c : ctiles - 1;
                fb[c][b] = B[(size_t)b * plane + ((size_t)ct * kchunks + kc) * 64];
            }
#pragma unroll
        for (int a = 0; a < GT; a++)
#pragma unroll
            for (int c = 0; c < CT; c++)
#pragma unroll
                for (int b = 0; b < NB; b++)
                    acc[a][c][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[a], fb[c][b], acc[a][c][b], 0, 0, 0);
    }
    // C/D map: column = lane & 15, row = (lane >> 4) * 4 + reg
    const size_t krow = (size_t)n + 1;
#pragma unroll
    for (int a = 0; a < GT; a++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int g = (gt0 + a) * 16 + (lane >> 4) * 4 + reg;
            if (g >= count) continue;
            const W corr = (W)0x8080808080808080ull * (W)(SW)dsum[g];
            W *dst = out + krow * (size_t)R::out_row(jobs[g], g);
#pragma unroll
            for (int c = 0; c < CT; c++) {
                const int col = (ct0 + c) * 16 + (lane & 15);
                if ((CT > 1 && ct0 + c >= ctiles) || col > n) continue;
                W s = corr;
#pragma unroll
                for (int b = 0; b < NB; b++) s += (W)(SW)acc[a][c][b][reg] << (8 * b);
                dst[col] = (col == n ? body[g] : (W)0) - s;
            }
        }
}

// ------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------
// A keyswitching key on the device: in_dim input words (+ body) -> out_dim mask words + body.
template <typename W> struct Key {
    const W *key = nullptr;         // [in_dim][l][out_dim+1]
    const int8_t *planes = nullptr; // byte planes for the matrix-core kernel, or null
    int in_dim = 0, out_dim = 0, l = 0, logB = 0, kchunks = 0, ctiles = 0;
};

// The key's byte planes in B-fragment order, [plane sizeof(W)][column tile][k chunk][lane 64][16], row r = t * LP + level;
// padding rows and columns hold -128 (they meet zero digits, or are discarded).  Empty when the in_dim * LP rows do not
// fill 64-row chunks.
struct Planes {
    std::vector<int8_t> bytes;
    int kchunks = 0, ctiles = 0;
};
template <typename W> Planes build_planes(const W *key, int in_dim, int ks_l, int LP, int n)
{
    Planes P;
    const int R = in_dim * LP;
    if (R % 64 != 0) return P;
    const int kchunks = R / 64, ctiles = (n + 1 + 15) / 16;
    const size_t frag_per_plane = (size_t)ctiles * kchunks * 64;
    P.bytes.assign(sizeof(W) * frag_per_plane * 16, (int8_t)-128);
    const size_t krow = (size_t)n + 1;
    for (int ct = 0; ct < ctiles; ct++)
        for (int kc = 0; kc < kchunks; kc++)
            for (int lane = 0; lane < 64; lane++) {
                const int c = ct * 16 + (lane & 15);
                if (c > n) continue;
                for (int j = 0; j < 16; j++) {
                    const int r = kc * 64 + 16 * (lane >> 4) + j, t = r / LP, lev = r % LP;
                    if (lev >= ks_l) continue;
                    const W w = key[((size_t)t * ks_l + lev) * krow + c];
                    for (int b = 0; b < (int)sizeof(W); b++)
                        P.bytes[((size_t)b * frag_per_plane + ((size_t)ct * kchunks + kc) * 64 + lane) * 16 + j] =
                            (int8_t)((int)((w >> (8 * b)) & 255u) - 128);
                }
            }
    P.kchunks = kchunks;
    P.ctiles = ctiles;
    return P;
}

// The vector-ALU launch of `count` jobs: four jobs and 256 columns per workgroup; narrow launches split the key rows until
// ~2 workgroups per CU exist (at most 16 slices of at least 64 input words), and wherever one slice's digits would not fit LDS.
struct Geometry {
    dim3 grid;
    int slices, t_chunk;
    size_t lds;
};
inline Geometry vector_geometry(int64_t count, int n, int kN, int ks_l, int n_cus)
{
    const unsigned gx = (unsigned)((count + 3) / 4), gy = (unsigned)((n + 1 + 255) / 256);
    int slices = 1;
    while (slices < 16 && (int64_t)gx * gy * slices < 2 * (int64_t)n_cus && kN / (slices * 2) >= 64) slices *= 2;
    // ... and at least as many as keep a slice's digit buffer within the 160 KiB of LDS a workgroup can have.  Unsliced it is
    // kN x ks_l x 4 B: at most 128 KiB for kN <= 4096 and ks_l <= 8, so every shape with kN <= 4096 keeps the grid clause's
    // geometry and this clause fires only on wide vector-ALU batches (one slice by the grid clause) beyond it: the 64-bit
    // engine's kN = 8192 with ks_l >= 6, and the boolean engine's kN >= 6912 with ks_l = 6 and kN >= 5376 with ks_l = 8 (there
    // only under HELM_HIP_KS_MFMA=0: ks_l = 8 has byte planes).  A slice of exactly 160 KiB (kN x ks_l = 40,960) goes out whole.
    // tests/ks_edges.py restates this function; tests/test_ks_geometry.py holds the two together.
    while ((size_t)((kN + slices - 1) / slices) * ks_l * sizeof(uint32_t) > (size_t)160 * 1024) slices *= 2;
    const int t_chunk = (kN + slices - 1) / slices;
    return Geometry{dim3(gx, gy, (unsigned)slices), slices, t_chunk, (size_t)t_chunk * ks_l * sizeof(uint32_t)};
}

// f(std::integral_constant<int, LV>) for the LV of the list that equals ks_l; false when none does
template <typename F, int... LV> bool for_level(int ks_l, std::integer_sequence<int, LV...>, F &&f)
{
    return ((ks_l == LV && (f(std::integral_constant<int, LV>{}), true)) || ...);
}

// One keyswitch launch: `jobs` read `src`, job g writes a row of `out`.  digits_of(lv) / vector_of(lv) name the row
// policy's kernels for KSL = lv(); out_jobs is the job list the product kernel takes its output rows from.  The engine
// trait E states what differs between the engines:
//   Word, Ctx (with stream, n_cus, and the scratch d_ksdig / d_ksdsum / d_ksbody), OutJob, Where
//   VectorLevels, DigitLevels      the KSL the engine instantiates its kernels for
//   padded_levels(l)               LP
//   CT, product_kernel()           column tiles per wave of its product kernel
//   matrix_path(ctx, K, count)     which form a launch takes
//   zero_rows(...)                 clears the output rows before a sliced launch
//   allow_lds<Tag>(ctx, kernel)    raises the vector kernel's dynamic-LDS limit where the engine's shapes need it
template <typename E, typename Job, typename DigitsOf, typename VectorOf>
hipError_t launch(typename E::Ctx *ctx, const Key<typename E::Word> &K, const Job *jobs, const typename E::OutJob *out_jobs,
                  int64_t count, const typename E::Word *src, typename E::Word *out, typename E::Where where,
                  DigitsOf digits_of, VectorOf vector_of)
{
    hipError_t e;
    if (E::matrix_path(ctx, K, count)) {
        // digits once per job, then the int8 GEMM over the key's byte planes
        const int64_t padded = (count + 63) / 64 * 64;
        if (ctx->d_ksdig.ensure((size_t)padded * K.in_dim * E::padded_levels(K.l)) || ctx->d_ksdsum.ensure((size_t)padded) ||
            ctx->d_ksbody.ensure((size_t)padded))
            return hipErrorOutOfMemory;
        if (!for_level(K.l, typename E::DigitLevels{}, [&](auto lv) {
                hipLaunchKernelGGL(digits_of(lv), dim3((unsigned)padded), dim3(256), 0, ctx->stream, jobs, src, ctx->d_ksdig.p,
                                   ctx->d_ksdsum.p, ctx->d_ksbody.p, K.in_dim, K.logB, (int)count, K.kchunks);
            }))
            return hipErrorInvalidValue;
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(E::product_kernel(), dim3((unsigned)(padded / 64), (unsigned)((K.ctiles + E::CT - 1) / E::CT)),
                           dim3(64), 0, ctx->stream, out_jobs, ctx->d_ksdig.p, ctx->d_ksdsum.p, ctx->d_ksbody.p, K.planes, out,
                           K.out_dim, (int)count, K.kchunks, K.ctiles);
        return hipGetLastError();
    }
    const Geometry geo = vector_geometry(count, K.out_dim, K.in_dim, K.l, ctx->n_cus);
    if (geo.slices > 1 && (e = E::zero_rows(ctx, out_jobs, where, out, count, K.out_dim)) != hipSuccess) return e;
    e = hipErrorInvalidValue;
    for_level(K.l, typename E::VectorLevels{}, [&](auto lv) {
        auto kernel = vector_of(lv);
        // the tag makes allow_lds's once-per-device flag one per kernel: VectorOf is the caller's own lambda type (one per
        // row policy - pass no functor shared between policies), lv the level
        e = E::template allow_lds<std::pair<VectorOf, decltype(lv)>>(ctx, reinterpret_cast<const void *>(kernel));
        if (e != hipSuccess) return;
        hipLaunchKernelGGL(kernel, geo.grid, dim3(256), geo.lds, ctx->stream, jobs, src, K.key, out, K.out_dim, K.in_dim, K.logB,
                           (int)count, geo.t_chunk);
        e = hipGetLastError();
    });
    return e;
}

} // namespace helm_ks
