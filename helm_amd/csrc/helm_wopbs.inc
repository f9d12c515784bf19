// helm_wopbs.inc — the WoP-PBS wide-LUT path on gfx950 (include/helm_wopbs.h): bit extraction, circuit bootstrap,
// vertical packing.  Included at the end of helm_shortint.hip: every bootstrap here is k_pbs64 (the constant
// accumulators of bit extraction and circuit bootstrap are ordinary look-up-table rows; the blind rotation and
// the CMUX tree of vertical packing are its MODE 1 / MODE 2 with a per-gate key), every LWE keyswitch is
// k_keyswitch64 / k_ks64_mfma with another key.  New here: the private functional packing keyswitch (an LWE ->
// GLWE keyswitch with 15-bit digits and 4,096 output words) and the row arithmetic between the stages.
//
// Replaces tfhe::integer::wopbs::WopbsKey::{keyswitch_to_wopbs_params, wopbs, keyswitch_to_pbs_params} as HELM's
// high_precision_lut() calls them (reference src/gates.rs:787-815).  There is no CPU fallback.
#include "../../include/helm_wopbs.h"

namespace {

struct PfJob {
    int32_t in_row;  // row of k*N+1 words (mask and body are both inputs)
    int32_t out_row; // row of (k+1)*N words
};

// dst[g] = ca * a[arow ? arow[g] : g] + cb * b[g]   (+ add[g % add_period] on the body), rows of dim+1 words
__global__ __launch_bounds__(256) void k_wop_axpy(uint64_t *__restrict__ dst, const int32_t *__restrict__ drow,
                                                  const uint64_t *__restrict__ a, const int32_t *__restrict__ arow,
                                                  uint64_t ca, const uint64_t *__restrict__ b, uint64_t cb,
                                                  const uint64_t *__restrict__ add, int add_period, int dim)
{
    const size_t row = (size_t)dim + 1;
    const int g = blockIdx.x;
    const uint64_t *pa = a + row * (size_t)(arow ? arow[g] : g);
    const uint64_t *pb = b ? b + row * (size_t)g : nullptr;
    uint64_t *pd = dst + row * (size_t)(drow ? drow[g] : g);
    for (int i = threadIdx.x; i <= dim; i += 256) {
        uint64_t v = ca * pa[i];
        if (pb) v += cb * pb[i];
        if (add && i == dim) v += add[g % add_period];
        pd[i] = v;
    }
}

// trivial GLWE rows from table polynomials: row q (of (k+1) N words) = (0, ..., 0, table words [q N, (q+1) N))
__global__ __launch_bounds__(256) void k_wop_trivial_glwe(const uint64_t *__restrict__ tables, uint64_t *__restrict__ glwe,
                                                          int K, int N)
{
    const size_t q = blockIdx.x;
    uint64_t *dst = glwe + q * (size_t)(K + 1) * N;
    for (int i = threadIdx.x; i < (K + 1) * N; i += 256) dst[i] = i < K * N ? 0ull : tables[q * N + (i - K * N)];
}

// ------------------------------------------------------------------------------------
// k_pfpks64: private functional packing keyswitch, four ciphertexts per key pass.
//   glwe[c] = - sum_{t <= in_dim} sum_j digit_j(in[t]) * key[t][j][c]
// Grid (ceil(jobs/4), column chunks of 256, slices of the input words); digits as int32 in LDS; with more than
// one slice the partial sums meet in `out` (zeroed beforehand) by 64-bit atomic add.
// ------------------------------------------------------------------------------------
template <int L>
__global__ __launch_bounds__(256) void k_pfpks64(const PfJob *__restrict__ jobs, const uint64_t *__restrict__ big,
                                                 const uint64_t *__restrict__ key, uint64_t *__restrict__ out,
                                                 int in_words, int glwe_words, int logB, int count, int t_chunk)
{
    constexpr int GN = 4;
    extern __shared__ __align__(16) unsigned char smem[];
    int32_t *DIG = reinterpret_cast<int32_t *>(smem); // [t_chunk * L][GN]
    const int g0 = blockIdx.x * GN;
    const int ng = min(GN, count - g0);
    const int t0 = blockIdx.z * t_chunk, t1 = min(in_words, t0 + t_chunk);
    PfJob job[GN];
#pragma unroll
    for (int g = 0; g < GN; g++) job[g] = jobs[g0 + (g < ng ? g : 0)];
    for (int t = t0 + threadIdx.x; t < t1; t += 256) {
#pragma unroll
        for (int g = 0; g < GN; g++) {
            int d[L];
#pragma unroll
            for (int j = 0; j < L; j++) d[j] = 0;
            if (g < ng) helm_ks::ks_decompose<L>(big[(size_t)in_words * (size_t)job[g].in_row + t], logB, d);
#pragma unroll
            for (int j = 0; j < L; j++) DIG[((t - t0) * L + j) * GN + g] = d[j];
        }
    }
    __syncthreads();
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= glwe_words) return;
    uint64_t acc[GN] = {0, 0, 0, 0};
    const uint64_t *kp = key + (size_t)t0 * L * glwe_words + c;
    const int rows = (t1 - t0) * L;
    const int4 *dig4 = reinterpret_cast<const int4 *>(DIG);
#pragma unroll 4
    for (int r = 0; r < rows; r++) {
        const uint64_t kw = kp[(size_t)r * glwe_words];
        const int4 d = dig4[r];
        acc[0] += (uint64_t)(int64_t)d.x * kw;
        acc[1] += (uint64_t)(int64_t)d.y * kw;
        acc[2] += (uint64_t)(int64_t)d.z * kw;
        acc[3] += (uint64_t)(int64_t)d.w * kw;
    }
#pragma unroll
    for (int g = 0; g < GN; g++) {
        if (g < ng) {
            uint64_t *dst = out + (size_t)glwe_words * (size_t)job[g].out_row + c;
            if (gridDim.z == 1) *dst = 0ull - acc[g];
            else atomicAdd(reinterpret_cast<unsigned long long *>(dst), (unsigned long long)(0ull - acc[g]));
        }
    }
}


// ------------------------------------------------------------------------------------
// The packing keyswitch on the matrix cores (k_ks64_mfma of helm_shortint.hip does the products).  A 15-bit digit
// d splits exactly into two signed bytes, d = 256 hi + lo (lo in [-128, 127], hi in [-64, 64]), and d K = hi (K << 8)
// + lo K mod 2^64: every (input element, level) becomes two virtual key rows, K << 8 and K, whose eight byte planes
// (recentred by -128, with the 0x80..80 * sum-of-digits correction) are built once per key on the device.
//   k_pfpks_digits   rows of k*N+1 words -> A fragments (2 L signed bytes per input element), digit sums, zero bodies
//   k_pfpks_planes   key [in_words][L][glwe_words] -> B fragments [plane 8][column tile][k chunk][lane 64][16]
// ------------------------------------------------------------------------------------
template <int L>
__global__ __launch_bounds__(256) void k_pfpks_digits(const PfJob *__restrict__ jobs, const uint64_t *__restrict__ big,
                                                      int8_t *__restrict__ dig, int32_t *__restrict__ dsum,
                                                      uint64_t *__restrict__ body, int in_words, int logB, int count,
                                                      int kchunks)
{
    constexpr int LP = 2 * (L <= 1 ? 1 : L <= 2 ? 2 : 4); // bytes per input element (levels padded to 1, 2, 4)
    const int g = blockIdx.x; // padded index; g >= count: an all-zero row
    __shared__ int red[256];
    int local = 0;
    const bool live = g < count;
    PfJob job{};
    if (live) job = jobs[g];
    int8_t *tile = dig + (size_t)(g >> 4) * kchunks * 1024;
    const int padded_words = kchunks * 64 / LP;
    for (int t = threadIdx.x; t < padded_words; t += 256) {
        int8_t b[LP];
#pragma unroll
        for (int j = 0; j < LP; j++) b[j] = 0;
        if (live && t < in_words) {
            int d[L];
            helm_ks::ks_decompose<L>(big[(size_t)in_words * (size_t)job.in_row + t], logB, d);
#pragma unroll
            for (int lev = 0; lev < L; lev++) {
                const int lo = ((d[lev] + 128) & 255) - 128, hi = (d[lev] - lo) >> 8;
                b[2 * lev] = (int8_t)hi;
                b[2 * lev + 1] = (int8_t)lo;
                local += hi + lo;
            }
        }
        const int r0 = t * LP, kc = r0 >> 6, kq = (r0 & 63) >> 4, j0 = r0 & 15;
        int8_t *dst = tile + ((size_t)kc * 64 + (kq << 4 | (g & 15))) * 16 + j0;
#pragma unroll
        for (int j = 0; j < LP; j++) dst[j] = b[j];
    }
    red[threadIdx.x] = local;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        dsum[g] = red[0];
        body[g] = 0ull;
    }
}

__global__ __launch_bounds__(256) void k_pfpks_planes(const uint64_t *__restrict__ key, int8_t *__restrict__ planes,
                                                      int in_words, int L, int LP, int glwe_words, int kchunks, int ctiles)
{
    const size_t frag = (size_t)blockIdx.x * 256 + threadIdx.x; // (column tile, k chunk, lane)
    const size_t per_plane = (size_t)ctiles * kchunks * 64;
    if (frag >= per_plane) return;
    const int lane = (int)(frag & 63), kc = (int)((frag >> 6) % kchunks), ct = (int)((frag >> 6) / kchunks);
    const int c = ct * 16 + (lane & 15);
    int8_t out[8][16];
    for (int j = 0; j < 16; j++) {
        const int r = kc * 64 + 16 * (lane >> 4) + j, t = r / LP, rem = r % LP, lev = rem >> 1;
        uint64_t w = 0;
        if (t < in_words && lev < L && c < glwe_words) {
            w = key[((size_t)t * L + lev) * glwe_words + c];
            if ((rem & 1) == 0) w <<= 8; // the row of the digit's high byte
        }
        for (int b = 0; b < 8; b++) out[b][j] = (int8_t)((int)((w >> (8 * b)) & 255u) - 128);
    }
    for (int b = 0; b < 8; b++) {
        int4 *dst = reinterpret_cast<int4 *>(planes + ((size_t)b * per_plane + frag) * 16);
        *dst = *reinterpret_cast<const int4 *>(out[b]);
    }
}

} // namespace

struct helm_wop_ctx {
    helm_si_ctx *pbs = nullptr; // borrowed: the LUT-mode engine whose wires the gates read and write
    helm_si_ctx *wop = nullptr; // owned: bootstrap + big -> small keyswitch under the WoP-side parameters
    helm_wop_params P{};
    int logN = 0, delta_log = 0;
    uint64_t *d_to_wop = nullptr, *d_to_pbs = nullptr, *d_pfpksk = nullptr;
    int8_t *d_pf_planes = nullptr; // matrix-core packing keyswitch: per key eight byte planes of the two rows per digit
    int pf_kchunks = 0, pf_ctiles = 0;
    KsKey k_to_wop, k_to_pbs;
    bool have[5] = {false, false, false, false, false};
    uint64_t *d_const = nullptr; // constant accumulators: cbs_l rows (circuit bootstrap), then 8 rows (bit extraction)
    uint64_t *d_adds = nullptr;  // the matching body corrections: cbs_l words, then 8 words, then 2^62
    DevBuf<uint64_t> d_clean, d_wbig, d_shift, d_small, d_pbsout, d_bits, d_ggsw, d_glwe, d_tables, d_vp;
    DevBuf<double> d_ggsw_ntt;
    DevBuf<char> d_jobs;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[8];
    helm_wop_timing tacc{};
};

namespace {

struct WopTimed { // HIP events around one stage, summed by helm_wop_get_timing
    helm_wop_ctx *ctx;
    int which;
    hipEvent_t a = nullptr, b = nullptr;
    WopTimed(helm_wop_ctx *c, int w) : ctx(c), which(w)
    {
        (void)hipEventCreate(&a);
        (void)hipEventCreate(&b);
        (void)hipEventRecord(a, ctx->wop->stream);
    }
    ~WopTimed()
    {
        (void)hipEventRecord(b, ctx->wop->stream);
        auto &list = ctx->ev[which];
        list.push_back({a, b});
        if (list.size() >= 64) fold(ctx, which); // a caller that never asks for the timing must not pile events up
    }
    // add the finished pairs of one stage to its total and release their events
    static void fold(helm_wop_ctx *ctx, int which)
    {
        double *acc[8] = {&ctx->tacc.clean_ms,  &ctx->tacc.to_wopbs_ms, &ctx->tacc.extract_ms, &ctx->tacc.cbs_pbs_ms,
                          &ctx->tacc.pfpks_ms, &ctx->tacc.convert_ms,  &ctx->tacc.packing_ms, &ctx->tacc.to_pbs_ms};
        for (auto &p : ctx->ev[which]) {
            float ms = 0;
            (void)hipEventSynchronize(p.second);
            if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) *acc[which] += ms;
            (void)hipEventDestroy(p.first);
            (void)hipEventDestroy(p.second);
        }
        ctx->ev[which].clear();
    }
};

// host job arrays of one call, uploaded in one copy
struct JobArena {
    std::vector<char> host;
    template <typename T> size_t put(const std::vector<T> &v)
    {
        const size_t off = (host.size() + 255) / 256 * 256;
        host.resize(off + v.size() * sizeof(T));
        if (!v.empty()) std::memcpy(host.data() + off, v.data(), v.size() * sizeof(T));
        return off;
    }
};

template <int MODE>
hipError_t launch_vp(helm_wop_ctx *ctx, const Pbs64Job *jobs, int64_t count, const uint64_t *small,
                     const uint64_t *glwe_rows, uint64_t *out, int n_steps, size_t key_stride, int key_first)
{
    helm_si_ctx *W = ctx->wop;
    const double *key = ctx->d_ggsw_ntt.p;
    const int logB = ctx->P.cbs_logB;
#define VP_CASE(LN, LV)                                                                                              \
    if (ctx->logN == LN && ctx->P.cbs_l == LV)                                                                       \
        return launch_pbs64_c<Pbs64Cfg<LN, LV>, MODE>(W, jobs, count, small, glwe_rows, out, key, n_steps, logB,     \
                                                      key_stride, key_first);
    VP_CASE(9, 2) VP_CASE(9, 3) VP_CASE(10, 2) VP_CASE(10, 3) VP_CASE(11, 2) VP_CASE(11, 3)
#undef VP_CASE
    return hipErrorInvalidValue;
}

hipError_t launch_convert_ggsw(helm_wop_ctx *ctx, const uint64_t *d_std, double *d_ntt, size_t n_ggsw)
{
    helm_si_ctx *W = ctx->wop;
    const int K1 = ctx->P.k + 1;
    const size_t polys = n_ggsw * ctx->P.cbs_l * K1 * K1;
#define CONV(LN)                                                                                                     \
    if (ctx->logN == LN) {                                                                                           \
        hipLaunchKernelGGL((k_bsk_convert64<F0, LN>), dim3((unsigned)polys), dim3(64), 0, W->stream, d_std, d_ntt,    \
                           W->keys->tw[0], W->keys->n_inv[0], W->keys->two32[0], K1, ctx->P.cbs_l, 0);               \
        hipLaunchKernelGGL((k_bsk_convert64<F1, LN>), dim3((unsigned)polys), dim3(64), 0, W->stream, d_std, d_ntt,    \
                           W->keys->tw[1], W->keys->n_inv[1], W->keys->two32[1], K1, ctx->P.cbs_l, 1);               \
    }
    CONV(9) CONV(10) CONV(11)
#undef CONV
    return hipGetLastError();
}

// wide batches: digits once for all k+1 keys (the same input rows), then one matrix-core pass per key
bool pfpks_on_matrix_cores(const helm_wop_ctx *ctx, int64_t count)
{
    return ctx->d_pf_planes && ctx->wop->keys->ks_mfma && count >= 64;
}

hipError_t launch_pfpks_mfma(helm_wop_ctx *ctx, const PfJob *const *jobs_per_key, int64_t count, const uint64_t *big,
                             uint64_t *out)
{
    helm_si_ctx *W = ctx->wop;
    const int in_words = ctx->P.k * ctx->P.N + 1, glwe_words = (ctx->P.k + 1) * ctx->P.N;
    const int64_t padded = (count + 63) / 64 * 64;
    if (W->d_ksdig.ensure((size_t)(padded / 16) * ctx->pf_kchunks * 1024) || W->d_ksdsum.ensure((size_t)padded) ||
        W->d_ksbody.ensure((size_t)padded))
        return hipErrorOutOfMemory;
#define PFD_CASE(LV)                                                                                                 \
    case LV:                                                                                                         \
        hipLaunchKernelGGL(k_pfpks_digits<LV>, dim3((unsigned)padded), dim3(256), 0, W->stream, jobs_per_key[0], big,    \
                           W->d_ksdig.p, W->d_ksdsum.p, W->d_ksbody.p, in_words, ctx->P.pfks_logB, (int)count,       \
                           ctx->pf_kchunks);                                                                         \
        break;
    switch (ctx->P.pfks_l) {
        PFD_CASE(1) PFD_CASE(2) PFD_CASE(3) PFD_CASE(4)
    default: return hipErrorInvalidValue;
    }
#undef PFD_CASE
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t planes_per_key = (size_t)8 * ctx->pf_ctiles * ctx->pf_kchunks * 1024;
    static_assert(sizeof(PfJob) == sizeof(Ks64Job), "the matrix-core kernel reads the jobs' out_row");
    for (int r = 0; r <= ctx->P.k; r++) {
        hipLaunchKernelGGL(k_ks64_mfma, dim3((unsigned)(padded / 64), (unsigned)ctx->pf_ctiles), dim3(64), 0, W->stream,
                           reinterpret_cast<const Ks64Job *>(jobs_per_key[r]), W->d_ksdig.p, W->d_ksdsum.p, W->d_ksbody.p,
                           ctx->d_pf_planes + (size_t)r * planes_per_key, out, glwe_words - 1, (int)count, ctx->pf_kchunks,
                           ctx->pf_ctiles);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_pfpks(helm_wop_ctx *ctx, int r, const PfJob *jobs, int64_t count, const uint64_t *big, uint64_t *out)
{
    helm_si_ctx *W = ctx->wop;
    const int in_words = ctx->P.k * ctx->P.N + 1, glwe_words = (ctx->P.k + 1) * ctx->P.N;
    const uint64_t *key = ctx->d_pfpksk + (size_t)r * in_words * ctx->P.pfks_l * glwe_words;
    const unsigned gx = (unsigned)((count + 3) / 4), gy = (unsigned)((glwe_words + 255) / 256);
    int slices = 1;
    while (slices < 16 && (int64_t)gx * gy * slices < 2 * (int64_t)W->n_cus && in_words / (slices * 2) >= 64) slices *= 2;
    const int t_chunk = (in_words + slices - 1) / slices;
    const size_t lds = (size_t)t_chunk * ctx->P.pfks_l * 4 * sizeof(int32_t);
#define PF_CASE(LV)                                                                                                  \
    case LV: {                                                                                                       \
        static bool done[64] = {false}; /* per device, as in launch_keyswitch64 */                                   \
        if (!done[W->device & 63]) {                                                                                 \
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_pfpks64<LV>),                        \
                                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);              \
            if (e != hipSuccess) return e;                                                                           \
            done[W->device & 63] = true;                                                                             \
        }                                                                                                            \
        hipLaunchKernelGGL(k_pfpks64<LV>, dim3(gx, gy, (unsigned)slices), dim3(256), lds, W->stream, jobs, big, key, out, \
                           in_words, glwe_words, ctx->P.pfks_logB, (int)count, t_chunk);                             \
        break;                                                                                                       \
    }
    switch (ctx->P.pfks_l) {
        PF_CASE(1) PF_CASE(2) PF_CASE(3) PF_CASE(4)
    default: return hipErrorInvalidValue;
    }
#undef PF_CASE
    return hipGetLastError();
}

int wop_ready(const helm_wop_ctx *ctx, bool whole_path)
{
    if (!ctx) return fail(HELM_ERR_INVALID, "null ctx");
    if (!ctx->have[HELM_WOP_KEY_BSK] || !ctx->have[HELM_WOP_KEY_KSK] || !ctx->have[HELM_WOP_KEY_PFPKSK])
        return fail(HELM_ERR_STATE, "WoP-PBS: bootstrapping, keyswitching or packing key not loaded");
    if (whole_path && (!ctx->have[HELM_WOP_KEY_KSK_TO_WOPBS] || !ctx->have[HELM_WOP_KEY_KSK_TO_PBS]))
        return fail(HELM_ERR_STATE, "WoP-PBS: the keyswitching keys between the two parameter sets are not loaded");
    return 0;
}

// ---- the three stages on device rows (stream-ordered, no synchronisation) ----------------------------------

// d_wbig rows [R] (WoP big key) -> d_bits rows: row bit_row[r * nb + i] = bit i (least significant first) of row r.
// Clobbers d_wbig.
int extract_bits_device(helm_wop_ctx *ctx, int64_t R, int delta_log, int nb, const std::vector<int32_t> &bit_row,
                        uint64_t *d_bits_rows)
{
    helm_si_ctx *W = ctx->wop;
    const int n = ctx->P.n, dim = ctx->P.k * ctx->P.N;
    if (nb < 1 || nb > 8 || delta_log + nb > 63 || delta_log < 1) return fail(HELM_ERR_INVALID, "extract_bits: bad bit range");
    if (ctx->d_shift.ensure((size_t)R * (dim + 1)) || ctx->d_small.ensure((size_t)R * (n + 1)) ||
        ctx->d_pbsout.ensure((size_t)R * (dim + 1)))
        return fail(HELM_ERR_OOM, "WoP-PBS scratch");
    JobArena A;
    std::vector<Ks64Job> ks((size_t)R);
    for (int64_t r = 0; r < R; r++) ks[(size_t)r] = Ks64Job{(int32_t)r, (int32_t)r};
    const size_t off_ks = A.put(ks);
    std::vector<size_t> off_rows((size_t)nb), off_pbs((size_t)nb);
    for (int i = 0; i < nb; i++) {
        std::vector<int32_t> rows((size_t)R);
        std::vector<Pbs64Job> pj((size_t)R);
        for (int64_t r = 0; r < R; r++) {
            rows[(size_t)r] = bit_row[(size_t)r * nb + i];
            pj[(size_t)r] = Pbs64Job{(int32_t)r, ctx->P.cbs_l + i, (int32_t)r, 0};
        }
        off_rows[(size_t)i] = A.put(rows);
        off_pbs[(size_t)i] = A.put(pj);
    }
    if (ctx->d_jobs.ensure(A.host.size())) return fail(HELM_ERR_OOM, "WoP-PBS jobs");
    HIP_TRY(hipMemcpyAsync(ctx->d_jobs.p, A.host.data(), A.host.size(), hipMemcpyHostToDevice, W->stream));
    HIP_TRY(hipStreamSynchronize(W->stream)); // pageable source: complete before `A` goes away
    const Ks64Job *d_ks = reinterpret_cast<const Ks64Job *>(ctx->d_jobs.p + off_ks);
    const uint64_t *adds = ctx->d_adds;
    for (int i = 0; i < nb; i++) {
        const int32_t *d_rows = reinterpret_cast<const int32_t *>(ctx->d_jobs.p + off_rows[(size_t)i]);
        const Pbs64Job *d_pj = reinterpret_cast<const Pbs64Job *>(ctx->d_jobs.p + off_pbs[(size_t)i]);
        const uint64_t shift = 1ull << (64 - delta_log - i - 1);
        hipLaunchKernelGGL(k_wop_axpy, dim3((unsigned)R), dim3(256), 0, W->stream, ctx->d_shift.p, (const int32_t *)nullptr,
                           ctx->d_wbig.p, (const int32_t *)nullptr, shift, (const uint64_t *)nullptr, 0ull,
                           (const uint64_t *)nullptr, 1, dim);
        HIP_TRY(launch_ks64(W, d_ks, R, ctx->d_shift.p, ctx->d_small.p));
        // the keyswitch output is the extracted bit (bit * 2^63 under the small key)
        hipLaunchKernelGGL(k_wop_axpy, dim3((unsigned)R), dim3(256), 0, W->stream, d_bits_rows, d_rows, ctx->d_small.p,
                           (const int32_t *)nullptr, 1ull, (const uint64_t *)nullptr, 0ull, (const uint64_t *)nullptr, 1, n);
        if (i == nb - 1) break;
        // remove the bit from the input: bootstrap (bit + q/4) with the constant accumulator -alpha, add alpha
        hipLaunchKernelGGL(k_wop_axpy, dim3((unsigned)R), dim3(256), 0, W->stream, ctx->d_small.p, (const int32_t *)nullptr,
                           ctx->d_small.p, (const int32_t *)nullptr, 1ull, (const uint64_t *)nullptr, 0ull,
                           adds + ctx->P.cbs_l + 8, 1, n); // + 2^62
        HIP_TRY(launch_pbs64(W, d_pj, R, ctx->d_small.p, ctx->d_const, ctx->d_pbsout.p));
        ctx->tacc.bootstraps += R;
        // in -= (bootstrap output + alpha)
        hipLaunchKernelGGL(k_wop_axpy, dim3((unsigned)R), dim3(256), 0, W->stream, ctx->d_pbsout.p, (const int32_t *)nullptr,
                           ctx->d_pbsout.p, (const int32_t *)nullptr, 1ull, (const uint64_t *)nullptr, 0ull,
                           adds + ctx->P.cbs_l + i, 1, dim);
        hipLaunchKernelGGL(k_wop_axpy, dim3((unsigned)R), dim3(256), 0, W->stream, ctx->d_wbig.p, (const int32_t *)nullptr,
                           ctx->d_wbig.p, (const int32_t *)nullptr, 1ull, ctx->d_pbsout.p, ~0ull /* -1 */,
                           (const uint64_t *)nullptr, 1, dim);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// d_bits rows [T] (bit * 2^63, small key; clobbered) -> d_ggsw [T][cbs_l][k+1][k+1][N] and its transform-domain copy
int circuit_bootstrap_device(helm_wop_ctx *ctx, int64_t T, uint64_t *d_bits_rows, bool convert)
{
    helm_si_ctx *W = ctx->wop;
    const helm_wop_params &P = ctx->P;
    const int n = P.n, dim = P.k * P.N, K1 = P.k + 1, L = P.cbs_l;
    const size_t glwe = (size_t)K1 * P.N;
    const int64_t X = T * L; // bootstraps
    if (ctx->d_pbsout.ensure((size_t)X * (dim + 1)) || ctx->d_ggsw.ensure((size_t)X * K1 * glwe) ||
        (convert && ctx->d_ggsw_ntt.ensure((size_t)X * K1 * K1 * P.N * 2)))
        return fail(HELM_ERR_OOM, "WoP-PBS scratch (GGSWs)");
    JobArena A;
    std::vector<Pbs64Job> pj((size_t)X);
    for (int64_t t = 0; t < T; t++)
        for (int j = 0; j < L; j++) pj[(size_t)(t * L + j)] = Pbs64Job{(int32_t)t, j, (int32_t)(t * L + j), 0};
    const size_t off_pbs = A.put(pj);
    size_t off_pf[8];
    for (int r = 0; r < K1; r++) {
        std::vector<PfJob> pf((size_t)X);
        for (int64_t x = 0; x < X; x++) pf[(size_t)x] = PfJob{(int32_t)x, (int32_t)(x * K1 + r)};
        off_pf[r] = A.put(pf);
    }
    if (ctx->d_jobs.ensure(A.host.size())) return fail(HELM_ERR_OOM, "WoP-PBS jobs");
    HIP_TRY(hipMemcpyAsync(ctx->d_jobs.p, A.host.data(), A.host.size(), hipMemcpyHostToDevice, W->stream));
    HIP_TRY(hipStreamSynchronize(W->stream));
    {
        WopTimed tm(ctx, 3);
        // + q/4, then cbs_l bootstraps per bit with the constant accumulators -2^(63 - cbs_logB j), + 2^(63 - cbs_logB j)
        hipLaunchKernelGGL(k_wop_axpy, dim3((unsigned)T), dim3(256), 0, W->stream, d_bits_rows, (const int32_t *)nullptr,
                           d_bits_rows, (const int32_t *)nullptr, 1ull, (const uint64_t *)nullptr, 0ull,
                           ctx->d_adds + L + 8, 1, n);
        HIP_TRY(launch_pbs64(W, reinterpret_cast<const Pbs64Job *>(ctx->d_jobs.p + off_pbs), X, d_bits_rows, ctx->d_const,
                             ctx->d_pbsout.p));
        ctx->tacc.bootstraps += X;
        hipLaunchKernelGGL(k_wop_axpy, dim3((unsigned)X), dim3(256), 0, W->stream, ctx->d_pbsout.p, (const int32_t *)nullptr,
                           ctx->d_pbsout.p, (const int32_t *)nullptr, 1ull, (const uint64_t *)nullptr, 0ull, ctx->d_adds, L,
                           dim);
    }
    if (pfpks_on_matrix_cores(ctx, X)) {
        WopTimed tm(ctx, 4);
        const PfJob *per_key[8];
        for (int r = 0; r < K1; r++) per_key[r] = reinterpret_cast<const PfJob *>(ctx->d_jobs.p + off_pf[r]);
        HIP_TRY(launch_pfpks_mfma(ctx, per_key, X, ctx->d_pbsout.p, ctx->d_ggsw.p));
    } else {
        WopTimed tm(ctx, 4);
        const int in_words = dim + 1;
        int slices = 1; // as launch_pfpks: sliced launches accumulate into zeroed rows
        const unsigned gx = (unsigned)((X + 3) / 4), gy = (unsigned)((glwe + 255) / 256);
        while (slices < 16 && (int64_t)gx * gy * slices < 2 * (int64_t)W->n_cus && in_words / (slices * 2) >= 64) slices *= 2;
        if (slices > 1) HIP_TRY(hipMemsetAsync(ctx->d_ggsw.p, 0, (size_t)X * K1 * glwe * sizeof(uint64_t), W->stream));
        for (int r = 0; r < K1; r++)
            HIP_TRY(launch_pfpks(ctx, r, reinterpret_cast<const PfJob *>(ctx->d_jobs.p + off_pf[r]), X, ctx->d_pbsout.p,
                                 ctx->d_ggsw.p));
    }
    if (convert) {
        WopTimed tm(ctx, 5);
        HIP_TRY(launch_convert_ggsw(ctx, ctx->d_ggsw.p, ctx->d_ggsw_ntt.p, (size_t)T));
    }
    return 0;
}

// per gate `bits` GGSWs in d_ggsw_ntt (index 0 = least significant), tables [G][max(2^bits, N)] on the device
// -> d_vp rows [G] (WoP big key)
// Several tables on one input tuple (helm_wop_eval_many_luts): one job per table, job j reads the GGSWs of key
// (key_off + j) / key_div, key_div = tables per tuple - the jobs of a tuple share its GGSWs.  The defaults are the single
// gate's: job j reads key j.
int vertical_packing_device(helm_wop_ctx *ctx, int64_t G, int bits, const uint64_t *d_tables, int64_t key_off = 0,
                            int key_div = 1)
{
    helm_si_ctx *W = ctx->wop;
    const helm_wop_params &P = ctx->P;
    const int N = P.N, K1 = P.k + 1, dim = P.k * N;
    const int nbr = std::min(bits, ctx->logN), tree = bits - nbr;
    const size_t glwe = (size_t)K1 * N, leaves = (size_t)1 << tree;
    const size_t per_ggsw = (size_t)K1 * K1 * P.cbs_l * 2 * N; // doubles
    const size_t key_stride = per_ggsw * bits;
    const size_t half = (size_t)G * ((leaves + 1) / 2);
    if (key_div < 1) return fail(HELM_ERR_INVALID, "vertical packing: bad key divisor");
    if (ctx->d_glwe.ensure(((size_t)G * leaves + half) * glwe) || ctx->d_vp.ensure((size_t)G * (dim + 1)))
        return fail(HELM_ERR_OOM, "WoP-PBS scratch (vertical packing)");
    const auto key_of = [&](int64_t g) { return (int32_t)((key_off + g) / key_div); };
    JobArena A;
    // synthetic small LWE: mask word i switches to -2^i (mod 2N), body to 0: step i multiplies by X^(-2^i bit_i)
    std::vector<uint64_t> rot((size_t)nbr + 1, 0);
    for (int i = 0; i < nbr; i++) rot[(size_t)i] = (uint64_t)(2 * N - (1 << i)) << (64 - (ctx->logN + 1));
    const size_t off_rot = A.put(rot);
    std::vector<size_t> off_tree((size_t)tree);
    {
        size_t rows_in = leaves;
        for (int lev = 0; lev < tree; lev++) {
            const size_t rows_out = rows_in / 2;
            std::vector<Pbs64Job> cj((size_t)G * rows_out);
            for (int64_t g = 0; g < G; g++)
                for (size_t q = 0; q < rows_out; q++)
                    cj[(size_t)g * rows_out + q] = Pbs64Job{(int32_t)(g * rows_in + 2 * q + 1), (int32_t)(g * rows_in + 2 * q),
                                                            (int32_t)(g * rows_out + q), key_of(g)};
            off_tree[(size_t)lev] = A.put(cj);
            rows_in = rows_out;
        }
    }
    std::vector<Pbs64Job> bj((size_t)G);
    for (int64_t g = 0; g < G; g++) bj[(size_t)g] = Pbs64Job{0, (int32_t)g, (int32_t)g, key_of(g)};
    const size_t off_br = A.put(bj);
    if (ctx->d_jobs.ensure(A.host.size())) return fail(HELM_ERR_OOM, "WoP-PBS jobs");
    HIP_TRY(hipMemcpyAsync(ctx->d_jobs.p, A.host.data(), A.host.size(), hipMemcpyHostToDevice, W->stream));
    HIP_TRY(hipStreamSynchronize(W->stream));
    WopTimed tm(ctx, 6);
    uint64_t *cur = ctx->d_glwe.p, *nxt = ctx->d_glwe.p + (size_t)G * leaves * glwe;
    hipLaunchKernelGGL(k_wop_trivial_glwe, dim3((unsigned)((size_t)G * leaves)), dim3(256), 0, W->stream, d_tables, cur, P.k, N);
    size_t rows_in = leaves;
    for (int lev = 0; lev < tree; lev++) { // the lowest tree bit pairs neighbouring polynomials
        const size_t rows_out = rows_in / 2;
        // ping-pong between the leaf area and the half-size area: level `lev` reads rows_in rows per gate
        HIP_TRY((launch_vp<2>(ctx, reinterpret_cast<const Pbs64Job *>(ctx->d_jobs.p + off_tree[(size_t)lev]),
                              (int64_t)((size_t)G * rows_out), nullptr, cur, nxt, 1, key_stride, nbr + lev)));
        std::swap(cur, nxt);
        rows_in = rows_out;
    }
    HIP_TRY((launch_vp<1>(ctx, reinterpret_cast<const Pbs64Job *>(ctx->d_jobs.p + off_br), G,
                          reinterpret_cast<const uint64_t *>(ctx->d_jobs.p + off_rot), cur, ctx->d_vp.p, nbr, key_stride, 0)));
    HIP_TRY(hipGetLastError());
    return 0;
}

int wop_upload(helm_wop_ctx *ctx, DevBuf<uint64_t> &buf, const uint64_t *host, size_t words)
{
    if (buf.ensure(words)) return fail(HELM_ERR_OOM, "WoP-PBS scratch");
    HIP_TRY(hipMemcpyAsync(buf.p, host, words * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->wop->stream));
    return 0;
}

// How stage 5 serves n_out tables on one input tuple (helm_wop_many_form): 0 single - one table, the launch of a single gate;
// 1 shared - one job per table, the jobs of a tuple read the same GGSWs.  (A packed form - the tuple's tables side by side in
// one polynomial where n_out 2^bits <= N, one rotation, n_out sample extracts through a launch argument of k_pbs64<., 1> - was
// built and measured at the S-box shape: 48.10 ms against the shared form's 48.27 ms per 256 outputs, inside the spreads;
// it was deleted, DESIGN 4.8.  Value 2 stays reserved for it.)
int wop_many_form_rule(int64_t n_out) { return n_out <= 1 ? 0 : 1; }

} // namespace

extern "C" {

int helm_wop_ctx_create(helm_si_ctx *pbs_side, const helm_wop_params *params, helm_wop_ctx **out)
{
    if (!pbs_side || !params || !out) return fail(HELM_ERR_INVALID, "null argument");
    *out = nullptr;
    const helm_wop_params &P = *params;
    if (P.cbs_l < 2 || P.cbs_l > 3 || P.cbs_logB < 1 || P.cbs_logB * P.cbs_l > 31)
        return fail(HELM_ERR_INVALID, "WoP-PBS: circuit-bootstrap levels must be 2 or 3 (built variants), cbs_logB * cbs_l <= 31");
    if (P.pfks_l < 1 || P.pfks_l > 4 || P.pfks_logB < 2 || P.pfks_logB > 30 || P.pfks_logB * P.pfks_l > 63)
        return fail(HELM_ERR_INVALID, "WoP-PBS: bad packing-keyswitch decomposition (pfks_l <= 4, pfks_logB <= 30)");
    if (pbs_side->keys->run.cls != SI_TUNED)
        return fail(HELM_ERR_INVALID, std::string("WoP-PBS: the PBS-side context runs the ") + SI_CLASS[pbs_side->keys->run.cls].wop +
                                          "; the WoP path is built for the tuned kernels only");
    if (pbs_side->order == 0)
        return fail(HELM_ERR_INVALID, "WoP-PBS: the PBS-side context was created with HELM_SI_CREATE_PBS_KS (helm_si_pbs_order 0: "
                                      "wire rows of n + 1 words); the WoP path's bit extraction, circuit bootstrap and result rows "
                                      "assume big wire rows (helm_si_pbs_order 1)");
    if (pbs_side->P.k != 1 || P.k != 1)
        return fail(HELM_ERR_INVALID, "WoP-PBS: built for k = 1 on both sides (every tfhe WOPBS set and its PBS partner)");
    helm_si_params S{};
    S.n = P.n; S.k = P.k; S.N = P.N;
    S.pbs_l = P.pbs_l; S.pbs_logB = P.pbs_logB;
    S.ks_l = P.ks_l; S.ks_logB = P.ks_logB;
    S.message_modulus = P.message_modulus; S.carry_modulus = P.carry_modulus;
    S.grouping_factor = 0;
    helm_si_ctx *W = nullptr;
    if (int rc = helm_si_ctx_create(pbs_side->device, &S, &W)) return rc;
    helm_wop_ctx *ctx = new (std::nothrow) helm_wop_ctx();
    if (!ctx) {
        helm_si_ctx_destroy(W);
        return fail(HELM_ERR_OOM, "ctx");
    }
    ctx->pbs = pbs_side;
    ctx->wop = W;
    ctx->P = P;
    ctx->logN = W->logN;
    const int t = P.message_modulus * P.carry_modulus;
    int tl = 0;
    while ((1 << tl) < t) tl++;
    ctx->delta_log = 63 - tl;
    // constant accumulators and their body corrections
    const int rows = P.cbs_l + 8;
    std::vector<uint64_t> acc((size_t)rows * P.N), adds((size_t)rows + 1);
    for (int j = 0; j < rows; j++) {
        uint64_t alpha;
        if (j < P.cbs_l) alpha = 1ull << (63 - P.cbs_logB * (j + 1));
        else alpha = ctx->delta_log - 1 + (j - P.cbs_l) < 63 ? 1ull << (ctx->delta_log - 1 + (j - P.cbs_l)) : 0ull;
        adds[(size_t)j] = alpha;
        for (int u = 0; u < P.N; u++) acc[(size_t)j * P.N + u] = 0ull - alpha;
    }
    adds[(size_t)rows] = 1ull << 62;
    auto guard = [&](hipError_t e) {
        if (e == hipSuccess) return 0;
        helm_wop_ctx_destroy(ctx);
        return fail(HELM_ERR_HIP, std::string("WoP-PBS context: ") + hipGetErrorString(e));
    };
    if (int rc = guard(hipMalloc(&ctx->d_const, acc.size() * sizeof(uint64_t)))) return rc;
    if (int rc = guard(hipMalloc(&ctx->d_adds, adds.size() * sizeof(uint64_t)))) return rc;
    if (int rc = guard(hipMemcpy(ctx->d_const, acc.data(), acc.size() * sizeof(uint64_t), hipMemcpyHostToDevice))) return rc;
    if (int rc = guard(hipMemcpy(ctx->d_adds, adds.data(), adds.size() * sizeof(uint64_t), hipMemcpyHostToDevice))) return rc;
    *out = ctx;
    return 0;
}

int helm_wop_ctx_destroy(helm_wop_ctx *ctx)
{
    if (!ctx) return 0;
    if (ctx->wop) {
        (void)hipSetDevice(ctx->wop->device);
        (void)hipStreamSynchronize(ctx->wop->stream);
    }
    for (auto &l : ctx->ev)
        for (auto &p : l) {
            (void)hipEventDestroy(p.first);
            (void)hipEventDestroy(p.second);
        }
    for (uint64_t *p : {ctx->d_to_wop, ctx->d_to_pbs, ctx->d_pfpksk, ctx->d_const, ctx->d_adds})
        if (p) (void)hipFree(p);
    if (ctx->d_pf_planes) (void)hipFree(ctx->d_pf_planes);
    ctx->d_clean.release(); ctx->d_wbig.release(); ctx->d_shift.release(); ctx->d_small.release();
    ctx->d_pbsout.release(); ctx->d_bits.release(); ctx->d_ggsw.release(); ctx->d_glwe.release();
    ctx->d_tables.release(); ctx->d_vp.release(); ctx->d_ggsw_ntt.release();
    ctx->d_jobs.release();
    if (ctx->wop) helm_si_ctx_destroy(ctx->wop);
    delete ctx;
    return 0;
}

int helm_wop_get_params(const helm_wop_ctx *ctx, helm_wop_params *out)
{
    if (!ctx || !out) return fail(HELM_ERR_INVALID, "null argument");
    *out = ctx->P;
    return 0;
}

int helm_wop_load_key(helm_wop_ctx *ctx, int which, const uint64_t *words, size_t n_words, int32_t l, int32_t logB)
{
    if (!ctx || !words) return fail(HELM_ERR_INVALID, "null argument");
    const helm_wop_params &P = ctx->P;
    const size_t kN = (size_t)P.k * P.N;
    HIP_TRY(hipSetDevice(ctx->wop->device));
    auto raw = [&](uint64_t *&dst, size_t want, const char *what) {
        if (n_words != want)
            return fail(HELM_ERR_INVALID, std::string(what) + ": expected " + std::to_string(want) + " words, got " +
                                              std::to_string(n_words));
        if (!dst) HIP_TRY(hipMalloc(&dst, want * sizeof(uint64_t)));
        HIP_TRY(hipMemcpy(dst, words, want * sizeof(uint64_t), hipMemcpyHostToDevice));
        return 0;
    };
    switch (which) {
    case HELM_WOP_KEY_BSK:
        if (int rc = helm_si_load_bootstrap_key(ctx->wop, words, n_words)) return rc;
        break;
    case HELM_WOP_KEY_KSK:
        if (int rc = helm_si_load_keyswitch_key(ctx->wop, words, n_words)) return rc;
        break;
    case HELM_WOP_KEY_KSK_TO_WOPBS: {
        if (l < 1 || l > 8 || logB < 1 || logB > 7) return fail(HELM_ERR_INVALID, "ksk_pbs_to_wopbs: bad decomposition");
        const size_t in_dim = (size_t)ctx->pbs->P.k * ctx->pbs->P.N;
        if (int rc = raw(ctx->d_to_wop, in_dim * l * (kN + 1), "ksk_pbs_to_wopbs")) return rc;
        ctx->k_to_wop = KsKey{ctx->d_to_wop, nullptr, (int)in_dim, (int)kN, l, logB, 0, 0};
        break;
    }
    case HELM_WOP_KEY_KSK_TO_PBS: {
        if (l < 1 || l > 8 || logB < 1 || logB > 7) return fail(HELM_ERR_INVALID, "ksk_wopbs_to_pbs: bad decomposition");
        if (int rc = raw(ctx->d_to_pbs, kN * l * ((size_t)ctx->pbs->P.n + 1), "ksk_wopbs_to_pbs")) return rc;
        ctx->k_to_pbs = KsKey{ctx->d_to_pbs, nullptr, (int)kN, ctx->pbs->P.n, l, logB, 0, 0};
        break;
    }
    case HELM_WOP_KEY_PFPKSK: {
        const size_t glwe_words = (size_t)(P.k + 1) * P.N, per_key = (kN + 1) * P.pfks_l * glwe_words;
        if (int rc = raw(ctx->d_pfpksk, (size_t)(P.k + 1) * per_key, "pfpksk")) return rc;
        // byte planes for the matrix cores: digits of at most 15 bits split into two signed bytes
        if (P.pfks_logB <= 15 && glwe_words % 16 == 0) {
            const int LP = 2 * (P.pfks_l <= 1 ? 1 : P.pfks_l <= 2 ? 2 : 4);
            const int kchunks = (int)(((kN + 1) * LP + 63) / 64), ctiles = (int)(glwe_words / 16);
            const size_t frags = (size_t)ctiles * kchunks * 64, planes_per_key = 8 * frags * 16;
            if (!ctx->d_pf_planes) HIP_TRY(hipMalloc(&ctx->d_pf_planes, planes_per_key * (P.k + 1)));
            for (int r = 0; r <= P.k; r++)
                hipLaunchKernelGGL(k_pfpks_planes, dim3((unsigned)((frags + 255) / 256)), dim3(256), 0, ctx->wop->stream,
                                   ctx->d_pfpksk + (size_t)r * per_key, ctx->d_pf_planes + (size_t)r * planes_per_key,
                                   (int)(kN + 1), P.pfks_l, LP, (int)glwe_words, kchunks, ctiles);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(ctx->wop->stream));
            ctx->pf_kchunks = kchunks;
            ctx->pf_ctiles = ctiles;
        }
        break;
    }
    default: return fail(HELM_ERR_INVALID, "helm_wop_load_key: unknown key");
    }
    ctx->have[which] = true;
    return 0;
}

int helm_wop_extract_bits_batch(helm_wop_ctx *ctx, const uint64_t *in_big, int32_t delta_log, int32_t nb,
                                uint64_t *out_small, int64_t count)
{
    if (int rc = wop_ready(ctx, false)) return rc;
    if (!in_big || !out_small || count < 0) return fail(HELM_ERR_INVALID, "bad argument");
    if (count == 0) return 0;
    helm_si_ctx *W = ctx->wop;
    HIP_TRY(hipSetDevice(W->device));
    const size_t brow = (size_t)ctx->P.k * ctx->P.N + 1, srow = (size_t)ctx->P.n + 1;
    if (nb < 1 || nb > 8) return fail(HELM_ERR_INVALID, "extract_bits: 1..8 bits");
    if (int rc = wop_upload(ctx, ctx->d_wbig, in_big, (size_t)count * brow)) return rc;
    if (ctx->d_bits.ensure((size_t)count * nb * srow)) return fail(HELM_ERR_OOM, "WoP-PBS scratch");
    std::vector<int32_t> bit_row((size_t)count * nb);
    for (size_t q = 0; q < bit_row.size(); q++) bit_row[q] = (int32_t)q;
    // the accumulators on the device are those of the context's own delta_log
    if (delta_log != ctx->delta_log && nb > 1)
        return fail(HELM_ERR_INVALID, "extract_bits: more than one bit needs delta_log = 63 - log2(message_modulus * carry_modulus)");
    if (int rc = extract_bits_device(ctx, count, delta_log, nb, bit_row, ctx->d_bits.p)) return rc;
    HIP_TRY(hipMemcpyAsync(out_small, ctx->d_bits.p, (size_t)count * nb * srow * sizeof(uint64_t), hipMemcpyDeviceToHost,
                           W->stream));
    HIP_TRY(hipStreamSynchronize(W->stream));
    return 0;
}

int helm_wop_circuit_bootstrap_batch(helm_wop_ctx *ctx, const uint64_t *in_small, uint64_t *ggsw_out, int64_t count)
{
    if (int rc = wop_ready(ctx, false)) return rc;
    if (!in_small || !ggsw_out || count < 0) return fail(HELM_ERR_INVALID, "bad argument");
    if (count == 0) return 0;
    helm_si_ctx *W = ctx->wop;
    HIP_TRY(hipSetDevice(W->device));
    const size_t srow = (size_t)ctx->P.n + 1;
    const size_t words = (size_t)count * ctx->P.cbs_l * (ctx->P.k + 1) * (ctx->P.k + 1) * ctx->P.N;
    if (int rc = wop_upload(ctx, ctx->d_bits, in_small, (size_t)count * srow)) return rc;
    if (int rc = circuit_bootstrap_device(ctx, count, ctx->d_bits.p, false)) return rc;
    HIP_TRY(hipMemcpyAsync(ggsw_out, ctx->d_ggsw.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost, W->stream));
    HIP_TRY(hipStreamSynchronize(W->stream));
    return 0;
}

int helm_wop_vertical_packing_batch(helm_wop_ctx *ctx, const uint64_t *ggsw, int32_t bits, const uint64_t *tables,
                                    uint64_t *out_big, int64_t count)
{
    if (!ctx || !ggsw || !tables || !out_big || count < 0) return fail(HELM_ERR_INVALID, "bad argument");
    if (bits < 1 || bits > ctx->logN + 6) return fail(HELM_ERR_INVALID, "vertical_packing: 1..log2(N)+6 bits");
    if (count == 0) return 0;
    helm_si_ctx *W = ctx->wop;
    HIP_TRY(hipSetDevice(W->device));
    const helm_wop_params &P = ctx->P;
    const size_t per = (size_t)P.cbs_l * (P.k + 1) * (P.k + 1) * P.N, brow = (size_t)P.k * P.N + 1;
    const size_t n_ggsw = (size_t)count * bits;
    if (int rc = wop_upload(ctx, ctx->d_ggsw, ggsw, n_ggsw * per)) return rc;
    if (ctx->d_ggsw_ntt.ensure(n_ggsw * per * 2)) return fail(HELM_ERR_OOM, "WoP-PBS scratch (GGSWs)");
    HIP_TRY(launch_convert_ggsw(ctx, ctx->d_ggsw.p, ctx->d_ggsw_ntt.p, n_ggsw));
    const size_t tw = helm_wop_table_words(&P, bits);
    if (int rc = wop_upload(ctx, ctx->d_tables, tables, (size_t)count * tw)) return rc;
    if (int rc = vertical_packing_device(ctx, count, bits, ctx->d_tables.p)) return rc;
    HIP_TRY(hipMemcpyAsync(out_big, ctx->d_vp.p, (size_t)count * brow * sizeof(uint64_t), hipMemcpyDeviceToHost, W->stream));
    HIP_TRY(hipStreamSynchronize(W->stream));
    return 0;
}

int helm_wop_many_form(const helm_wop_ctx *ctx, int32_t bits, int32_t n_out)
{
    if (!ctx) return fail(HELM_ERR_INVALID, "null ctx");
    if (bits < 1 || bits > ctx->logN + 6 || n_out < 1) return fail(HELM_ERR_INVALID, "many_form: 1..log2(N)+6 bits, n_out >= 1");
    return wop_many_form_rule(n_out);
}

int helm_wop_vertical_packing_many_batch(helm_wop_ctx *ctx, const uint64_t *ggsw, int32_t bits, const uint64_t *tables,
                                         int32_t n_out, uint64_t *out_big, int64_t count)
{
    if (!ctx || !ggsw || !tables || !out_big || count < 0) return fail(HELM_ERR_INVALID, "bad argument");
    if (bits < 1 || bits > ctx->logN + 6) return fail(HELM_ERR_INVALID, "vertical_packing: 1..log2(N)+6 bits");
    if (n_out < 1 || count * n_out > INT32_MAX) return fail(HELM_ERR_INVALID, "vertical_packing: n_out >= 1, count * n_out rows must fit the row index");
    if (count == 0) return 0;
    helm_si_ctx *W = ctx->wop;
    HIP_TRY(hipSetDevice(W->device));
    const helm_wop_params &P = ctx->P;
    const size_t per = (size_t)P.cbs_l * (P.k + 1) * (P.k + 1) * P.N, brow = (size_t)P.k * P.N + 1;
    const size_t n_ggsw = (size_t)count * bits;
    if (int rc = wop_upload(ctx, ctx->d_ggsw, ggsw, n_ggsw * per)) return rc;
    if (ctx->d_ggsw_ntt.ensure(n_ggsw * per * 2)) return fail(HELM_ERR_OOM, "WoP-PBS scratch (GGSWs)");
    HIP_TRY(launch_convert_ggsw(ctx, ctx->d_ggsw.p, ctx->d_ggsw_ntt.p, n_ggsw));
    const size_t tw = helm_wop_table_words(&P, bits);
    if (int rc = wop_upload(ctx, ctx->d_tables, tables, (size_t)count * n_out * tw)) return rc;
    if (int rc = vertical_packing_device(ctx, count * n_out, bits, ctx->d_tables.p, 0, n_out)) return rc;
    HIP_TRY(hipMemcpyAsync(out_big, ctx->d_vp.p, (size_t)count * n_out * brow * sizeof(uint64_t), hipMemcpyDeviceToHost,
                           W->stream));
    HIP_TRY(hipStreamSynchronize(W->stream));
    return 0;
}

size_t helm_wop_table_words(const helm_wop_params *params, int32_t total_bits)
{
    if (!params || total_bits < 0 || total_bits > 40) return 0;
    const size_t e = (size_t)1 << total_bits;
    return e < (size_t)params->N ? (size_t)params->N : e;
}

int helm_wop_make_table(const helm_wop_params *params, int32_t n_blocks, int32_t bits_per_block, const uint64_t *truth,
                        size_t truth_len, uint64_t *table_out)
{
    if (!params || !truth || !table_out || n_blocks < 1 || bits_per_block < 1 || n_blocks * bits_per_block > 30)
        return fail(HELM_ERR_INVALID, "helm_wop_make_table: bad argument");
    const uint64_t basis = (uint64_t)params->message_modulus;
    const uint64_t delta = (1ull << 63) / (uint64_t)(params->message_modulus * params->carry_modulus);
    const int total = n_blocks * bits_per_block;
    const size_t words = helm_wop_table_words(params, total);
    // modulus = basis^n_blocks (saturating: indices are far smaller)
    uint64_t modulus = 1;
    for (int j = 0; j < n_blocks; j++) modulus = modulus > (~0ull) / basis ? ~0ull : modulus * basis;
    for (size_t v = 0; v < words; v++) {
        uint64_t entry = 0;
        if (v < ((size_t)1 << total)) {
            uint64_t x = 0, w = 1; // decode_radix(encode_mix_radix(v)): block j's field times basis^j
            for (int j = 0; j < n_blocks; j++) {
                const uint64_t field = (v >> (j * bits_per_block)) & ((1ull << bits_per_block) - 1);
                x += field * w;
                w *= basis;
            }
            x %= modulus;
            const uint64_t f = x < truth_len ? (truth[x] & 1ull) : 0ull; // eval_luts (gates.rs:746-748)
            entry = (f % modulus % basis) * delta;                         // block 0 of encode_radix(f mod modulus)
        }
        table_out[v] = entry;
    }
    return 0;
}

int helm_wop_eval_luts(helm_wop_ctx *ctx, helm_si_wires *w, const int32_t *in_idx, int32_t n_inputs,
                       int32_t bits_per_block, const uint64_t *tables, const int32_t *out_idx, int64_t count)
{
    return helm_wop_eval_many_luts(ctx, w, in_idx, n_inputs, bits_per_block, tables, out_idx, 1, count);
}

// `count` groups of n_out tables on one input tuple each; n_out = 1 is a batch of single gates, launch for launch
int helm_wop_eval_many_luts(helm_wop_ctx *ctx, helm_si_wires *w, const int32_t *in_idx, int32_t n_inputs,
                            int32_t bits_per_block, const uint64_t *tables, const int32_t *out_idx, int32_t n_out,
                            int64_t count)
{
    if (int rc = wop_ready(ctx, true)) return rc;
    if (!w || !in_idx || !tables || !out_idx || count < 0) return fail(HELM_ERR_INVALID, "bad argument");
    if (n_out < 1) return fail(HELM_ERR_INVALID, "WoP-PBS: n_out must be at least 1");
    if (count * n_out > INT32_MAX) return fail(HELM_ERR_INVALID, "WoP-PBS: count * n_out outputs do not fit the row index");
    if (w->owner != ctx->pbs) return fail(HELM_ERR_INVALID, "wire table belongs to another context");
    const helm_wop_params &P = ctx->P;
    int tl = 0;
    while ((1 << tl) < P.message_modulus * P.carry_modulus) tl++;
    if (n_inputs < 1 || bits_per_block < 1 || bits_per_block > tl)
        return fail(HELM_ERR_INVALID, "WoP-PBS: bits_per_block must be in [1, log2(message_modulus * carry_modulus)]");
    const int bits = n_inputs * bits_per_block;
    if (bits > ctx->logN + 6) return fail(HELM_ERR_INVALID, "WoP-PBS: more than log2(N) + 6 index bits");
    if (count == 0) return 0;
    if (int rc = check_rows(w, in_idx, count * n_inputs, false)) return rc;
    if (int rc = check_rows(w, out_idx, count * n_out, false)) return rc;
    {
        // the gates of a call are independent: the batch runs in chunks (and, sharded, in groups per rank), each writing
        // its output rows before the next reads its inputs, so an output row that is an input row of ANOTHER gate of the
        // call would make the result depend on the chunking.  Refused; evaluate dependent gates in separate calls
        // (levels).  A gate may write over one of its own inputs: its stages read them before its last one writes.
        // (A gate here is a group: its n_out outputs are written after every stage that reads its inputs.)
        std::vector<std::pair<int32_t, int64_t>> outs((size_t)(count * n_out));
        for (int64_t q = 0; q < count * n_out; q++) outs[(size_t)q] = {out_idx[q], q / n_out};
        std::sort(outs.begin(), outs.end());
        if (n_out > 1) // a group's outputs leave in passes: which of two writers of a row lands last is no property of the call
            for (size_t q = 1; q < outs.size(); q++)
                if (outs[q].first == outs[q - 1].first)
                    return fail(HELM_ERR_INVALID, "WoP-PBS: two outputs of the call name row " + std::to_string(outs[q].first));
        for (int64_t g = 0; g < count; g++)
            for (int q = 0; q < n_inputs; q++) {
                const int32_t r = in_idx[g * n_inputs + q];
                auto it = std::lower_bound(outs.begin(), outs.end(), std::make_pair(r, (int64_t)-1));
                for (; it != outs.end() && it->first == r; ++it)
                    if (it->second != g)
                        return fail(HELM_ERR_INVALID, "WoP-PBS: an output row of the call is an input row of another of its gates (gates of a call must be independent)");
            }
    }
    helm_si_ctx *S = ctx->pbs, *W = ctx->wop;
    HIP_TRY(hipSetDevice(S->device));
    // one stream for both engines
    hipStream_t saved = W->stream;
    W->stream = S->stream;
    struct Restore {
        helm_si_ctx *W;
        hipStream_t s;
        ~Restore() { W->stream = s; }
    } restore{W, saved};
    const int dimS = S->P.k * S->P.N, dimW = P.k * P.N;
    const size_t tw = helm_wop_table_words(&P, bits);
    std::vector<uint64_t> ident((size_t)S->P.message_modulus * S->P.carry_modulus), id_lut((size_t)S->P.N);
    for (size_t v = 0; v < ident.size(); v++) ident[v] = v;
    if (int rc = helm_si_make_lut(S, ident.data(), id_lut.data())) return rc;
    // Chunks bound the GGSW scratch (~0.6 MB per bit).  A group has `bits` GGSWs, as a single gate has, so with n_out > 1 the
    // groups run in chunks of the same size, and within a chunk stages 5 and 6 run in passes of at most `chunk` tables:
    // d_glwe, d_vp and d_tables never grow beyond what a chunk of single-output gates needs.
    const int64_t chunk = std::max<int64_t>(1, 16384 / bits);
    const int form = wop_many_form_rule(n_out);
    // gates [first, first + G) of the call through stages 1-6; the result rows go to dst (rows of the PBS-side big key):
    // row out_rows[g] of the wire table, or rows 0.. of the exchange staging buffer of a sharded call
    // (with n_out > 1 a gate is a group: stages 1-4 once, stages 5 and 6 per output; result row g * n_out + o)
    auto run_gates = [&](int64_t first, int64_t G, uint64_t *dst, const int32_t *out_rows) -> int {
        if (G == 0) return 0;
        const int64_t R = G * n_inputs, T = G * bits;
        if (ctx->d_clean.ensure((size_t)R * (dimS + 1)) || ctx->d_wbig.ensure((size_t)R * (dimW + 1)) ||
            ctx->d_bits.ensure((size_t)T * (P.n + 1)))
            return fail(HELM_ERR_OOM, "WoP-PBS scratch");
        if (form == 0) {
            if (int rc = wop_upload(ctx, ctx->d_tables, tables + (size_t)first * tw, (size_t)G * tw)) return rc;
        }
        // 1: cleaning bootstrap, PBS side (row r = gate g, input q)
        std::vector<Ks64Job> ks((size_t)R);
        std::vector<Pbs64Job> pj((size_t)R);
        for (int64_t r = 0; r < R; r++) {
            ks[(size_t)r] = Ks64Job{in_idx[(size_t)first * n_inputs + r], (int32_t)r};
            pj[(size_t)r] = Pbs64Job{(int32_t)r, 0, (int32_t)r, 0};
        }
        {
            WopTimed tm(ctx, 0);
            if (int rc = apply_luts_device(S, w->d, ctx->d_clean.p, ks, pj, id_lut.data(), 1)) return rc;
            ctx->tacc.bootstraps += R;
        }
        // 2: to the WoP big key
        JobArena A;
        for (int64_t r = 0; r < R; r++) ks[(size_t)r] = Ks64Job{(int32_t)r, (int32_t)r};
        const size_t off_ks = A.put(ks);
        if (ctx->d_jobs.ensure(A.host.size())) return fail(HELM_ERR_OOM, "WoP-PBS jobs");
        HIP_TRY(hipMemcpyAsync(ctx->d_jobs.p, A.host.data(), A.host.size(), hipMemcpyHostToDevice, W->stream));
        HIP_TRY(hipStreamSynchronize(W->stream));
        {
            WopTimed tm(ctx, 1);
            HIP_TRY(launch_ks64_key(W, ctx->k_to_wop, reinterpret_cast<const Ks64Job *>(ctx->d_jobs.p + off_ks), R,
                                    ctx->d_clean.p, ctx->d_wbig.p));
        }
        // 3: bits; input q of a gate is block n_inputs-1-q (first input = most significant block)
        std::vector<int32_t> bit_row((size_t)R * bits_per_block);
        for (int64_t g = 0; g < G; g++)
            for (int q = 0; q < n_inputs; q++)
                for (int i = 0; i < bits_per_block; i++)
                    bit_row[((size_t)g * n_inputs + q) * bits_per_block + i] =
                        (int32_t)(g * bits + (n_inputs - 1 - q) * bits_per_block + i);
        {
            WopTimed tm(ctx, 2);
            if (int rc = extract_bits_device(ctx, R, ctx->delta_log, bits_per_block, bit_row, ctx->d_bits.p)) return rc;
        }
        // 4: one GGSW per bit
        if (int rc = circuit_bootstrap_device(ctx, T, ctx->d_bits.p, true)) return rc;
        // 5 and 6 on result rows [r0, r0 + n) of the chunk, n rows in d_vp: back to the PBS side
        auto way_back = [&](int64_t r0, int64_t n) -> int {
            ks.resize((size_t)n);
            pj.resize((size_t)n);
            for (int64_t g = 0; g < n; g++) {
                ks[(size_t)g] = Ks64Job{(int32_t)g, (int32_t)g};
                pj[(size_t)g] = Pbs64Job{(int32_t)g, 0, out_rows ? out_rows[r0 + g] : (int32_t)(r0 + g), 0};
            }
            WopTimed tm(ctx, 7);
            if (int rc = apply_luts_device(S, ctx->d_vp.p, dst, ks, pj, id_lut.data(), 1, &ctx->k_to_pbs)) return rc;
            ctx->tacc.bootstraps += n;
            return 0;
        };
        if (form == 0) {
            // 5: table look-up
            if (int rc = vertical_packing_device(ctx, G, bits, ctx->d_tables.p)) return rc;
            // 6: back to the PBS side
            if (int rc = way_back(0, G)) return rc;
        } else {
            // shared: one job per table, the jobs of a group read the group's GGSWs; passes of at most `chunk` tables
            for (int64_t r0 = 0; r0 < G * n_out; r0 += chunk) {
                const int64_t n = std::min(chunk, G * n_out - r0);
                if (r0) HIP_TRY(hipStreamSynchronize(S->stream)); // d_tables, d_vp and the job arrays of the last pass
                if (int rc = wop_upload(ctx, ctx->d_tables, tables + ((size_t)first * n_out + r0) * tw, (size_t)n * tw)) return rc;
                if (int rc = vertical_packing_device(ctx, n, bits, ctx->d_tables.p, r0, n_out)) return rc;
                if (int rc = way_back(r0, n)) return rc;
            }
        }
        HIP_TRY(hipStreamSynchronize(S->stream)); // the scratch of this chunk is reused by the next
        ctx->tacc.gates += G * n_out;
        return 0;
    };
    if (S->x_on && count >= S->x_min) {
        // Sharded (helm_si_set_exchange on the PBS side): the gates of a round are split into `world` contiguous chunks,
        // this rank evaluates its chunk - every stage locally, the keys are replicated - into the staging buffer, the
        // caller's all-gather brings every rank's result rows and they are scattered into the table: identical
        // ciphertexts to the unsharded call.  Every rank makes the same calls, also one whose chunk is empty.
        // With n_out > 1 the call is cut by group: a rank's slot carries its groups' n_out result rows each (so a round takes
        // x_cap / n_out groups per rank, as apply_many_luts_sharded does) and gathered row i n_out + o is output o of group
        // base + i.
        const int64_t world = S->x_world, cap = S->x_cap / n_out;
        if (cap < 1)
            return fail(HELM_ERR_INVALID, "WoP-PBS: n_out = " + std::to_string(n_out) + " exceeds the exchange's capacity_rows = " +
                                              std::to_string(S->x_cap) + " (one group's outputs do not fit a rank's slot)");
        for (int64_t base = 0; base < count;) {
            const int64_t per = std::min({count - base, cap * world, chunk * world});
            const int64_t rows = (per + world - 1) / world;
            const int64_t lo = std::min(base + per, base + S->x_rank * rows), hi = std::min(base + per, lo + rows);
            if (int rc = run_gates(lo, hi - lo, S->x_slot(rows * n_out), nullptr)) return rc;
            if (int rc = si_exchange(S, rows * n_out)) return rc;
            if (int rc = drain(S)) return rc;
            if (int rc = upload(S, S->d_idx2, out_idx + base * n_out, (size_t)(per * n_out))) return rc;
            hipLaunchKernelGGL(k_rows64, dim3((unsigned)(per * n_out)), dim3(256), 0, S->stream, S->x_gather,
                               (const int32_t *)nullptr, w->d, S->d_idx2.p, dimS);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(S->stream));
            S->x_batches++;
            S->x_rows += rows * n_out * world;
            base += per;
        }
        return 0;
    }
    for (int64_t base = 0; base < count; base += chunk)
        if (int rc = run_gates(base, std::min(chunk, count - base), w->d, out_idx + base * n_out)) return rc;
    return 0;
}

int helm_wop_get_timing(helm_wop_ctx *ctx, helm_wop_timing *out, int reset)
{
    if (!ctx || !out) return fail(HELM_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(ctx->wop->device));
    HIP_TRY(hipStreamSynchronize(ctx->pbs->stream));
    HIP_TRY(hipStreamSynchronize(ctx->wop->stream));
    for (int q = 0; q < 8; q++) WopTimed::fold(ctx, q);
    *out = ctx->tacc;
    if (reset) ctx->tacc = helm_wop_timing{};
    return 0;
}

} // extern "C"
