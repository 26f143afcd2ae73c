// mvm_batch4.hip -- CloverMatrix4 mvm for several right-hand sides: ONE pass over the matrix for up to CLM4_MVM_BATCH_MAX vectors.
//
// The single-vector kernel (matrix4.hip) is bound by the matrix bytes; a caller with several vectors and one matrix (IHT / GD recovery
// of many signals with one Phi) pays them once per vector.  Here a workgroup loads each 16 matrix bytes once and runs the chain
// arithmetic of every vector of the group on them.  The chains of different vectors are independent and each vector's instruction
// sequence is the one of mvm_device.h, so the results equal the single calls bit for bit.
#include "mvm_batch_device.h"
#include "mvm_device.h"

#include <algorithm>
#include <atomic>
#include <stdlib.h>
#include <string.h>

// Columns of x staged in LDS per pass.  The single-vector kernel stages 65536 (36 KiB); NV vectors at that size would leave one workgroup
// per CU.  8192 columns are 4 KiB of nibbles + 512 B of block factors per vector: 38 KiB at NV = 8, four workgroups per CU as there.
#define MVMB_CHUNK 8192u
#define MVMB_THREADS 256
#define MVMB_U(NV) ((NV) <= 4 ? 8 : 4)          // 4 accumulators per vector + 4 U registers of matrix words

// the vectors of one pass, BY VALUE in the kernel arguments: no pointer table in device memory, nothing to allocate, captures into a graph.
// Slots >= nv are absent: NULL, never dereferenced.
template <int NV>
struct MvmBatchArgs {
    const uint8_t *x[NV];
    const float *sx[NV];
    uint32_t *r[NV];         // all NULL: the mvm result is not stored (FUSE only)
    float *sr[NV];
};
template <int NV>
struct MvmBatchFuse {        // see MvmFuse
    const uint32_t *qu[NV];
    const float *su[NV];
    uint32_t *r2[NV];        // may be qu (in place)
    float *sr2[NV];
    float a;
};

// MvmBatchRng (where the draws of a launch lie in the XORShift stream), wave_pow_apply_many, mvmb_noise and the jump-ahead prologue:
// mvm_batch_device.h, shared with the mixed batched kernel (mvm_batch8.hip)

#define MVMB_X_BYTES(NV) ((NV) * (MVMB_CHUNK / 2 + (MVMB_CHUNK / 64) * sizeof(float) + 64 * sizeof(float)))
// ST: behind the row dots, per vector and window the start of each of the 4 generator lanes (32 B): 512 B at NV = 8 fused, 39 424 B in all
#define MVMB_LDS_BYTES(NV, ST, FUSE) (MVMB_X_BYTES(NV) + ((ST) ? (NV) * ((FUSE) ? 2 : 1) * 4 * sizeof(uint64_t) : 0))

// Registers: the single-vector kernel runs four waves per SIMD (123 VGPRs, 36 KiB of LDS: four workgroups per CU), which is what hides
// the HBM latency.  amdgpu_waves_per_eu(4, 4) holds every instantiation to the same 128 registers; U (matrix loads in flight per lane)
// is chosen per NV so that they fit without scratch: MVMB_U below, figures in DESIGN.md 3.
// Mapping of k_m4_mvm64: workgroup = one 64-row block, lane = (row rho = tid >> 2, quarter q = tid & 3) owning chains 4q..4q+3 of its row;
// per vector 4 accumulators.  Vector v's epilogue (tree result -> re-quantise [-> scaleAndAdd]) runs on wave v & 3.
// ST (stochastic re-quantisation, the epilogue of k_m4_mvm64<., ., true, FUSE>): the jump-ahead runs in the PROLOGUE, before x is staged --
// wave k owns generator lane k and applies T^e for every vector and window to the state it read, in one walk (NV = 8 fused: two) over the table
// levels (wave_pow_apply_many: up to 16 exponents for NV = 8 fused, plus the committed state in workgroup 0), leaving the starts in LDS;
// nothing of it lives in registers across the column loop.  Workgroup 0 stamps the committed state behind the last barrier.
template <int NV, int U, bool NT, bool FUSE, bool ST>
__global__ __launch_bounds__(MVMB_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_m4_mvm_batch(
    const uint8_t *__restrict__ A, const float *__restrict__ sA, uint64_t cols, int nv, MvmBatchArgs<NV> arg, MvmBatchFuse<NV> fuse,
    MvmBatchRng rs)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr uint32_t XS = MVMB_CHUNK / 32, CS = MVMB_CHUNK / 64;          // per vector: u32x4 of x, factors
    u32x4 *xs = reinterpret_cast<u32x4 *>(smem);                            // NV x MVMB_CHUNK / 2 bytes
    float *cs = reinterpret_cast<float *>(smem + NV * (MVMB_CHUNK / 2));    // NV x MVMB_CHUNK / 64 factors c[b] = (sA[b] * 1/49) * sx[b]
    float *dsh = cs + NV * CS;                                              // NV x 64 row dots
    static_assert(XS == MVMB_THREADS && 2 * CS == MVMB_THREADS, "one u32x4 of x per thread and vector, one factor per thread of the first two waves");
    constexpr int NW = FUSE ? 2 : 1;                                        // windows per vector: the mvm's draws, the scaleAndAdd's
    uint64_t *sbase = reinterpret_cast<uint64_t *>(dsh + NV * 64);          // ST: [NV][NW][4] lane starts

    const uint64_t rb = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t st_seq = 0;
    uint64_t *st_next = nullptr;
    if constexpr (ST) st_next = mvmb_rng_prologue<NV, NW>(rs, nv, rb, sbase, st_seq);

    const int q = tid & 3, rho = tid >> 2;
    const uint64_t row = rb * 64 + rho;
    const u32x4 *Arow = reinterpret_cast<const u32x4 *>(A + row * (cols / 2));
    const float *sArow = sA + rb * (cols / 64);

    float acc[NV][4];
#pragma unroll
    for (int v = 0; v < NV; v++) acc[v][0] = acc[v][1] = acc[v][2] = acc[v][3] = 0.0f;

    for (uint64_t c0 = 0; c0 < cols; c0 += MVMB_CHUNK) {
        const uint32_t cw = (uint32_t)((cols - c0) < MVMB_CHUNK ? (cols - c0) : MVMB_CHUNK);
        if (c0) __syncthreads();
        {   // stage x and c[b] of every present vector: the loads first, then the LDS writes
            const uint32_t nx = cw / 32, nc = cw / 64;
            const uint32_t ix = (uint32_t)tid < nx ? tid : 0, ic = (uint32_t)tid < nc ? tid : 0;
            u32x4 xr[NV];
            float sv[NV];
            const float sa = sArow[c0 / 64 + ic];
#pragma unroll
            for (int v = 0; v < NV; v++)
                if (v < nv) {
                    xr[v] = reinterpret_cast<const u32x4 *>(arg.x[v] + c0 / 2)[ix];
                    sv[v] = arg.sx[v][c0 / 64 + ic];
                }
#pragma unroll
            for (int v = 0; v < NV; v++)
                if (v < nv) {
                    if ((uint32_t)tid < nx) xs[v * XS + tid] = xr[v];
                    if ((uint32_t)tid < nc) cs[v * CS + tid] = (sa * CLV_RCP49) * sv[v];
                }
        }
        __syncthreads();

        const u32x4 *Ap = Arow + c0 / 32;
        const uint32_t npairs = cw / 128;
        uint32_t t = 0;
        for (; t + U <= npairs; t += U) {
            u32x4 a[U];
            mvm_load<U, NT>(Ap, q, t, a);                                   // each matrix dwordx4 ONCE for all vectors
#pragma unroll
            for (int v = 0; v < NV; v++)
                if (v < nv) mvm_consume<U>(a, xs + v * XS, cs + v * CS, q, t, acc[v][0], acc[v][1], acc[v][2], acc[v][3]);
        }
        for (; t < npairs; t++) {
            u32x4 a[1];
            mvm_load<1, NT>(Ap, q, t, a);
#pragma unroll
            for (int v = 0; v < NV; v++)
                if (v < nv) mvm_consume<1>(a, xs + v * XS, cs + v * CS, q, t, acc[v][0], acc[v][1], acc[v][2], acc[v][3]);
        }
    }

    // FUSE: this row group's block of u of the vectors whose epilogue this wave runs, requested here, behind the
    // column loop (they would cost registers across it), so that the tree and the barrier cover the latency
    uint32_t fuse_w[(NV + 3) / 4] = {};
    float fuse_s[(NV + 3) / 4] = {};
    if (FUSE) {
#pragma unroll
        for (int v = 0; v < NV; v++)
            if (v < nv && wave == (v & 3)) {
                fuse_w[v >> 2] = fuse.qu[v][rb * 8 + (lane >> 3)];
                fuse_s[v >> 2] = fuse.su[v][rb];
            }
    }

#pragma unroll
    for (int v = 0; v < NV; v++)
        if (v < nv) {
            const float dot = mvm_tree(acc[v][0], acc[v][1], acc[v][2], acc[v][3]);
            if (q == 0) dsh[v * 64 + rho] = dot;
        }
    __syncthreads();
    if constexpr (ST) mvmb_rng_stamp(st_next, st_seq);        // every wave's part of the new state was written before the barrier
#pragma unroll
    for (int v = 0; v < NV; v++)
        if (v < nv && wave == (v & 3)) {
            uint32_t *r = arg.r[v];
            float m, noise = 0.0f;
            if constexpr (ST) noise = mvmb_noise(sbase + (v * NW) * 4, lane & 7, lane >> 3);
            const int qv = requantize_wave(dsh[v * 64 + lane], noise, r ? r + rb * 8 : nullptr, r ? arg.sr[v] + rb : nullptr, &m);
            if (FUSE) {
                const float su7 = div7(fuse_s[v >> 2]), sv7 = div7(m * fuse.a);
                const float val = __builtin_fmaf((float)qv, sv7, (float)unpack1(fuse_w[v >> 2], lane & 7) * su7);
                float m2, noise2 = 0.0f;
                if constexpr (ST) noise2 = mvmb_noise(sbase + (v * NW + 1) * 4, (lane & 7) ^ 1, lane >> 3);
                requantize_wave(val, noise2, fuse.r2[v] + rb * 8, fuse.sr2[v] + rb, &m2);
            }
        }
}

// ---- overlap check of the batch calls -----------------------------------------------------------------------------------------
static void range_error(const char *fn, const ClvRange &a, const ClvRange &b)
{
    char va[40], vb[40];
    auto who = [](const ClvRange &r, char *buf) {
        if (r.vec == ~0ull) snprintf(buf, 40, "the matrix");
        else snprintf(buf, 40, "vector %llu", (unsigned long long)r.vec);
    };
    who(a, va);
    who(b, vb);
    clv_set_error("%s: %s `%s` of %s overlaps %s `%s` of %s", fn, a.output ? "output" : "input", a.name, va, b.output ? "output" : "input", b.name, vb);
}

int clv_internal_check_ranges(const char *fn, std::vector<ClvRange> &ranges)
{
    std::sort(ranges.begin(), ranges.end(), [](const ClvRange &a, const ClvRange &b) { return a.begin < b.begin; });
    const ClvRange *out = nullptr, *in = nullptr;          // of the ranges seen so far: the output / the input that ends last
    for (const ClvRange &r : ranges) {
        if (r.begin == r.end) continue;
        if (out && out->end > r.begin) { range_error(fn, r, *out); return CLV_ERR_INVALID; }
        if (r.output && in && in->end > r.begin) { range_error(fn, r, *in); return CLV_ERR_INVALID; }
        const ClvRange *&last = r.output ? out : in;
        if (!last || r.end > last->end) last = &r;
    }
    return CLV_OK;
}

// ---- dispatch ----------------------------------------------------------------------------------------------------------------
// Whether a group of g vectors runs as one batched launch or as g single launches.  CLV_MVM_BATCH (read on every call, as
// CLV_IHT_PERSISTENT: the tests and tools/kernel_bench.py flip it inside one process): 1 = always batched, 0 = never; unset = the rule
// measured on the MI355X (profiles/mvm_batch_kernel_bench.json; stochastic: profiles/mvm_batch_st_kernel_bench.json).
// With an rng, CLV_MVM_BATCH=1 also puts a remainder group of ONE vector (nvec = 9, 17, ...) on the batched kernel: a forced call then hands
// the state from batched launch to batched launch throughout, which is what the tests of that hand-over need.
static bool mvm_batch_selected(uint64_t rows, uint64_t cols, uint64_t g, bool stochastic)
{
    if (g < 2 && !stochastic) return false;
    const char *e = clv_env("CLV_MVM_BATCH");
    if (e && *e) return atoi(e) != 0;
    if (g < 2) return false;
    (void)rows;
    (void)cols;
    return true;
}

static std::atomic<uint64_t> g_mvm_batch_launches{0};
extern "C" uint64_t clv_mvm_batch_launches(void) { return g_mvm_batch_launches.load(std::memory_order_relaxed); }
void clv_internal_mvm_batch_count(void) { g_mvm_batch_launches.fetch_add(1, std::memory_order_relaxed); }

// the draws of a batched launch on the host side: rng == NULL = rounding disabled
struct MvmBatchDraws {
    uint64_t *rng;
    uint64_t base, stride, commit;
};

template <int NV>
static int launch_mvm_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t g, const int8_t *const *x,
                            const float *const *sx, int8_t *const *r, float *const *sr, const int8_t *const *qu, const float *const *su,
                            float a, int8_t *const *r2, float *const *sr2, const MvmBatchDraws &dr, hipStream_t st)
{
    MvmBatchArgs<NV> arg;
    MvmBatchFuse<NV> fuse;
    for (uint64_t v = 0; v < NV; v++) {
        const bool in = v < g;
        arg.x[v] = in ? (const uint8_t *)x[v] : nullptr;
        arg.sx[v] = in ? sx[v] : nullptr;
        arg.r[v] = in && r ? (uint32_t *)r[v] : nullptr;
        arg.sr[v] = in && r ? sr[v] : nullptr;
        fuse.qu[v] = in && qu ? (const uint32_t *)qu[v] : nullptr;
        fuse.su[v] = in && qu ? su[v] : nullptr;
        fuse.r2[v] = in && qu ? (uint32_t *)r2[v] : nullptr;
        fuse.sr2[v] = in && qu ? sr2[v] : nullptr;
    }
    fuse.a = a;
    MvmBatchRng rs = {nullptr, 0, nullptr, 0, 0, 0};
    if (dr.rng) {
        RngTables T = {nullptr, nullptr, nullptr};
        int rc = clv_rng_tables(&T);
        if (rc) return rc;
        // every launch takes a number of its own, committing or not: it is what picks the slot to read
        rs = MvmBatchRng{dr.rng, clv_rng_seq_for(dr.rng, st), T.pow_rows, dr.base, dr.stride, dr.commit};
    }
    const dim3 grid((unsigned)(rows / 64)), block(MVMB_THREADS);
    // nontemporal loads by the rule of launch_mvm: once the matrix cannot live in the 256 MiB Infinity Cache
    const bool streaming = rows * (cols / 2) > (256ull << 20);
#define MVMB_LAUNCH(NT, FUSE, ST)                                                                                                       \
    hipLaunchKernelGGL((k_m4_mvm_batch<NV, MVMB_U(NV), NT, FUSE, ST>), grid, block, MVMB_LDS_BYTES(NV, ST, FUSE), st, (const uint8_t *)A, sA, \
                       cols, (int)g, arg, fuse, rs)
#define MVMB_LAUNCH_R(NT, FUSE) do { if (dr.rng) MVMB_LAUNCH(NT, FUSE, true); else MVMB_LAUNCH(NT, FUSE, false); } while (0)
    if (streaming) { if (qu) MVMB_LAUNCH_R(true, true); else MVMB_LAUNCH_R(true, false); }
    else { if (qu) MVMB_LAUNCH_R(false, true); else MVMB_LAUNCH_R(false, false); }
#undef MVMB_LAUNCH_R
#undef MVMB_LAUNCH
    CLV_LAUNCH_CHECK();
    clv_internal_mvm_batch_count();
    return CLV_OK;
}

static int launch_group(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t j0, uint64_t g, const int8_t *const *x,
                        const float *const *sx, int8_t *const *r, float *const *sr, const int8_t *const *qu, const float *const *su, float a,
                        int8_t *const *r2, float *const *sr2, const MvmBatchDraws &dr, hipStream_t st)
{
#define MVMB_GROUP(NV) \
    launch_mvm_batch<NV>(A, sA, rows, cols, g, x + j0, sx + j0, r ? r + j0 : nullptr, r ? sr + j0 : nullptr, qu ? qu + j0 : nullptr, \
                         qu ? su + j0 : nullptr, a, qu ? r2 + j0 : nullptr, qu ? sr2 + j0 : nullptr, dr, st)
    return g <= 2 ? MVMB_GROUP(2) : g <= 4 ? MVMB_GROUP(4) : MVMB_GROUP(8);
#undef MVMB_GROUP
}

// the checked arguments of clm4_mvm_batch (qu == NULL) / clm4_mvm_scale_and_add_batch on the stream, group by group; r / sr NULL: the mvm
// result is not stored (fused form only).  With an rng every group starts at the state the group before it left: a batched group's windows
// lie 2 G (fused: 4 G) draws apart from position 0 and its launch commits all of them, a forwarded group's single calls advance the state
// themselves -- so the two kinds mix freely.
int clv_internal_mvm_batch_run(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                               const float *const *sx, int8_t *const *r, float *const *sr, const int8_t *const *qu, const float *const *su,
                               float a, int8_t *const *r2, float *const *sr2, uint64_t *rng, void *stream)
{
    hipStream_t st = as_stream(stream);
    const uint64_t per_vector = (qu ? 4ull : 2ull) * (rows / 64);
    for (uint64_t j0 = 0; j0 < nvec; j0 += CLM4_MVM_BATCH_MAX) {
        const uint64_t g = nvec - j0 < CLM4_MVM_BATCH_MAX ? nvec - j0 : CLM4_MVM_BATCH_MAX;
        int rc = CLV_OK;
        if (!mvm_batch_selected(rows, cols, g, rng != nullptr)) {
            for (uint64_t j = j0; j < j0 + g && !rc; j++)
                rc = qu ? clm4_mvm_scale_and_add(A, sA, rows, cols, x[j], sx[j], qu[j], su[j], a, r ? r[j] : nullptr, r ? sr[j] : nullptr, r2[j],
                                                 sr2[j], rng, stream)
                        : clm4_mvm(A, sA, rows, cols, x[j], sx[j], r[j], sr[j], rng, stream);
        } else {
            rc = launch_group(A, sA, rows, cols, j0, g, x, sx, r, sr, qu, su, a, r2, sr2, MvmBatchDraws{rng, 0, per_vector, g * per_vector}, st);
        }
        if (rc) return rc;
    }
    return CLV_OK;
}

// The positioned form: vector j's window begins draw_base + j * draw_stride draws behind the state the call finds, across groups too;
// only the last group's launch commits.  Always the batched kernel (a window that is not where a single call would draw cannot be
// forwarded).  rng == NULL: the deterministic kernel, the positions unused.  The caller has checked the positions (clv_internal_first_bad_window).
int clv_internal_mvm_batch_at(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                              const float *const *sx, int8_t *const *r, float *const *sr, const int8_t *const *qu, const float *const *su,
                              float a, int8_t *const *r2, float *const *sr2, uint64_t *rng, uint64_t draw_base, uint64_t draw_stride,
                              uint64_t commit_draws, void *stream)
{
    hipStream_t st = as_stream(stream);
    for (uint64_t j0 = 0; j0 < nvec; j0 += CLM4_MVM_BATCH_MAX) {
        const uint64_t g = nvec - j0 < CLM4_MVM_BATCH_MAX ? nvec - j0 : CLM4_MVM_BATCH_MAX;
        const bool last = j0 + g == nvec;
        int rc = launch_group(A, sA, rows, cols, j0, g, x, sx, r, sr, qu, su, a, r2, sr2,
                              MvmBatchDraws{rng, draw_base + j0 * draw_stride, draw_stride, last ? commit_draws : 0}, st);
        if (rc) return rc;
    }
    return CLV_OK;
}

// the first of nvec windows of `window` draws each that does not end at or below 2^55, the exponents wave_pow_apply has table levels
// for; nvec if there is none
uint64_t clv_internal_first_bad_window(uint64_t nvec, uint64_t draw_base, uint64_t draw_stride, uint64_t window)
{
    const unsigned __int128 lim = (unsigned __int128)1 << (RNG_POW_LEVELS - 1);
    for (uint64_t j = 0; j < nvec; j++) {
        if ((unsigned __int128)draw_base + (unsigned __int128)j * draw_stride + window > lim) return j;
        if (!draw_stride) break;
    }
    return nvec;
}

// ---- C ABI -------------------------------------------------------------------------------------------------------------------
// every check of both calls, before any device work
static int check_batch_args(const char *fn, const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                            const float *const *sx, const int8_t *const *qu, const float *const *su, int8_t *const *t, float *const *st_,
                            int8_t *const *r, float *const *sr, bool fused)
{
    // a NULL vector array is reported as such, not as one of check_mvm_args' pointers
    int rc = check_mvm_args(fn, A, sA, rows, cols, A, sA);
    if (rc) return rc;
    if (!nvec) return CLV_OK;
    CLV_REQUIRE(x && sx && r && sr && (!fused || (qu && su)), "%s: null pointer array", fn);
    CLV_REQUIRE((t == nullptr) == (st_ == nullptr), "%s: t and st must both be given or both be NULL", fn);
    for (uint64_t j = 0; j < nvec; j++)
        CLV_REQUIRE(x[j] && sx[j] && r[j] && sr[j] && (!fused || (qu[j] && su[j])) && (!t || (t[j] && st_[j])), "%s: null pointer in vector %llu", fn,
                    (unsigned long long)j);
    std::vector<ClvRange> rg;
    rg.reserve(8 * nvec + 2);
    const uint64_t sc = sizeof(float);
    rg.push_back(clv_range(A, rows * (cols / 2), false, ~0ull, "A"));
    rg.push_back(clv_range(sA, (rows / 64) * (cols / 64) * sc, false, ~0ull, "sA"));
    for (uint64_t j = 0; j < nvec; j++) {
        rg.push_back(clv_range(x[j], cols / 2, false, j, "x"));
        rg.push_back(clv_range(sx[j], cols / 64 * sc, false, j, "sx"));
        rg.push_back(clv_range(r[j], rows / 2, true, j, "r"));
        rg.push_back(clv_range(sr[j], rows / 64 * sc, true, j, "sr"));
        if (fused) {
            // the in-place form r[j] == qu[j], sr[j] == su[j]: the result IS the input, only workgroup rb touches block rb of either
            const bool in_place = (const void *)r[j] == (const void *)qu[j] && (const void *)sr[j] == (const void *)su[j];
            if (!in_place) {
                rg.push_back(clv_range(qu[j], rows / 2, false, j, "qu"));
                rg.push_back(clv_range(su[j], rows / 64 * sc, false, j, "su"));
            }
        }
        if (t) {
            rg.push_back(clv_range(t[j], rows / 2, true, j, "t"));
            rg.push_back(clv_range(st_[j], rows / 64 * sc, true, j, "st"));
        }
    }
    return clv_internal_check_ranges(fn, rg);
}

extern "C" int clm4_mvm_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                              const float *const *sx, int8_t *const *r, float *const *sr, uint64_t *rng_state_dev, void *stream)
{
    int rc = check_batch_args("clm4_mvm_batch", A, sA, rows, cols, nvec, x, sx, nullptr, nullptr, nullptr, nullptr, r, sr, false);
    if (rc) return rc;
    if (!nvec || !rows) return CLV_OK;
    if (nvec == 1) return clm4_mvm(A, sA, rows, cols, x[0], sx[0], r[0], sr[0], rng_state_dev, stream);
    return clv_internal_mvm_batch_run(A, sA, rows, cols, nvec, x, sx, r, sr, nullptr, nullptr, 0.0f, nullptr, nullptr, rng_state_dev, stream);
}

extern "C" int clm4_mvm_batch_at(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                                 const float *const *sx, int8_t *const *r, float *const *sr, uint64_t *rng_state_dev, uint64_t draw_base,
                                 uint64_t draw_stride, uint64_t commit_draws, void *stream)
{
    const char *fn = "clm4_mvm_batch_at";
    int rc = check_batch_args(fn, A, sA, rows, cols, nvec, x, sx, nullptr, nullptr, nullptr, nullptr, r, sr, false);
    if (rc) return rc;
    if (!rng_state_dev) return clm4_mvm_batch(A, sA, rows, cols, nvec, x, sx, r, sr, nullptr, stream);
    CLV_REQUIRE(commit_draws < (1ull << (RNG_POW_LEVELS - 1)), "%s: commit_draws=%llu must stay below 2^55", fn, (unsigned long long)commit_draws);
    const uint64_t bad = clv_internal_first_bad_window(nvec, draw_base, draw_stride, 2 * (rows / 64));
    CLV_REQUIRE(bad == nvec, "%s: the draws of vector %llu (draw_base=%llu, draw_stride=%llu) do not stay below 2^55", fn, (unsigned long long)bad,
                (unsigned long long)draw_base, (unsigned long long)draw_stride);
    if (!nvec || !rows) return CLV_OK;
    return clv_internal_mvm_batch_at(A, sA, rows, cols, nvec, x, sx, r, sr, nullptr, nullptr, 0.0f, nullptr, nullptr, rng_state_dev, draw_base,
                                     draw_stride, commit_draws, stream);
}

extern "C" int clm4_mvm_scale_and_add_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec,
                                            const int8_t *const *x, const float *const *sx, const int8_t *const *qu, const float *const *su,
                                            float a, int8_t *const *t, float *const *st_, int8_t *const *r, float *const *sr,
                                            uint64_t *rng_state_dev, void *stream)
{
    int rc = check_batch_args("clm4_mvm_scale_and_add_batch", A, sA, rows, cols, nvec, x, sx, qu, su, t, st_, r, sr, true);
    if (rc) return rc;
    if (!nvec || !rows) return CLV_OK;
    if (nvec == 1)
        return clm4_mvm_scale_and_add(A, sA, rows, cols, x[0], sx[0], qu[0], su[0], a, t ? t[0] : nullptr, t ? st_[0] : nullptr, r[0], sr[0],
                                      rng_state_dev, stream);
    return clv_internal_mvm_batch_run(A, sA, rows, cols, nvec, x, sx, t, st_, qu, su, a, r, sr, rng_state_dev, stream);
}
