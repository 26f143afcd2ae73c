// mvm_batch4.hip -- CloverMatrix4 mvm for several right-hand sides: ONE pass over the matrix for up to CLM4_MVM_BATCH_MAX vectors.
//
// The single-vector kernel (matrix4.hip) is bound by the matrix bytes; a caller with several vectors and one matrix (IHT / GD recovery
// of many signals with one Phi) pays them once per vector.  Here a workgroup loads each 16 matrix bytes once and runs the chain
// arithmetic of every vector of the group on them.  The chains of different vectors are independent and each vector's instruction
// sequence is the one of mvm_device.h, so the results equal the single calls bit for bit.
#include "mvm_batch_host.h"
#include "mvm_device.h"
#include "mvm_t4_batch.h"

#include "clover_hip_batch_t.h"

#include <algorithm>
#include <atomic>

// Columns of x staged in LDS per pass.  The single-vector kernel stages 65536 (36 KiB); NV vectors at that size would leave one workgroup
// per CU.  8192 columns are 4 KiB of nibbles + 512 B of block factors per vector: 38 KiB at NV = 8, four workgroups per CU as there.
#define MVMB_CHUNK 8192u
#define MVMB_THREADS 256
#define MVMB_U(NV) ((NV) <= 4 ? 8 : 4)          // 4 accumulators per vector + 4 U registers of matrix words

// MvmBatchArgs / MvmBatchFuse (the vectors of one pass, by value in the kernel arguments): mvm_device.h, shared with the transposed batched
// kernel (mvm_t4_batch.hip)

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
    if constexpr (ST) st_next = mvmb_rng_prologue<NV, NW>(rs, nv, rb, gridDim.x, sbase, st_seq);

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
static std::atomic<uint64_t> g_mvm_batch_launches{0};
extern "C" uint64_t clv_mvm_batch_launches(void) { return g_mvm_batch_launches.load(std::memory_order_relaxed); }
void clv_internal_mvm_batch_count(void) { g_mvm_batch_launches.fetch_add(1, std::memory_order_relaxed); }

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

// what the host driver (mvm_batch_host.h) needs to know of this family
struct Mvm4Batch : MvmBatchByRows {
    template <int NV> using Args = MvmBatchArgs<NV>;
    template <int NV> using Fuse = MvmBatchFuse<NV>;
    static uint64_t matrix_bytes(uint64_t rows, uint64_t cols) { return rows * (cols / 2); }
    static uint64_t vector_bytes(uint64_t n) { return n / 2; }
    static int check_matrix(const char *fn, const int8_t *A, const float *sA, uint64_t rows, uint64_t cols) { return check_mvm_args(fn, A, sA, rows, cols, A, sA); }
    static bool result_may_not_alias_x(bool) { return false; }
    static constexpr auto mvm = clm4_mvm;
    static constexpr auto scale_and_add = clm4_mvm_scale_and_add;
    static constexpr auto iht = clm4_iht;
    static constexpr auto clear = clv_internal_v4_clear;
    static constexpr auto threshold_batch = clv4_threshold_batch;
    // A single clm4_iht at m, n <= 8192 (threshold FAST or none) takes the persistent kernel, 9.4 us per iteration and signal at N = 8192:
    // against it the batched loop was measured for a full group of 8 only (64.2 us per iteration for 8 signals against 75.5),
    // so smaller groups of that class run as single calls (not measured: by the mvm rows a group of 2 would lose).  With an rng the same
    // rule: the full group of 8 beat the stochastic persistent kernel too (80.2 us per iteration for 8 signals against 94.7,
    // profiles/mvm_batch_st_kernel_bench.json).  Elsewhere the single call is the launch-per-step loop with the same three launches per
    // iteration per SIGNAL, and the batched fused mvm was faster at 2, 4 and 8 vectors, either rounding.
    static bool iht_prefers_single(uint64_t m, uint64_t n, uint64_t iterations, int threshold, bool, uint64_t g)
    {
        return g < CLM4_MVM_BATCH_MAX && threshold <= 1 && iterations && m <= 8192 && n <= 8192 && clv_env_int("CLV_IHT_PERSISTENT", 1) != 0;
    }
    template <int NV, bool NT, bool FUSE, bool ST>
    static void launch(dim3 grid, hipStream_t st, const uint8_t *A, const float *sA, uint64_t, uint64_t cols, int nv, const Args<NV> &arg, const Fuse<NV> &fuse,
                       const MvmBatchRng &rs)
    {
        hipLaunchKernelGGL((k_m4_mvm_batch<NV, MVMB_U(NV), NT, FUSE, ST>), grid, dim3(MVMB_THREADS), MVMB_LDS_BYTES(NV, ST, FUSE), st, A, sA, cols, nv,
                           arg, fuse, rs);
    }
};

// ---- C ABI -------------------------------------------------------------------------------------------------------------------
extern "C" int clm4_mvm_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                              const float *const *sx, int8_t *const *r, float *const *sr, uint64_t *rng_state_dev, void *stream)
{
    return mvm_batch_entry<Mvm4Batch>("clm4_mvm_batch", A, sA, rows, cols, nvec, x, sx, r, sr, rng_state_dev, stream);
}

extern "C" int clm4_mvm_batch_at(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                                 const float *const *sx, int8_t *const *r, float *const *sr, uint64_t *rng_state_dev, uint64_t draw_base,
                                 uint64_t draw_stride, uint64_t commit_draws, void *stream)
{
    return mvm_batch_at_entry<Mvm4Batch>("clm4_mvm_batch_at", "clm4_mvm_batch", A, sA, rows, cols, nvec, x, sx, r, sr,
                                         rng_state_dev, draw_base, draw_stride, commit_draws, stream);
}

extern "C" int clm4_mvm_scale_and_add_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec,
                                            const int8_t *const *x, const float *const *sx, const int8_t *const *qu, const float *const *su,
                                            float a, int8_t *const *t, float *const *st_, int8_t *const *r, float *const *sr,
                                            uint64_t *rng_state_dev, void *stream)
{
    return mvm_batch_fused_entry<Mvm4Batch>("clm4_mvm_scale_and_add_batch", A, sA, rows, cols, nvec, x, sx, qu, su, a, t, st_, r, sr,
                                            rng_state_dev, stream);
}

extern "C" int clm4_iht_batch(const int8_t *Phi, const float *sPhi, const int8_t *PhiT, const float *sPhiT, uint64_t m, uint64_t n, uint64_t nvec,
                              int8_t *const *x, float *const *sx, uint64_t x_len, const int8_t *const *y, const float *const *sy,
                              int8_t *const *t1, float *const *st1, int8_t *const *t2, float *const *st2, int8_t *const *t3, float *const *st3,
                              uint64_t iterations, uint64_t K, float mu, int threshold, uint64_t *rng_state_dev, void *stream)
{
    return mvm_batch_iht<Mvm4Batch>("clm4_iht_batch", Phi, sPhi, PhiT, sPhiT, m, n, nvec, x, sx, x_len, y, sy, t1, st1, t2, st2, t3, st3, iterations, K,
                                    mu, threshold, rng_state_dev, stream);
}

// The same loop with ONE matrix (include/clover_hip_batch_t.h): step 1 is this family's fused launch on Phi, step 2 the transposed
// family's (mvm_t4_batch.hip) on the same bytes; the draws lie where the two-matrix loop has them.
extern "C" int clm4_iht_batch_one_matrix(const int8_t *Phi, const float *sPhi, uint64_t m, uint64_t n, uint64_t nvec, int8_t *const *x,
                                         float *const *sx, uint64_t x_len, const int8_t *const *y, const float *const *sy, int8_t *const *t1,
                                         float *const *st1, int8_t *const *t2, float *const *st2, int8_t *const *t3, float *const *st3,
                                         uint64_t iterations, uint64_t K, float mu, int threshold, uint64_t *rng_state_dev, void *stream)
{
    return mvm_batch_iht<Mvm4Batch, MvmT4Batch>("clm4_iht_batch_one_matrix", Phi, sPhi, nullptr, nullptr, m, n, nvec, x, sx, x_len, y, sy, t1, st1, t2,
                                                st2, t3, st3, iterations, K, mu, threshold, rng_state_dev, stream);
}
