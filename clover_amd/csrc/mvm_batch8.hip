// mvm_batch8.hip -- CloverMatrix4 x CloverVector8 (the configuration the reference publishes as "4-bit", 02_bit04.cpp:140) for several
// right-hand sides: ONE pass over the matrix for up to CLM4_MVM_BATCH_MAX vectors, as mvm_batch4.hip does for CloverVector4.
//
// The single-vector kernel k_m4_mvm8 (mixed8.hip) is bound by VALU work as well as by the matrix bytes: per matrix dword a quad transpose,
// two masks and two v_perm_b32 before any arithmetic with x.  Here a workgroup loads, transposes and widens each 16 matrix bytes once and
// runs only the per-vector part -- the LDS reads of x, four v_dot4_i32_i8, two shifts, two converts and two fmas per block -- for every
// vector of the group.  Each vector's instruction sequence is the one of mvm8_device.h, so the results equal the single calls bit for bit.
#include "mvm_batch_host.h"
#include "mvm8_device.h"
#include "mvm_t8_batch.h"

#include "clover_hip_batch_t_v8.h"

// Columns of x staged in LDS per pass.  The single-vector kernel stages 32768 (32 KiB + factors); NV vectors at that size would not fit.
// 4096 columns are 4 KiB of int8 + 256 B of block factors + 256 B of row dots per vector: 36 KiB at NV = 8 (36.5 KiB with the generator
// starts of the fused stochastic form), four workgroups per CU out of 160 KiB.
#define MVMB8_CHUNK 4096u
#define MVMB8_THREADS 256
#define MVMB8_U(NV) ((NV) <= 4 ? 8 : 4)         // 16-byte matrix loads in flight per lane: 2 accumulators per vector + 4 U registers of matrix words

// Mvm8BatchArgs / Mvm8BatchFuse (the vectors of one pass, by value in the kernel arguments): mvm8_device.h, shared with the transposed batched
// kernel (mvm_t8_batch.hip)

#define MVMB8_X_BYTES(NV) ((NV) * (MVMB8_CHUNK + (MVMB8_CHUNK / 64) * sizeof(float) + 64 * sizeof(float)))
// ST: behind the row dots, per vector and window the start of each of the 4 generator lanes (32 B): 512 B at NV = 8 fused
#define MVMB8_LDS_BYTES(NV, ST, FUSE) (MVMB8_X_BYTES(NV) + ((ST) ? (NV) * ((FUSE) ? 2 : 1) * 4 * sizeof(uint64_t) : 0))

// one step = 128 columns of this lane's row: the quad's 64 bytes transposed and widened ONCE, then every vector's chains
template <int NV>
__device__ __forceinline__ void mvmb8_step(const u32x4 av, uint32_t t, int m, int nv, const u32x4 *xs, const float *cs, float (&a_even)[NV],
                                           float (&a_odd)[NV])
{
    constexpr uint32_t XS = MVMB8_CHUNK / 16, CS = MVMB8_CHUNK / 64;
    uint32_t w0 = av.x, w1 = av.y, w2 = av.z, w3 = av.w;
    quad_transpose4(w0, w1, w2, w3, m);               // now: word m, word 4+m of block 2t; word m, word 4+m of the next
    const Mvm8Words b0 = mvm8_widen(w0, w1), b1 = mvm8_widen(w2, w3);
    const uint32_t b = 2 * t;
#pragma unroll
    for (int v = 0; v < NV; v++)
        if (v < nv) {
            const u32x2 *xq = reinterpret_cast<const u32x2 *>(xs + v * XS);
            mvm8_dot(b0, xq + 8 * b, m, cs[v * CS + b], a_even[v], a_odd[v]);
            mvm8_dot(b1, xq + 8 * (b + 1), m, cs[v * CS + b + 1], a_even[v], a_odd[v]);
        }
}

// Mapping of k_m4_mvm8: workgroup = one 64-row group, lane = (row rho = tid >> 2, m = tid & 3) owning chains 2m and 2m+1 of its row; per
// vector 2 accumulators.  amdgpu_waves_per_eu(4, 4) holds every instantiation to 128 registers (four waves per SIMD, as the single kernel);
// U is chosen per NV so that they fit without scratch (figures: DESIGN.md 3).  Vector v's epilogue (tree result -> re-quantise
// [-> scaleAndAdd]) runs on wave v & 3.  ST: the jump-ahead of k_m4_mvm_batch (mvm_batch_device.h); the draw layout is k_m4_mvm8's.
template <int NV, int U, bool NT, bool FUSE, bool ST>
__global__ __launch_bounds__(MVMB8_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_m4_mvm8_batch(
    const uint8_t *__restrict__ A, const float *__restrict__ sA, uint64_t cols, int nv, Mvm8BatchArgs<NV> arg, Mvm8BatchFuse<NV> fuse,
    MvmBatchRng rs)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr uint32_t XS = MVMB8_CHUNK / 16, CS = MVMB8_CHUNK / 64;        // per vector: u32x4 of x, factors
    u32x4 *xs = reinterpret_cast<u32x4 *>(smem);                            // NV x MVMB8_CHUNK bytes of int8
    float *cs = reinterpret_cast<float *>(smem + NV * MVMB8_CHUNK);         // NV x MVMB8_CHUNK / 64 factors
    float *dsh = cs + NV * CS;                                              // NV x 64 row dots
    static_assert(XS == MVMB8_THREADS && CS == 64, "one u32x4 of x per thread and vector, one factor per lane of the first wave");
    constexpr int NW = FUSE ? 2 : 1;                                        // windows per vector: the mvm's draws, the scaleAndAdd's
    uint64_t *sbase = reinterpret_cast<uint64_t *>(dsh + NV * 64);          // ST: [NV][NW][4] lane starts

    const uint64_t rb = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t st_seq = 0;
    uint64_t *st_next = nullptr;
    if constexpr (ST) st_next = mvmb_rng_prologue<NV, NW>(rs, nv, rb, gridDim.x, sbase, st_seq);

    const int m = tid & 3, rho = tid >> 2;
    const uint64_t row = rb * 64 + rho;
    const u32x4 *Arow = reinterpret_cast<const u32x4 *>(A + row * (cols / 2));
    const float *sArow = sA + rb * (cols / 64);

    float a_even[NV], a_odd[NV];
#pragma unroll
    for (int v = 0; v < NV; v++) a_even[v] = a_odd[v] = 0.0f;

    for (uint64_t c0 = 0; c0 < cols; c0 += MVMB8_CHUNK) {
        const uint32_t cw = (uint32_t)((cols - c0) < MVMB8_CHUNK ? (cols - c0) : MVMB8_CHUNK);
        if (c0) __syncthreads();
        {   // stage x and the factors of every present vector: the loads first, then the LDS writes
            const uint32_t nx = cw / 16, nc = cw / 64;
            const uint32_t ix = (uint32_t)tid < nx ? tid : 0, ic = (uint32_t)tid < nc ? tid : 0;
            u32x4 xr[NV];
            float sv[NV];
            const float sa = sArow[c0 / 64 + ic];
#pragma unroll
            for (int v = 0; v < NV; v++)
                if (v < nv) {
                    xr[v] = reinterpret_cast<const u32x4 *>(arg.x[v] + c0)[ix];
                    sv[v] = arg.sx[v][c0 / 64 + ic];
                }
#pragma unroll
            for (int v = 0; v < NV; v++)
                if (v < nv) {
                    if ((uint32_t)tid < nx) xs[v * XS + tid] = xr[v];
                    if ((uint32_t)tid < nc) cs[v * CS + tid] = mvm8_factor(sa, sv[v]);
                }
        }
        __syncthreads();

        const u32x4 *Ap = Arow + c0 / 32;
        const uint32_t nsteps = cw / 128;                                   // two blocks per step
        uint32_t t = 0;
        for (; t + U <= nsteps; t += U) {
            u32x4 a[U];                                                     // each matrix dwordx4 ONCE for all vectors
#pragma unroll
            for (int u = 0; u < U; u++) a[u] = NT ? __builtin_nontemporal_load(&Ap[4 * (t + u) + m]) : Ap[4 * (t + u) + m];
#pragma unroll
            for (int u = 0; u < U; u++) mvmb8_step<NV>(a[u], t + u, m, nv, xs, cs, a_even, a_odd);
        }
        for (; t < nsteps; t++) {
            const u32x4 av = NT ? __builtin_nontemporal_load(&Ap[4 * t + m]) : Ap[4 * t + m];
            mvmb8_step<NV>(av, t, m, nv, xs, cs, a_even, a_odd);
        }
    }

    // FUSE: this row group's block of u of the vectors whose epilogue this wave runs, requested here, behind the
    // column loop (they would cost registers across it), so that the tree and the barrier cover the latency
    int fuse_q[(NV + 3) / 4] = {};
    float fuse_s[(NV + 3) / 4] = {};
    if (FUSE) {
#pragma unroll
        for (int v = 0; v < NV; v++)
            if (v < nv && wave == (v & 3)) {
                fuse_q[v >> 2] = fuse.qu[v][rb * 64 + lane];
                fuse_s[v >> 2] = fuse.su[v][rb];
            }
    }

#pragma unroll
    for (int v = 0; v < NV; v++)
        if (v < nv) {
            const float dot = mvm8_tree(a_even[v], a_odd[v]);
            if (m == 0) dsh[v * 64 + rho] = dot;
        }
    __syncthreads();
    if constexpr (ST) mvmb_rng_stamp(st_next, st_seq);        // every wave's part of the new state was written before the barrier
#pragma unroll
    for (int v = 0; v < NV; v++)
        if (v < nv && wave == (v & 3)) {
            int8_t *r = arg.r[v];
            float noise = 0.0f, noise2 = 0.0f;
            if constexpr (ST) {
                // k_m4_mvm8's lanes.  mvm: lane l takes word l & 7 of draw (l >> 3) >> 2, byte (l >> 3) & 3;
                // scaleAndAdd: draw l >> 5, word (l & 31) >> 2, byte l & 3
                noise = mvmb_noise(sbase + (v * NW) * 4, lane >> 3, lane & 7);
                if (FUSE) noise2 = mvmb_noise(sbase + (v * NW + 1) * 4, ((lane >> 5) << 2) | (lane & 3), (lane & 31) >> 2);
            }
            mvm8_requantize_wave<FUSE>(dsh[v * 64 + lane], noise, noise2, lane, r ? r + rb * 64 : nullptr, r ? arg.sr[v] + rb : nullptr,
                                       fuse_q[v >> 2], fuse_s[v >> 2], fuse.a, FUSE ? fuse.r2[v] + rb * 64 : nullptr,
                                       FUSE ? fuse.sr2[v] + rb : nullptr);
        }
}

// ---- dispatch ----------------------------------------------------------------------------------------------------------------
// what the host driver (mvm_batch_host.h) needs to know of this family
struct Mvm8Batch : MvmBatchByRows {
    template <int NV> using Args = Mvm8BatchArgs<NV>;
    template <int NV> using Fuse = Mvm8BatchFuse<NV>;
    static uint64_t matrix_bytes(uint64_t rows, uint64_t cols) { return rows * (cols / 2); }
    static uint64_t vector_bytes(uint64_t n) { return n; }
    static int check_matrix(const char *fn, const int8_t *A, const float *sA, uint64_t rows, uint64_t cols) { return check_mvm8_args(fn, A, sA, rows, cols, A, sA); }
    static bool result_may_not_alias_x(bool fused) { return fused; }
    static constexpr auto mvm = clm4_mvm_v8;
    static constexpr auto scale_and_add = clm4_mvm_v8_scale_and_add;
    static constexpr auto iht = clm4_iht_v8;
    static constexpr auto clear = clv_internal_v8_clear;
    static constexpr auto threshold_batch = clv8_threshold_batch;
    // Where a single clm4_iht_v8 takes the persistent kernel (clm4_iht_v8_persistent_eligible) the comparison is against g x that kernel,
    // measured for a full group of 8 at N = 8192 (profiles/mvm_v8_batch_kernel_bench.json and ..._st_...): rounding disabled
    // 113.4 us per iteration for 8 signals batched against 107.0 -- slower, so no group of that class runs batched; with an rng 127.5
    // against 133.1, so the full group does.  Smaller groups of that class were not measured and run as single calls.  Elsewhere the single
    // call is the launch-per-step loop with the same three launches per iteration per SIGNAL, and the batched fused mvm was faster at 2, 4
    // and 8 vectors, either rounding.
    static bool iht_prefers_single(uint64_t m, uint64_t n, uint64_t iterations, int threshold, bool stochastic, uint64_t g)
    {
        return !(stochastic && g == CLM4_MVM_BATCH_MAX) && clm4_iht_v8_persistent_eligible(m, n, iterations, threshold, stochastic);
    }
    template <int NV, bool NT, bool FUSE, bool ST>
    static void launch(dim3 grid, hipStream_t st, const uint8_t *A, const float *sA, uint64_t, uint64_t cols, int nv, const Args<NV> &arg, const Fuse<NV> &fuse,
                       const MvmBatchRng &rs)
    {
        hipLaunchKernelGGL((k_m4_mvm8_batch<NV, MVMB8_U(NV), NT, FUSE, ST>), grid, dim3(MVMB8_THREADS), MVMB8_LDS_BYTES(NV, ST, FUSE), st, A, sA, cols,
                           nv, arg, fuse, rs);
    }
};

// ---- C ABI -------------------------------------------------------------------------------------------------------------------
extern "C" int clm4_mvm_v8_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                                 const float *const *sx, int8_t *const *r, float *const *sr, uint64_t *rng_state_dev, void *stream)
{
    return mvm_batch_entry<Mvm8Batch>("clm4_mvm_v8_batch", A, sA, rows, cols, nvec, x, sx, r, sr, rng_state_dev, stream);
}

extern "C" int clm4_mvm_v8_batch_at(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                                    const float *const *sx, int8_t *const *r, float *const *sr, uint64_t *rng_state_dev, uint64_t draw_base,
                                    uint64_t draw_stride, uint64_t commit_draws, void *stream)
{
    return mvm_batch_at_entry<Mvm8Batch>("clm4_mvm_v8_batch_at", "clm4_mvm_v8_batch", A, sA, rows, cols, nvec, x, sx, r, sr,
                                         rng_state_dev, draw_base, draw_stride, commit_draws, stream);
}

extern "C" int clm4_mvm_v8_scale_and_add_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec,
                                               const int8_t *const *x, const float *const *sx, const int8_t *const *qu, const float *const *su,
                                               float a, int8_t *const *t, float *const *st_, int8_t *const *r, float *const *sr,
                                               uint64_t *rng_state_dev, void *stream)
{
    return mvm_batch_fused_entry<Mvm8Batch>("clm4_mvm_v8_scale_and_add_batch", A, sA, rows, cols, nvec, x, sx, qu, su, a, t, st_, r, sr,
                                            rng_state_dev, stream);
}

extern "C" int clm4_iht_v8_batch(const int8_t *Phi, const float *sPhi, const int8_t *PhiT, const float *sPhiT, uint64_t m, uint64_t n, uint64_t nvec,
                                 int8_t *const *x, float *const *sx, uint64_t x_len, const int8_t *const *y, const float *const *sy,
                                 int8_t *const *t1, float *const *st1, int8_t *const *t2, float *const *st2, int8_t *const *t3, float *const *st3,
                                 uint64_t iterations, uint64_t K, float mu, int threshold, uint64_t *rng_state_dev, void *stream)
{
    return mvm_batch_iht<Mvm8Batch>("clm4_iht_v8_batch", Phi, sPhi, PhiT, sPhiT, m, n, nvec, x, sx, x_len, y, sy, t1, st1, t2, st2, t3, st3, iterations,
                                    K, mu, threshold, rng_state_dev, stream);
}

// The same loop with ONE matrix (include/clover_hip_batch_t_v8.h): step 1 is this family's fused launch on Phi, step 2 the transposed
// family's (mvm_t8_batch.hip) on the same bytes; the draws lie where the two-matrix loop has them.
extern "C" int clm4_iht_v8_batch_one_matrix(const int8_t *Phi, const float *sPhi, uint64_t m, uint64_t n, uint64_t nvec, int8_t *const *x,
                                            float *const *sx, uint64_t x_len, const int8_t *const *y, const float *const *sy, int8_t *const *t1,
                                            float *const *st1, int8_t *const *t2, float *const *st2, int8_t *const *t3, float *const *st3,
                                            uint64_t iterations, uint64_t K, float mu, int threshold, uint64_t *rng_state_dev, void *stream)
{
    return mvm_batch_iht<Mvm8Batch, MvmT8Batch>("clm4_iht_v8_batch_one_matrix", Phi, sPhi, nullptr, nullptr, m, n, nvec, x, sx, x_len, y, sy, t1, st1,
                                                t2, st2, t3, st3, iterations, K, mu, threshold, rng_state_dev, stream);
}
