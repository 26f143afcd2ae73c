// matrix8_batch.hip -- CloverMatrix8 x CloverVector8 (the reference's pure 8-bit configuration, 02_bit08.cpp) for several right-hand
// sides: ONE pass over the matrix for up to CLM4_MVM_BATCH_MAX vectors, as mvm_batch8.hip does for the 4-bit matrix.
//
// The 8-bit matrix has twice the bytes of the 4-bit one and needs no nibble transpose or widening: a workgroup loads each 16 matrix bytes
// of a lane once and runs, per vector and block, one 16-byte LDS read of x, one of the factor, four v_dot4_i32_i8, two converts and two
// fmas.  Each vector's instruction sequence is the one of m8_mvm_body (matrix8.hip), so the results equal the single calls bit for bit;
// the re-quantisation and the scaleAndAdd behind it are mvm8_requantize_wave (mvm8_device.h), the same arithmetic as k_m8_mvm_saa's.
#include "mvm_batch_host.h"
#include "mvm8_device.h"
#include "matrix8_t_batch.h"

#include "clover_hip_batch_t8.h"

// Columns of x staged in LDS per pass: 4 KiB of int8 + 256 B of block factors + 256 B of row dots per vector, 36 KiB at NV = 8 (36.5 KiB
// with the generator starts of the fused stochastic form): four workgroups per CU, the budget of mvm_batch8.hip.
#define M8B_CHUNK 4096u
#define M8B_THREADS 256
#define M8B_U 8          // blocks in flight per lane: 4 U registers of matrix words + 2 accumulators per vector

// the size rules of clm8_mvm (matrix8.hip)
int clv_internal_m8_check_mvm(const char *fn, const void *A, const void *sA, uint64_t rows, uint64_t cols, const void *x, const void *r);

// M8BatchArgs / M8BatchFuse (the vectors of one pass, by value in the kernel arguments): mvm8_device.h, shared with the transposed batched
// kernel (matrix8_t_batch.hip)

#define M8B_X_BYTES(NV) ((NV) * (M8B_CHUNK + (M8B_CHUNK / 64) * sizeof(float) + 64 * sizeof(float)))
// ST: behind the row dots, per vector and window the start of each of the 4 generator lanes (32 B): 512 B at NV = 8 fused
#define M8B_LDS_BYTES(NV, ST, FUSE) (M8B_X_BYTES(NV) + ((ST) ? (NV) * ((FUSE) ? 2 : 1) * 4 * sizeof(uint64_t) : 0))

// one block (64 columns) of this lane's row: lo = bytes 8p..8p+7, hi = bytes 32+8p..32+8p+7, for every vector of the group.  x lies in
// LDS in the LANE's order: u32x4 number 4 b + p of a vector holds {x[8p..8p+7], x[32+8p..32+8p+7]} of block b, one 16-byte read.
template <int NV>
__device__ __forceinline__ void m8b_block(const u32x2 lo, const u32x2 hi, uint32_t b, int p, int nv, const u32x4 *xs, const float *cs,
                                          float (&a0)[NV], float (&a1)[NV])
{
    constexpr uint32_t XS = M8B_CHUNK / 16, CS = M8B_CHUNK / 64;
#pragma unroll
    for (int v = 0; v < NV; v++)
        if (v < nv) {
            const u32x4 xv = xs[v * XS + 4 * b + p];
            const float c = cs[v * CS + b];
            a0[v] = __builtin_fmaf(c, (float)sdot4(hi.x, xv.z, sdot4(lo.x, xv.x, 0)), a0[v]);      // chain 2p
            a1[v] = __builtin_fmaf(c, (float)sdot4(hi.y, xv.w, sdot4(lo.y, xv.y, 0)), a1[v]);      // chain 2p + 1
        }
}

// Mapping of k_m8_mvm: workgroup = one 64-row group, lane = (row rho = tid >> 2, quarter p = tid & 3) owning chains 2p and 2p + 1 of its
// row, two 8-byte matrix loads per block; per vector 2 accumulators.  amdgpu_waves_per_eu(4, 4) holds every instantiation to 128
// registers (four waves per SIMD, what the LDS allows; figures: DESIGN.md 3).  Vector v's epilogue (tree -> re-quantise [-> scaleAndAdd])
// runs on wave v & 3.  ST: the jump-ahead of mvm_batch_device.h; the draw layout is k_m8_mvm's.
template <int NV, int U, bool NT, bool FUSE, bool ST>
__global__ __launch_bounds__(M8B_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_m8_mvm_batch(
    const uint8_t *__restrict__ A, const float *__restrict__ sA, uint64_t cols, int nv, M8BatchArgs<NV> arg, M8BatchFuse<NV> fuse, MvmBatchRng rs)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr uint32_t XS = M8B_CHUNK / 16, CS = M8B_CHUNK / 64;            // per vector: u32x4 of x, factors
    u32x4 *xs = reinterpret_cast<u32x4 *>(smem);                            // NV x M8B_CHUNK bytes of int8
    float *cs = reinterpret_cast<float *>(smem + NV * M8B_CHUNK);           // NV x M8B_CHUNK / 64 factors
    float *dsh = cs + NV * CS;                                              // NV x 64 row dots
    static_assert(XS == M8B_THREADS && CS == 64, "one u32x4 of x per thread and vector, one factor per lane of the first wave");
    constexpr int NW = FUSE ? 2 : 1;                                        // windows per vector: the mvm's draws, the scaleAndAdd's
    uint64_t *sbase = reinterpret_cast<uint64_t *>(dsh + NV * 64);          // ST: [NV][NW][4] lane starts

    const uint64_t rb = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t st_seq = 0;
    uint64_t *st_next = nullptr;
    if constexpr (ST) st_next = mvmb_rng_prologue<NV, NW>(rs, nv, rb, gridDim.x, sbase, st_seq);

    const int p = tid & 3, rho = tid >> 2;
    const uint64_t row = rb * 64 + rho;
    const u32x2 *Arow = reinterpret_cast<const u32x2 *>(A + row * cols);
    const float *sArow = sA + rb * (cols / 64);

    float a0[NV], a1[NV];
#pragma unroll
    for (int v = 0; v < NV; v++) a0[v] = a1[v] = 0.0f;

    for (uint64_t c0 = 0; c0 < cols; c0 += M8B_CHUNK) {
        const uint32_t cw = (uint32_t)((cols - c0) < M8B_CHUNK ? (cols - c0) : M8B_CHUNK);
        if (c0) __syncthreads();
        {   // stage x and the factors of every present vector: the loads first, then the LDS writes.  Thread tid holds bytes 16 q .. 16 q + 15
            // of block tid >> 2 (q = tid & 3): the 8-byte units 2 q and 2 q + 1; unit j goes to lane j & 3's u32x4, half j >> 2
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
            const uint32_t j = 2 * (tid & 3), slot = 8 * (tid >> 2) + 2 * (j & 3) + (j >> 2);      // unit j + 1: slot + 2
#pragma unroll
            for (int v = 0; v < NV; v++)
                if (v < nv) {
                    u32x2 *xw = reinterpret_cast<u32x2 *>(xs + v * XS);
                    if ((uint32_t)tid < nx) {
                        xw[slot] = u32x2{xr[v].x, xr[v].y};
                        xw[slot + 2] = u32x2{xr[v].z, xr[v].w};
                    }
                    if ((uint32_t)tid < nc) cs[v * CS + tid] = (sa * (1.0f / 127.0f)) * (sv[v] * (1.0f / 127.0f));
                }
        }
        __syncthreads();

        const u32x2 *Ap = Arow + c0 / 8;
        const uint32_t nb = cw / 64;
        uint32_t b = 0;
        for (; b + U <= nb; b += U) {
            u32x2 lo[U], hi[U];                                             // each matrix byte ONCE for all vectors
#pragma unroll
            for (int u = 0; u < U; u++) {
                lo[u] = NT ? __builtin_nontemporal_load(&Ap[8 * (b + u) + p]) : Ap[8 * (b + u) + p];
                hi[u] = NT ? __builtin_nontemporal_load(&Ap[8 * (b + u) + 4 + p]) : Ap[8 * (b + u) + 4 + p];
            }
#pragma unroll
            for (int u = 0; u < U; u++) m8b_block<NV>(lo[u], hi[u], b + u, p, nv, xs, cs, a0, a1);
        }
        for (; b < nb; b++) {
            const u32x2 lo = NT ? __builtin_nontemporal_load(&Ap[8 * b + p]) : Ap[8 * b + p];
            const u32x2 hi = NT ? __builtin_nontemporal_load(&Ap[8 * b + 4 + p]) : Ap[8 * b + 4 + p];
            m8b_block<NV>(lo, hi, b, p, nv, xs, cs, a0, a1);
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

    // lane p holds acc[2p], acc[2p+1]: ((a0+a4)+(a2+a6))+((a1+a5)+(a3+a7)) is mvm8_tree's order (lanes p ^ 2, then p ^ 1)
#pragma unroll
    for (int v = 0; v < NV; v++)
        if (v < nv) {
            const float dot = mvm8_tree(a0[v], a1[v]);
            if (p == 0) dsh[v * 64 + rho] = dot;
        }
    __syncthreads();
    if constexpr (ST) mvmb_rng_stamp(st_next, st_seq);        // every wave's part of the new state was written before the barrier
#pragma unroll
    for (int v = 0; v < NV; v++)
        if (v < nv && wave == (v & 3)) {
            int8_t *r = arg.r[v];
            float noise = 0.0f, noise2 = 0.0f;
            if constexpr (ST) {
                // k_m8_mvm's lanes.  mvm: lane l takes draw l >> 5, word l & 7, byte (l >> 3) & 3;
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
struct M8Batch : MvmBatchByRows {
    template <int NV> using Args = M8BatchArgs<NV>;
    template <int NV> using Fuse = M8BatchFuse<NV>;
    static uint64_t matrix_bytes(uint64_t rows, uint64_t cols) { return rows * cols; }
    static uint64_t vector_bytes(uint64_t n) { return n; }
    static int check_matrix(const char *fn, const int8_t *A, const float *sA, uint64_t rows, uint64_t cols) { return clv_internal_m8_check_mvm(fn, A, sA, rows, cols, A, A); }
    static bool result_may_not_alias_x(bool) { return true; }
    static constexpr auto mvm = clm8_mvm;
    static constexpr auto scale_and_add = clm8_mvm_scale_and_add;
    static constexpr auto iht = clm8_iht;
    static constexpr auto clear = clv_internal_v8_clear;
    static constexpr auto threshold_batch = clv8_threshold_batch;
    // no single clm8_iht takes a persistent kernel: it is the launch-per-step loop with the same three launches per iteration per SIGNAL,
    // so the rule of the fused mvm holds (mvm_batch_selected)
    static bool iht_prefers_single(uint64_t, uint64_t, uint64_t, int, bool, uint64_t) { return false; }
    template <int NV, bool NT, bool FUSE, bool ST>
    static void launch(dim3 grid, hipStream_t st, const uint8_t *A, const float *sA, uint64_t, uint64_t cols, int nv, const Args<NV> &arg, const Fuse<NV> &fuse,
                       const MvmBatchRng &rs)
    {
        hipLaunchKernelGGL((k_m8_mvm_batch<NV, M8B_U, NT, FUSE, ST>), grid, dim3(M8B_THREADS), M8B_LDS_BYTES(NV, ST, FUSE), st, A, sA, cols, nv, arg, fuse,
                           rs);
    }
};

// ---- C ABI -------------------------------------------------------------------------------------------------------------------
extern "C" int clm8_mvm_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                              const float *const *sx, int8_t *const *r, float *const *sr, uint64_t *rng_state_dev, void *stream)
{
    return mvm_batch_entry<M8Batch>("clm8_mvm_batch", A, sA, rows, cols, nvec, x, sx, r, sr, rng_state_dev, stream);
}

extern "C" int clm8_mvm_batch_at(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                                 const float *const *sx, int8_t *const *r, float *const *sr, uint64_t *rng_state_dev, uint64_t draw_base,
                                 uint64_t draw_stride, uint64_t commit_draws, void *stream)
{
    return mvm_batch_at_entry<M8Batch>("clm8_mvm_batch_at", "clm8_mvm_batch", A, sA, rows, cols, nvec, x, sx, r, sr,
                                       rng_state_dev, draw_base, draw_stride, commit_draws, stream);
}

extern "C" int clm8_mvm_scale_and_add_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                                            const float *const *sx, const int8_t *const *qu, const float *const *su, float a, int8_t *const *t,
                                            float *const *st_, int8_t *const *r, float *const *sr, uint64_t *rng_state_dev, void *stream)
{
    return mvm_batch_fused_entry<M8Batch>("clm8_mvm_scale_and_add_batch", A, sA, rows, cols, nvec, x, sx, qu, su, a, t, st_, r, sr,
                                          rng_state_dev, stream);
}

extern "C" int clm8_iht_batch(const int8_t *Phi, const float *sPhi, const int8_t *PhiT, const float *sPhiT, uint64_t m, uint64_t n, uint64_t nvec,
                              int8_t *const *x, float *const *sx, uint64_t x_len, const int8_t *const *y, const float *const *sy,
                              int8_t *const *t1, float *const *st1, int8_t *const *t2, float *const *st2, int8_t *const *t3, float *const *st3,
                              uint64_t iterations, uint64_t K, float mu, int threshold, uint64_t *rng_state_dev, void *stream)
{
    return mvm_batch_iht<M8Batch>("clm8_iht_batch", Phi, sPhi, PhiT, sPhiT, m, n, nvec, x, sx, x_len, y, sy, t1, st1, t2, st2, t3, st3, iterations, K, mu,
                                  threshold, rng_state_dev, stream);
}

// The same loop with ONE matrix (include/clover_hip_batch_t8.h): step 1 is this family's fused launch on Phi, step 2 the transposed
// family's (matrix8_t_batch.hip) on the same bytes; the draws lie where the two-matrix loop has them.
extern "C" int clm8_iht_batch_one_matrix(const int8_t *Phi, const float *sPhi, uint64_t m, uint64_t n, uint64_t nvec, int8_t *const *x,
                                         float *const *sx, uint64_t x_len, const int8_t *const *y, const float *const *sy, int8_t *const *t1,
                                         float *const *st1, int8_t *const *t2, float *const *st2, int8_t *const *t3, float *const *st3,
                                         uint64_t iterations, uint64_t K, float mu, int threshold, uint64_t *rng_state_dev, void *stream)
{
    return mvm_batch_iht<M8Batch, M8TBatch>("clm8_iht_batch_one_matrix", Phi, sPhi, nullptr, nullptr, m, n, nvec, x, sx, x_len, y, sy, t1, st1, t2,
                                            st2, t3, st3, iterations, K, mu, threshold, rng_state_dev, stream);
}
