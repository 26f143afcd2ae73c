// matrix8_t_batch.hip -- the transposed 8-bit mvm for several vectors: r[j] = quantize8(A' x[j]) for up to CLM4_MVM_BATCH_MAX CloverVector8
// in ONE pass over a CloverMatrix8's own bytes, no stored transpose.
//
// Contract: byte for byte the sequence of single calls clm8_mvm_transposed / clm8_mvm_transposed_scale_and_add (matrix8_t.hip) for vector
// 0, 1, ... on the same stream, the generator state included -- and so, as those are defined through the stored transpose, what
// clm8_mvm_batch / clm8_mvm_scale_and_add_batch give on clm8_transpose(A).
//
// The kernel keeps the mapping of k_m8_mvm_t: workgroup = M8TB_W = 2 adjacent output blocks = 128 columns = one whole 128-byte line of
// every row, 256 threads, all rows; thread = (column quad cq = tid & 31, chain L = tid >> 5).  Per 64-row block a thread does its 8 dword
// loads and the two 4 x 4 byte transposes (16 v_perm) ONCE; per present vector it runs the link of the single kernel (m8t_link,
// matrix8_t_device.h): two sdot4 per column against that vector's x dwords, one convert, one fma into 4 accumulators of the vector's own.
// The chains of different vectors are independent, which is what makes the results bit-identical.
//   x, factors = staged per M8TB_CHUNK rows in LDS: the int8 of every present vector, sA * 1/127 of the workgroup's 2 column tiles ONCE
//                and sx * 1/127 per (block, vector); the lane forms c = (sA * 1/127) * (sx * 1/127) itself -- the three roundings of
//                m8_factor, in its order;
//   loads      = the look-ahead form of k_m8_mvm_t: two register sets of U blocks take turns, the set ahead is requested -- unconditionally,
//                clamped to the last block -- before the links of the current one; every address stays inside the matrix;
//   epilogue   = one vector at a time: the 8 chain ends of every column through LDS (the staging area again) to one wave per output block,
//                mvm8_tree8, mvm8_requantize_wave<FUSE>.  The block of u of every vector is fetched before anything is written, so r2
//                may be u.
// Stochastic rounding: vector v's window begins draw_base + v * draw_stride draws behind the state the launch reads (MvmBatchRng);
// inside it output block cb takes draws 2 cb, 2 cb + 1 and, fused, 2 G + 2 cb, 2 G + 2 cb + 1 (G = cols / 64), the positions of the
// single kernel.  The jump-ahead to the workgroup's first block runs in the prologue (mvmb_rng_prologue), gen_blocks produces the two
// consecutive blocks of every window in the epilogue, workgroup 0 commits and stamps.
#include "matrix8_t_batch.h"
#include "matrix8_t_device.h"

#include "clover_hip_batch_t8.h"

// Rows staged in LDS per pass.  The single kernel stages 16384 (18 KiB for one vector); eight of those do not fit.  4096 rows are 4 KiB of
// x + 256 B of sx * 1/127 per vector and 512 B of matrix factors.  With the generator starts and raw draws of the fused stochastic form
// (NV * 2 windows * (32 + 128) B) the budget per workgroup is
//   NV = 2:  9216 B staged,  9856 B in all;   NV = 4: 17920 B staged, 19200 B in all;   NV = 8: 35328 B staged, 37888 B in all
// so that four workgroups per CU (160 KiB) fit at every NV.  Not swept: only this chunk was built.
#define M8TB_CHUNK 4096u
#define M8TB_STEP 64u       // rows per block: every thread takes part in every block
// Blocks of matrix loads per register set = blocks requested ahead of the links: 2 x 8 x U load registers beside 4 NV accumulators and the
// x dwords of the vectors.  2 is the depth the single kernel measured best (M8T_U); at NV = 8 the fused stochastic instantiation needs
// scratch with it under the 128 registers of four waves per SIMD, so 8 vectors look 1 block ahead -- the links of 8 vectors on one block
// are about as long as those of 4 on two.  Chosen by the register budget, NOT swept: no other depth was timed for any NV.
#define M8TB_U(NV) ((NV) <= 4 ? 2 : 1)
#define M8TB_CB (M8TB_CHUNK / M8TB_STEP)      // blocks per chunk
#define M8TB_XW (M8TB_CHUNK / 4)              // x dwords per vector and chunk

static_assert(M8TB_W == 2, "the lane map (32 column quads x 8 chains) assumes 128 columns: cols % 128 == 0 makes every workgroup whole");
static_assert(M8TB_CHUNK / 16 == 256 && M8TB_CB * M8TB_W <= 256 && M8TB_CB <= 256, "the staging assumes one u32x4 of x per thread and vector, at most one factor per thread");

constexpr size_t m8tb_stage_bytes(int nv)
{
    const size_t staged = (size_t)nv * M8TB_CHUNK + M8TB_CB * M8TB_W * sizeof(float) + (size_t)nv * M8TB_CB * sizeof(float);
    const size_t part = 8 * 64 * M8TB_W * sizeof(float);          // the chain ends reuse the staging area
    return staged > part ? staged : part;
}

// stage the chunk that starts at row r0: x and sx * 1/127 of every present vector, sA * 1/127 of the workgroup's column tiles; all loads
// first (one round trip), then the LDS writes
template <int NV>
__device__ __forceinline__ void m8tb_stage(uint32_t *xs, float *sas, float *svs, const float *__restrict__ sA, const M8BatchArgs<NV> &arg, int nv,
                                           uint64_t rows, uint64_t r0, uint64_t G, uint64_t cb0, int tid)
{
    const uint32_t ch = (uint32_t)((rows - r0) < M8TB_CHUNK ? (rows - r0) : M8TB_CHUNK);
    const uint32_t nx = ch / 16, nb = ch / 64, nc = nb * M8TB_W;
    const uint32_t ix = (uint32_t)tid < nx ? tid : 0, ib = (uint32_t)tid < nb ? tid : 0, ic = (uint32_t)tid < nc ? tid : 0;
    if (r0) __syncthreads();                             // the previous chunk's x and factors have been consumed
    u32x4 xr[NV];
    float sv[NV];
    const float sa = sA[(r0 / 64 + ic / M8TB_W) * G + cb0 + ic % M8TB_W];
    // an absent slot reads vector 0 again (its own pointers are NULL) and stores nothing: no branch around a load, so the registers of
    // xr[] stay plain registers
#pragma unroll
    for (int v = 0; v < NV; v++) {
        const int vv = v < nv ? v : 0;
        xr[v] = reinterpret_cast<const u32x4 *>(arg.x[vv] + r0)[ix];
        sv[v] = arg.sx[vv][r0 / 64 + ib];
    }
    if ((uint32_t)tid < nc) sas[tid] = sa * (1.0f / 127.0f);
#pragma unroll
    for (int v = 0; v < NV; v++) {
        if (v < nv && (uint32_t)tid < nx) reinterpret_cast<u32x4 *>(xs + v * M8TB_XW)[tid] = xr[v];
        if (v < nv && (uint32_t)tid < nb) svs[v * M8TB_CB + tid] = sv[v] * (1.0f / 127.0f);
    }
    __syncthreads();
}

// one block: the transposes once, the link of every present vector.  xs / svs: the block's x dwords and sx * 1/127 of vector 0 in LDS
template <int NV>
__device__ __forceinline__ void m8tb_block(const uint32_t (&a)[8], const uint32_t *xs, float sa, const float *svs, int L, int nv, float (&acc)[NV][4])
{
    uint32_t lo[4], hi[4];
    m8t_transpose4x4(a, lo);
    m8t_transpose4x4(a + 4, hi);
#pragma unroll
    for (int v = 0; v < NV; v++)
        if (v < nv) {
            const uint32_t xl = xs[v * M8TB_XW + L], xh = xs[v * M8TB_XW + 8 + L];      // x of rows 4 L .. 4 L + 3 and 32 + 4 L .. 32 + 4 L + 3
            m8t_link(lo, hi, xl, xh, sa * svs[v * M8TB_CB], acc[v]);
        }
}

// group g of the walk from `cur` (loaded a group ago) while the next group's loads go to `nxt` -- issued UNCONDITIONALLY (beyond the last
// block: the last block again), as m8t_group (matrix8_t.hip) does
template <int NV, int U, bool NT>
__device__ __forceinline__ void m8tb_group(const uint32_t (&cur)[U][8], uint32_t (&nxt)[U][8], const uint32_t *__restrict__ Aq, uint64_t stride,
                                           uint32_t g, uint32_t nblk, const uint32_t *xs, const float *sas, const float *svs, int L, int tile, int nv,
                                           float (&acc)[NV][4])
{
    m8t_load<U, NT>(Aq, stride, g + 1, nblk, nxt);
    const uint32_t b0 = g * U, lb = b0 % M8TB_CB;        // a group never straddles a chunk
    if (nblk - b0 >= (uint32_t)U) {
#pragma unroll
        for (int u = 0; u < U; u++) m8tb_block<NV>(cur[u], xs + 16 * (lb + u), sas[M8TB_W * (lb + u) + tile], svs + lb + u, L, nv, acc);
    } else {
#pragma unroll
        for (int u = 0; u < U; u++)
            if (b0 + u < nblk) m8tb_block<NV>(cur[u], xs + 16 * (lb + u), sas[M8TB_W * (lb + u) + tile], svs + lb + u, L, nv, acc);
    }
}

template <int NV, int U, bool NT, bool FUSE, bool ST>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void k_m8_mvm_t_batch(const uint8_t *__restrict__ A, const float *__restrict__ sA, uint64_t rows, uint64_t cols,
                                                        int nv, M8BatchArgs<NV> arg, M8BatchFuse<NV> fuse, MvmBatchRng rs)
{
    static_assert(M8TB_CB % (2 * U) == 0, "a chunk is whole pairs of load groups");
    constexpr int NW = FUSE ? 2 : 1;                                               // windows per vector: the mvm's draws, the scaleAndAdd's
    __shared__ __attribute__((aligned(16))) char stage[m8tb_stage_bytes(NV)];
    __shared__ uint64_t sbase[ST ? NV * NW * 4 : 1];                                // ST: [NV][NW][4] lane starts at the workgroup's first block
    __shared__ uint64_t raw[ST ? NV * NW * 8 * M8TB_W : 1];                         // ST: per window the raw draws of M8TB_W blocks
    uint32_t *xs = reinterpret_cast<uint32_t *>(stage);                             // [NV][M8TB_XW]
    float *sas = reinterpret_cast<float *>(stage + NV * M8TB_CHUNK);                // [M8TB_CB][M8TB_W]: sA * 1/127
    float *svs = sas + M8TB_CB * M8TB_W;                                            // [NV][M8TB_CB]: sx * 1/127
    float *part = reinterpret_cast<float *>(stage);                                 // epilogue: part[chain][column]

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint64_t G = cols / 64;                                   // output blocks = column tiles of A
    const uint64_t cb0 = (uint64_t)blockIdx.x * M8TB_W, cb = cb0 + wave;
    uint64_t st_seq = 0;
    uint64_t *st_next = nullptr;
    if constexpr (ST) st_next = mvmb_rng_prologue<NV, NW>(rs, nv, cb0, G, sbase, st_seq);

    const int cq = tid & 31, L = tid >> 5, tile = cq >> 4;
    const uint64_t stride = cols / 4;                               // dwords per row
    const uint32_t *Aq = reinterpret_cast<const uint32_t *>(A) + cb0 * 16 + cq + (uint64_t)(4 * L) * stride;

    float acc[NV][4];
#pragma unroll
    for (int v = 0; v < NV; v++)
#pragma unroll
        for (int k = 0; k < 4; k++) acc[v][k] = 0.0f;

    // the walk over all rows in groups of U blocks; a chunk is a whole, even number of groups, so x and the factors are re-staged in front
    // of an even group.  Two register sets take turns: no copies, and the loads of the group ahead stay in flight across the staging
    constexpr uint32_t CG = M8TB_CB / U;
    const uint32_t nblk = (uint32_t)(rows / 64), ngroups = (nblk + U - 1) / U;
    uint32_t a[U][8], b[U][8];
    m8t_load<U, NT>(Aq, stride, 0, nblk, a);
    uint32_t g = 0;
    for (; g + 1 < ngroups; g += 2) {
        if (g % CG == 0) m8tb_stage<NV>(xs, sas, svs, sA, arg, nv, rows, (uint64_t)g * U * 64, G, cb0, tid);
        m8tb_group<NV, U, NT>(a, b, Aq, stride, g, nblk, xs, sas, svs, L, tile, nv, acc);
        m8tb_group<NV, U, NT>(b, a, Aq, stride, g + 1, nblk, xs, sas, svs, L, tile, nv, acc);
    }
    if (g < ngroups) {
        if (g % CG == 0) m8tb_stage<NV>(xs, sas, svs, sA, arg, nv, rows, (uint64_t)g * U * 64, G, cb0, tid);
        m8tb_group<NV, U, NT>(a, b, Aq, stride, g, nblk, xs, sas, svs, L, tile, nv, acc);
    }

    // FUSE: this wave's block of u of every vector, requested here, behind the row loop (they would cost registers across it) and before
    // any block of any result is written (r2 may be u); the first vector's barriers cover the latency
    int fuse_q[NV] = {};
    float fuse_s[NV] = {};
    if (FUSE && wave < M8TB_W) {
#pragma unroll
        for (int v = 0; v < NV; v++)
            if (v < nv) {
                fuse_q[v] = fuse.qu[v][cb * 64 + lane];
                fuse_s[v] = fuse.su[v][cb];
            }
    }
    if constexpr (ST) {
        // thread i = (window i >> 2 = v * NW + w, generator lane i & 3): the window's draws of the workgroup's two consecutive blocks
        if (tid < NV * NW * 4 && (tid >> 2) / NW < nv) gen_blocks(sbase[tid], M8TB_W, raw + (size_t)(tid >> 2) * 8 * M8TB_W, tid & 3);
    }

    // one vector at a time: the 8 chain ends of every column meet in the wave of the column's output block
#pragma unroll
    for (int v = 0; v < NV; v++)
        if (v < nv) {
            __syncthreads();                                        // the staging area / the previous vector's chain ends have been read
            const f32x4 mine = {acc[v][0], acc[v][1], acc[v][2], acc[v][3]};
            reinterpret_cast<f32x4 *>(part)[L * 16 * M8TB_W + cq] = mine;
            __syncthreads();                                        // and, for v = 0, raw[] has been written
            if (wave < M8TB_W) {                                    // wave-uniform: one wave per output block
                float ends[8];
#pragma unroll
                for (int l = 0; l < 8; l++) ends[l] = part[l * 64 * M8TB_W + 64 * wave + lane];
                float noise = 0.0f, noise2 = 0.0f;
                if constexpr (ST) {
                    noise = m8_mvm_noise(raw + (size_t)(v * NW) * 8 * M8TB_W + 8 * wave, lane);
                    if (FUSE) noise2 = m8_saa_noise(raw + (size_t)(v * NW + 1) * 8 * M8TB_W + 8 * wave, lane);
                }
                int8_t *r = arg.r[v];
                mvm8_requantize_wave<FUSE>(mvm8_tree8(ends), noise, noise2, lane, r ? r + cb * 64 : nullptr, r ? arg.sr[v] + cb : nullptr, fuse_q[v],
                                           fuse_s[v], fuse.a, FUSE ? fuse.r2[v] + cb * 64 : nullptr, FUSE ? fuse.sr2[v] + cb : nullptr);
            }
        }
    if constexpr (ST) mvmb_rng_stamp(st_next, st_seq);              // behind the barriers above: every wave's part of the new state was written
}

// ---- launches: declared in matrix8_t_batch.h, instantiated here for the driver's NV = 2, 4, 8 ---------------------------------------
template <int NV, bool NT, bool FUSE, bool ST>
void M8TBatch::launch(dim3 grid, hipStream_t st, const uint8_t *A, const float *sA, uint64_t rows, uint64_t cols, int nv, const Args<NV> &arg,
                      const Fuse<NV> &fuse, const MvmBatchRng &rs)
{
    hipLaunchKernelGGL((k_m8_mvm_t_batch<NV, M8TB_U(NV), NT, FUSE, ST>), grid, dim3(256), 0, st, A, sA, rows, cols, nv, arg, fuse, rs);
}
MVM_BATCH_INSTANTIATE_LAUNCHES(M8TBatch)

// ---- C ABI (include/clover_hip_batch_t8.h) ---------------------------------------------------------------------------------------
extern "C" int clm8_mvm_transposed_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                                         const float *const *sx, int8_t *const *r, float *const *sr, uint64_t *rng_state_dev, void *stream)
{
    return mvm_batch_entry<M8TBatch>("clm8_mvm_transposed_batch", A, sA, rows, cols, nvec, x, sx, r, sr, rng_state_dev, stream);
}

extern "C" int clm8_mvm_transposed_batch_at(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                                            const float *const *sx, int8_t *const *r, float *const *sr, uint64_t *rng_state_dev,
                                            uint64_t draw_base, uint64_t draw_stride, uint64_t commit_draws, void *stream)
{
    return mvm_batch_at_entry<M8TBatch>("clm8_mvm_transposed_batch_at", "clm8_mvm_transposed_batch", A, sA, rows, cols, nvec, x, sx, r, sr,
                                        rng_state_dev, draw_base, draw_stride, commit_draws, stream);
}

extern "C" int clm8_mvm_transposed_scale_and_add_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec,
                                                       const int8_t *const *x, const float *const *sx, const int8_t *const *qu,
                                                       const float *const *su, float a, int8_t *const *t, float *const *st_, int8_t *const *r,
                                                       float *const *sr, uint64_t *rng_state_dev, void *stream)
{
    return mvm_batch_fused_entry<M8TBatch>("clm8_mvm_transposed_scale_and_add_batch", A, sA, rows, cols, nvec, x, sx, qu, su, a, t, st_, r, sr,
                                           rng_state_dev, stream);
}
