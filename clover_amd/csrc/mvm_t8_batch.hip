// mvm_t8_batch.hip -- the transposed mixed mvm for several vectors: r[j] = quantize8(A' x[j]) for up to CLM4_MVM_BATCH_MAX CloverVector8
// in ONE pass over a CloverMatrix4's own 4-bit bytes, no stored transpose.
//
// Contract: byte for byte the sequence of single calls clm4_mvm_v8_transposed / clm4_mvm_v8_transposed_scale_and_add (mvm_t8.hip) for
// vector 0, 1, ... on the same stream, the generator state included -- and so, as those are defined through the stored transpose, what
// clm4_mvm_v8_batch / clm4_mvm_v8_scale_and_add_batch (mvm_batch8.hip) give on clm4_transpose(A).
//
// Arithmetic per vector: that of k_m4_mvm8_t.  For every (column, chain L) the links acc = fma(c_b, (float)I_b, acc) run over the 64-row
// blocks b in order in ONE register; I_b is the exact integer sum over rows 4 L .. 4 L + 3 and 32 + 4 L .. 32 + 4 L + 3 of block b
// (mvt8_int, mvm_t8_device.h), c_b = mvm8_factor(sA[b][column / 64], sx_v[b]) with its three roundings in its order; then mvm8_tree8 and
// mvm8_requantize_wave<FUSE>.  Chains of different vectors are independent.
//
// Mapping: map (b) of DESIGN.md 3 "A'x for CloverVector8" -- NO hand-over through LDS.  The single kernel gives each of its four waves a
// row block of its own and hands the integers to the thread that owns the chain; its hand-over is 18 KiB per vector, 144 KiB for eight.
// Here every thread takes part in every block, so a chain never leaves its lane:
//   workgroup = MVT8B_W = 2 adjacent output blocks = 128 columns = 64 contiguous bytes of every row, 256 threads, all rows.  The two
//               workgroups that share a 128-byte line are placed on one XCD (the blockIdx remap of k_m4_mvm8_t);
//   thread    = (chain L = tid >> 5, half h = (tid >> 4) & 1, column group cg = tid & 15): lanes l and l ^ 16 of a wave are a PAIR with
//               the same chain and the same 8 columns 8 cg .. 8 cg + 7.  Per block lane h loads the dword of those columns in the 4 rows
//               4 L .. 4 L + 3 (h = 0) or 32 + 4 L .. 32 + 4 L + 3 (h = 1) of the chain -- a wave's load instruction reads 4 rows x 64 B,
//               every matrix byte is requested once --, the pair swaps its dwords through the LDS crossbar (__shfl_xor, no LDS memory),
//               both transpose the 8 x 8 nibbles and lane h widens the words of ITS 4 columns 8 cg + 4 h .. + 3: none of this depends
//               on x, it runs once per block.  The transpose (about 40 VALU instructions) is done twice, which is what 256 threads on
//               128 columns cost: with 128 threads half the SIMDs would idle at cols / 128 <= 256 workgroups.  (The first form built had
//               the two halves in different waves, each loading all 8 rows: with nontemporal loads every byte then crossed the fabric
//               twice, 2 and 4 vectors at 65536^2 took the same 0.98 ms: profiles/mvm_v8_transposed_batch_variants.json.)  Per present
//               vector: 2 LDS dwords of x, and per column 2 sdot4, shift, convert, fma into 4 accumulators of the vector's own;
//   x, factors = staged per MVT8B_CHUNK rows in LDS: the int8 of every present vector, sA * 1/7 of the workgroup's 2 column tiles ONCE and
//                sx * 1/127 per (block, vector); the lane forms c = (sA * 1/7) * (sx * 1/127) itself -- mvm8_factor's roundings, in order;
//   loads      = look-ahead: two register sets of U blocks take turns, the set ahead is requested -- unconditionally, clamped to the last
//                block -- before the links of the current one; every address stays inside the matrix;
//   epilogue   = one vector at a time: the 8 chain ends of every column through LDS (the staging area again) to one wave per output block,
//                mvm8_tree8, mvm8_requantize_wave<FUSE>.  The block of u of every vector is fetched before anything is written, so r2
//                may be u.
// Stochastic rounding: vector v's window begins draw_base + v * draw_stride draws behind the state the launch reads (MvmBatchRng);
// inside it output block cb takes draws 2 cb, 2 cb + 1 and, fused, 2 G + 2 cb, 2 G + 2 cb + 1 (G = cols / 64), the positions of the
// single kernel.  The jump-ahead to the workgroup's first block runs in the prologue (mvmb_rng_prologue), gen_blocks produces the two
// consecutive blocks of every window in the epilogue, workgroup 0 commits and stamps.  The element <-> noise maps are those at the end of
// k_m4_mvm8_t, which are m8_mvm_noise / m8_saa_noise (mvm8_device.h).
#include "mvm_t8_batch.h"
#include "mvm_t8_device.h"

#include "clover_hip_batch_t_v8.h"

// Rows staged in LDS per pass: one u32x4 of x per thread and vector, as MVTB_CHUNK and M8TB_CHUNK.  4096 rows are 4 KiB of x + 256 B of
// sx * 1/127 per vector and 512 B of matrix factors.  With the generator starts and raw draws of the fused stochastic form
// (NV * 2 windows * (32 + 128) B) the budget per workgroup is
//   NV = 2:  9216 B staged,  9856 B in all;   NV = 4: 17920 B staged, 19200 B in all;   NV = 8: 35328 B staged, 37888 B in all
// so that four workgroups per CU (160 KiB) fit at every NV.  Not swept: only this chunk was built.
#define MVT8B_CHUNK 4096u
#define MVT8B_STEP 64u      // rows per block: every thread takes part in every block
// Blocks of matrix loads per register set = blocks requested ahead of the links: 2 x 4 x U load registers beside 4 NV accumulators, the 8
// widened words and the x dwords of a vector.  4 blocks are the 16 dwords per lane k_m4_mvm8_t keeps in flight; 8 vectors look 1 block
// ahead: with 2 the deterministic instantiations need 36 bytes of scratch per lane.  Chosen by the register budget, NOT swept.
#define MVT8B_U(NV) ((NV) <= 4 ? 4 : 1)
#define MVT8B_CB (MVT8B_CHUNK / MVT8B_STEP)   // blocks per chunk
#define MVT8B_XW (MVT8B_CHUNK / 4)            // x dwords per vector and chunk

static_assert(MVT8B_W == 2, "the lane map (8 chains x 2 halves x 16 column groups) assumes 128 columns: cols % 128 == 0 makes every workgroup whole");
static_assert(MVT8B_CHUNK / 16 == 256 && MVT8B_CB * MVT8B_W <= 256 && MVT8B_CB <= 256, "the staging assumes one u32x4 of x per thread and vector, at most one factor per thread");

constexpr size_t mvt8b_stage_bytes(int nv)
{
    const size_t staged = (size_t)nv * MVT8B_CHUNK + MVT8B_CB * MVT8B_W * sizeof(float) + (size_t)nv * MVT8B_CB * sizeof(float);
    const size_t part = 8 * 64 * MVT8B_W * sizeof(float);         // the chain ends reuse the staging area
    return staged > part ? staged : part;
}

// stage the chunk that starts at row r0: x and sx * 1/127 of every present vector, sA * 1/7 of the workgroup's column tiles; all loads
// first (one round trip), then the LDS writes
template <int NV>
__device__ __forceinline__ void mvt8b_stage(uint32_t *xs, float *sas, float *svs, const float *__restrict__ sA, const Mvm8BatchArgs<NV> &arg, int nv,
                                            uint64_t rows, uint64_t r0, uint64_t G, uint64_t cb0, int tid)
{
    const uint32_t ch = (uint32_t)((rows - r0) < MVT8B_CHUNK ? (rows - r0) : MVT8B_CHUNK);
    const uint32_t nx = ch / 16, nb = ch / 64, nc = nb * MVT8B_W;
    const uint32_t ix = (uint32_t)tid < nx ? tid : 0, ib = (uint32_t)tid < nb ? tid : 0, ic = (uint32_t)tid < nc ? tid : 0;
    if (r0) __syncthreads();                             // the previous chunk's x and factors have been consumed
    u32x4 xr[NV];
    float sv[NV];
    const float sa = sA[(r0 / 64 + ic / MVT8B_W) * G + cb0 + ic % MVT8B_W];
    // an absent slot reads vector 0 again (its own pointers are NULL) and stores nothing: no branch around a load, so the registers of
    // xr[] stay plain registers
#pragma unroll
    for (int v = 0; v < NV; v++) {
        const int vv = v < nv ? v : 0;
        xr[v] = reinterpret_cast<const u32x4 *>(arg.x[vv] + r0)[ix];
        sv[v] = arg.sx[vv][r0 / 64 + ib];
    }
    if ((uint32_t)tid < nc) sas[tid] = sa * (1.0f / 7.0f);
#pragma unroll
    for (int v = 0; v < NV; v++) {
        if (v < nv && (uint32_t)tid < nx) reinterpret_cast<u32x4 *>(xs + v * MVT8B_XW)[tid] = xr[v];
        if (v < nv && (uint32_t)tid < nb) svs[v * MVT8B_CB + tid] = sv[v] * (1.0f / 127.0f);
    }
    __syncthreads();
}

// one block: the pair's swap, the transpose and the widening of this thread's 4 columns once, the link of every present vector.  a: this
// lane's 4 rows; xs / svs: the block's x dwords and sx * 1/127 of vector 0 in LDS
template <int NV>
__device__ __forceinline__ void mvt8b_block(const uint32_t (&a)[4], const uint32_t *xs, float sa, const float *svs, int L, int h, int nv,
                                            float (&acc)[NV][4])
{
    uint32_t Wd[8], O[8], f[4], s[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t other = (uint32_t)__shfl_xor((int)a[i], 16);
        Wd[i] = h ? other : a[i];                        // rows 4 L + i
        Wd[4 + i] = h ? a[i] : other;                    // rows 32 + 4 L + i
    }
    transpose8x8_nibbles(Wd, O);                          // O[e]: column 8 cg + e, elements 0 .. 3 = rows 4 L .. 4 L + 3, 4 .. 7 = rows 32 + 4 L ..
#pragma unroll
    for (int k = 0; k < 4; k++) widen8(h ? O[4 + k] : O[k], f[k], s[k]);
#pragma unroll
    for (int v = 0; v < NV; v++)
        if (v < nv) {
            const uint32_t x0 = xs[v * MVT8B_XW + L], x1 = xs[v * MVT8B_XW + 8 + L];    // x of rows 4 L .. 4 L + 3 and 32 + 4 L .. 32 + 4 L + 3
            const float c = sa * svs[v * MVT8B_CB];
#pragma unroll
            for (int k = 0; k < 4; k++) acc[v][k] = __builtin_fmaf(c, (float)mvt8_int(f[k], x0, s[k], x1), acc[v][k]);
        }
}

// this thread's loads of the U blocks of group g (beyond the last block: the last block again).  Aq: the thread's column group in row
// 4 L + 32 h of block 0
template <int U, bool NT>
__device__ __forceinline__ void mvt8b_load(const uint32_t *__restrict__ Aq, uint64_t stride, uint32_t g, uint32_t nblk, uint32_t (&a)[U][4])
{
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint32_t blk = g * U + u < nblk ? g * U + u : nblk - 1;
        mvt8_load<4, 1, NT>(Aq + (uint64_t)blk * 64 * stride, stride, a[u]);
    }
}

// group g of the walk from `cur` (loaded a group ago) while the next group's loads go to `nxt` -- issued UNCONDITIONALLY (beyond the last
// block: the last block again), as mvt8_round (mvm_t8.hip) does
template <int NV, int U, bool NT>
__device__ __forceinline__ void mvt8b_group(const uint32_t (&cur)[U][4], uint32_t (&nxt)[U][4], const uint32_t *__restrict__ Aq, uint64_t stride,
                                            uint32_t g, uint32_t nblk, const uint32_t *xs, const float *sas, const float *svs, int L, int h, int tile,
                                            int nv, float (&acc)[NV][4])
{
    mvt8b_load<U, NT>(Aq, stride, g + 1, nblk, nxt);
    const uint32_t b0 = g * U, lb = b0 % MVT8B_CB;       // a group never straddles a chunk
    if (nblk - b0 >= (uint32_t)U) {
#pragma unroll
        for (int u = 0; u < U; u++) mvt8b_block<NV>(cur[u], xs + 16 * (lb + u), sas[MVT8B_W * (lb + u) + tile], svs + lb + u, L, h, nv, acc);
    } else {
#pragma unroll
        for (int u = 0; u < U; u++)
            if (b0 + u < nblk) mvt8b_block<NV>(cur[u], xs + 16 * (lb + u), sas[MVT8B_W * (lb + u) + tile], svs + lb + u, L, h, nv, acc);
    }
}

template <int NV, int U, bool NT, bool FUSE, bool ST>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void k_m4_mvm8_t_batch(const uint8_t *__restrict__ A, const float *__restrict__ sA, uint64_t rows, uint64_t cols,
                                                         int nv, Mvm8BatchArgs<NV> arg, Mvm8BatchFuse<NV> fuse, MvmBatchRng rs)
{
    static_assert(MVT8B_CB % (2 * U) == 0, "a chunk is whole pairs of load groups");
    constexpr int NW = FUSE ? 2 : 1;                                               // windows per vector: the mvm's draws, the scaleAndAdd's
    __shared__ __attribute__((aligned(16))) char stage[mvt8b_stage_bytes(NV)];
    __shared__ uint64_t sbase[ST ? NV * NW * 4 : 1];                                // ST: [NV][NW][4] lane starts at the workgroup's first block
    __shared__ uint64_t raw[ST ? NV * NW * 8 * MVT8B_W : 1];                        // ST: per window the raw draws of MVT8B_W blocks
    uint32_t *xs = reinterpret_cast<uint32_t *>(stage);                             // [NV][MVT8B_XW]
    float *sas = reinterpret_cast<float *>(stage + NV * MVT8B_CHUNK);               // [MVT8B_CB][MVT8B_W]: sA * 1/7
    float *svs = sas + MVT8B_CB * MVT8B_W;                                          // [NV][MVT8B_CB]: sx * 1/127
    float *part = reinterpret_cast<float *>(stage);                                 // epilogue: part[chain][column]

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint64_t G = cols / 64;                                   // output blocks = column tiles of A
    // Two workgroups share every 128-byte line of a row: blocks b and b + 8 are dealt to one XCD and take adjacent column strips, as in
    // k_m4_mvm8_t (speed only: any map is correct)
    const uint32_t bx = blockIdx.x, wg = bx < (gridDim.x & ~15u) ? (bx & ~15u) + 2 * (bx & 7) + ((bx >> 3) & 1) : bx;
    const uint64_t cb0 = (uint64_t)wg * MVT8B_W, cb = cb0 + wave;
    uint64_t st_seq = 0;
    uint64_t *st_next = nullptr;
    if constexpr (ST) st_next = mvmb_rng_prologue<NV, NW>(rs, nv, cb0, G, sbase, st_seq);

    const int L = tid >> 5, h = (tid >> 4) & 1, cg = tid & 15, tile = cg >> 3;
    const uint64_t stride = cols / 8;                               // dwords per row
    const uint32_t *Aq = reinterpret_cast<const uint32_t *>(A) + cb0 * 8 + cg + (uint64_t)(4 * L + 32 * h) * stride;

    float acc[NV][4];
#pragma unroll
    for (int v = 0; v < NV; v++)
#pragma unroll
        for (int k = 0; k < 4; k++) acc[v][k] = 0.0f;

    // the walk over all rows in groups of U blocks; a chunk is a whole, even number of groups, so x and the factors are re-staged in front
    // of an even group.  Two register sets take turns: no copies, and the loads of the group ahead stay in flight across the staging
    constexpr uint32_t CG = MVT8B_CB / U;
    const uint32_t nblk = (uint32_t)(rows / 64), ngroups = (nblk + U - 1) / U;
    uint32_t a[U][4], b[U][4];
    mvt8b_load<U, NT>(Aq, stride, 0, nblk, a);
    uint32_t g = 0;
    for (; g + 1 < ngroups; g += 2) {
        if (g % CG == 0) mvt8b_stage<NV>(xs, sas, svs, sA, arg, nv, rows, (uint64_t)g * U * 64, G, cb0, tid);
        mvt8b_group<NV, U, NT>(a, b, Aq, stride, g, nblk, xs, sas, svs, L, h, tile, nv, acc);
        mvt8b_group<NV, U, NT>(b, a, Aq, stride, g + 1, nblk, xs, sas, svs, L, h, tile, nv, acc);
    }
    if (g < ngroups) {
        if (g % CG == 0) mvt8b_stage<NV>(xs, sas, svs, sA, arg, nv, rows, (uint64_t)g * U * 64, G, cb0, tid);
        mvt8b_group<NV, U, NT>(a, b, Aq, stride, g, nblk, xs, sas, svs, L, h, tile, nv, acc);
    }

    // FUSE: this wave's block of u of every vector, requested here, behind the row loop (they would cost registers across it) and before
    // any block of any result is written (r2 may be u); the first vector's barriers cover the latency
    int fuse_q[NV] = {};
    float fuse_s[NV] = {};
    if (FUSE && wave < MVT8B_W) {
#pragma unroll
        for (int v = 0; v < NV; v++)
            if (v < nv) {
                fuse_q[v] = fuse.qu[v][cb * 64 + lane];
                fuse_s[v] = fuse.su[v][cb];
            }
    }
    if constexpr (ST) {
        // thread i = (window i >> 2 = v * NW + w, generator lane i & 3): the window's draws of the workgroup's two consecutive blocks
        if (tid < NV * NW * 4 && (tid >> 2) / NW < nv) gen_blocks(sbase[tid], MVT8B_W, raw + (size_t)(tid >> 2) * 8 * MVT8B_W, tid & 3);
    }

    // one vector at a time: the 8 chain ends of every column meet in the wave of the column's output block
#pragma unroll
    for (int v = 0; v < NV; v++)
        if (v < nv) {
            __syncthreads();                                        // the staging area / the previous vector's chain ends have been read
            const f32x4 mine = {acc[v][0], acc[v][1], acc[v][2], acc[v][3]};
            reinterpret_cast<f32x4 *>(part)[L * 16 * MVT8B_W + 2 * cg + h] = mine;      // part[L][8 cg + 4 h + k]
            __syncthreads();                                        // and, for v = 0, raw[] has been written
            if (wave < MVT8B_W) {                                   // wave-uniform: one wave per output block
                float ends[8];
#pragma unroll
                for (int l = 0; l < 8; l++) ends[l] = part[l * 64 * MVT8B_W + 64 * wave + lane];
                float noise = 0.0f, noise2 = 0.0f;
                if constexpr (ST) {
                    noise = m8_mvm_noise(raw + (size_t)(v * NW) * 8 * MVT8B_W + 8 * wave, lane);
                    if (FUSE) noise2 = m8_saa_noise(raw + (size_t)(v * NW + 1) * 8 * MVT8B_W + 8 * wave, lane);
                }
                int8_t *r = arg.r[v];
                mvm8_requantize_wave<FUSE>(mvm8_tree8(ends), noise, noise2, lane, r ? r + cb * 64 : nullptr, r ? arg.sr[v] + cb : nullptr, fuse_q[v],
                                           fuse_s[v], fuse.a, FUSE ? fuse.r2[v] + cb * 64 : nullptr, FUSE ? fuse.sr2[v] + cb : nullptr);
            }
        }
    if constexpr (ST) mvmb_rng_stamp(st_next, st_seq);              // behind the barriers above: every wave's part of the new state was written
}

// ---- launches: declared in mvm_t8_batch.h, instantiated here for the driver's NV = 2, 4, 8 ------------------------------------------
template <int NV, bool NT, bool FUSE, bool ST>
void MvmT8Batch::launch(dim3 grid, hipStream_t st, const uint8_t *A, const float *sA, uint64_t rows, uint64_t cols, int nv, const Args<NV> &arg,
                        const Fuse<NV> &fuse, const MvmBatchRng &rs)
{
    hipLaunchKernelGGL((k_m4_mvm8_t_batch<NV, MVT8B_U(NV), NT, FUSE, ST>), grid, dim3(256), 0, st, A, sA, rows, cols, nv, arg, fuse, rs);
}
MVM_BATCH_INSTANTIATE_LAUNCHES(MvmT8Batch)

// ---- C ABI (include/clover_hip_batch_t_v8.h) ---------------------------------------------------------------------------------------
extern "C" int clm4_mvm_v8_transposed_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                                            const float *const *sx, int8_t *const *r, float *const *sr, uint64_t *rng_state_dev, void *stream)
{
    return mvm_batch_entry<MvmT8Batch>("clm4_mvm_v8_transposed_batch", A, sA, rows, cols, nvec, x, sx, r, sr, rng_state_dev, stream);
}

extern "C" int clm4_mvm_v8_transposed_batch_at(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                                               const float *const *sx, int8_t *const *r, float *const *sr, uint64_t *rng_state_dev,
                                               uint64_t draw_base, uint64_t draw_stride, uint64_t commit_draws, void *stream)
{
    return mvm_batch_at_entry<MvmT8Batch>("clm4_mvm_v8_transposed_batch_at", "clm4_mvm_v8_transposed_batch", A, sA, rows, cols, nvec, x, sx, r, sr,
                                          rng_state_dev, draw_base, draw_stride, commit_draws, stream);
}

extern "C" int clm4_mvm_v8_transposed_scale_and_add_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec,
                                                          const int8_t *const *x, const float *const *sx, const int8_t *const *qu,
                                                          const float *const *su, float a, int8_t *const *t, float *const *st_, int8_t *const *r,
                                                          float *const *sr, uint64_t *rng_state_dev, void *stream)
{
    return mvm_batch_fused_entry<MvmT8Batch>("clm4_mvm_v8_transposed_scale_and_add_batch", A, sA, rows, cols, nvec, x, sx, qu, su, a, t, st_, r, sr,
                                             rng_state_dev, stream);
}
