// mvm_t4_batch.hip -- the transposed 4-bit mvm for several vectors: r[j] = quantize(A' x[j]) for up to CLM4_MVM_BATCH_MAX vectors in ONE
// pass over A's own bytes, no stored transpose.
//
// Contract: byte for byte the sequence of single calls clm4_mvm_transposed / clm4_mvm_transposed_scale_and_add (mvm_t4.hip) for vector 0,
// 1, ... on the same stream, the generator state included -- and so, as those are defined through the stored transpose, what
// clm4_mvm_batch / clm4_mvm_scale_and_add_batch give on clm4_transpose(A).
//
// The kernel keeps the mapping of k_m4_mvm_t: workgroup = MVTB_W = 4 adjacent output blocks = 256 columns, 256 threads, all rows; lane =
// (chain k = tid >> 4, column pair cg = tid & 15), per 128-row step 8 x 8 B of matrix.  What a step costs beyond the loads is the
// transpose8x8_nibbles of its two 8 x 8 pieces and, per vector, 16 links (v_dot8_i32_i4, conversion, fma): the transpose is done ONCE per
// piece, the links repeat per vector on 16 accumulators of its own.  The chains of different vectors are independent and each vector's
// instruction sequence is that of mvm_device.h, which is what makes the results bit-identical.
//   x, factors = staged per MVTB_CHUNK rows in LDS: the x words of every present vector, sA * 1/49 of the workgroup's 4 column tiles ONCE
//                and sx per (block, vector); the lane forms c = (sA * 1/49) * sx itself -- the two roundings of the single kernel's
//                staged factor, in its order;
//   loads      = the U steps after the ones being consumed are requested before the links run (the work of NV vectors on one step is long
//                enough to cover the latency that the single kernel hides with a second step in flight);
//   epilogue   = one vector at a time through the single kernel's `part` buffer (16 chains x stride 257) to four lanes per column, the
//                256 dots of every vector to dsh; then wave w re-quantises output block cb0 + w of every vector (MvmFuse epilogue as
//                in k_m4_mvm_t).
// The last workgroup of a cols / 64 that is no multiple of 4 is masked as in k_m4_mvm_t: its missing columns read column pair 0 and their
// blocks are not stored.
// Stochastic rounding: vector v's window begins draw_base + v * draw_stride draws behind the state the launch reads (MvmBatchRng);
// inside it output block cb takes draws 2 cb, 2 cb + 1 and, fused, 2 G + 2 cb, 2 G + 2 cb + 1 (G = cols / 64), the positions of the
// single kernel.  The jump-ahead to the workgroup's first block runs in the prologue (mvmb_rng_prologue), gen_blocks produces the four
// consecutive blocks of every window in the epilogue, workgroup 0 commits and stamps.
#include "mvm_t4_batch.h"
#include "nibble_transpose.h"

#include "clover_hip_batch_t.h"

// Rows staged in LDS per pass.  The single kernel stages 32768 (24 KiB for one vector); per vector that is 16 KiB of x words, and eight
// do not fit.  8192 rows are 4 KiB of x words + 512 B of sx per vector and 2 KiB of matrix factors: 38 KiB at NV = 8.
#define MVTB_CHUNK 8192u
// 128-row steps per group of loads (one group consumed, the next in flight): 2 x 16 x U load registers beside 16 NV accumulators
#define MVTB_U(NV) ((NV) <= 4 ? 2 : 1)
#define MVTB_PART_STRIDE (64 * MVTB_W + 1)
#define MVTB_XW (MVTB_CHUNK / 8)       // x words per vector and chunk
#define MVTB_CS (MVTB_CHUNK / 64)      // 64-row blocks per chunk

static_assert(MVTB_W == 4, "the lane map (16 column pairs of 16 columns, one wave per output block) assumes 256 columns per workgroup");
static_assert(MVTB_CHUNK / 32 == 256 && MVTB_CS * MVTB_W == 2 * 256 && MVTB_CS <= 256, "the staging assumes one u32x4 of x per thread and vector, two matrix factors per thread");

constexpr size_t mvtb_stage_bytes(int nv)
{
    const size_t staged = (size_t)nv * MVTB_XW * 4 + MVTB_CS * MVTB_W * sizeof(float) + (size_t)nv * MVTB_CS * sizeof(float);
    const size_t part = 16 * MVTB_PART_STRIDE * sizeof(float);      // the chain ends reuse the staging area
    return staged > part ? staged : part;
}

// the loads of U steps from step t0 on (steps beyond the last, S - 1, read the last again: addresses stay inside the matrix).
// Ap: this lane's column pair in row 8 k; stride: u32x2 per matrix row
template <int U, bool NT>
__device__ __forceinline__ void mvtb_load(const u32x2 *__restrict__ Ap, uint64_t stride, uint64_t t0, uint64_t S, u32x2 (&a)[U][8])
{
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint64_t t = t0 + u < S ? t0 + u : S - 1;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const u32x2 *p = Ap + (t * 128 + i) * stride;
            a[u][i] = NT ? __builtin_nontemporal_load(p) : *p;
        }
    }
}

// the links of U loaded steps (s0 .. s0 + U - 1 of the chunk, those below nsteps) for every present vector
template <int NV, int U>
__device__ __forceinline__ void mvtb_consume(const u32x2 (&a)[U][8], const uint32_t *xs, const float *sas, const float *svs, int k, int tile,
                                             uint32_t s0, uint32_t nsteps, int nv, float (&acc)[NV][16])
{
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint32_t s = s0 + u;
        if (s < nsteps) {
            const float sa = sas[MVTB_W * (2 * s + (k >> 3)) + tile];
            uint32_t W[8], O0[8], O1[8];
#pragma unroll
            for (int i = 0; i < 8; i++) W[i] = a[u][i].x;
            transpose8x8_nibbles(W, O0);
#pragma unroll
            for (int i = 0; i < 8; i++) W[i] = a[u][i].y;
            transpose8x8_nibbles(W, O1);
#pragma unroll
            for (int v = 0; v < NV; v++)
                if (v < nv) {
                    const uint32_t xw = xs[v * MVTB_XW + 16 * s + k];
                    const float c = sa * svs[v * MVTB_CS + 2 * s + (k >> 3)];
#pragma unroll
                    for (int e = 0; e < 8; e++) acc[v][e] = mvm_chain_word(c, O0[e], xw, acc[v][e]);
#pragma unroll
                    for (int e = 0; e < 8; e++) acc[v][8 + e] = mvm_chain_word(c, O1[e], xw, acc[v][8 + e]);
                }
        }
    }
}

template <int NV, int U, bool NT, bool FUSE, bool ST>
__global__ __launch_bounds__(256) void k_m4_mvm_t_batch(const uint8_t *__restrict__ A, const float *__restrict__ sA, uint64_t rows, uint64_t cols,
                                                        int nv, MvmBatchArgs<NV> arg, MvmBatchFuse<NV> fuse, MvmBatchRng rs)
{
    static_assert((MVTB_CHUNK / 128) % U == 0, "a group of U steps never straddles two chunks");
    constexpr int NW = FUSE ? 2 : 1;                                               // windows per vector: the mvm's draws, the scaleAndAdd's
    __shared__ __attribute__((aligned(16))) char stage[mvtb_stage_bytes(NV)];
    __shared__ float dsh[NV * 64 * MVTB_W];                                         // the dots of every vector
    __shared__ uint64_t sbase[ST ? NV * NW * 4 : 1];                                // ST: [NV][NW][4] lane starts at the workgroup's first block
    __shared__ uint64_t raw[ST ? NV * NW * 8 * MVTB_W : 1];                         // ST: per window the raw draws of MVTB_W blocks
    uint32_t *xs = reinterpret_cast<uint32_t *>(stage);                             // [NV][MVTB_XW]
    float *sas = reinterpret_cast<float *>(stage + NV * MVTB_XW * 4);               // [MVTB_CS][MVTB_W]: sA * 1/49
    float *svs = sas + MVTB_CS * MVTB_W;                                            // [NV][MVTB_CS]: sx
    float *part = reinterpret_cast<float *>(stage);                                 // epilogue: [16 chains][MVTB_PART_STRIDE]

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint64_t G = cols / 64;                                   // output blocks = column tiles of A
    const uint64_t cb0 = (uint64_t)blockIdx.x * MVTB_W, cb = cb0 + wave;
    uint64_t st_seq = 0;
    uint64_t *st_next = nullptr;
    if constexpr (ST) st_next = mvmb_rng_prologue<NV, NW>(rs, nv, cb0, G, sbase, st_seq);

    const int k = tid >> 4, cg = tid & 15, tile = cg >> 2;
    const uint64_t stride = cols / 16;                              // u32x2 per row
    const uint64_t colg = cb0 * 4 + cg;                             // this lane's column pair; beyond the matrix: column pair 0
    const u32x2 *Ap = reinterpret_cast<const u32x2 *>(A) + (colg < stride ? colg : 0) + (uint64_t)(8 * k) * stride;
    const uint64_t S = rows / 128;                                  // steps in all

    float acc[NV][16];
#pragma unroll
    for (int v = 0; v < NV; v++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[v][e] = 0.0f;

    u32x2 cur[U][8], nxt[U][8];
    mvtb_load<U, NT>(Ap, stride, 0, S, cur);
    for (uint64_t r0 = 0; r0 < rows; r0 += MVTB_CHUNK) {
        const uint32_t ch = (uint32_t)((rows - r0) < MVTB_CHUNK ? (rows - r0) : MVTB_CHUNK);
        if (r0) __syncthreads();
        {   // stage the x words and sx of every present vector and the matrix factors: the loads first, then the LDS writes
            const uint32_t nx = ch / 32, nb = ch / 64, nc = nb * MVTB_W;
            const uint32_t ix = (uint32_t)tid < nx ? tid : 0, ib = (uint32_t)tid < nb ? tid : 0;
            u32x4 xr[NV];
            float sv[NV], sa[2];
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const uint32_t i = tid + 256 * j, ii = i < nc ? i : 0;
                const uint64_t b = r0 / 64 + ii / MVTB_W, t = cb0 + ii % MVTB_W;
                sa[j] = sA[b * G + (t < G ? t : 0)];
            }
#pragma unroll
            for (int v = 0; v < NV; v++)
                if (v < nv) {
                    xr[v] = reinterpret_cast<const u32x4 *>(arg.x[v] + r0 / 2)[ix];
                    sv[v] = arg.sx[v][r0 / 64 + ib];
                }
#pragma unroll
            for (int j = 0; j < 2; j++) { const uint32_t i = tid + 256 * j; if (i < nc) sas[i] = sa[j] * CLV_RCP49; }
#pragma unroll
            for (int v = 0; v < NV; v++)
                if (v < nv) {
                    if ((uint32_t)tid < nx) reinterpret_cast<u32x4 *>(xs + v * MVTB_XW)[tid] = xr[v];
                    if ((uint32_t)tid < nb) svs[v * MVTB_CS + tid] = sv[v];
                }
        }
        __syncthreads();

        const uint32_t nsteps = ch / 128;
        const uint64_t g0 = r0 / 128;                                // the chunk's first step
        for (uint32_t s = 0; s < nsteps; s += U) {
            mvtb_load<U, NT>(Ap, stride, g0 + s + U, S, nxt);        // the group after this one, across the chunk's end too
            mvtb_consume<NV, U>(cur, xs, sas, svs, k, tile, s, nsteps, nv, acc);
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int i = 0; i < 8; i++) cur[u][i] = nxt[u][i];
        }
    }

    // FUSE: this wave's block of u of every vector, requested here, behind the row loop (they would cost registers across it): the
    // trees and their barriers cover the latency
    uint32_t fuse_w[NV] = {};
    float fuse_s[NV] = {};
    if (FUSE && cb < G) {
#pragma unroll
        for (int v = 0; v < NV; v++)
            if (v < nv) {
                fuse_w[v] = fuse.qu[v][cb * 8 + (lane >> 3)];
                fuse_s[v] = fuse.su[v][cb];
            }
    }

    // one vector at a time: the 16 chain ends of column c (local) = part[chain][c]; four lanes per column hold them as mvm_tree wants,
    // quarter q = chains 4q .. 4q + 3
#pragma unroll
    for (int v = 0; v < NV; v++)
        if (v < nv) {
            __syncthreads();                                        // the staging area / the previous vector's chain ends have been read
#pragma unroll
            for (int e = 0; e < 16; e++) part[k * MVTB_PART_STRIDE + 16 * cg + e] = acc[v][e];
            __syncthreads();
#pragma unroll
            for (int rr = 0; rr < MVTB_W; rr++) {
                const int col = 64 * rr + (tid >> 2), q = tid & 3;
                const float *p = part + 4 * q * MVTB_PART_STRIDE + col;
                const float dot = mvm_tree(p[0], p[MVTB_PART_STRIDE], p[2 * MVTB_PART_STRIDE], p[3 * MVTB_PART_STRIDE]);
                if (q == 0) dsh[v * 64 * MVTB_W + col] = dot;
            }
        }
    if constexpr (ST) {
        // thread i = (window i >> 2 = v * NW + w, generator lane i & 3): the window's draws of the workgroup's four consecutive blocks
        if (tid < NV * NW * 4 && (tid >> 2) / NW < nv) gen_blocks(sbase[tid], MVTB_W, raw + (size_t)(tid >> 2) * 8 * MVTB_W, tid & 3);
    }
    __syncthreads();
    if constexpr (ST) mvmb_rng_stamp(st_next, st_seq);              // every wave's part of the new state was written before the barrier
    if (cb < G) {                                                   // wave-uniform: one wave per output block
#pragma unroll
        for (int v = 0; v < NV; v++)
            if (v < nv) {
                uint32_t *r = arg.r[v];
                float m, noise = 0.0f;
                if constexpr (ST) {
                    const int grp = lane & 7, j = lane >> 3;
                    const uint64_t *rw = raw + (size_t)(v * NW) * 8 * MVTB_W;
                    noise = noise_of(reinterpret_cast<const uint32_t *>(rw + 8 * wave + (size_t)(grp >> 2) * 4)[j], grp & 3);
                }
                const int qv = requantize_wave(dsh[v * 64 * MVTB_W + tid], noise, r ? r + cb * 8 : nullptr, r ? arg.sr[v] + cb : nullptr, &m);
                if (FUSE) {
                    const float su7 = div7(fuse_s[v]), sv7 = div7(m * fuse.a);
                    const float val = __builtin_fmaf((float)qv, sv7, (float)unpack1(fuse_w[v], lane & 7) * su7);
                    float m2, noise2 = 0.0f;
                    if constexpr (ST) {
                        const int g = (lane & 7) ^ 1, j = lane >> 3;
                        const uint64_t *rw = raw + (size_t)(v * NW + 1) * 8 * MVTB_W;
                        noise2 = noise_of(reinterpret_cast<const uint32_t *>(rw + 8 * wave + (size_t)(g >> 2) * 4)[j], g & 3);
                    }
                    requantize_wave(val, noise2, fuse.r2[v] + cb * 8, fuse.sr2[v] + cb, &m2);
                }
            }
    }
}

// ---- launches: declared in mvm_t4_batch.h, instantiated here for the driver's NV = 2, 4, 8 -----------------------------------------
template <int NV, bool NT, bool FUSE, bool ST>
void MvmT4Batch::launch(dim3 grid, hipStream_t st, const uint8_t *A, const float *sA, uint64_t rows, uint64_t cols, int nv, const Args<NV> &arg,
                        const Fuse<NV> &fuse, const MvmBatchRng &rs)
{
    hipLaunchKernelGGL((k_m4_mvm_t_batch<NV, MVTB_U(NV), NT, FUSE, ST>), grid, dim3(256), 0, st, A, sA, rows, cols, nv, arg, fuse, rs);
}
MVM_BATCH_INSTANTIATE_LAUNCHES(MvmT4Batch)

// ---- C ABI (include/clover_hip_batch_t.h) ----------------------------------------------------------------------------------------
extern "C" int clm4_mvm_transposed_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                                         const float *const *sx, int8_t *const *r, float *const *sr, uint64_t *rng_state_dev, void *stream)
{
    return mvm_batch_entry<MvmT4Batch>("clm4_mvm_transposed_batch", A, sA, rows, cols, nvec, x, sx, r, sr, rng_state_dev, stream);
}

extern "C" int clm4_mvm_transposed_batch_at(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                                            const float *const *sx, int8_t *const *r, float *const *sr, uint64_t *rng_state_dev,
                                            uint64_t draw_base, uint64_t draw_stride, uint64_t commit_draws, void *stream)
{
    return mvm_batch_at_entry<MvmT4Batch>("clm4_mvm_transposed_batch_at", "clm4_mvm_transposed_batch", A, sA, rows, cols, nvec, x, sx, r, sr,
                                          rng_state_dev, draw_base, draw_stride, commit_draws, stream);
}

extern "C" int clm4_mvm_transposed_scale_and_add_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec,
                                                       const int8_t *const *x, const float *const *sx, const int8_t *const *qu,
                                                       const float *const *su, float a, int8_t *const *t, float *const *st_, int8_t *const *r,
                                                       float *const *sr, uint64_t *rng_state_dev, void *stream)
{
    return mvm_batch_fused_entry<MvmT4Batch>("clm4_mvm_transposed_scale_and_add_batch", A, sA, rows, cols, nvec, x, sx, qu, su, a, t, st_, r, sr,
                                             rng_state_dev, stream);
}
