// mvm_f32_t_device.h -- the transposed product r = A' x of a quantized matrix with fp32 vectors, written once: the column walk of
// k_m4_mvm_f32_t (mvm_f32_t.hip, CloverMatrix4) and k_m8_mvm_f32_t (matrix8_f32_t.hip, CloverMatrix8).  x is fp32 and every
// (column, chain) pair has a register of its own, so nothing is transposed: a lane converts the elements of its own piece of a row and feeds
// each to its own accumulator.
// Mapping:
//   workgroup = a strip of W::COLS columns of every row; it walks ALL rows (a chain is ordered over the rows, so rows are never split between
//               workgroups).  Where W::PARTIAL, the last strip may lie half outside: its lanes beyond `cols` read the strip's first piece
//               (addresses stay inside the matrix) and store nothing;
//   lane      = (piece p = tid % PIECES, chain k = tid / PIECES): one W::piece = W::NACC columns of row 32 b + k of every 32-row block b, one
//               accumulator per column: the lane's one chain is k.  32 * PIECES threads;
//   per block = ONE x value (x[32 b + k]) and ONE factor W::factor(s) per lane -- the lane's columns lie in one 64-column tile, the block in
//               one 64-row tile -- both staged in LDS per W::CHUNK rows: all loads first, then the LDS writes;
//   pipeline  = U blocks of loads per register set, two sets that take turns: the set ahead is loaded -- unconditionally, clamped to the last
//               block -- before the arithmetic of the current one (f16t_group, half16_t.hip);
//   fast path = where W::HAS_FAST, the barrier of the staging tells whether every factor of the strip's chunk passes W::fast_ok; the chunk
//               then takes W::step<true>, otherwise W::step<false>.  Same bits either way.  A width without one stages behind a plain barrier;
//   epilogue  = the 32 chain ends of every column through LDS (stride W::COLS + 1, in the staging area) to one lane per column: the
//               (acc1 + acc2) + (acc3 + acc4) sums, the _mm256_haddf32_ps tree and the fused epilogue (m4f32_store).  u[c] is fetched before
//               the walk, so r2 may be u.
// A width's traits struct W holds exactly what differs:
//   piece, NACC                           what a lane loads of a row, and the columns = accumulators in it
//   COLS, CHUNK                           columns per workgroup; rows of x staged in LDS per pass
//   PARTIAL, CLAMP_TILE                   whether the last strip may reach beyond `cols`; whether the staging clamps the tile index
//   factor(s)                             the factor of a tile from its scale, in the expression of the width's row-major kernel
//   HAS_FAST, fast_ok(c)                  whether a per-chunk fast path exists, and its test of one factor
//   step<FAST>(piece, xv, c, acc)         one chain step of the lane's NACC columns: xv = x of the lane's row, c = the factor of its tile
#pragma once

#include "mvm_f32_device.h"

template <class W> struct MvmF32T {
    static constexpr int PIECES = W::COLS / W::NACC;                 // lanes per row
    static constexpr int THREADS = 32 * PIECES;
    static constexpr int TILES = (W::COLS + 63) / 64;                // column tiles (of A's scale grid) a strip touches
    static constexpr int PART_STRIDE = W::COLS + 1;
    static constexpr uint32_t STAGE = W::CHUNK + W::CHUNK / 64 * TILES;      // floats: x, then [CHUNK / 64][TILES] factors
    static_assert(THREADS >= W::COLS && THREADS <= 1024, "one lane per column in the epilogue");
    static_assert(W::CHUNK % (4 * THREADS) == 0, "a chunk is whole rounds of staging threads");
    static_assert(32 * PART_STRIDE <= STAGE, "the chain ends reuse the staging area");
};

template <bool NT, class P> __device__ __forceinline__ P mvm_f32_t_ld(const P *p) { return NT ? __builtin_nontemporal_load(p) : *p; }

// stage x and the factors of the chunk that starts at row r0: all loads first (one round trip), then the LDS writes.  Returns (to every
// thread) whether every factor of the chunk passes W::fast_ok; a width without a fast path gets `false` behind a plain barrier
template <class W>
__device__ __forceinline__ bool mvm_f32_t_stage(float *xs, float *cs, const float *__restrict__ x, const float *__restrict__ sA, uint64_t rows, uint64_t G,
                                                uint64_t tile0, uint64_t r0, int tid)
{
    constexpr int THREADS = MvmF32T<W>::THREADS, TILES = MvmF32T<W>::TILES;
    constexpr int NX = W::CHUNK / 4 / THREADS;               // 16-byte pieces of x per thread
    constexpr int NC = (W::CHUNK / 64 * TILES + THREADS - 1) / THREADS;      // factors per thread
    const uint32_t ch = (uint32_t)((rows - r0) < W::CHUNK ? (rows - r0) : W::CHUNK);
    if (r0) __syncthreads();                                 // the previous chunk's x has been consumed
    const f32x4 *xg = reinterpret_cast<const f32x4 *>(x) + r0 / 4;
    const uint32_t nx = ch / 4, nc = ch / 64 * TILES;
    f32x4 xr[NX];
#pragma unroll
    for (int j = 0; j < NX; j++) { const uint32_t i = tid + THREADS * j; xr[j] = xg[i < nx ? i : 0]; }
    float c[NC];
#pragma unroll
    for (int j = 0; j < NC; j++) {
        const uint32_t i = tid + THREADS * j, ci = i < nc ? i : 0;
        uint64_t t = tile0 + ci % TILES;
        if constexpr (W::CLAMP_TILE) t = t < G ? t : 0;      // a tile beyond the matrix (masked last strip): tile 0 of the same row tile
        c[j] = W::factor(sA[(r0 / 64 + ci / TILES) * G + t]);
    }
#pragma unroll
    for (int j = 0; j < NX; j++) { const uint32_t i = tid + THREADS * j; if (i < nx) reinterpret_cast<f32x4 *>(xs)[i] = xr[j]; }
    bool fast = true;
#pragma unroll
    for (int j = 0; j < NC; j++) {
        const uint32_t i = tid + THREADS * j;
        if (i < nc) cs[i] = c[j];
        if constexpr (W::HAS_FAST) fast = fast && W::fast_ok(c[j]);      // a clamped index repeats a factor of the chunk
    }
    if constexpr (W::HAS_FAST) return __syncthreads_and(fast) != 0;
    __syncthreads();
    return false;
}

// the loads of group g (U blocks) of the lane whose row of block 0 and piece Ap points at; blocks beyond the last read the last one again
template <class W, int U, bool NT>
__device__ __forceinline__ void mvm_f32_t_load(const typename W::piece *__restrict__ Ap, uint64_t stride, uint32_t g, uint32_t nblk,
                                               typename W::piece (&a)[U])
{
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint32_t b = g * U + u, bc = b < nblk ? b : nblk - 1;
        a[u] = mvm_f32_t_ld<NT>(Ap + (uint64_t)bc * 32 * stride);
    }
}

// group g of the walk from `cur` (loaded a group ago) while the next group's loads go to `nxt` -- issued UNCONDITIONALLY (beyond the last
// block: the last block again), so that the wait for `cur` lets them stay in flight.  xl = xs + the lane's chain, cl = cs + the lane's tile
template <class W, int U, bool NT, bool FAST>
__device__ __forceinline__ void mvm_f32_t_group(const typename W::piece (&cur)[U], typename W::piece (&nxt)[U], const typename W::piece *__restrict__ Ap,
                                                uint64_t stride, uint32_t g, uint32_t nblk, const float *xl, const float *cl, float (&acc)[W::NACC])
{
    constexpr uint32_t CB = W::CHUNK / 32;               // blocks per chunk
    mvm_f32_t_load<W, U, NT>(Ap, stride, g + 1, nblk, nxt);
    const uint32_t b0 = g * U, lb = b0 % CB;             // a group never straddles a chunk
#pragma unroll
    for (int u = 0; u < U; u++)
        if (b0 + u < nblk) W::template step<FAST>(cur[u], xl[32 * (lb + u)], cl[MvmF32T<W>::TILES * ((lb + u) >> 1)], acc);
}

// the body of a width's kernel.  FUSE... = nothing or one M4F32Fuse.  r (t of the fused ABI) may be NULL under FUSE; fuse.r2 may be fuse.u
template <class W, int U, bool NT, typename... FUSE>
__device__ __forceinline__ void mvm_f32_t_walk(const uint8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, float *r, FUSE... fuse)
{
    typedef MvmF32T<W> M;
    typedef typename W::piece piece;
    static_assert((W::CHUNK / 32) % (2 * U) == 0, "a chunk is whole pairs of load groups");
    __shared__ __attribute__((aligned(16))) float stage[M::STAGE];
    float *xs = stage;                                   // W::CHUNK values of x
    float *cs = stage + W::CHUNK;                        // [W::CHUNK / 64][TILES] factors
    float *part = stage;                                 // epilogue: [32 chains][PART_STRIDE]
    constexpr bool FUSED = sizeof...(FUSE) != 0;
    constexpr int NACC = W::NACC;

    const int tid = threadIdx.x, p = tid % M::PIECES, k = tid / M::PIECES;
    const uint64_t strip0 = (uint64_t)blockIdx.x * W::COLS, G = cols / 64;
    // the epilogue's lane of column strip0 + tid: its element of u, fetched now so that the epilogue does not wait for it (and r2 may be u)
    const uint64_t col = strip0 + tid;
    const bool owner = tid < W::COLS && (!W::PARTIAL || col < cols);
    float fuse_u = 0.0f;
    if (FUSED && owner) fuse_u = m4f32_fuse_load_u(col, fuse...);

    const uint64_t stride = cols / NACC;                 // pieces per row
    uint64_t p0 = strip0 / NACC + p;                     // the lane's piece of row k
    if (W::PARTIAL && NACC * p0 >= cols) p0 = strip0 / NACC;      // loads stay inside the matrix; nothing of it is stored
    const piece *Ap = reinterpret_cast<const piece *>(A) + p0 + (uint64_t)k * stride;
    const float *xl = xs + k, *cl = cs + (NACC * p) / 64;

    float acc[NACC];
#pragma unroll
    for (int e = 0; e < NACC; e++) acc[e] = 0.0f;

    // the walk over all rows in groups of U blocks; a chunk is a whole, even number of groups, so x is re-staged in front of an even group.
    // Two register sets take turns: no copies, and the loads of the group ahead stay in flight across the staging
    constexpr uint32_t CG = W::CHUNK / 32 / U;
    const uint32_t nblk = (uint32_t)(rows / 32), ngroups = (nblk + U - 1) / U;
    piece a[U], b[U];
    mvm_f32_t_load<W, U, NT>(Ap, stride, 0, nblk, a);
    bool fast = false;
    uint32_t g = 0;
    for (; g + 1 < ngroups; g += 2) {
        if (g % CG == 0) fast = mvm_f32_t_stage<W>(xs, cs, x, sA, rows, G, strip0 / 64, (uint64_t)g * U * 32, tid);
        if (W::HAS_FAST && fast) {                       // the same for every lane of the workgroup: a real branch
            mvm_f32_t_group<W, U, NT, true>(a, b, Ap, stride, g, nblk, xl, cl, acc);
            mvm_f32_t_group<W, U, NT, true>(b, a, Ap, stride, g + 1, nblk, xl, cl, acc);
        } else {
            mvm_f32_t_group<W, U, NT, false>(a, b, Ap, stride, g, nblk, xl, cl, acc);
            mvm_f32_t_group<W, U, NT, false>(b, a, Ap, stride, g + 1, nblk, xl, cl, acc);
        }
    }
    if (g < ngroups) {
        if (g % CG == 0) fast = mvm_f32_t_stage<W>(xs, cs, x, sA, rows, G, strip0 / 64, (uint64_t)g * U * 32, tid);
        if (W::HAS_FAST && fast) mvm_f32_t_group<W, U, NT, true>(a, b, Ap, stride, g, nblk, xl, cl, acc);
        else mvm_f32_t_group<W, U, NT, false>(a, b, Ap, stride, g, nblk, xl, cl, acc);
    }

    // the 32 chain ends of every column meet in the column's lane
    __syncthreads();                                     // x and the factors have been consumed: the area is reused
#pragma unroll
    for (int e = 0; e < NACC; e++) part[k * M::PART_STRIDE + NACC * p + e] = acc[e];
    __syncthreads();
    if (owner) {
        const float *q = part + tid;
        float s[8];
#pragma unroll
        for (int l = 0; l < 8; l++)
            s[l] = (q[l * M::PART_STRIDE] + q[(8 + l) * M::PART_STRIDE]) + (q[(16 + l) * M::PART_STRIDE] + q[(24 + l) * M::PART_STRIDE]);
        const float t0 = s[4] + s[0], t1 = s[5] + s[1], t2 = s[6] + s[2], t3 = s[7] + s[3];
        m4f32_store(r, col, (t0 + t2) + (t1 + t3), fuse_u, fuse...);
    }
}
