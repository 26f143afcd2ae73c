// matrix8_t.hip -- the transposed 8-bit mvm: r = quantize8(A' x) for a CloverMatrix8 A and a CloverVector8 x straight from A's own bytes,
// no stored transpose.
//
// Contract: byte for byte what clm8_transpose(A -> At) followed by clm8_mvm(At, cols, rows, x -> r) gives, the generator state included.
// Output element j is row j of A' under the definition of m8_mvm_steps (matrix8.hip): 8 sequential fp32 fma chains; for every 64-row block
// b of A, in order of b, chain L does acc_L = fma(c_b, (float)I, acc_L) with I the exact int32 sum of A[64 b + e][j] * x[64 b + e] over
// e in {4 L .. 4 L + 3, 32 + 4 L .. 32 + 4 L + 3} and c_b = m8_factor(sA[b][j / 64], sx[b]) read from A's OWN scale grid; then mvm8_tree8
// and the 64-wide re-quantisation mvm8_requantize_wave with the noise maps m8_mvm_noise / m8_saa_noise: all functions of mvm8_device.h,
// the ones k_m8_mvm uses or bit-equal restatements of its expressions (the existing CloverMatrix8 tests hold matrix8.hip to its bits).
//
// Mapping: the integers are exact, so they are made where the bytes land; only the fma of one (column, chain) is ordered over b, and it
// stays in ONE register of ONE lane for the whole walk -- no hand-over through LDS.
//   workgroup = M8T_W = 2 adjacent output blocks = 128 columns = ONE whole 128-byte line of every row, 256 threads; it walks ALL rows.
//               cols / 128 workgroups; no line is shared between workgroups;
//   thread    = (cq = tid & 31, L = tid >> 5): columns 4 cq .. 4 cq + 3 of the strip, chain L: 4 accumulators.  Per block it loads the
//               dword at its column quad from rows 64 b + 4 L + i and 64 b + 32 + 4 L + i, i = 0 .. 3 (8 loads; a wave's load instruction
//               reads 2 rows x 128 B), transposes the two 4 x 4 byte pieces in registers (8 v_perm each), and per column does two sdot4
//               against the dwords x[64 b + 4 L .. + 3] and x[64 b + 32 + 4 L .. + 3] (LDS, the same pair for all lanes of one L), one
//               convert and one fma;
//   pipeline  = M8T_U blocks of loads per register set, two sets that take turns: the set ahead is loaded -- unconditionally, clamped to
//               the last block, see m8t_group -- before the arithmetic of the current one;
//   x, c      = staged per M8T_CHUNK rows in LDS: x as int8 and c[b][tile] of the 2 column tiles, all loads first, then the LDS writes;
//   epilogue  = the 8 chain ends of every column through LDS to one wave per output block: mvm8_tree8, mvm8_requantize_wave<FUSE>.  The
//               block of u is fetched before the walk, so r may be u.
// Stochastic rounding: output block cb takes the draws clm8_mvm gives row group cb of a stored A': 2 cb, 2 cb + 1 and, fused,
// 2 G + 2 cb, 2 G + 2 cb + 1 (G = cols / 64); the state is left advanced by 2 G (4 G).  The four waves are the four generator lanes.
#include "rng_device.h"
#include "matrix8_t_device.h"      // m8t_transpose4x4, m8t_load, m8t_link: shared with k_m8_mvm_t_batch (matrix8_t_batch.hip)

#define M8T_CHUNK 16384u    // rows staged in LDS per pass
#define M8T_STEP 64u        // rows per block: every thread takes part in every block
#define M8T_U 2             // blocks of matrix loads per register set = blocks issued ahead of the arithmetic (the depths measured: DESIGN.md 3)
#define M8T_W 2             // output blocks (64 columns each) per workgroup

static_assert(M8T_W == 2, "the lane map (32 column quads x 8 chains) assumes 128 columns: cols % 128 == 0 makes every workgroup whole");
static_assert(M8T_CHUNK % (64 * 256) == 0 && (M8T_CHUNK / M8T_STEP) % (2 * M8T_U) == 0, "a chunk is whole pairs of load groups and whole rounds of 256 staging threads");

// stage x and c[b][tile] of the chunk that starts at row r0: all loads first (one round trip), then the LDS writes (as mvt8_stage, mvm_t8.hip)
__device__ __forceinline__ void m8t_stage(char *stage, float *cs, const float *__restrict__ sA, const int8_t *__restrict__ x,
                                          const float *__restrict__ sx, uint64_t rows, uint64_t r0, uint64_t G, uint64_t cb0, int tid)
{
    constexpr int NX = M8T_CHUNK / 16 / 256;             // 16-byte pieces of x per thread
    constexpr int NC = M8T_CHUNK / 64 * M8T_W / 256;     // factors per thread
    const uint32_t ch = (uint32_t)((rows - r0) < M8T_CHUNK ? (rows - r0) : M8T_CHUNK);
    const u32x4 *xg = reinterpret_cast<const u32x4 *>(x + r0);
    u32x4 xr[NX];
    float sa[NC], sv[NC];
    const uint32_t nx = ch / 16, nc = ch / 64 * M8T_W;
    if (r0) __syncthreads();                             // the previous chunk's x and factors have been consumed
#pragma unroll
    for (int j = 0; j < NX; j++) { const uint32_t i = tid + 256 * j; xr[j] = xg[i < nx ? i : 0]; }
#pragma unroll
    for (int j = 0; j < NC; j++) {
        const uint32_t i = tid + 256 * j, ii = i < nc ? i : 0;
        const uint64_t b = r0 / 64 + ii / M8T_W;
        sa[j] = sA[b * G + cb0 + ii % M8T_W];
        sv[j] = sx[b];
    }
#pragma unroll
    for (int j = 0; j < NX; j++) { const uint32_t i = tid + 256 * j; if (i < nx) reinterpret_cast<u32x4 *>(stage)[i] = xr[j]; }
#pragma unroll
    for (int j = 0; j < NC; j++) { const uint32_t i = tid + 256 * j; if (i < nc) cs[i] = m8_factor(sa[j], sv[j]); }
    __syncthreads();
}

// the chain link of one block for the thread's 4 columns: xs / cs = the block's x dwords and factors in LDS
__device__ __forceinline__ void m8t_block(const uint32_t (&a)[8], const uint32_t *xs, const float *cs, int L, int tile, float (&acc)[4])
{
    const uint32_t xl = xs[L], xh = xs[8 + L];           // x of rows 4 L .. 4 L + 3 and 32 + 4 L .. 32 + 4 L + 3
    const float c = cs[tile];
    uint32_t lo[4], hi[4];
    m8t_transpose4x4(a, lo);
    m8t_transpose4x4(a + 4, hi);
    m8t_link(lo, hi, xl, xh, c, acc);
}

// group g of the walk from `cur` (loaded a group ago) while the next group's loads go to `nxt` -- issued UNCONDITIONALLY (beyond the last
// block: the last block again), so that the wait for `cur` lets them stay in flight: a branch around them makes hipcc wait for everything
// at the join (mvt8_round, mvm_t8.hip)
template <int U, bool NT>
__device__ __forceinline__ void m8t_group(const uint32_t (&cur)[U][8], uint32_t (&nxt)[U][8], const uint32_t *__restrict__ Aq, uint64_t stride,
                                          uint32_t g, uint32_t nblk, const uint32_t *xs, const float *cs, int L, int tile, float (&acc)[4])
{
    constexpr uint32_t CB = M8T_CHUNK / 64;              // blocks per chunk
    m8t_load<U, NT>(Aq, stride, g + 1, nblk, nxt);
    const uint32_t b0 = g * U, lb = b0 % CB;             // a group never straddles a chunk
    if (nblk - b0 >= (uint32_t)U) {
#pragma unroll
        for (int u = 0; u < U; u++) m8t_block(cur[u], xs + 16 * (lb + u), cs + M8T_W * (lb + u), L, tile, acc);
    } else {
#pragma unroll
        for (int u = 0; u < U; u++)
            if (b0 + u < nblk) m8t_block(cur[u], xs + 16 * (lb + u), cs + M8T_W * (lb + u), L, tile, acc);
    }
}

template <int U, bool NT, bool ST, bool FUSE>
__global__ __launch_bounds__(256) void k_m8_mvm_t(const uint8_t *__restrict__ A, const float *__restrict__ sA, uint64_t rows, uint64_t cols,
                                                  const int8_t *__restrict__ x, const float *__restrict__ sx, int8_t *r, float *sr,
                                                  uint64_t *rng_state, uint64_t seq, const uint64_t *__restrict__ pow_rows, Mvm8Fuse fuse)
{
    __shared__ __attribute__((aligned(16))) char stage[M8T_CHUNK + M8T_CHUNK / 64 * M8T_W * sizeof(float)];
    __shared__ __attribute__((aligned(16))) float part[8 * 64 * M8T_W];                                        // epilogue: part[chain][column]
    __shared__ uint64_t rbase[4], raw[8 * M8T_W], rbase2[4], raw2[8 * M8T_W];     // ST: 4 lane bases, the raw draws of M8T_W blocks (twice with FUSE)
    const uint32_t *xs = reinterpret_cast<const uint32_t *>(stage);                // M8T_CHUNK bytes of int8
    float *cs = reinterpret_cast<float *>(stage + M8T_CHUNK);                      // [M8T_CHUNK / 64][M8T_W]

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint64_t G = cols / 64;                                   // output blocks = column tiles of A
    const uint64_t cb0 = (uint64_t)blockIdx.x * M8T_W, cb = cb0 + wave;
    if (ST) {
        const uint64_t a0 = rng_workgroup_begin(rng_state, seq, pow_rows, cb0, 1, (FUSE ? 4ull : 2ull) * G, rbase);
        if (FUSE) {
            const uint64_t b2 = wave_pow_apply(pow_rows, a0, G + cb0, 1);
            if (lane == 0) rbase2[wave] = b2;                                      // read in the epilogue, barriers in between
        }
    }
    // FUSE: this wave's block of u, fetched now so that the epilogue does not wait for it (and r2 may be u)
    int fuse_q = 0;
    float fuse_s = 0.0f;
    if (FUSE && wave < M8T_W) {
        fuse_q = fuse.qu[cb * 64 + lane];
        fuse_s = fuse.su[cb];
    }

    const int cq = tid & 31, L = tid >> 5, tile = cq >> 4;
    const uint64_t stride = cols / 4;                               // dwords per row
    const uint32_t *Aq = reinterpret_cast<const uint32_t *>(A) + cb0 * 16 + cq + (uint64_t)(4 * L) * stride;

    float acc[4];
#pragma unroll
    for (int k = 0; k < 4; k++) acc[k] = 0.0f;

    // the walk over all rows in groups of U blocks; a chunk is a whole, even number of groups, so x and the factors are re-staged in front
    // of an even group.  Two register sets take turns: no copies, and the loads of the group ahead stay in flight across the staging
    constexpr uint32_t CG = M8T_CHUNK / 64 / U;
    const uint32_t nblk = (uint32_t)(rows / 64), ngroups = (nblk + U - 1) / U;
    uint32_t a[U][8], b[U][8];
    m8t_load<U, NT>(Aq, stride, 0, nblk, a);
    uint32_t g = 0;
    for (; g + 1 < ngroups; g += 2) {
        if (g % CG == 0) m8t_stage(stage, cs, sA, x, sx, rows, (uint64_t)g * U * 64, G, cb0, tid);
        m8t_group<U, NT>(a, b, Aq, stride, g, nblk, xs, cs, L, tile, acc);
        m8t_group<U, NT>(b, a, Aq, stride, g + 1, nblk, xs, cs, L, tile, acc);
    }
    if (g < ngroups) {
        if (g % CG == 0) m8t_stage(stage, cs, sA, x, sx, rows, (uint64_t)g * U * 64, G, cb0, tid);
        m8t_group<U, NT>(a, b, Aq, stride, g, nblk, xs, cs, L, tile, acc);
    }

    // the 8 chain ends of every column meet in the wave of the column's output block
    const f32x4 mine = {acc[0], acc[1], acc[2], acc[3]};
    reinterpret_cast<f32x4 *>(part)[L * 16 * M8T_W + cq] = mine;
    if (ST && tid < 4) {
        gen_blocks(rbase[tid], M8T_W, raw, tid);
        if (FUSE) gen_blocks(rbase2[tid], M8T_W, raw2, tid);
    }
    __syncthreads();
    if (wave < M8T_W) {                                             // wave-uniform: one wave per output block
        float ends[8];
#pragma unroll
        for (int l = 0; l < 8; l++) ends[l] = part[l * 64 * M8T_W + 64 * wave + lane];
        float noise = 0.0f, noise2 = 0.0f;
        if (ST) {
            noise = m8_mvm_noise(raw + 8 * wave, lane);
            if (FUSE) noise2 = m8_saa_noise(raw2 + 8 * wave, lane);
        }
        mvm8_requantize_wave<FUSE>(mvm8_tree8(ends), noise, noise2, lane, r ? r + cb * 64 : nullptr, r ? sr + cb : nullptr, fuse_q, fuse_s, fuse.a,
                                   FUSE ? fuse.r2 + cb * 64 : nullptr, FUSE ? fuse.sr2 + cb : nullptr);
    }
}

static int launch_m8_mvm_t(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const int8_t *x, const float *sx, int8_t *r, float *sr,
                           uint64_t *rng, hipStream_t st, const Mvm8Fuse *fuse)
{
    const dim3 grid((unsigned)(cols / (64 * M8T_W))), block(256);
    RngTables T = {nullptr, nullptr, nullptr};
    uint64_t seq = 0;
    if (rng) {
        int rc = clv_rng_tables(&T);
        if (rc) return rc;
        seq = clv_rng_seq_for(rng, st);
    }
    const Mvm8Fuse no_fuse = {nullptr, nullptr, 0.0f, nullptr, nullptr};
#define M8T_LAUNCH_F(NT, ST, FUSE)                                                                                                    \
    hipLaunchKernelGGL((k_m8_mvm_t<M8T_U, NT, ST, FUSE>), grid, block, 0, st, (const uint8_t *)A, sA, rows, cols, x, sx, r, sr, rng, seq, \
                       T.pow_rows, FUSE ? *fuse : no_fuse)
#define M8T_LAUNCH(NT, ST)                                   \
    do {                                                     \
        if (fuse) M8T_LAUNCH_F(NT, ST, true);                \
        else M8T_LAUNCH_F(NT, ST, false);                    \
    } while (0)
    // streaming (nt) loads once the matrix cannot live in the 256 MiB Infinity Cache: the rule of clm8_mvm
    const bool streaming = rows * cols > (256ull << 20);
    if (streaming) {
        if (rng) M8T_LAUNCH(true, true); else M8T_LAUNCH(true, false);
    } else {
        if (rng) M8T_LAUNCH(false, true); else M8T_LAUNCH(false, false);
    }
#undef M8T_LAUNCH
#undef M8T_LAUNCH_F
    CLV_LAUNCH_CHECK();
    return CLV_OK;
}

extern "C" int clm8_mvm_transposed(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const int8_t *x, const float *sx, int8_t *r,
                                   float *sr, uint64_t *rng_state_dev, void *stream)
{
    const int rc = clv_internal_check_mvm8_t_args("clm8_mvm_transposed", A, rows * cols, sA, rows, cols, x, sx, false, nullptr, nullptr, nullptr,
                                                  nullptr, r, sr);
    if (rc) return rc > 0 ? CLV_OK : rc;
    CLV_REQUIRE(rows / 64 <= 0x7FFFFFFFull, "clm8_mvm_transposed: too many rows");
    return launch_m8_mvm_t(A, sA, rows, cols, x, sx, r, sr, rng_state_dev, as_stream(stream), nullptr);
}

extern "C" int clm8_mvm_transposed_scale_and_add(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const int8_t *x, const float *sx,
                                                 const int8_t *qu, const float *su, float a, int8_t *t, float *st_, int8_t *r, float *sr,
                                                 uint64_t *rng_state_dev, void *stream)
{
    const int rc = clv_internal_check_mvm8_t_args("clm8_mvm_transposed_scale_and_add", A, rows * cols, sA, rows, cols, x, sx, true, qu, su, t, st_,
                                                  r, sr);
    if (rc) return rc > 0 ? CLV_OK : rc;
    CLV_REQUIRE(rows / 64 <= 0x7FFFFFFFull, "clm8_mvm_transposed_scale_and_add: too many rows");
    const Mvm8Fuse fuse = {qu, su, a, r, sr};
    return launch_m8_mvm_t(A, sA, rows, cols, x, sx, t, st_, rng_state_dev, as_stream(stream), &fuse);
}

// clm8_iht (matrix8.hip) with ONE matrix: Phi' t2 comes straight from Phi, so no PhiT exists.  The same number of launches per iteration,
// and bit-identical to clm8_iht called with PhiT = transpose(Phi): x, t1 .. t3 and the generator state.
extern "C" int clm8_iht_one_matrix(const int8_t *Phi, const float *sPhi, uint64_t m, uint64_t n, int8_t *x, float *sx, uint64_t x_len,
                                   const int8_t *y, const float *sy, int8_t *t1, float *st1, int8_t *t2, float *st2, int8_t *t3, float *st3,
                                   uint64_t iterations, uint64_t K, float mu, int threshold, uint64_t *rng_state_dev, void *stream)
{
    CLV_REQUIRE(Phi && sPhi && x && sx && y && sy && t1 && st1 && t2 && st2 && t3 && st3, "clm8_iht_one_matrix: null pointer");
    CLV_REQUIRE(m % 128 == 0 && n % 128 == 0 && x_len <= n, "clm8_iht_one_matrix: m=%llu n=%llu x_len=%llu", (unsigned long long)m,
                (unsigned long long)n, (unsigned long long)x_len);
    int rc = clv_internal_v8_clear(x, sx, n, as_stream(stream));      // x.clear()
    for (uint64_t it = 0; !rc && it < iterations; it++) {
        rc = clm8_mvm_scale_and_add(Phi, sPhi, m, n, x, sx, y, sy, -1.0f, t1, st1, t2, st2, rng_state_dev, stream);                       // t1 = Phi x; t2 = y - t1
        if (!rc) rc = clm8_mvm_transposed_scale_and_add(Phi, sPhi, m, n, t2, st2, x, sx, mu, t3, st3, x, sx, rng_state_dev, stream);      // t3 = Phi' t2; x += mu t3
        if (!rc && threshold)
            rc = clv8_threshold_mode(x, sx, x_len, n, K, threshold == 2 ? CLV_THRESHOLD_REFERENCE : CLV_THRESHOLD_FAST, nullptr, stream);
    }
    return rc;
}
