// mvm_t8.hip -- the transposed mixed mvm: r = quantize8(A' x) for a CloverVector8 x straight from A's own 4-bit bytes, no stored transpose.
//
// Contract: byte for byte what clm4_transpose(A -> At) followed by clm4_mvm_v8(At, cols, rows, x -> r) gives, the generator state included.
// Output element j is row j of A' under the definition of k_m4_mvm8 (mixed8.hip): 8 sequential fp32 fma chains; for every 64-row block b
// of A, in order of b, chain L does acc_L = fma(c_b, (float)I, acc_L) with I the exact integer sum of A[64 b + e][j] * x[64 b + e] over
// e in {4 L .. 4 L + 3, 32 + 4 L .. 32 + 4 L + 3} and c_b = mvm8_factor(sA[b][j / 64], sx[b]) read from A's OWN scale grid; then the fixed
// tree and the 64-wide 8-bit re-quantisation.  widen8 / sdot4 / mvm8_factor / mvm8_tree8 / mvm8_requantize_wave are the functions of
// mvm8_device.h; the column words come out of transpose8x8_nibbles (nibble_transpose.h), the very words clm4_transpose stores.
//
// Mapping (map (a) of DESIGN.md 3, "A'x for CloverVector8"): the integers are exact, so they are made wherever the bytes land; only the
// fma of one (column, chain) is ordered over b and stays in ONE register of ONE lane.
//   workgroup = MVT8_W = 2 adjacent output blocks = 128 columns = 64 contiguous bytes of every row, 256 threads; it walks ALL rows.  Two
//               workgroups per CU at 65536 columns (two waves per SIMD: a wave alone issues a VALU instruction every 4 cycles, two
//               share the SIMD at 2), cols / 128 workgroups.  The two workgroups that share the 128-byte lines of a strip are placed
//               on one XCD (blockIdx remap below);
//   producer  = wave w takes row block 4 R + w of round R (MVT8_STEP = 256 rows per round): lane (m = lane >> 4, cg = lane & 15) loads
//               4 B (columns 8 cg .. 8 cg + 7) of rows 8 m .. 8 m + 7 and 32 + 8 m .. 32 + 8 m + 7 of its block -- a wave's load
//               instruction reads 4 rows x 64 B --, transposes the two 8 x 8 pieces in registers and, per column, gets the block integers
//               of chains 2 m and 2 m + 1 (both halves of either chain sit in this lane) against x from LDS.  |I| <= 8 * 7 * 127 fits
//               int16: the pair goes to LDS as one dword, hand[buffer][w][m][16 e + cg] (stride 144 per m: no bank conflicts either way);
//   consumer  = thread t owns column 8 (s & 15) + (s >> 4), s = t & 127, and its chains 4 q .. 4 q + 3, q = t >> 7: after the round's
//               barrier it reads the two dwords of each of the round's blocks in order of b and does the 4 fmas.  The hand-over is double
//               buffered: one barrier per round, and the next round's 16 loads of a lane are issued -- unconditionally, see mvt8_round --
//               before this round's arithmetic (MVT8_U = 1 round of loads ahead), in two register sets that take turns;
//   x, c      = staged per MVT8_CHUNK rows in LDS: x as int8 (MVT8_CHUNK bytes) and c[b][tile] of the 2 column tiles;
//   epilogue  = chains 4 .. 7 of every column through LDS to the thread that holds chains 0 .. 3, mvm8_tree8 there, the 128 dots through
//               LDS to one wave per output block: mvm8_requantize_wave<FUSE>.
// cols is a multiple of 128, so every workgroup has both its output blocks; the clamps of a masked last workgroup (missing columns read
// column 0, their blocks are not stored) stay for a W that does not divide 2.
// Stochastic rounding: output block cb takes the draws clm4_mvm_v8 gives row group cb of a stored A' (mvm8_prologue, mixed8.hip): 2 cb,
// 2 cb + 1 and, fused, 2 G + 2 cb, 2 G + 2 cb + 1 (G = cols / 64); the state is left advanced by 2 G (4 G).
#include "rng_device.h"
#include "mvm_t8_device.h"         // mvt8_load, mvt8_int: shared with k_m4_mvm8_t_batch (mvm_t8_batch.hip)

#include <vector>

#define MVT8_CHUNK 16384u   // rows staged in LDS per pass
#define MVT8_STEP 256u      // rows per round: one 64-row block per wave
#define MVT8_U 1            // rounds of matrix loads issued ahead of the arithmetic (the forms measured: DESIGN.md 3)
#define MVT8_W 2            // output blocks (64 columns each) per workgroup
#define MVT8_HAND_M 144     // dwords per chain pair m of one block's hand-over: 8 columns x 16 column groups + 16 (bank = 16 m + 16 e + cg)
#define MVT8_HAND_BLOCK (4 * MVT8_HAND_M)

static_assert(MVT8_W == 2 && MVT8_STEP == 64 * 4, "the lane map (four waves, one row block each; 16 column groups of 8 columns) assumes 128 columns and 256 rows");
static_assert(MVT8_CHUNK % (64 * 256) == 0 && MVT8_CHUNK % (2 * MVT8_STEP) == 0, "the staging loops assume whole rounds of 256 threads");
static_assert(MVT8_U == 1, "mvt8_round keeps exactly one round of loads ahead");

// this lane's 16 loads of one row block -- rows 8 m + i (lo) and 32 + 8 m + i (hi); Ap: the lane's column group in row 8 m of the block --
// are mvt8_load<8, 2, NT> (mvm_t8_device.h)

// the block integers of chains 2 m, 2 m + 1 for the lane's 8 columns, packed as int16 pairs into the hand-over.  xb: the block's x in LDS
__device__ __forceinline__ void mvt8_produce(const uint32_t (&a)[16], const u32x2 *xb, int m, uint32_t *out)
{
    const u32x2 x0 = xb[m], x1 = xb[4 + m];              // x of rows 8 m .. 8 m + 7 and 32 + 8 m .. 32 + 8 m + 7
    uint32_t W[8], Olo[8], Ohi[8];
#pragma unroll
    for (int i = 0; i < 8; i++) W[i] = a[i];
    transpose8x8_nibbles(W, Olo);
#pragma unroll
    for (int i = 0; i < 8; i++) W[i] = a[8 + i];
    transpose8x8_nibbles(W, Ohi);
#pragma unroll
    for (int e = 0; e < 8; e++) {                        // column 8 cg + e
        uint32_t f03, f47, s03, s47;
        widen8(Olo[e], f03, f47);
        widen8(Ohi[e], s03, s47);
        const int ie = mvt8_int(f03, x0.x, s03, x1.x);                  // chain 2 m   (exact: the sum is a multiple of 16)
        const int io = mvt8_int(f47, x0.y, s47, x1.y);                  // chain 2 m + 1
        out[16 * e] = ((uint32_t)ie & 0xFFFFu) | ((uint32_t)io << 16);
    }
}

// the 4 chain links of one block for the consumer's column and chain half: in = the dwords of chain pairs 2 q and 2 q + 1
__device__ __forceinline__ void mvt8_consume(const uint32_t *in, float c, float (&acc)[4])
{
#pragma unroll
    for (int p = 0; p < 2; p++) {
        const uint32_t d = in[p * MVT8_HAND_M];
        acc[2 * p] = __builtin_fmaf(c, (float)((int)(d << 16) >> 16), acc[2 * p]);
        acc[2 * p + 1] = __builtin_fmaf(c, (float)((int)d >> 16), acc[2 * p + 1]);
    }
}

// stage x and c[b][tile] of the chunk that starts at row r0: all loads first (one round trip), then the LDS writes, as k_m4_mvm8 does
__device__ __forceinline__ void mvt8_stage(char *stage, float *cs, const float *__restrict__ sA, const int8_t *__restrict__ x,
                                           const float *__restrict__ sx, uint64_t rows, uint64_t r0, uint64_t G, uint64_t cb0, int tid)
{
    constexpr int NX = MVT8_CHUNK / 16 / 256;            // 16-byte pieces of x per thread
    constexpr int NC = MVT8_CHUNK / 64 * MVT8_W / 256;   // factors per thread
    const uint32_t ch = (uint32_t)((rows - r0) < MVT8_CHUNK ? (rows - r0) : MVT8_CHUNK);
    const u32x4 *xg = reinterpret_cast<const u32x4 *>(x + r0);
    u32x4 xr[NX];
    float sa[NC], sv[NC];
    const uint32_t nx = ch / 16, nc = ch / 64 * MVT8_W;
    if (r0) __syncthreads();                             // the previous chunk's x and factors have been consumed
#pragma unroll
    for (int j = 0; j < NX; j++) { const uint32_t i = tid + 256 * j; xr[j] = xg[i < nx ? i : 0]; }
#pragma unroll
    for (int j = 0; j < NC; j++) {
        const uint32_t i = tid + 256 * j, ii = i < nc ? i : 0;
        const uint64_t b = r0 / 64 + ii / MVT8_W, t = cb0 + ii % MVT8_W;
        sa[j] = sA[b * G + (t < G ? t : 0)];
        sv[j] = sx[b];
    }
#pragma unroll
    for (int j = 0; j < NX; j++) { const uint32_t i = tid + 256 * j; if (i < nx) reinterpret_cast<u32x4 *>(stage)[i] = xr[j]; }
#pragma unroll
    for (int j = 0; j < NC; j++) { const uint32_t i = tid + 256 * j; if (i < nc) cs[i] = mvm8_factor(sa[j], sv[j]); }
    __syncthreads();
}

// round R of the walk: this wave's block 4 R + wave from `cur` (loaded a round ago) while the next round's loads go to `nxt` -- issued
// UNCONDITIONALLY (beyond the last block: the last block again), so that the wait for `cur` lets them stay in flight: a branch around
// them makes hipcc wait for everything at the join.  Then, behind the barrier, every thread's chain links of the round's blocks in order.
template <bool NT>
__device__ __forceinline__ void mvt8_round(const uint32_t (&cur)[16], uint32_t (&nxt)[16], const uint32_t *__restrict__ Acol, uint64_t stride,
                                           uint32_t R, uint32_t nblk, int wave, int m, const u32x2 *xs, const float *cs, int tile,
                                           uint32_t *hand_out, const uint32_t *hand_in, float (&acc)[4])
{
    constexpr uint32_t CB = MVT8_CHUNK / 64;                                   // blocks per chunk
    const uint32_t blk = 4 * R + wave, next = blk + 4 < nblk ? blk + 4 : nblk - 1, buf = (R & 1) * (4 * MVT8_HAND_BLOCK);
    mvt8_load<8, 2, NT>(Acol + (uint64_t)next * 64 * stride, stride, nxt);
    if (blk < nblk) mvt8_produce(cur, xs + 8 * (blk % CB), m, hand_out + buf); // wave-uniform
    __syncthreads();
    const float *c = cs + MVT8_W * (4 * R % CB) + tile;
    if (nblk - 4 * R >= 4) {
#pragma unroll
        for (int j = 0; j < 4; j++) mvt8_consume(hand_in + buf + j * MVT8_HAND_BLOCK, c[MVT8_W * j], acc);
    } else {
        for (uint32_t j = 0; j < nblk - 4 * R; j++) mvt8_consume(hand_in + buf + j * MVT8_HAND_BLOCK, c[MVT8_W * j], acc);
    }
}

template <int U, bool NT, bool ST, bool FUSE>
__global__ __launch_bounds__(256) void k_m4_mvm8_t(const uint8_t *__restrict__ A, const float *__restrict__ sA, uint64_t rows, uint64_t cols,
                                                   const int8_t *__restrict__ x, const float *__restrict__ sx, int8_t *r, float *sr,
                                                   uint64_t *rng_state, uint64_t seq, const uint64_t *__restrict__ pow_rows, Mvm8Fuse fuse)
{
    __shared__ __attribute__((aligned(16))) char stage[MVT8_CHUNK + MVT8_CHUNK / 64 * MVT8_W * sizeof(float)];
    __shared__ uint32_t hand[2][4 * MVT8_HAND_BLOCK];                              // [buffer][wave = block of the round][m][16 e + cg]
    __shared__ float part[4 * 64 * MVT8_W], dsh[64 * MVT8_W];                      // epilogue: chains 4 .. 7 of every column, the dots
    __shared__ uint64_t rbase[4], raw[8 * MVT8_W], rbase2[4], raw2[8 * MVT8_W];   // ST: 4 lane bases, the raw draws of MVT8_W blocks (twice with FUSE)
    const u32x2 *xs = reinterpret_cast<const u32x2 *>(stage);                      // MVT8_CHUNK bytes of int8
    float *cs = reinterpret_cast<float *>(stage + MVT8_CHUNK);                     // [MVT8_CHUNK / 64][MVT8_W]

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint64_t G = cols / 64;                                   // output blocks = column tiles of A
    // Two workgroups share every 128-byte line of a row.  Blocks b and b + 8 are dealt to one XCD: within whole groups of 16 they take
    // adjacent column strips, so the second half of a line is found in the L2 the first half was fetched into (speed only: any map is correct)
    const uint32_t bx = blockIdx.x, wg = bx < (gridDim.x & ~15u) ? (bx & ~15u) + 2 * (bx & 7) + ((bx >> 3) & 1) : bx;
    const uint64_t cb0 = (uint64_t)wg * MVT8_W, cb = cb0 + wave;
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
    if (FUSE && wave < MVT8_W && cb < G) {
        fuse_q = fuse.qu[cb * 64 + lane];
        fuse_s = fuse.su[cb];
    }

    const int m = lane >> 4, cg = lane & 15;
    const uint64_t stride = cols / 8;                               // dwords per row
    const uint64_t colg = cb0 * 8 + cg;                             // this lane's column group; beyond the matrix: column group 0
    const uint32_t *Acol = reinterpret_cast<const uint32_t *>(A) + (colg < stride ? colg : 0) + (uint64_t)(8 * m) * stride;
    uint32_t *hand_out = &hand[0][wave * MVT8_HAND_BLOCK + m * MVT8_HAND_M + cg];
    const int slot = tid & (64 * MVT8_W - 1), q = tid >> 7;         // the consumer's column 8 (slot & 15) + (slot >> 4), chains 4 q .. 4 q + 3
    const uint32_t *hand_in = &hand[0][2 * q * MVT8_HAND_M + slot];
    const int ccol = 8 * (slot & 15) + (slot >> 4), tile = ccol >> 6;

    float acc[4];
#pragma unroll
    for (int e = 0; e < 4; e++) acc[e] = 0.0f;

    // the walk over all rows in rounds of 4 blocks; a chunk is a whole, even number of rounds, so x and the factors are re-staged in front
    // of an even round.  Two register sets take turns: no copies, and the loads of the round ahead stay in flight across the staging
    constexpr uint32_t CR = MVT8_CHUNK / MVT8_STEP;
    const uint32_t nblk = (uint32_t)(rows / 64), nrounds = (nblk + 3) / 4;
    uint32_t a[16], b[16];
    mvt8_load<8, 2, NT>(Acol + (uint64_t)((uint32_t)wave < nblk ? wave : nblk - 1) * 64 * stride, stride, a);
    uint32_t R = 0;
    for (; R + 1 < nrounds; R += 2) {
        if (R % CR == 0) mvt8_stage(stage, cs, sA, x, sx, rows, (uint64_t)R * MVT8_STEP, G, cb0, tid);
        mvt8_round<NT>(a, b, Acol, stride, R, nblk, wave, m, xs, cs, tile, hand_out, hand_in, acc);
        mvt8_round<NT>(b, a, Acol, stride, R + 1, nblk, wave, m, xs, cs, tile, hand_out, hand_in, acc);
    }
    if (R < nrounds) {
        if (R % CR == 0) mvt8_stage(stage, cs, sA, x, sx, rows, (uint64_t)R * MVT8_STEP, G, cb0, tid);
        mvt8_round<NT>(a, b, Acol, stride, R, nblk, wave, m, xs, cs, tile, hand_out, hand_in, acc);
    }

    // the 8 chain ends of a column meet in the thread of its lower half
    if (q) {
#pragma unroll
        for (int e = 0; e < 4; e++) part[e * 64 * MVT8_W + slot] = acc[e];
    }
    __syncthreads();
    if (!q) {
        const float ends[8] = {acc[0], acc[1], acc[2], acc[3], part[slot], part[64 * MVT8_W + slot], part[2 * 64 * MVT8_W + slot], part[3 * 64 * MVT8_W + slot]};
        dsh[ccol] = mvm8_tree8(ends);
    }
    if (ST && tid < 4) {
        gen_blocks(rbase[tid], MVT8_W, raw, tid);
        if (FUSE) gen_blocks(rbase2[tid], MVT8_W, raw2, tid);
    }
    __syncthreads();
    if (wave < MVT8_W && cb < G) {                                  // wave-uniform: one wave per output block
        float noise = 0.0f, noise2 = 0.0f;
        if (ST) {                                                   // the element <-> noise maps of mvm8_epilogue (mixed8.hip)
            const int g = lane >> 3, j = lane & 7;
            noise = noise_of(reinterpret_cast<const uint32_t *>(raw + 8 * wave + (size_t)(g >> 2) * 4)[j], g & 3);
            if (FUSE) noise2 = noise_of(reinterpret_cast<const uint32_t *>(raw2 + 8 * wave + (size_t)(lane >> 5) * 4)[(lane & 31) >> 2], lane & 3);
        }
        mvm8_requantize_wave<FUSE>(dsh[64 * wave + lane], noise, noise2, lane, r ? r + cb * 64 : nullptr, r ? sr + cb : nullptr, fuse_q, fuse_s, fuse.a,
                                   FUSE ? fuse.r2 + cb * 64 : nullptr, FUSE ? fuse.sr2 + cb : nullptr);
    }
}

static int launch_mvm8_t(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const int8_t *x, const float *sx, int8_t *r, float *sr,
                         uint64_t *rng, hipStream_t st, const Mvm8Fuse *fuse)
{
    const uint64_t G = cols / 64;
    const dim3 grid((unsigned)((G + MVT8_W - 1) / MVT8_W)), block(256);
    RngTables T = {nullptr, nullptr, nullptr};
    uint64_t seq = 0;
    if (rng) {
        int rc = clv_rng_tables(&T);
        if (rc) return rc;
        seq = clv_rng_seq_for(rng, st);
    }
    const Mvm8Fuse no_fuse = {nullptr, nullptr, 0.0f, nullptr, nullptr};
#define MVT8_LAUNCH_F(NT, ST, FUSE)                                                                                                   \
    hipLaunchKernelGGL((k_m4_mvm8_t<MVT8_U, NT, ST, FUSE>), grid, block, 0, st, (const uint8_t *)A, sA, rows, cols, x, sx, r, sr, rng, seq, \
                       T.pow_rows, FUSE ? *fuse : no_fuse)
#define MVT8_LAUNCH(NT, ST)                                  \
    do {                                                     \
        if (fuse) MVT8_LAUNCH_F(NT, ST, true);               \
        else MVT8_LAUNCH_F(NT, ST, false);                   \
    } while (0)
    // streaming (nt) loads once the matrix cannot live in the 256 MiB Infinity Cache: the rule of launch_mvm (matrix4.hip)
    const bool streaming = rows * (cols / 2) > (256ull << 20);
    if (streaming) {
        if (rng) MVT8_LAUNCH(true, true); else MVT8_LAUNCH(true, false);
    } else {
        if (rng) MVT8_LAUNCH(false, true); else MVT8_LAUNCH(false, false);
    }
#undef MVT8_LAUNCH
#undef MVT8_LAUNCH_F
    CLV_LAUNCH_CHECK();
    return CLV_OK;
}

// the argument checks of the transposed calls with CloverVector8 vectors, before any device work (the rules of check_mvm_t_args, mvm_t4.hip,
// with CloverVector8 byte counts); declared in mvm8_device.h, shared with matrix8_t.hip
int clv_internal_check_mvm8_t_args(const char *fn, const void *A, uint64_t a_bytes, const float *sA, uint64_t rows, uint64_t cols, const int8_t *x,
                                   const float *sx, bool fused, const int8_t *qu, const float *su, const int8_t *t, const float *st_, const int8_t *r,
                                   const float *sr)
{
    CLV_REQUIRE(A && sA && x && sx && r && sr && (!fused || (qu && su)), "%s: null pointer", fn);
    CLV_REQUIRE((t == nullptr) == (st_ == nullptr), "%s: t and st must both be given or both be NULL", fn);
    CLV_REQUIRE(rows % 128 == 0 && cols % 128 == 0, "%s: rows=%llu cols=%llu must be multiples of 128", fn, (unsigned long long)rows,
                (unsigned long long)cols);
    CLV_REQUIRE(cols / 64 <= 0x7FFFFFFFull, "%s: too many columns", fn);
    if (!rows || !cols) return 1;
    std::vector<ClvRange> rg;
    rg.reserve(10);
    const uint64_t sc = sizeof(float);
    rg.push_back(clv_range(A, a_bytes, false, ~0ull, "A"));
    rg.push_back(clv_range(sA, (rows / 64) * (cols / 64) * sc, false, ~0ull, "sA"));
    rg.push_back(clv_range(x, rows, false, 0, "x"));
    rg.push_back(clv_range(sx, rows / 64 * sc, false, 0, "sx"));
    rg.push_back(clv_range(r, cols, true, 0, "r"));
    rg.push_back(clv_range(sr, cols / 64 * sc, true, 0, "sr"));
    if (fused) {
        // the in-place result IS its input: a wave reads its own block of u before it writes it
        if ((const void *)qu != (const void *)r) rg.push_back(clv_range(qu, cols, false, 0, "qu"));
        if ((const void *)su != (const void *)sr) rg.push_back(clv_range(su, cols / 64 * sc, false, 0, "su"));
        if (t) {
            rg.push_back(clv_range(t, cols, true, 0, "t"));
            rg.push_back(clv_range(st_, cols / 64 * sc, true, 0, "st"));
        }
    }
    return clv_internal_check_ranges(fn, rg);
}

extern "C" int clm4_mvm_v8_transposed(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const int8_t *x, const float *sx, int8_t *r,
                                      float *sr, uint64_t *rng_state_dev, void *stream)
{
    const int rc = clv_internal_check_mvm8_t_args("clm4_mvm_v8_transposed", A, rows * (cols / 2), sA, rows, cols, x, sx, false, nullptr, nullptr, nullptr, nullptr, r, sr);
    if (rc) return rc > 0 ? CLV_OK : rc;
    return launch_mvm8_t(A, sA, rows, cols, x, sx, r, sr, rng_state_dev, as_stream(stream), nullptr);
}

extern "C" int clm4_mvm_v8_transposed_scale_and_add(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const int8_t *x,
                                                    const float *sx, const int8_t *qu, const float *su, float a, int8_t *t, float *st_, int8_t *r,
                                                    float *sr, uint64_t *rng_state_dev, void *stream)
{
    const int rc = clv_internal_check_mvm8_t_args("clm4_mvm_v8_transposed_scale_and_add", A, rows * (cols / 2), sA, rows, cols, x, sx, true, qu, su, t, st_, r, sr);
    if (rc) return rc > 0 ? CLV_OK : rc;
    const Mvm8Fuse fuse = {qu, su, a, r, sr};
    return launch_mvm8_t(A, sA, rows, cols, x, sx, t, st_, rng_state_dev, as_stream(stream), &fuse);
}

// mixed8.hip
int clv_internal_v8_clear(int8_t *x, float *sx, uint64_t n_pad, hipStream_t st);

// clm4_iht_v8 (mixed8.hip) with ONE matrix: Phi' t2 comes straight from Phi, so no PhiT exists.  Always the launch-per-step loop -- the
// persistent kernel keeps both matrices in LDS -- and bit-identical to clm4_iht_v8 called with PhiT = transpose(Phi): x, t1 .. t3 and the
// generator state.
extern "C" int clm4_iht_v8_one_matrix(const int8_t *Phi, const float *sPhi, uint64_t m, uint64_t n, int8_t *x, float *sx, uint64_t x_len,
                                      const int8_t *y, const float *sy, int8_t *t1, float *st1, int8_t *t2, float *st2, int8_t *t3, float *st3,
                                      uint64_t iterations, uint64_t K, float mu, int threshold, uint64_t *rng_state_dev, void *stream)
{
    CLV_REQUIRE(Phi && sPhi && x && sx && y && sy && t1 && st1 && t2 && st2 && t3 && st3, "clm4_iht_v8_one_matrix: null pointer");
    CLV_REQUIRE(m % 128 == 0 && n % 128 == 0 && x_len <= n, "clm4_iht_v8_one_matrix: m=%llu n=%llu x_len=%llu", (unsigned long long)m,
                (unsigned long long)n, (unsigned long long)x_len);
    int rc0 = clv_internal_v8_clear(x, sx, n, as_stream(stream));      // x.clear()
    if (rc0) return rc0;
    for (uint64_t it = 0; it < iterations; it++) {
        int rc = clm4_mvm_v8_scale_and_add(Phi, sPhi, m, n, x, sx, y, sy, -1.0f, t1, st1, t2, st2, rng_state_dev, stream);                // t1 = Phi x; t2 = y - t1
        if (!rc) rc = clm4_mvm_v8_transposed_scale_and_add(Phi, sPhi, m, n, t2, st2, x, sx, mu, t3, st3, x, sx, rng_state_dev, stream);   // t3 = Phi' t2; x += mu t3
        if (!rc && threshold)
            rc = clv8_threshold_mode(x, sx, x_len, n, K, threshold == 2 ? CLV_THRESHOLD_REFERENCE : CLV_THRESHOLD_FAST, nullptr, stream);
        if (rc) return rc;
    }
    return CLV_OK;
}
