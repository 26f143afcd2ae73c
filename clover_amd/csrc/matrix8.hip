// matrix8.hip -- CloverMatrix8 on gfx950: quantize, restore, mvm (8-bit and fp32 vectors) and transpose.
//
// HBM layout = the reference's (CloverMatrix8.h:36-90): row-major int8 values (rows*cols bytes), then one fp32 scale per
// 64x64 tile in a row-major (rows/64) x (cols/64) grid.  Value = q * (scale / 127).  Every kernel below reproduces the
// reference's SIMD arithmetic order bit for bit; tests/matrix8_restate.c states the same orders on the CPU.
#include "rng_device.h"
#include "mvm8_device.h"
#include "mvm_f32_device.h"

#include <stdlib.h>

// v_dot4_i32_i8: the exact sum of the four signed byte products of two dwords, plus c
__device__ __forceinline__ int i8dot4(uint32_t a, uint32_t b, int c) { return __builtin_amdgcn_sdot4((int)a, (int)b, c, false); }

// ================================================================================================
// quantize  (CloverMatrix8.h:203-480)
// ================================================================================================
// Workgroup = one 64x64 tile (256 threads).  Thread t: float4 column c = t & 15, rows (t >> 4) + 16 j, j = 0..3; a wave-instruction
// reads four contiguous 256-byte tile rows, a thread writes one dword (4 bytes) per row.
// Per tile: m = max |x| (0 -> 1.0), k = 127 / m, q = trunc(fma(|x|, k, noise)) with the sign of x re-applied (:293-306, :404-428).
// Stochastic stream (:345-400): tiles in column-major order (b_j outer, b_i inner), and per tile row two draws.  Tile row i, column
// e takes draw 2i + (e >> 5), 32-bit word e & 7, byte (e >> 3) & 3 of that word (the slli 0/8/16/24 of rnd_i8_1..4 feed u_1..u_4 =
// columns 0-7, 8-15, 16-23, 24-31).  Here float4 c uses draw 2i + (c >> 3), words 4 (c & 1) .. 4 (c & 1) + 3, byte (c >> 1) & 3.
template <bool ST>
__global__ __launch_bounds__(256) void k_m8_quantize(const f32x4 *__restrict__ A, uint64_t cols, uint32_t h_blocks, uint32_t v_blocks,
                                                     uint32_t *__restrict__ q, float *__restrict__ s, uint64_t *state, uint64_t seq,
                                                     RngTables T)
{
    __shared__ __attribute__((aligned(16))) uint64_t raw[128 * 4];     // ST: the tile's 128 draws, raw[draw * 4 + lane k]
    __shared__ uint64_t base[4];
    __shared__ float wmax[4];
    const int tid = threadIdx.x, wave = tid >> 6;
    const uint32_t b_i = blockIdx.x / h_blocks, b_j = blockIdx.x - b_i * h_blocks;      // neighbouring workgroups: neighbouring tiles of a row
    const int c = tid & 15, r0 = tid >> 4;
    const uint64_t cols4 = cols / 4;
    const uint64_t base4 = (uint64_t)b_i * 64 * cols4 + (uint64_t)b_j * 16 + c;

    SegRows<8> segs;
    if (ST) {
        if (wave == 0) segs.load(T.seg_rows, 0);                      // T^(16 e): 8 segments of 16 draws (8 tile rows)
        const uint64_t t = (uint64_t)b_j * v_blocks + b_i;             // the tile's position in the reference's loop order
        rng_workgroup_begin(state, seq, T.pow_rows, t, 7, 128ull * h_blocks * v_blocks, base);
    }
    f32x4 v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = __builtin_nontemporal_load(&A[base4 + (uint64_t)(r0 + 16 * j) * cols4]);
    if (ST && wave == 0) {
        uint64_t a = segs.starts(base);
        if ((tid & 63) < 32) gen_blocks(a, 8, raw + (size_t)((tid & 63) >> 2) * 64, tid & 3);
    }
    float m = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; j++)
        m = fmaxf(m, fmaxf(fmaxf(__builtin_fabsf(v[j].x), __builtin_fabsf(v[j].y)), fmaxf(__builtin_fabsf(v[j].z), __builtin_fabsf(v[j].w))));
    m = wave_max(m);
    if ((tid & 63) == 0) wmax[wave] = m;
    __syncthreads();
    m = fix_zero_max(fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3])));
    const float k = 127.0f / m;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int i = r0 + 16 * j;
        uint32_t w;
        if (ST) {
            const u32x4 W = reinterpret_cast<const u32x4 *>(raw)[(size_t)(2 * i + (c >> 3)) * 2 + (c & 1)];
            const int sh = (c >> 1) & 3;
            w = ((uint32_t)quant1_st(v[j].x, k, noise_of(W.x, sh)) & 0xFFu) | (((uint32_t)quant1_st(v[j].y, k, noise_of(W.y, sh)) & 0xFFu) << 8) |
                (((uint32_t)quant1_st(v[j].z, k, noise_of(W.z, sh)) & 0xFFu) << 16) | ((uint32_t)quant1_st(v[j].w, k, noise_of(W.w, sh)) << 24);
        } else {
            w = ((uint32_t)quant1_det(v[j].x, k) & 0xFFu) | (((uint32_t)quant1_det(v[j].y, k) & 0xFFu) << 8) |
                (((uint32_t)quant1_det(v[j].z, k) & 0xFFu) << 16) | ((uint32_t)quant1_det(v[j].w, k) << 24);
        }
        // k == inf (tile maximum below 127 / FLT_MAX, about 3.7e-37): the reference's cvttps gives 0x80000000, whose low byte is 0
        __builtin_nontemporal_store(k < __builtin_inff() ? w : 0u, &q[base4 + (uint64_t)i * cols4]);
    }
    if (tid == 0) s[(uint64_t)b_i * h_blocks + b_j] = m;
}

// ================================================================================================
// restore  (CloverMatrix8.h:117-131, get):  A[i][j] = f32(s_tile / 127) * q;  lane = one input dword, one output float4
// ================================================================================================
template <bool NT>
__global__ __launch_bounds__(256) void k_m8_restore(const uint32_t *__restrict__ q, const float *__restrict__ s, f32x4 *__restrict__ A,
                                                    uint64_t nquads, uint64_t cols)
{
    const uint64_t f0 = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 256;
    const int lane = threadIdx.x & 63;
    const uint64_t h_blocks = cols / 64;
    uint32_t wd[4];
    float sc[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint64_t f = f0 + 64 * j + lane, fc = f < nquads ? f : 0;
        const uint64_t e = fc * 4, row = e / cols, col = e - row * cols;
        wd[j] = q[fc];
        sc[j] = s[(row >> 6) * h_blocks + (col >> 6)];
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint64_t f = f0 + 64 * j + lane;
        const float k = div127(sc[j]);
        f32x4 v;
        v.x = (float)((int)(wd[j] << 24) >> 24) * k;
        v.y = (float)((int)(wd[j] << 16) >> 24) * k;
        v.z = (float)((int)(wd[j] << 8) >> 24) * k;
        v.w = (float)((int)wd[j] >> 24) * k;
        if (f < nquads) {
            if (NT) __builtin_nontemporal_store(v, &A[f]);
            else A[f] = v;
        }
    }
}

// ================================================================================================
// mvm, 8-bit vector in and out  (CloverMatrix8.h:1002-1299; mvm_parallel, :664-998, has the same per-row order)
// ================================================================================================
// Per 64-column block b, 32-bit lane k (0..7) of dot_32 is the exact integer sum of the byte products {4k..4k+3} and {32+4k..32+4k+3}
// (maddubs + madd of each half, then add_epi32).  Lane k keeps ONE fp32 chain over all blocks:
//     acc[k] = fma(f32(f32(su * 1/127) * f32(sv * 1/127)), (float)dot_32[k], acc[k])
// and the row value is ((acc0+acc4) + (acc2+acc6)) + ((acc1+acc5) + (acc3+acc7)) (extractf128 / movehl / shuffle 0x55).
// The 64 values of a row group are then re-quantised as CloverVector8::quantize does (:1140-1299), row l taking draw 2 rb + (l >> 5),
// word l & 7, byte (l >> 3) & 3 of the stream (the stochastic form consumes draws 2 rb, 2 rb + 1 for row group rb).
// Mapping: workgroup = one 64-row group (256 threads), lane (row rho = tid >> 2, quarter p = tid & 3) owns chains 2p, 2p + 1 and reads
// dwords 2p, 2p + 1 (bytes 8p..8p+7) and 8 + 2p, 9 + 2p of every block: the four lanes of a row read its 64 bytes per block.  x and the
// scales come through the cache (every wave of the workgroup reads the same x; a wave-instruction asks for 32 distinct bytes of it).
#define M8_MVM_U 8       // blocks in flight per lane

template <bool NT>
__device__ __forceinline__ void m8_mvm_steps(const u32x2 *__restrict__ Ar, const u32x2 *__restrict__ xg, const float *__restrict__ sAr,
                                             const float *__restrict__ sx, int p, uint32_t b0, int nb, float &a0, float &a1)
{
    u32x2 lo[M8_MVM_U], hi[M8_MVM_U], xl[M8_MVM_U], xh[M8_MVM_U];
    float su[M8_MVM_U], sv[M8_MVM_U];
#pragma unroll
    for (int u = 0; u < M8_MVM_U; u++) {
        const uint32_t b = b0 + (u < nb ? u : 0);
        lo[u] = NT ? __builtin_nontemporal_load(&Ar[8 * b + p]) : Ar[8 * b + p];
        hi[u] = NT ? __builtin_nontemporal_load(&Ar[8 * b + 4 + p]) : Ar[8 * b + 4 + p];
        xl[u] = xg[8 * b + p];
        xh[u] = xg[8 * b + 4 + p];
        su[u] = sAr[b];
        sv[u] = sx[b];
    }
#pragma unroll
    for (int u = 0; u < M8_MVM_U; u++) {
        if (u < nb) {
            const float c = m8_factor(su[u], sv[u]);
            a0 = __builtin_fmaf(c, (float)i8dot4(hi[u].x, xh[u].x, i8dot4(lo[u].x, xl[u].x, 0)), a0);
            a1 = __builtin_fmaf(c, (float)i8dot4(hi[u].y, xh[u].y, i8dot4(lo[u].y, xl[u].y, 0)), a1);
        }
    }
}

// FUSE (clm8_mvm_scale_and_add): the CloverVector8::scaleAndAdd that follows this mvm in the IHT / GD loops (CloverVector8.h:1089-1358),
// done on the row group while the first wave still holds it: r2 = quantize8(u + a * quantize8(A x)).  Its two draws per block follow ALL
// the mvm draws in the stream (row group rb: draws 2 G + 2 rb, + 1 with G = rows / 64), as two separate calls leave them; element l takes
// draw l >> 5, word (l & 31) >> 2, byte l & 3 (k_v8_scale_and_add_st).  r (the quantised A x) may be NULL under FUSE: it is then not stored.
struct M8Fuse {
    const int8_t *qu;        // u, one 64-element block per row group
    const float *su;
    float a;
    int8_t *r2;              // may alias qu (the in-place form): the block of u is read before the streaming loop
    float *sr2;
};

template <bool NT, bool ST, bool FUSE>
__device__ __forceinline__ void m8_mvm_body(const uint8_t *__restrict__ A, const float *__restrict__ sA, uint64_t cols, const uint8_t *__restrict__ x,
                                            const float *__restrict__ sx, int8_t *r, float *sr, uint64_t *rng_state, uint64_t seq,
                                            const uint64_t *__restrict__ pow_rows, const M8Fuse &fuse)
{
    __shared__ float dsh[64];
    __shared__ __attribute__((aligned(16))) uint64_t raw[8];          // ST: the row group's two draws
    __shared__ uint64_t rbase[4];
    __shared__ __attribute__((aligned(16))) uint64_t raw2[8];         // ST && FUSE: the two draws of the scaleAndAdd
    __shared__ uint64_t rbase2[4];
    if (ST && !FUSE) rng_workgroup_begin(rng_state, seq, pow_rows, blockIdx.x, 1, 2ull * gridDim.x, rbase);
    if (ST && FUSE) {
        // rng_workgroup_begin with a second base, both written before its barrier
        const int k = threadIdx.x >> 6;
        seq = rng_effective_seq(rng_state, seq);
        const int slot = rng_read_slot(rng_state, seq);
        const uint64_t g0 = rng_state[slot * RNG_SLOT_WORDS + 4 + k];
        const uint64_t b1 = wave_pow_apply(pow_rows, g0, blockIdx.x, 1);
        const uint64_t b2 = wave_pow_apply(pow_rows, g0, (uint64_t)gridDim.x + blockIdx.x, 1);
        if ((threadIdx.x & 63) == 0) {
            rbase[k] = b1;
            rbase2[k] = b2;
        }
        rng_commit(rng_state, seq, slot, pow_rows, g0, 4ull * gridDim.x);
    }
    const uint64_t rb = blockIdx.x;
    const int tid = threadIdx.x, p = tid & 3, rho = tid >> 2;
    int fuse_q = 0;
    float fuse_s = 0.0f;
    if (FUSE && tid < 64) {                                           // this row group's block of u, ahead of the streaming loop
        fuse_q = fuse.qu[rb * 64 + tid];
        fuse_s = fuse.su[rb];
    }
    const uint64_t row = rb * 64 + rho;
    const uint32_t nblk = (uint32_t)(cols / 64);
    const u32x2 *Ar = reinterpret_cast<const u32x2 *>(A + row * cols);
    const u32x2 *xg = reinterpret_cast<const u32x2 *>(x);
    const float *sAr = sA + rb * nblk;
    float a0 = 0.0f, a1 = 0.0f;
    uint32_t b = 0;
    for (; b + M8_MVM_U <= nblk; b += M8_MVM_U) m8_mvm_steps<NT>(Ar, xg, sAr, sx, p, b, M8_MVM_U, a0, a1);
    if (b < nblk) m8_mvm_steps<NT>(Ar, xg, sAr, sx, p, b, (int)(nblk - b), a0, a1);

    // lane p holds acc[2p], acc[2p+1];  acc[k] + acc[k+4] sits in lanes p, p ^ 2;  then t[k] + t[k+2] in lanes p, p ^ 1
    const float t0 = a0 + __shfl_xor(a0, 2), t1 = a1 + __shfl_xor(a1, 2);
    const float x0 = t0 + __shfl_xor(t0, 1), x1 = t1 + __shfl_xor(t1, 1);
    if (p == 0) dsh[rho] = x0 + x1;
    if (ST && tid < 4) {
        gen_blocks(rbase[tid], 1, raw, tid);
        if (FUSE) gen_blocks(rbase2[tid], 1, raw2, tid);
    }
    __syncthreads();
    if (tid < 64) {
        const float d = dsh[tid];
        float noise = 0.0f;
        if (ST) noise = m8_mvm_noise(raw, tid);
        const float m = fix_zero_max(wave_max(__builtin_fabsf(d)));
        const float k = 127.0f / m;
        const int qv = quant1(d, k, noise);
        if (!FUSE || r) {
            r[rb * 64 + tid] = (int8_t)qv;
            if (tid == 0) sr[rb] = m;
        }
        if (FUSE) {
            const float val = __builtin_fmaf((float)qv, div127(m * fuse.a), (float)fuse_q * div127(fuse_s));
            float noise2 = 0.0f;
            if (ST) noise2 = m8_saa_noise(raw2, tid);
            const float m2 = fix_zero_max(wave_max(__builtin_fabsf(val)));
            fuse.r2[rb * 64 + tid] = (int8_t)quant1(val, 127.0f / m2, noise2);
            if (tid == 0) fuse.sr2[rb] = m2;
        }
    }
}

template <bool NT, bool ST>
__global__ __launch_bounds__(256) void k_m8_mvm(const uint8_t *__restrict__ A, const float *__restrict__ sA, uint64_t cols,
                                                const uint8_t *__restrict__ x, const float *__restrict__ sx, int8_t *__restrict__ r,
                                                float *__restrict__ sr, uint64_t *rng_state, uint64_t seq, const uint64_t *__restrict__ pow_rows)
{
    const M8Fuse none = {nullptr, nullptr, 0.0f, nullptr, nullptr};
    m8_mvm_body<NT, ST, false>(A, sA, cols, x, sx, r, sr, rng_state, seq, pow_rows, none);
}

// r / sr: the quantised A x (t of the ABI), NULL = not stored.  No __restrict__ on the vectors: fuse.r2 may be fuse.qu.
template <bool NT, bool ST>
__global__ __launch_bounds__(256) void k_m8_mvm_saa(const uint8_t *__restrict__ A, const float *__restrict__ sA, uint64_t cols,
                                                    const uint8_t *__restrict__ x, const float *__restrict__ sx, int8_t *r, float *sr,
                                                    uint64_t *rng_state, uint64_t seq, const uint64_t *__restrict__ pow_rows, M8Fuse fuse)
{
    m8_mvm_body<NT, ST, true>(A, sA, cols, x, sx, r, sr, rng_state, seq, pow_rows, fuse);
}

// ================================================================================================
// mvm, fp32 vector in and out  (CloverMatrix8.h:558-662)
// ================================================================================================
// Per block b: f = su[b] / 127.0f; element 8j + l of the block (j = 0..7, l = 0..7: the restore_perm shuffles put the 64 bytes back
// in natural order, q_(j+1) lane l) feeds accumulator j mod 4, AVX lane l, as fma(f32(v * f), (float)q, acc) -- j = 0..3 first, then
// j = 4..7.  Row value: sum = (acc1 + acc2) + (acc3 + acc4), then _mm256_haddf32_ps (CloverBase.h:149-157):
//     x[i] = sum[i + 4] + sum[i],  (x0 + x2) + (x1 + x3).
// Mapping: 8 lanes per row, lane e (0..7) owns accumulator e >> 1, AVX lanes 4 (e & 1) .. 4 (e & 1) + 3, i.e. elements 4e..4e+3 and
// 32+4e..32+4e+3 of every block -- dword e and dword 8 + e of the row's block.  Workgroup = 32 rows.
// FUSE... = nothing (clm8_mvm_f32) or one M4F32Fuse (mvm_f32_device.h): r is then t of the fused call and may be NULL
template <bool NT, typename... FUSE>
__global__ __launch_bounds__(256) void k_m8_mvm_f32(const uint32_t *__restrict__ A, const float *__restrict__ sA, uint64_t cols,
                                                    const f32x4 *__restrict__ x, float *__restrict__ r, FUSE... fuse)
{
    constexpr bool FUSED = sizeof...(FUSE) != 0;
    const int tid = threadIdx.x, e = tid & 7;
    const uint64_t row = (uint64_t)blockIdx.x * 32 + (tid >> 3);
    float fuse_u = 0.0f;
    if (FUSED && e == 0) fuse_u = m4f32_fuse_load_u(row, fuse...);      // ahead of the streaming loop: the epilogue waits on nothing
    const uint32_t nblk = (uint32_t)(cols / 64);
    const uint32_t *Ar = A + row * (cols / 4);
    const float *sAr = sA + (row >> 6) * nblk;
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f;
    constexpr int U = 8;
    for (uint32_t b0 = 0; b0 < nblk; b0 += U) {
        uint32_t lo[U], hi[U];
        f32x4 vl[U], vh[U];
        float sc[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t b = b0 + u < nblk ? b0 + u : b0;
            lo[u] = NT ? __builtin_nontemporal_load(&Ar[16 * b + e]) : Ar[16 * b + e];
            hi[u] = NT ? __builtin_nontemporal_load(&Ar[16 * b + 8 + e]) : Ar[16 * b + 8 + e];
            vl[u] = x[16 * b + e];
            vh[u] = x[16 * b + 8 + e];
            sc[u] = sAr[b];
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (b0 + u < nblk) {
                const float f = sc[u] / 127.0f;
                c0 = __builtin_fmaf(vl[u].x * f, (float)((int)(lo[u] << 24) >> 24), c0);
                c1 = __builtin_fmaf(vl[u].y * f, (float)((int)(lo[u] << 16) >> 24), c1);
                c2 = __builtin_fmaf(vl[u].z * f, (float)((int)(lo[u] << 8) >> 24), c2);
                c3 = __builtin_fmaf(vl[u].w * f, (float)((int)lo[u] >> 24), c3);
                c0 = __builtin_fmaf(vh[u].x * f, (float)((int)(hi[u] << 24) >> 24), c0);
                c1 = __builtin_fmaf(vh[u].y * f, (float)((int)(hi[u] << 16) >> 24), c1);
                c2 = __builtin_fmaf(vh[u].z * f, (float)((int)(hi[u] << 8) >> 24), c2);
                c3 = __builtin_fmaf(vh[u].w * f, (float)((int)hi[u] >> 24), c3);
            }
        }
    }
    // lane e: accumulator e >> 1, AVX lanes 4 (e & 1) + i in c_i.  acc1 + acc2 / acc3 + acc4: lanes e, e ^ 2 (e & 2 == 0 keeps it);
    // their sum: lanes e, e ^ 4;  sum[i] + sum[i + 4]: lanes e, e ^ 1
    float s0 = c0 + __shfl_xor(c0, 2), s1 = c1 + __shfl_xor(c1, 2), s2 = c2 + __shfl_xor(c2, 2), s3 = c3 + __shfl_xor(c3, 2);
    s0 = s0 + __shfl_xor(s0, 4);
    s1 = s1 + __shfl_xor(s1, 4);
    s2 = s2 + __shfl_xor(s2, 4);
    s3 = s3 + __shfl_xor(s3, 4);
    const float x0 = s0 + __shfl_xor(s0, 1), x1 = s1 + __shfl_xor(s1, 1), x2 = s2 + __shfl_xor(s2, 1), x3 = s3 + __shfl_xor(s3, 1);
    if (e == 0) m4f32_store(r, row, (x0 + x2) + (x1 + x3), fuse_u, fuse...);
}

// ================================================================================================
// transpose  (CloverMatrix8.h:1312-1386): values and the scale grid; exact by definition
// ================================================================================================
// Workgroup = one 128x128-byte tile (rows and cols are multiples of 128: no edge tiles).  Thread t reads 16 bytes of input rows
// (t >> 3) + 32 j (128 contiguous bytes per row), the tile goes through LDS (row stride 132 bytes: the byte gathers of one
// wave-instruction spread over the banks), and thread t writes 16 bytes of output rows (t >> 3) + 32 j.
#define TR8_T 128
#define TR8_STRIDE (TR8_T + 4)
template <bool NT>
__global__ __launch_bounds__(256) void k_m8_transpose(const uint8_t *__restrict__ q, const float *__restrict__ s, uint64_t rows, uint64_t cols,
                                                      uint8_t *__restrict__ qt, float *__restrict__ st, uint32_t tiles_x)
{
    __shared__ __attribute__((aligned(16))) uint8_t tl[TR8_T * TR8_STRIDE];
    const uint32_t bj = blockIdx.x % tiles_x;
    const uint64_t bi = blockIdx.x / tiles_x;
    const int tid = threadIdx.x, cq = tid & 7, rr = tid >> 3;
    const uint64_t r0 = bi * TR8_T, c0 = (uint64_t)bj * TR8_T;
    u32x4 in[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const u32x4 *src = reinterpret_cast<const u32x4 *>(q + (r0 + rr + 32 * j) * cols + c0 + 16 * cq);
        in[j] = NT ? __builtin_nontemporal_load(src) : *src;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        uint32_t *d = reinterpret_cast<uint32_t *>(tl + (rr + 32 * j) * TR8_STRIDE + 16 * cq);
        d[0] = in[j].x;
        d[1] = in[j].y;
        d[2] = in[j].z;
        d[3] = in[j].w;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int oc = rr + 32 * j;              // output row within the tile = input column
        uint32_t w[4];
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const uint8_t *src = tl + (16 * cq + 4 * d) * TR8_STRIDE + oc;
            w[d] = (uint32_t)src[0] | ((uint32_t)src[TR8_STRIDE] << 8) | ((uint32_t)src[2 * TR8_STRIDE] << 16) | ((uint32_t)src[3 * TR8_STRIDE] << 24);
        }
        const u32x4 o = {w[0], w[1], w[2], w[3]};
        u32x4 *dst = reinterpret_cast<u32x4 *>(qt + (c0 + oc) * rows + r0 + 16 * cq);
        if (NT) __builtin_nontemporal_store(o, dst);
        else *dst = o;
    }
    // this tile covers a 2x2 patch of the scale grid
    if (tid < 4) {
        const uint64_t ti = bi * 2 + (tid >> 1), tj = (uint64_t)bj * 2 + (tid & 1);
        st[tj * (rows / 64) + ti] = s[ti * (cols / 64) + tj];
    }
}

// ================================================================================================
// C ABI
// ================================================================================================
static int m8_check_shape(const char *fn, uint64_t rows, uint64_t cols)
{
    CLV_REQUIRE(rows % 128 == 0 && cols % 128 == 0, "%s: rows=%llu cols=%llu must be multiples of 128", fn, (unsigned long long)rows,
                (unsigned long long)cols);
    return CLV_OK;
}

extern "C" int clm8_quantize(const float *A, uint64_t rows, uint64_t cols, int8_t *q, float *s, uint64_t *rng_state_dev, void *stream)
{
    CLV_REQUIRE(A && q && s, "clm8_quantize: null pointer");
    int rc = m8_check_shape("clm8_quantize", rows, cols);
    if (rc) return rc;
    if (!rows || !cols) return CLV_OK;
    const uint64_t tiles = (rows / 64) * (cols / 64);
    CLV_REQUIRE(tiles <= 0x7FFFFFFFull && tiles * 128 < (1ull << 50), "clm8_quantize: too many tiles");
    hipStream_t st = as_stream(stream);
    RngTables T = {nullptr, nullptr, nullptr};
    if (rng_state_dev) {
        rc = clv_rng_tables(&T);
        if (rc) return rc;
        hipLaunchKernelGGL(k_m8_quantize<true>, dim3((unsigned)tiles), dim3(256), 0, st, (const f32x4 *)A, cols, (uint32_t)(cols / 64),
                           (uint32_t)(rows / 64), (uint32_t *)q, s, rng_state_dev, clv_rng_seq_for(rng_state_dev, st), T);
    } else {
        hipLaunchKernelGGL(k_m8_quantize<false>, dim3((unsigned)tiles), dim3(256), 0, st, (const f32x4 *)A, cols, (uint32_t)(cols / 64),
                           (uint32_t)(rows / 64), (uint32_t *)q, s, (uint64_t *)nullptr, 0ull, T);
    }
    CLV_LAUNCH_CHECK();
    return CLV_OK;
}

extern "C" int clm8_restore(const int8_t *q, const float *s, uint64_t rows, uint64_t cols, float *A, void *stream)
{
    CLV_REQUIRE(A && q && s, "clm8_restore: null pointer");
    int rc = m8_check_shape("clm8_restore", rows, cols);
    if (rc) return rc;
    if (!rows || !cols) return CLV_OK;
    const uint64_t nquads = rows * cols / 4, waves = (nquads + 255) / 256;
    CLV_REQUIRE((waves + 3) / 4 <= 0x7FFFFFFFull, "clm8_restore: matrix too large");
    if (rows * cols * sizeof(float) > (256ull << 20))
        hipLaunchKernelGGL(k_m8_restore<true>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, as_stream(stream), (const uint32_t *)q, s,
                           (f32x4 *)A, nquads, cols);
    else
        hipLaunchKernelGGL(k_m8_restore<false>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, as_stream(stream), (const uint32_t *)q, s,
                           (f32x4 *)A, nquads, cols);
    CLV_LAUNCH_CHECK();
    return CLV_OK;
}

int clv_internal_m8_check_mvm(const char *fn, const void *A, const void *sA, uint64_t rows, uint64_t cols, const void *x, const void *r)
{
    CLV_REQUIRE(A && sA && x && r, "%s: null pointer", fn);
    // a whole CloverMatrix8 has rows % 128 == 0; a multiple of 64 is a row shard of one (as for clm4_mvm)
    CLV_REQUIRE(rows % 64 == 0 && cols % 128 == 0, "%s: rows=%llu must be a multiple of 64 and cols=%llu of 128", fn,
                (unsigned long long)rows, (unsigned long long)cols);
    CLV_REQUIRE(rows / 32 <= 0x7FFFFFFFull && cols / 64 <= 0xFFFFFFFFull, "%s: matrix too large", fn);
    return CLV_OK;
}

extern "C" int clm8_mvm(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const int8_t *x, const float *sx, int8_t *r, float *sr,
                        uint64_t *rng_state_dev, void *stream)
{
    int rc = clv_internal_m8_check_mvm("clm8_mvm", A, sA, rows, cols, x, r);
    if (rc) return rc;
    CLV_REQUIRE(sx && sr, "clm8_mvm: null pointer");
    CLV_REQUIRE((const void *)r != (const void *)x, "clm8_mvm: the result must not alias the vector being multiplied");
    if (!rows) return CLV_OK;
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)(rows / 64)), block(256);
    // streaming loads once the matrix cannot stay in the 256 MiB Infinity Cache (the clm4_mvm rule)
    const bool streaming = rows * cols > (256ull << 20);
    if (rng_state_dev) {
        RngTables T;
        rc = clv_rng_tables(&T);
        if (rc) return rc;
        const uint64_t seq = clv_rng_seq_for(rng_state_dev, st);
        if (streaming)
            hipLaunchKernelGGL((k_m8_mvm<true, true>), grid, block, 0, st, (const uint8_t *)A, sA, cols, (const uint8_t *)x, sx, r, sr,
                               rng_state_dev, seq, T.pow_rows);
        else
            hipLaunchKernelGGL((k_m8_mvm<false, true>), grid, block, 0, st, (const uint8_t *)A, sA, cols, (const uint8_t *)x, sx, r, sr,
                               rng_state_dev, seq, T.pow_rows);
    } else {
        if (streaming)
            hipLaunchKernelGGL((k_m8_mvm<true, false>), grid, block, 0, st, (const uint8_t *)A, sA, cols, (const uint8_t *)x, sx, r, sr,
                               (uint64_t *)nullptr, 0ull, (const uint64_t *)nullptr);
        else
            hipLaunchKernelGGL((k_m8_mvm<false, false>), grid, block, 0, st, (const uint8_t *)A, sA, cols, (const uint8_t *)x, sx, r, sr,
                               (uint64_t *)nullptr, 0ull, (const uint64_t *)nullptr);
    }
    CLV_LAUNCH_CHECK();
    return CLV_OK;
}

#define M8_SAA "clm8_mvm_scale_and_add"
extern "C" int clm8_mvm_scale_and_add(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const int8_t *x, const float *sx,
                                      const int8_t *qu, const float *su, float a, int8_t *t, float *st_, int8_t *r, float *sr,
                                      uint64_t *rng_state_dev, void *stream)
{
    int rc = clv_internal_m8_check_mvm(M8_SAA, A, sA, rows, cols, x, r);
    if (rc) return rc;
    CLV_REQUIRE(sx && qu && su && sr, M8_SAA ": null pointer");
    CLV_REQUIRE((t == nullptr) == (st_ == nullptr), M8_SAA ": t and st must both be given or both be NULL");
    CLV_REQUIRE((const void *)r != (const void *)x && (const void *)sr != (const void *)sx && (!t || ((const void *)t != (const void *)x && st_ != sx)),
                M8_SAA ": the results must not alias the vector being multiplied");
    CLV_REQUIRE(!t || (r != t && sr != st_), M8_SAA ": r must not alias t");
    if (!rows) return CLV_OK;
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)(rows / 64)), block(256);
    const bool streaming = rows * cols > (256ull << 20);      // the clm8_mvm rule
    const M8Fuse fuse = {qu, su, a, r, sr};
    RngTables T = {nullptr, nullptr, nullptr};
    uint64_t seq = 0;
    if (rng_state_dev) {
        rc = clv_rng_tables(&T);
        if (rc) return rc;
        seq = clv_rng_seq_for(rng_state_dev, st);
    }
#define M8_SAA_LAUNCH(NT, ST)                                                                                                             \
    hipLaunchKernelGGL((k_m8_mvm_saa<NT, ST>), grid, block, 0, st, (const uint8_t *)A, sA, cols, (const uint8_t *)x, sx, t, st_, rng_state_dev, \
                       seq, T.pow_rows, fuse)
    if (streaming) {
        if (rng_state_dev) M8_SAA_LAUNCH(true, true); else M8_SAA_LAUNCH(true, false);
    } else {
        if (rng_state_dev) M8_SAA_LAUNCH(false, true); else M8_SAA_LAUNCH(false, false);
    }
#undef M8_SAA_LAUNCH
    CLV_LAUNCH_CHECK();
    return CLV_OK;
}
#undef M8_SAA

// Q_IHT / Q_GD (test/performance/01_measure.h:923-946, 999-1021) over a CloverMatrix8 with CloverVector8 vectors, the reference's pure
// 8-bit configuration (02_bit08.cpp).  One call enqueues all iterations: 3 launches per iteration (2 for GD), nothing copied back.
extern "C" int clm8_iht(const int8_t *Phi, const float *sPhi, const int8_t *PhiT, const float *sPhiT, uint64_t m, uint64_t n, int8_t *x,
                        float *sx, uint64_t x_len, const int8_t *y, const float *sy, int8_t *t1, float *st1, int8_t *t2, float *st2,
                        int8_t *t3, float *st3, uint64_t iterations, uint64_t K, float mu, int threshold, uint64_t *rng_state_dev,
                        void *stream)
{
    CLV_REQUIRE(Phi && sPhi && PhiT && sPhiT && x && sx && y && sy && t1 && st1 && t2 && st2 && t3 && st3, "clm8_iht: null pointer");
    CLV_REQUIRE(m % 128 == 0 && n % 128 == 0 && x_len <= n, "clm8_iht: m=%llu n=%llu x_len=%llu", (unsigned long long)m,
                (unsigned long long)n, (unsigned long long)x_len);
    int rc = clv_internal_v8_clear(x, sx, n, as_stream(stream));      // x.clear()
    for (uint64_t it = 0; !rc && it < iterations; it++) {
        rc = clm8_mvm_scale_and_add(Phi, sPhi, m, n, x, sx, y, sy, -1.0f, t1, st1, t2, st2, rng_state_dev, stream);              // t1 = Phi x; t2 = y - t1
        if (!rc) rc = clm8_mvm_scale_and_add(PhiT, sPhiT, n, m, t2, st2, x, sx, mu, t3, st3, x, sx, rng_state_dev, stream);      // t3 = Phi' t2; x += mu t3
        if (!rc && threshold)                                                                    // keep the K largest (2: the reference's survivor order)
            rc = clv8_threshold_mode(x, sx, x_len, n, K, threshold == 2 ? CLV_THRESHOLD_REFERENCE : CLV_THRESHOLD_FAST, nullptr, stream);
    }
    return rc;
}

// the launch of k_m8_mvm_f32 for checked arguments: 32 rows per workgroup, nontemporal under the rule of m8f32_streaming
template <typename... FUSE>
static int m8f32_launch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, float *r, hipStream_t st, FUSE... fuse)
{
    const dim3 grid((unsigned)(rows / 32)), block(256);
    if (m8f32_streaming(rows, cols))
        hipLaunchKernelGGL((k_m8_mvm_f32<true, FUSE...>), grid, block, 0, st, (const uint32_t *)A, sA, cols, (const f32x4 *)x, r, fuse...);
    else
        hipLaunchKernelGGL((k_m8_mvm_f32<false, FUSE...>), grid, block, 0, st, (const uint32_t *)A, sA, cols, (const f32x4 *)x, r, fuse...);
    CLV_LAUNCH_CHECK();
    return CLV_OK;
}

extern "C" int clm8_mvm_f32(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, float *r, void *stream)
{
    int rc = clv_internal_m8_check_mvm("clm8_mvm_f32", A, sA, rows, cols, x, r);
    if (rc) return rc;
    if (!rows) return CLV_OK;
    return m8f32_launch(A, sA, rows, cols, x, r, as_stream(stream));
}

// clm8_mvm_f32_scale_and_add (mvm_f32_host.h checks the arguments): the launch of clm8_mvm_f32 with the epilogue pack
int clv_internal_m8_mvm_f32_fused(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, float *t, const M4F32Fuse &fuse,
                                  hipStream_t st)
{
    return m8f32_launch(A, sA, rows, cols, x, t, st, fuse);
}

extern "C" int clm8_transpose(const int8_t *q, const float *s, uint64_t rows, uint64_t cols, int8_t *qt, float *st, void *stream)
{
    CLV_REQUIRE(q && s && qt && st, "clm8_transpose: null pointer");
    int rc = m8_check_shape("clm8_transpose", rows, cols);
    if (rc) return rc;
    CLV_REQUIRE(q != qt, "clm8_transpose: in-place transposition is not supported");
    if (!rows || !cols) return CLV_OK;
    const uint64_t tiles_x = cols / TR8_T, tiles = (rows / TR8_T) * tiles_x;
    CLV_REQUIRE(tiles <= 0x7FFFFFFFull, "clm8_transpose: too many tiles");
    // streaming loads and stores once input + output cannot live in the Infinity Cache (the clm4_transpose rule)
    if (rows * cols > (128ull << 20))
        hipLaunchKernelGGL(k_m8_transpose<true>, dim3((unsigned)tiles), dim3(256), 0, as_stream(stream), (const uint8_t *)q, s, rows, cols,
                           (uint8_t *)qt, st, (uint32_t)tiles_x);
    else
        hipLaunchKernelGGL(k_m8_transpose<false>, dim3((unsigned)tiles), dim3(256), 0, as_stream(stream), (const uint8_t *)q, s, rows, cols,
                           (uint8_t *)qt, st, (uint32_t)tiles_x);
    CLV_LAUNCH_CHECK();
    return CLV_OK;
}
