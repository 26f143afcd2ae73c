// mvm8_device.h -- device helpers shared by the mvm kernels with CloverVector8 vectors: the mixed ones (4-bit matrix: k_m4_mvm8, mixed8.hip;
// k_m4_mvm8_batch, mvm_batch8.hip; k_m4_mvm8_t, mvm_t8.hip; k_m4_mvm8_t_batch, mvm_t8_batch.hip) and, for the factor, the noise maps, the tree and the re-quantisation, the
// CloverMatrix8 ones (k_m8_mvm, matrix8.hip; k_m8_mvm_t, matrix8_t.hip; k_m8_mvm_batch, matrix8_batch.hip; k_m8_mvm_t_batch, matrix8_t_batch.hip).  The bits of a result are fixed by this instruction sequence, so
// the kernels take it from here (as mvm_device.h does for the 4-bit pair).
#pragma once

#include "rng_device.h"

// the size rules of the mixed mvm family (mixed8.hip): rows % 64 == 0, cols % 128 == 0, no NULL among the four pointers
int check_mvm8_args(const char *fn, const void *A, const void *sA, uint64_t rows, uint64_t cols, const void *x, const void *sx);

// the argument checks of the transposed calls that take CloverVector8 vectors (mvm_t8.hip; clm4_mvm_v8_transposed* and clm8_mvm_transposed*),
// before any device work: a_bytes = the bytes of A's values (rows * cols / 2 for a CloverMatrix4, rows * cols for a CloverMatrix8).
// qu == NULL: the plain call.  > 0: nothing to do (an empty matrix)
int clv_internal_check_mvm8_t_args(const char *fn, const void *A, uint64_t a_bytes, const float *sA, uint64_t rows, uint64_t cols, const int8_t *x,
                                   const float *sx, bool fused, const int8_t *qu, const float *su, const int8_t *t, const float *st_, const int8_t *r,
                                   const float *sr);

// 8 nibbles of a dword (elements e0..e7) -> int8 dwords {e0..e3} and {e4..e7}, each value times 16
__device__ __forceinline__ void widen8(uint32_t w, uint32_t &d03, uint32_t &d47)
{
    const uint32_t lo = w & 0xF0F0F0F0u;                 // bytes [e0, e2, e4, e6] * 16
    const uint32_t hi = (w << 4) & 0xF0F0F0F0u;          // bytes [e1, e3, e5, e7] * 16
    d03 = __builtin_amdgcn_perm(hi, lo, 0x05010400u);    // [lo.b0, hi.b0, lo.b1, hi.b1]
    d47 = __builtin_amdgcn_perm(hi, lo, 0x07030602u);    // [lo.b2, hi.b2, lo.b3, hi.b3]
}

__device__ __forceinline__ int sdot4(uint32_t a, uint32_t b, int c) { return __builtin_amdgcn_sdot4((int)a, (int)b, c, false); }

// The matrix part of one block (64 columns) for lane m: word m and word 4+m of the block, widened.  It does not depend on x: the
// batched kernel computes it once per group of vectors.
struct Mvm8Words {
    uint32_t f03, f47, s03, s47;
};
__device__ __forceinline__ Mvm8Words mvm8_widen(uint32_t w_first, uint32_t w_second)
{
    Mvm8Words w;
    widen8(w_first, w.f03, w.f47);
    widen8(w_second, w.s03, w.s47);
    return w;
}

// The vector part: xb = the block's 64 int8 of x in LDS, c = the block factor f32(f32(sA*1/7) * f32(sx*1/127))
__device__ __forceinline__ void mvm8_dot(const Mvm8Words &w, const u32x2 *xb, int m, float c, float &a_even, float &a_odd)
{
    const u32x2 x0 = xb[m], x1 = xb[4 + m];          // elements 8m..8m+7 and 32+8m..32+8m+7
    const int ie = sdot4(w.s03, x1.x, sdot4(w.f03, x0.x, 0)) >> 4;      // chain 2m   (exact: the sum is a multiple of 16)
    const int io = sdot4(w.s47, x1.y, sdot4(w.f47, x0.y, 0)) >> 4;      // chain 2m+1
    a_even = __builtin_fmaf(c, (float)ie, a_even);
    a_odd = __builtin_fmaf(c, (float)io, a_odd);
}

// one block for lane m: w_first = word m, w_second = word 4+m of the block
__device__ __forceinline__ void mvm8_block(uint32_t w_first, uint32_t w_second, const u32x2 *xb, int m, float c, float &a_even, float &a_odd)
{
    mvm8_dot(mvm8_widen(w_first, w_second), xb, m, c, a_even, a_odd);
}

// the block factor of the chains (CloverMatrix4.h:1147-1149)
__device__ __forceinline__ float mvm8_factor(float sa, float sx) { return (sa * (1.0f / 7.0f)) * (sx * (1.0f / 127.0f)); }

// the block factor of the CloverMatrix8 chains (CloverMatrix8.h:1002-1299): k_m8_mvm (matrix8.hip) and k_m8_mvm_t (matrix8_t.hip)
__device__ __forceinline__ float m8_factor(float sa, float sx) { return (sa * (1.0f / 127.0f)) * (sx * (1.0f / 127.0f)); }

// chain 2m / 2m+1 in lane m of the row's quad.  CloverMatrix4.h:1229-1234: h[L] = a[L+4] + a[L]; (h0 + h2) + (h1 + h3); the row's dot
// product comes out in all four lanes
__device__ __forceinline__ float mvm8_tree(float a_even, float a_odd)
{
    const float he = a_even + __shfl_xor(a_even, 2), ho = a_odd + __shfl_xor(a_odd, 2);      // m = 0,2: h0, h1;  m = 1,3: h2, h3
    const float ge = he + __shfl_xor(he, 1), go = ho + __shfl_xor(ho, 1);                    // h0 + h2,  h1 + h3
    return ge + go;
}

// the same tree on the eight chain ends of a row held by ONE lane (k_m4_mvm8_t, mvm_t8.hip), same association
__device__ __forceinline__ float mvm8_tree8(const float (&a)[8])
{
    const float h0 = a[0] + a[4], h1 = a[1] + a[5], h2 = a[2] + a[6], h3 = a[3] + a[7];
    return (h0 + h2) + (h1 + h3);
}

// FUSE: the CloverVector8::scaleAndAdd that follows this mvm in the IHT / GD loops, done on the row group while it is still in
// the wave: r2 = quantize8(u + a * quantize8(A x)); its draws follow ALL the mvm draws in the stream, as in two separate calls.
struct Mvm8Fuse {
    const int8_t *qu;        // u, one 64-element block per row group
    const float *su;
    float a;
    int8_t *r2;              // may alias qu (the in-place overload)
    float *sr2;
};

// the vectors of one batched CloverMatrix4 x CloverVector8 pass (k_m4_mvm8_batch, mvm_batch8.hip; k_m4_mvm8_t_batch, mvm_t8_batch.hip), BY
// VALUE in the kernel arguments (see MvmBatchArgs, mvm_device.h).  Slots >= nv are absent: NULL, never dereferenced.
template <int NV>
struct Mvm8BatchArgs {
    const int8_t *x[NV];
    const float *sx[NV];
    int8_t *r[NV];           // all NULL: the mvm result is not stored (FUSE only)
    float *sr[NV];
};
template <int NV>
struct Mvm8BatchFuse {       // see Mvm8Fuse
    const int8_t *qu[NV];
    const float *su[NV];
    int8_t *r2[NV];          // may be qu (in place)
    float *sr2[NV];
    float a;
};

// the vectors of one batched CloverMatrix8 pass (k_m8_mvm_batch, matrix8_batch.hip; k_m8_mvm_t_batch, matrix8_t_batch.hip), BY VALUE in the
// kernel arguments (see MvmBatchArgs, mvm_device.h).  Slots >= nv are absent: NULL, never dereferenced.
template <int NV>
struct M8BatchArgs {
    const int8_t *x[NV];
    const float *sx[NV];
    int8_t *r[NV];           // all NULL: the mvm result is not stored (FUSE only)
    float *sr[NV];
};
template <int NV>
struct M8BatchFuse {         // see Mvm8Fuse
    const int8_t *qu[NV];
    const float *su[NV];
    int8_t *r2[NV];          // may be qu (in place)
    float *sr2[NV];
    float a;
};

// 64 row dots of a row group, one per lane of a FULL wave: re-quantise to 8 bits (CloverMatrix4.h:1246-1440) and, with FUSE,
// CloverVector8::scaleAndAdd on the block (CloverVector8.h:1089-1358).  r / sr (NULL: the mvm result is not stored) and r2 / sr2 point at
// the row group's block; noise, noise2 = this lane's noise of either step (0: rounding disabled); fuse_q / fuse_s = this lane's element
// of u and the block's scale, read BEFORE the call (r2 may be u).
template <bool FUSE>
__device__ __forceinline__ void mvm8_requantize_wave(float d, float noise, float noise2, int lane, int8_t *r, float *sr, int fuse_q, float fuse_s,
                                                     float a, int8_t *r2, float *sr2)
{
    float mx = wave_max(__builtin_fabsf(d));
    mx = fix_zero_max(mx);
    const int qv = quant1(d, 127.0f / mx, noise);
    if (r) {
        r[lane] = (int8_t)qv;
        if (lane == 0) *sr = mx;
    }
    if (FUSE) {
        const float val = __builtin_fmaf((float)qv, div127(mx * a), (float)fuse_q * div127(fuse_s));
        float m2 = wave_max(__builtin_fabsf(val));
        m2 = fix_zero_max(m2);
        r2[lane] = (int8_t)quant1(val, 127.0f / m2, noise2);
        if (lane == 0) *sr2 = m2;
    }
}

// The element <-> noise maps of a 64-element block re-quantised by one wave (CloverMatrix8.h:1140-1299, CloverVector8.h:1089-1358): raw =
// the block's two draws as gen_blocks leaves them (raw[4 draw + generator lane]), l = the element.  The mvm's re-quantisation takes draw
// l >> 5, word l & 7, byte (l >> 3) & 3; the scaleAndAdd behind it draw l >> 5, word (l & 31) >> 2, byte l & 3.
__device__ __forceinline__ float m8_mvm_noise(const uint64_t *raw, int l)
{
    return noise_of(reinterpret_cast<const uint32_t *>(raw + (size_t)(l >> 5) * 4)[l & 7], (l >> 3) & 3);
}
__device__ __forceinline__ float m8_saa_noise(const uint64_t *raw, int l)
{
    return noise_of(reinterpret_cast<const uint32_t *>(raw + (size_t)(l >> 5) * 4)[(l & 31) >> 2], l & 3);
}
