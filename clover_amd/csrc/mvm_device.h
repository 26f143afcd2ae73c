// mvm_device.h -- device helpers shared by the 4-bit mvm kernels: k_m4_mvm64 (matrix4.hip) and k_m4_mvm_batch (mvm_batch4.hip).  The bits
// of an mvm result are fixed by this instruction sequence, so both kernels take it from here.
#pragma once

#include "common.h"

// the size rules of the 4-bit mvm family (matrix4.hip): rows % 64 == 0, cols % 128 == 0, no NULL among the four pointers
int check_mvm_args(const char *fn, const void *A, const void *sA, uint64_t rows, uint64_t cols, const void *x, const void *sx);

// the U matrix loads of one step: 16 B of this lane's row per block pair
template <int U, bool NT>
__device__ __forceinline__ void mvm_load(const u32x4 *__restrict__ Ap, int q, uint32_t t0, u32x4 (&a)[U])
{
#pragma unroll
    for (int u = 0; u < U; u++) a[u] = NT ? __builtin_nontemporal_load(&Ap[4 * (t0 + u) + q]) : Ap[4 * (t0 + u) + q];
}

// one link of a chain: the exact integer of a matrix word against its x word (v_dot8_i32_i4), its conversion and one fma with the block
// factor c.  mvm_consume below applies it to the four words of a lane; k_m4_mvm_t (mvm_t4.hip) to the eight column words of a piece.
__device__ __forceinline__ float mvm_chain_word(float c, uint32_t a, uint32_t x, float acc)
{
    return __builtin_fmaf(c, (float)sdot8(a, x, 0), acc);
}

// the chain arithmetic of one step on loaded matrix words: per word the exact integer (v_dot8_i32_i4), its conversion and one fma with
// the block factor c -- the order every mvm kernel of the 4-bit path has to keep
template <int U>
__device__ __forceinline__ void mvm_consume(const u32x4 (&a)[U], const u32x4 *xs, const float *cs, int q, uint32_t t0, float &a0, float &a1,
                                            float &a2, float &a3)
{
#pragma unroll
    for (int u = 0; u < U; u++) {
        const u32x4 xv = xs[4 * (t0 + u) + q];
        const float c = cs[2 * (t0 + u) + (q >> 1)];
        a0 = mvm_chain_word(c, a[u].x, xv.x, a0);
        a1 = mvm_chain_word(c, a[u].y, xv.y, a1);
        a2 = mvm_chain_word(c, a[u].z, xv.z, a2);
        a3 = mvm_chain_word(c, a[u].w, xv.w, a3);
    }
}

template <int U, bool NT>
__device__ __forceinline__ void mvm_steps(const u32x4 *__restrict__ Ap, const u32x4 *xs, const float *cs, int q,
                                          uint32_t t0, float &a0, float &a1, float &a2, float &a3)
{
    u32x4 a[U];
    mvm_load<U, NT>(Ap, q, t0, a);
    mvm_consume<U>(a, xs, cs, q, t0, a0, a1, a2, a3);
}

// chain (4q+i) of a row sits in lane quarter q: accumulator a = q>>1, AVX lane w = 4(q&1)+i.  Fixed tree of CloverBase.h:149-157; the
// row's dot product comes out in all four lanes of the row
__device__ __forceinline__ float mvm_tree(float a0, float a1, float a2, float a3)
{
    const float v0 = a0 + __shfl_xor(a0, 2);     // acc[0][w] + acc[1][w]
    const float v1 = a1 + __shfl_xor(a1, 2);
    const float v2 = a2 + __shfl_xor(a2, 2);
    const float v3 = a3 + __shfl_xor(a3, 2);
    const float x0 = v0 + __shfl_xor(v0, 1);     // v[i+4] + v[i]
    const float x1 = v1 + __shfl_xor(v1, 1);
    const float x2 = v2 + __shfl_xor(v2, 1);
    const float x3 = v3 + __shfl_xor(v3, 1);
    return (x0 + x2) + (x1 + x3);
}

// re-quantise 64 values held one per lane of a full wave (CloverMatrix4.h:919-1080); returns this lane's nibble value,
// *scale = the block maximum.  r_words / sr may be NULL (result not stored).
__device__ __forceinline__ int requantize_wave(float d, float noise, uint32_t *r_words, float *sr, float *scale)
{
    const int lane = threadIdx.x & 63;
    float m = wave_max(__builtin_fabsf(d));
    m = fix_zero_max(m);
    const float k = 7.0f / m;
    const int qv = quant1(d, k, noise);
    if (r_words) {
        uint32_t w = ((uint32_t)qv & 0xFu) << nib_shift(lane & 7);
        w |= __shfl_xor(w, 1);
        w |= __shfl_xor(w, 2);
        w |= __shfl_xor(w, 4);
        if ((lane & 7) == 0) r_words[lane >> 3] = w;
        if (lane == 0) *sr = m;
    }
    *scale = m;
    return qv;
}

// FUSE: the scaleAndAdd that follows mvm in the IHT / GD loops (t2 = y - Phi x;  x += mu Phi' t2), done on the row
// group while it is still in the wave:  r2 = quantize(u + a * quantize(A x))  (CloverVector4.h:1196-1478).
struct MvmFuse {
    const uint32_t *qu;      // u, one 64-element block per row group
    const float *su;
    float a;
    uint32_t *r2;            // may alias qu (the in-place overload)
    float *sr2;
};

// the vectors of one batched pass (k_m4_mvm_batch, k_m4_mvm_t_batch), BY VALUE in the kernel arguments: no pointer table in device memory,
// nothing to allocate, captures into a graph.  Slots >= nv are absent: NULL, never dereferenced.
template <int NV>
struct MvmBatchArgs {
    const uint8_t *x[NV];
    const float *sx[NV];
    uint32_t *r[NV];         // all NULL: the mvm result is not stored (FUSE only)
    float *sr[NV];
};
template <int NV>
struct MvmBatchFuse {        // see MvmFuse
    const uint32_t *qu[NV];
    const float *su[NV];
    uint32_t *r2[NV];        // may be qu (in place)
    float *sr2[NV];
    float a;
};

