// matrix8_t_device.h -- the pieces of the transposed 8-bit mvm that its two kernels share: k_m8_mvm_t (matrix8_t.hip, one vector) and
// k_m8_mvm_t_batch (matrix8_t_batch.hip, up to CLM4_MVM_BATCH_MAX vectors).  The lane map, the loads and the chain link are the same
// instruction sequence in both, which is what makes the batched results equal the single calls bit for bit.
#pragma once

#include "mvm8_device.h"

// 4 x 4 bytes: d[i] = row i, byte k = column k  ->  c[k] = column k, byte i = row i
__device__ __forceinline__ void m8t_transpose4x4(const uint32_t *d, uint32_t (&c)[4])
{
    const uint32_t l01 = __builtin_amdgcn_perm(d[1], d[0], 0x05010400u), h01 = __builtin_amdgcn_perm(d[1], d[0], 0x07030602u);   // [d0.b0 d1.b0 d0.b1 d1.b1], [.. b2 .. b3]
    const uint32_t l23 = __builtin_amdgcn_perm(d[3], d[2], 0x05010400u), h23 = __builtin_amdgcn_perm(d[3], d[2], 0x07030602u);
    c[0] = __builtin_amdgcn_perm(l23, l01, 0x05040100u);
    c[1] = __builtin_amdgcn_perm(l23, l01, 0x07060302u);
    c[2] = __builtin_amdgcn_perm(h23, h01, 0x05040100u);
    c[3] = __builtin_amdgcn_perm(h23, h01, 0x07060302u);
}

// this thread's 8 loads of each of the U blocks of group g (beyond the last block: the last block again).  Aq: the thread's column quad in
// row 4 L of block 0
template <int U, bool NT>
__device__ __forceinline__ void m8t_load(const uint32_t *__restrict__ Aq, uint64_t stride, uint32_t g, uint32_t nblk, uint32_t (&a)[U][8])
{
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint32_t blk = g * U + u < nblk ? g * U + u : nblk - 1;
        const uint32_t *p0 = Aq + (uint64_t)blk * 64 * stride;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const uint32_t *p = p0 + (uint64_t)((i & 3) + 32 * (i >> 2)) * stride;
            a[u][i] = NT ? __builtin_nontemporal_load(p) : *p;
        }
    }
}

// the chain link of one block for the thread's 4 columns: lo / hi = the two transposed 4 x 4 pieces, xl / xh = x of rows 4 L .. 4 L + 3
// and 32 + 4 L .. 32 + 4 L + 3, c = the block factor
__device__ __forceinline__ void m8t_link(const uint32_t (&lo)[4], const uint32_t (&hi)[4], uint32_t xl, uint32_t xh, float c, float (&acc)[4])
{
#pragma unroll
    for (int k = 0; k < 4; k++) acc[k] = __builtin_fmaf(c, (float)sdot4(hi[k], xh, sdot4(lo[k], xl, 0)), acc[k]);
}
