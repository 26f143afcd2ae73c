// mvm_t8_device.h -- the pieces the transposed mixed mvm kernels share: k_m4_mvm8_t (mvm_t8.hip) and k_m4_mvm8_t_batch (mvm_t8_batch.hip).
// Both read a CloverMatrix4's own bytes in dwords (8 columns of one row), transpose 8 x 8 nibbles in registers (nibble_transpose.h), widen
// the column words (widen8, mvm8_device.h) and form the exact block integer of a chain against x.  The integers are exact, so the two
// kernels may cut the 64 rows of a block differently; the fma chains that consume them are ordered in either.
#pragma once

#include "mvm8_device.h"
#include "nibble_transpose.h"

// a lane's NH * NR loads of one row block: rows i of the first half (and, NH = 2, rows 32 + i of the second), i < NR, counted from the row
// Ap points at
template <int NR, int NH, bool NT>
__device__ __forceinline__ void mvt8_load(const uint32_t *__restrict__ Ap, uint64_t stride, uint32_t (&a)[NH * NR])
{
#pragma unroll
    for (int i = 0; i < NH * NR; i++) {
        const uint32_t *p = Ap + (uint64_t)((i % NR) + 32 * (i / NR)) * stride;
        a[i] = NT ? __builtin_nontemporal_load(p) : *p;
    }
}

// the block integer of one chain of one column: f = the widened column bytes (times 16) of the chain's rows in the first half of the
// block, s = those of the second half, x0 / x1 = the 4 int8 of x of the same rows.  Exact: the sum is a multiple of 16
__device__ __forceinline__ int mvt8_int(uint32_t f, uint32_t x0, uint32_t s, uint32_t x1) { return sdot4(s, x1, sdot4(f, x0, 0)) >> 4; }
