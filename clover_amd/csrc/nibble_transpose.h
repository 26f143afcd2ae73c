// nibble_transpose.h -- the 8 x 8 nibble transpose in registers, shared by k_m4_transpose (transpose4.hip) and k_m4_mvm_t (mvm_t4.hip): the
// words the second multiplies by are, bit for bit, the words the first would have stored.
#pragma once

#include "common.h"

// 8 x 8 nibble transpose: W[r] = the word of input row r (element e at nib_shift(e): EVEN elements in the high nibble of their byte),
// O[e] = the word of output row e.  In "position" space (position p = bits 4p .. 4p + 3, element e sits at position e ^ 1) this is the
// plain matrix transpose of the rows taken in the order r ^ 1, read out in the order e ^ 1: the two permutations are register renaming.
__device__ __forceinline__ void transpose8x8_nibbles(const uint32_t W[8], uint32_t O[8])
{
    uint32_t R[8];
#pragma unroll
    for (int r = 0; r < 8; r++) R[r] = W[r ^ 1];
#pragma unroll
    for (int i = 0; i < 8; i += 2) {                                       // nibbles: (row 2i, position 2j + 1) <-> (row 2i + 1, position 2j)
        const uint32_t a = R[i], b = R[i + 1];
        R[i] = (a & 0x0F0F0F0Fu) | ((b << 4) & 0xF0F0F0F0u);               // v_lshlrev + v_bfi
        R[i + 1] = (b & 0xF0F0F0F0u) | ((a >> 4) & 0x0F0F0F0Fu);
    }
#pragma unroll
    for (int r = 0; r < 8; r++)
        if ((r & 2) == 0) {                                                // bytes: rows r, r + 2
            const uint32_t a = R[r], b = R[r + 2];
            R[r] = __builtin_amdgcn_perm(b, a, 0x06020400u);               // [a.b0, b.b0, a.b2, b.b2]
            R[r + 2] = __builtin_amdgcn_perm(b, a, 0x07030501u);           // [a.b1, b.b1, a.b3, b.b3]
        }
#pragma unroll
    for (int r = 0; r < 4; r++) {                                          // halfwords: rows r, r + 4
        const uint32_t a = R[r], b = R[r + 4];
        R[r] = __builtin_amdgcn_perm(b, a, 0x05040100u);                   // [a.lo, b.lo]
        R[r + 4] = __builtin_amdgcn_perm(b, a, 0x07060302u);               // [a.hi, b.hi]
    }
#pragma unroll
    for (int e = 0; e < 8; e++) O[e] = R[e ^ 1];
}
