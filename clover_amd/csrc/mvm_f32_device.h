// mvm_f32_device.h -- what mvm_f32.hip (rows of A) and mvm_f32_t.hip (columns of A) share: the epilogue of the fused
// CloverMatrix4 x CloverVector32 step and the row-major fused launch; and the same for CloverMatrix8 (matrix8.hip, matrix8_f32_t.hip).
// The column walk of the two transposed kernels (mvm_f32_t_device.h) and the host driver of both widths (mvm_f32_host.h) include it.
#pragma once

#include "common.h"

// FUSED (clm4_mvm_f32_scale_and_add, clm4_mvm_f32_transposed_scale_and_add): the CloverVector32::scaleAndAdd that follows the mvm in the IHT / GD
// loops, done by the lane that stores the value: d = what clm4_mvm_f32 stores; t[i] = d when t is given; r2[i] = fma(d, a, u[i]) -- what the two
// separate calls compute.  u[i] is requested before the streaming loop, so r2 may be u.
struct M4F32Fuse {
    const float *u;
    float a;
    float *r2;
};

__device__ __forceinline__ float m4f32_fuse_load_u(uint64_t i) { return 0.0f; }
__device__ __forceinline__ float m4f32_fuse_load_u(uint64_t i, const M4F32Fuse &f) { return f.u[i]; }
// r: the plain result, or t of the fused call (may be NULL there)
__device__ __forceinline__ void m4f32_store(float *r, uint64_t i, float d, float) { r[i] = d; }
__device__ __forceinline__ void m4f32_store(float *r, uint64_t i, float d, float fuse_u, const M4F32Fuse &f)
{
    if (r) r[i] = d;
    f.r2[i] = __builtin_fmaf(d, f.a, fuse_u);
}

// streaming (nontemporal) matrix loads once the nibbles cannot live in the 256 MiB Infinity Cache: the rule of clm4_mvm_f32
static inline bool m4f32_streaming(uint64_t rows, uint64_t cols) { return rows * (cols / 2) > (256ull << 20); }

// mvm_f32.hip: k_m4_mvm_f32 with the fused epilogue; the arguments are checked by the caller (mvm_f32_host.h: one layer for the three products)
int clv_internal_m4_mvm_f32_fused(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, float *t, const M4F32Fuse &fuse,
                                  hipStream_t st);

// CloverMatrix8 x CloverVector32 (matrix8.hip: rows of A; matrix8_f32_t.hip: columns of A; include/clover_hip_m8_f32.h) takes the same
// epilogue pack: the step after the product does not depend on the width of the matrix.  Streaming under the clm8_mvm rule
static inline bool m8f32_streaming(uint64_t rows, uint64_t cols) { return rows * cols > (256ull << 20); }
// matrix8.hip: k_m8_mvm_f32 with the fused epilogue; the arguments are checked by the caller (mvm_f32_host.h)
int clv_internal_m8_mvm_f32_fused(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, float *t, const M4F32Fuse &fuse,
                                  hipStream_t st);
