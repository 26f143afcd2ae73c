/*
 * clover_hip_m8_f32.h -- C ABI of libclover_hip.so for a CloverMatrix8 that works on fp32 vectors (CloverVector32 storage): the fused
 * mvm + scaleAndAdd step, r = A' x straight from A's own bytes (no stored transpose) with its fused form, and the IHT / GD loop of
 * <CloverMatrix8, CloverVector32> in one call, with two matrices or with one.
 *
 * A header of its own beside clover_hip.h, whose conventions hold unchanged: plain C99, every data pointer a DEVICE pointer, `stream` a
 * hipStream_t as void* (NULL = the default stream), every call only enqueues, returns CLV_OK or a negative CLV_ERR_* code with the text in
 * clv_last_error(), and checks its arguments before anything touches the device.  Vectors are plain fp32.  A matrix is a CloverMatrix8
 * image as clm8_mvm_f32 takes it: rows x cols bytes, row-major (cols bytes per row, -128 a legal byte), and the grid sA of
 * (rows / 64) x (cols / 64) tile scales, row-major.  The wording follows clover_hip_m4_f32.h, the same column for CloverMatrix4.
 *
 * Contract: bit for bit, no tolerance.
 *   clm8_mvm_f32_scale_and_add             = clm8_mvm_f32 (d, stored to t[row] when t is given) + clv_f32_scale_and_add:
 *                                            r2[row] = fma(d, a, u[row]), ONE fused multiply-add, subnormals kept;
 *   clm8_mvm_f32_transposed                = clm8_transpose(A -> At) + clm8_mvm_f32(At, cols, rows, x -> r).  Written out, output column c
 *                                            is 32 sequential fma chains, row i of A on chain i mod 32 in increasing i, each from +0.0f:
 *                                            acc = fma(f32(x[i] * f32(sA[i / 64][c / 64] / 127.0f)), (float)q(i, c), acc) -- the scale
 *                                            multiplies x, not q; then per l < 8
 *                                            s[l] = (acc[l] + acc[8 + l]) + (acc[16 + l] + acc[24 + l]), t[k] = s[k + 4] + s[k],
 *                                            r[c] = (t0 + t2) + (t1 + t3);
 *   clm8_mvm_f32_transposed_scale_and_add  = clm8_mvm_f32_scale_and_add on a stored At;
 *   clm8_iht_f32                           = the five calls of an iteration made one by one (below);
 *   clm8_iht_f32_one_matrix                = clm8_iht_f32 with PhiT = clm8_transpose(Phi): x, t1, t2 and t3.
 *
 * Arguments.  No required pointer is NULL (t of the fused calls may be).  A and x are 16-byte aligned, the other pointers 4-byte.  No
 * output overlaps the matrix, its scales, x or another output; the one exception is the in-place form r2 == u.  rows * cols <= 2^48.  A
 * violation returns CLV_ERR_INVALID, the message names the call and the argument, before any device work.  The calls take no workspace,
 * keep no state, allocate nothing and take no generator (this path has no stochastic rounding by definition); the three products capture
 * into a hipGraph, the loops where clm_f32_iht does.
 */
#ifndef CLOVER_HIP_M8_F32_H
#define CLOVER_HIP_M8_F32_H

#include "clover_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rows of x staged in LDS per pass of the transposed kernel (the tests take their two-chunk shape from it) */
#define CLM8_F32_T_CHUNK 8192

/* clm8_mvm_f32 immediately followed by clv_f32_scale_and_add on its result, one launch.  rows is a multiple of 64, cols of 128 (as
 * clm8_mvm_f32); x has cols values, u, t and r2 have rows.  t may be NULL (the product is not stored); r2 may be u. */
int  clm8_mvm_f32_scale_and_add(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x,
                                const float *u, float a, float *t /* NULL: t is not stored */, float *r2, void *stream);
/* r = A' x straight from A (rows x cols as stored): x has rows floats, r has cols floats.  rows and cols are multiples of 128;
 * rows == 0 or cols == 0 returns CLV_OK with checked arguments and does nothing. */
int  clm8_mvm_f32_transposed(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, float *r, void *stream);
/* the same epilogue on the transposed product: u, t and r2 have cols values. */
int  clm8_mvm_f32_transposed_scale_and_add(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x,
                                           const float *u, float a, float *t /* NULL: t is not stored */, float *r2, void *stream);
/* Q_IHT / Q_GD (test/performance/01_measure.h:923-946, 999-1021) on <CloverMatrix8, CloverVector32>; arguments as clm_f32_iht with 8-bit
 * matrices, Phi m x n and PhiT n x m: x.clear() over all n values (a kernel), then `iterations` times
 *   t1 = Phi x; t2 = y - t1; t3 = PhiT t2; x += mu t3; x.threshold(K) over the first x_len elements
 * (threshold: 0 = none, Q_GD; 1 = FAST; 2 = REFERENCE, through clv_f32_threshold_mode) -- one fused launch per product plus the
 * threshold: 3 launches per iteration with FAST while n <= 16384, 2 without threshold.  m and n are multiples of 128, x_len <= n; x and
 * t3 have n values, y, t1 and t2 have m; the six vectors are distinct buffers; the matrices, x and t2 are 16-byte aligned.
 * iterations == 0 clears x and touches nothing else.  Captures into a hipGraph whenever its threshold step needs no first-use
 * allocation: GD, and FAST with n <= 16384; REFERENCE and FAST beyond that take the stream's scratch (first call outside a capture). */
int  clm8_iht_f32(const int8_t *Phi, const float *sPhi, const int8_t *PhiT, const float *sPhiT, uint64_t m, uint64_t n,
                  float *x, uint64_t x_len, const float *y, float *t1, float *t2, float *t3,
                  uint64_t iterations, uint64_t K, float mu, int threshold, void *stream);
/* the same with ONE matrix: the gradient step is clm8_mvm_f32_transposed_scale_and_add on Phi. */
int  clm8_iht_f32_one_matrix(const int8_t *Phi, const float *sPhi, uint64_t m, uint64_t n,
                             float *x, uint64_t x_len, const float *y, float *t1, float *t2, float *t3,
                             uint64_t iterations, uint64_t K, float mu, int threshold, void *stream);

#ifdef __cplusplus
}
#endif

#endif
