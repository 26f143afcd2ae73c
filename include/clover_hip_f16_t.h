/*
 * clover_hip_f16_t.h -- C ABI of libclover_hip.so for the TRANSPOSED HALF-PRECISION mvm: r = f16(A' x) for a CloverMatrix16 A and a
 * CloverVector16 (or fp32) x straight from A's own bytes, no stored transpose, its fused mvm + scaleAndAdd form and the half-precision
 * IHT / GD loop that holds ONE matrix.
 *
 * A header of its own beside clover_hip.h, whose conventions hold unchanged: plain C99, every data pointer a DEVICE pointer, `stream` a
 * hipStream_t as void* (NULL = the default stream), every call only enqueues, returns CLV_OK or a negative CLV_ERR_* code with the text in
 * clv_last_error(), and checks its arguments before anything touches the device.  Vectors and the matrix are raw IEEE binary16 bit
 * patterns, no scales.
 *
 * Contract.  A is rows x cols, row-major.  x has `rows` elements; r, u and t have `cols`.  Each call gives, bit for bit, what
 * clm_f16_transpose(A -> At) followed by the call of clover_hip.h on At (cols x rows) gives: clm_f16_mvm, clm_f16_mvm_f32,
 * clm_f16_mvm_scale_and_add, clm_f16_iht.  Written out, output column j is 32 sequential fp32 chains, row i on chain i mod 32 in
 * increasing i, each from +0.0f, one step acc = fmaf(f32(x[i]), f32(A[i][j]), acc); then s[l] = (acc[l] + acc[8 + l]) + (acc[16 + l] +
 * acc[24 + l]), t[k] = s[k + 4] + s[k], d = (t0 + t2) + (t1 + t3).
 *
 * Arguments.  rows and cols are multiples of 128; rows == 0 or cols == 0 returns CLV_OK with checked arguments and does nothing.  No
 * required pointer is NULL.  A and x are 16-byte aligned, the other pointers need their element alignment.  No output overlaps A or x or
 * another output; the one exception is the in-place form r == u.  A violation returns CLV_ERR_INVALID (the message names the call) before
 * any device work.  The calls take no workspace, keep no state and allocate nothing; the three products capture into a hipGraph, the loop
 * where clm_f16_iht does (Q_GD, and the FAST threshold up to n = 32768).
 */
#ifndef CLOVER_HIP_F16_T_H
#define CLOVER_HIP_F16_T_H

#include "clover_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* r = f16(A' x): the bits of clm_f16_transpose + clm_f16_mvm. */
int  clm_f16_mvm_transposed(const uint16_t *A, uint64_t rows, uint64_t cols, const uint16_t *x, uint16_t *r, void *stream);
/* r = A' x with an fp32 vector in and out: the bits of clm_f16_transpose + clm_f16_mvm_f32. */
int  clm_f16_mvm_f32_transposed(const uint16_t *A, uint64_t rows, uint64_t cols, const float *x, float *r, void *stream);
/* t = f16(A' x); r[j] = f16(fma(f32(t[j]), a, f32(u[j]))), from the ROUNDED t widened again: the bits of clm_f16_transpose +
 * clm_f16_mvm_scale_and_add.  t may be NULL (the product is not stored); r may be u (in place). */
int  clm_f16_mvm_transposed_scale_and_add(const uint16_t *A, uint64_t rows, uint64_t cols, const uint16_t *x, const uint16_t *u, float a,
                                          uint16_t *t /* NULL: t is not stored */, uint16_t *r, void *stream);
/* clm_f16_iht with ONE matrix: Phi' t2 comes straight from Phi (m x n).  x is cleared; then per iteration t1 = Phi x, t2 = y - t1
 * (clm_f16_mvm_scale_and_add), t3 = Phi' t2, x += mu t3 (the fused call above) and the threshold on the first x_len elements (0 = none,
 * 1 = FAST, 2 = REFERENCE): three launches per iteration, two without a threshold.  x, t1, t2, t3 end as clm_f16_iht with
 * PhiT = transpose(Phi) leaves them.  x and t3 have n elements, y, t1 and t2 m; Phi, x and t2 are 16-byte aligned. */
int  clm_f16_iht_one_matrix(const uint16_t *Phi, uint64_t m, uint64_t n, uint16_t *x, uint64_t x_len, const uint16_t *y,
                            uint16_t *t1, uint16_t *t2, uint16_t *t3, uint64_t iterations, uint64_t K, float mu, int threshold, void *stream);

#ifdef __cplusplus
}
#endif

#endif
