/*
 * clover_hip_fp32.h -- C ABI of libclover_hip.so for the reference's 32-bit classes, CloverVector32 / CloverMatrix32: its comparison
 * baseline and the containers every caller's data starts in, on the device.
 *
 * A header of its own beside clover_hip.h, whose conventions hold unchanged: plain C99, every data pointer a DEVICE pointer, `stream` a
 * hipStream_t as void* (NULL = the default stream), sizes are the padded sizes of the containers (multiples of 128), `workspace` arguments
 * NULL or 16-byte aligned device memory of the bytes the size query returns, every call only enqueues, returns CLV_OK or a negative
 * CLV_ERR_* code with the text in clv_last_error(), and checks its arguments before anything touches the device.
 *
 * Storage: plain fp32 values, no scales.  Vector: n_pad values, the padding zero; matrix: rows x cols values, row-major.
 * Results are defined by the functions of include/clover_fp32.h (namespace clover_fp32) and equal them bit for bit, subnormal results
 * included (nothing is flushed); the one exception, clv_f32_dot in CLV_DOT_FAST mode, is spelled out there.
 */
#ifndef CLOVER_HIP_FP32_H
#define CLOVER_HIP_FP32_H

#include "clover_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* CloverVector32::scaleAndAdd, both overloads and _parallel (CloverVector32.h:291-323, the FMA branch; clover_fp32::axpy_fma):
 * r[i] = fma(v[i], a, u[i]), one fused fma per element.  u, v and r hold n_pad values and are 16-byte aligned; r may be u (the in-place
 * overload), not v.  None may be NULL. */
int  clv_f32_scale_and_add(const float *u, const float *v, float a, uint64_t n_pad, float *r, void *stream);
/* CloverVector32::dot (CloverVector32.h:406-451; clover_fp32::dot_chains32): 32 fma chains, element j in chain j mod 32, (a1 + a2) + (a3 + a4)
 * per lane, then _mm256_haddf32_ps (CloverBase.h:149-157).  CLV_DOT_EXACT: that order, bit for bit (n / 32 dependent fmas per chain:
 * latency-bound by definition, one workgroup).  CLV_DOT_FAST (dot_parallel): the same fused products in a fixed tree order, one launch,
 * memory-bound; the same bits on every call with the same inputs on the same device, and |d - exact| <= gamma_D sum |u_i v_i| with
 * gamma_k = k 2^-24 / (1 - k 2^-24) and D = ceil(n_pad / 1024 / grid) + 26, grid = min(ceil(n_pad / 1024), 4 x compute units, 2048)
 * workgroups.  FAST hands over through the stream's slots as clv4_dot does: first call on a stream outside a capture.
 * u and v are 16-byte aligned, out_dev (one float, device memory) 4-byte; none may be NULL.  Neither mode uses `workspace`: the query
 * returns 0, the argument may be NULL, a non-NULL one must still be 16-byte aligned.  n_pad == 0 stores +0. */
uint64_t clv_f32_dot_workspace_bytes(uint64_t n_pad);
int  clv_f32_dot(const float *u, const float *v, uint64_t n_pad, int mode, float *out_dev, void *workspace, void *stream);
/* CloverVector32::threshold / threshold_parallel (CloverVector32.h:549-600; clover_fp32::keep_top_k) on |x|: keep the k largest magnitudes
 * among the first n elements, the others of them become +0; elements n .. n_pad - 1 are left as they are.  The key is the bit pattern
 * x & 0x7FFFFFFF compared as an integer, i.e. |x| for every number.  CLV_THRESHOLD_REFERENCE keeps the reference's survivors index for
 * index (its heap walk), CLV_THRESHOLD_FAST the same multiset of magnitudes with the lowest indices among equal ones.
 * NaN: under FAST the key order puts every NaN pattern ABOVE infinity, so NaNs are kept first; the reference's walk compares with `>`,
 * which never admits a NaN after the first k elements -- inputs with NaNs are outside what the two modes agree on.
 * k >= n keeps everything (no device work), k == 0 clears the first n elements; n <= n_pad, n < 2^32.
 * FAST up to n_pad = 16384 is ONE launch of a one-workgroup kernel without workspace (a caller's workspace is validated and left
 * untouched); CLV_F32_THRESHOLD_SMALL=0 in the environment, read per call, keeps the large-vector path at every n -- same bits.
 * Workspace (NULL = the stream's scratch, allocated on first use: first call on a stream outside a capture):
 * clv_f32_threshold_workspace_bytes(n_pad) for FAST, clv_threshold_reference_workspace_bytes_k(n_pad, k) for REFERENCE; 16-byte
 * aligned, no initialisation.  x is 16-byte aligned and not NULL. */
uint64_t clv_f32_threshold_workspace_bytes(uint64_t n_pad);
int  clv_f32_threshold_mode(float *x, uint64_t n, uint64_t n_pad, uint64_t k, int mode, void *workspace, void *stream);
/* CloverMatrix32::mvm / mvm_parallel (CloverMatrix32.h:90-128; clover_fp32::mvm_rows): r[i] = the dot above (EXACT order) of row i of A
 * against x.  A is rows x cols row-major, x has cols values, r rows values; rows and cols are multiples of 128 (a row shard of a matrix
 * at a pointer offset is such a matrix).  A and x are 16-byte aligned, r 4-byte; r must not be x; none may be NULL.  All addressing is
 * 64-bit.  Bit-identical to the host loops (the reference itself hands this to sgemv, whose order is unspecified). */
int  clm_f32_mvm(const float *A, uint64_t rows, uint64_t cols, const float *x, float *r, void *stream);
/* clm_f32_mvm immediately followed by clv_f32_scale_and_add on its result, one launch -- the pair of steps the IHT / GD loops repeat
 * (test/performance/01_measure.h:940-943, 1016-1019).  Per row: d = the row value, stored to t[row] only if t is given (t may be NULL);
 * r2[row] = fma(d, a, u[row]).  Bit-identical to the two calls.  u, t and r2 have `rows` values and are 4-byte aligned; r2 may be u (the
 * in-place form x += a t); t and r2 must not alias x or each other, and t must not be u.  Sizes and the alignment of A and x as
 * clm_f32_mvm.  No workspace and no state: captures into a hipGraph. */
int  clm_f32_mvm_scale_and_add(const float *A, uint64_t rows, uint64_t cols, const float *x, const float *u, float a,
                               float *t, float *r2, void *stream);
/* CloverMatrix32::transpose / transpose_parallel (CloverMatrix32.h:169-179; clover_fp32::transpose): At(j, i) = A(i, j); A is rows x cols,
 * At is cols x rows (multiples of 4: a whole matrix has multiples of 128); both 16-byte aligned, not NULL, not in place.  Exact. */
int  clm_f32_transpose(const float *A, uint64_t rows, uint64_t cols, float *At, void *stream);
/* Q_IHT / Q_GD (test/performance/01_measure.h:923-946, 999-1021) on <CloverMatrix32, CloverVector32>, the baseline of the reference's
 * tables.  Arguments as clm_f16_iht with fp32 storage, Phi (m x n) and PhiT (n x m) row-major: x.clear() over all n elements (a kernel),
 * then `iterations` times
 *   t1 = Phi x; t2 = y - t1; t3 = PhiT t2; x += mu t3; x.threshold(K) over the first x_len elements
 * (threshold: 0 = none, Q_GD; 1 = FAST; 2 = REFERENCE) -- 3 launches per iteration with FAST while n <= 16384, 2 without threshold, all
 * on `stream`, nothing copied back, bit-identical to the method calls one by one.  m and n are multiples of 128, x_len <= n; x and t3
 * have n values, y, t1 and t2 have m; the six vectors are distinct buffers; the matrices, x and t2 are 16-byte aligned; none may be NULL.
 * iterations == 0 clears x and touches nothing else.  Captures into a hipGraph whenever its threshold step needs no first-use
 * allocation: GD, and FAST with n <= 16384; REFERENCE and FAST beyond that take the stream's scratch (first call outside a capture). */
int  clm_f32_iht(const float *Phi, const float *PhiT, uint64_t m, uint64_t n, float *x, uint64_t x_len,
                 const float *y, float *t1, float *t2, float *t3,
                 uint64_t iterations, uint64_t K, float mu, int threshold, void *stream);

#ifdef __cplusplus
}
#endif

#endif
