/*
 * clover_hip_batch_f16_t.h -- C ABI of libclover_hip.so for the batched TRANSPOSED HALF-PRECISION mvm: r[j] = f16(A' x[j]) for several
 * CloverVector16 with one CloverMatrix16 in ONE pass over A's own bytes (no stored transpose), its fused mvm + scaleAndAdd form and the
 * half-precision IHT / GD loop for several signals that holds ONE matrix.
 *
 * A header of its own beside clover_hip.h, whose conventions hold unchanged, as in clover_hip_batch_f16.h and clover_hip_f16_t.h: plain
 * C99, every data pointer a DEVICE pointer, `stream` a hipStream_t as void* (NULL = the default stream), every call only enqueues, returns
 * CLV_OK or a negative CLV_ERR_* code with the text in clv_last_error(), and checks every argument before anything touches the device.
 * Pointer ARRAYS (x, u, t, r, ...) are HOST arrays of nvec device pointers, read during the call, nothing kept.  Vectors and the matrix
 * are raw IEEE binary16 bit patterns, no scales.  The calls allocate nothing, keep no state and take no workspace.
 *
 * Contract.  Each call is bit-identical to the single calls of clover_hip_f16_t.h made for vector 0, then 1, and so on, on the same
 * stream (clm_f16_mvm_transposed, clm_f16_mvm_transposed_scale_and_add, clm_f16_iht_one_matrix; t1 .. t3 included), and through those to
 * clm_f16_mvm_batch / clm_f16_mvm_scale_and_add_batch / clm_f16_iht_batch of clover_hip_batch_f16.h on clm_f16_transpose(A).  Written
 * out, output column c of vector j is 32 sequential fp32 chains, row i on chain i mod 32 in increasing i, each from +0.0f, one step
 * acc = fmaf(f32(x[j][i]), f32(A[i][c]), acc); then s[l] = (acc[l] + acc[8 + l]) + (acc[16 + l] + acc[24 + l]), t[k] = s[k + 4] + s[k],
 * d = (t0 + t2) + (t1 + t3).  The 16-bit classes do not round stochastically: there is no generator argument and no positioned (_at)
 * form.  The fp32-vector product (clm_f16_mvm_f32_transposed) has no batch call, as its row-major counterpart has none.
 *
 * Sizes and groups.  A is rows x cols binary16, row-major.  x[j] has `rows` elements; r[j], u[j] and t[j] have `cols`.  rows and cols
 * are multiples of 128 and within the limits of the single transposed call.  The matrix and every x[j] are 16-byte aligned; u[j], t[j]
 * and r[j] 2-byte.  nvec == 0, rows == 0 or cols == 0 returns CLV_OK with checked arguments and does nothing; nvec == 1 is the single
 * call; groups of at most CLM4_MVM_BATCH_MAX vectors run one matrix pass each.
 *
 * Dispatch.  CLV_MVM_BATCH=1 / 0 in the environment (read per call) forces every group of a call of two or more vectors to run batched
 * (a remainder group of one vector too: ceil(nvec / 8) launches) / forwards every group to the single transposed calls; batched launches
 * count in clv_mvm_batch_launches().  With CLV_MVM_BATCH unset a group runs batched where the batched launch was measured faster than
 * the single calls by more than their spread: every group of two or more, over a matrix above 256 MiB and over a smaller
 * one alike.  The bits are the same either way.
 *
 * Checks (CLV_ERR_INVALID, the message names the call and the vector index): no pointer array is NULL and no entry is NULL, except the
 * whole `t` array of the fused call; r[j] != x[j] and t[j] != x[j]; t[j] is neither r[j] nor u[j]; no output range overlaps any input
 * range of any vector of the call, nor the matrix; no two outputs overlap.  The one exception is the in-place form r[j] == u[j].
 * Repeated INPUT pointers are allowed.
 *
 * The two products capture into a hipGraph; the loop where clm_f16_iht_batch does (Q_GD, and the FAST threshold up to n = 32768).
 */
#ifndef CLOVER_HIP_BATCH_F16_T_H
#define CLOVER_HIP_BATCH_F16_T_H

#include "clover_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* r[j] = f16(A' x[j]), j = 0 .. nvec - 1: clm_f16_mvm_transposed per vector, in order. */
int  clm_f16_mvm_transposed_batch(const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t nvec,
                                  const uint16_t *const *x, uint16_t *const *r, void *stream);
/* t[j] = f16(A' x[j]); r[j] = f16(fma(f32(t[j]), a, f32(u[j]))): clm_f16_mvm_transposed_scale_and_add per vector, in order.  t may be
 * NULL (the product is not stored); r[j] may be u[j] (in place). */
int  clm_f16_mvm_transposed_scale_and_add_batch(const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t nvec,
                                                const uint16_t *const *x, const uint16_t *const *u, float a,
                                                uint16_t *const *t /* NULL: t is not stored */, uint16_t *const *r, void *stream);
/* clm_f16_iht_batch without PhiT: Q_IHT / Q_GD for nvec signals with ONE matrix Phi (m x n), clm_f16_iht_one_matrix per signal, in
 * order.  Every x[j] is cleared; then per iteration and group t1 = Phi x, t2 = y - t1 (one batched fused launch on Phi), t3 = Phi' t2,
 * x += mu t3 (one batched transposed fused launch on the same Phi) and the threshold on the first x_len elements
 * (clv_f16_threshold_batch; 0 = none, 1 = FAST, 2 = REFERENCE).  m and n are multiples of 128, x_len <= n; Phi, x[j] and t2[j] are
 * 16-byte aligned.  x[j] and t3[j] have n elements, y[j], t1[j] and t2[j] m. */
int  clm_f16_iht_batch_one_matrix(const uint16_t *Phi, uint64_t m, uint64_t n, uint64_t nvec,
                                  uint16_t *const *x, uint64_t x_len, const uint16_t *const *y,
                                  uint16_t *const *t1, uint16_t *const *t2, uint16_t *const *t3,
                                  uint64_t iterations, uint64_t K, float mu, int threshold, void *stream);

#ifdef __cplusplus
}
#endif

#endif
