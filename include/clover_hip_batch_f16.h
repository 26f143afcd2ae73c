/*
 * clover_hip_batch_f16.h -- C ABI of libclover_hip.so for the batched HALF-PRECISION mvm: r[j] = f16(A x[j]) for several CloverVector16
 * with one CloverMatrix16 in ONE pass over the matrix, the fused mvm + scaleAndAdd for several vectors, the threshold of several vectors
 * in one launch and the half-precision IHT / GD loop for several signals (the reference's 02_bit16 configuration).
 *
 * A header of its own beside clover_hip.h, whose conventions hold unchanged: plain C99, every data pointer a DEVICE pointer, `stream` a
 * hipStream_t as void* (NULL = the default stream), every call only enqueues, returns CLV_OK or a negative CLV_ERR_* code with the text in
 * clv_last_error(), and checks its arguments before anything touches the device.  Pointer ARRAYS (x, u, t, r, ...) are HOST arrays of
 * nvec device pointers, read during the call, nothing kept -- exactly as in the clm8_*_batch family of clover_hip.h.  Vectors are raw IEEE
 * binary16 bit patterns, no scales.
 *
 * Contract.  Each call is bit-identical to the sequence of single calls made for vector 0, then 1, and so on, on the same stream:
 * clm_f16_mvm, clm_f16_mvm_scale_and_add, clv_f16_threshold_mode and clm_f16_iht.  The identity includes t1 .. t3.  The 16-bit classes do
 * not round stochastically: there is no generator argument and no positioned (_at) form.
 *
 * Sizes and groups.  A is rows x cols binary16, row-major.  x[j] has `cols` elements; r[j], u[j] and t[j] have `rows`.  cols is a
 * multiple of 128; any row count is valid (a row shard of a matrix), rows / 16 <= 2^31 - 2.  The matrix and every x[j] are 16-byte
 * aligned; u[j], t[j] and r[j] 2-byte.  nvec == 0 or rows == 0 returns CLV_OK with checked arguments and does nothing; nvec == 1 is the
 * single call; groups of at most CLM4_MVM_BATCH_MAX vectors run one matrix pass each.
 *
 * Dispatch.  CLV_MVM_BATCH=1 / 0 in the environment (read per call) forces every group of a call of two or more vectors to run batched
 * (a remainder group of one vector too: ceil(nvec / 8) launches) / forwards every group to the single calls, as for the other batched
 * families; batched launches count in clv_mvm_batch_launches().  With CLV_MVM_BATCH unset a group runs batched where the batched
 * launch was measured faster than the single calls by more than their spread: groups of two or more over a matrix above
 * 256 MiB, groups of three or more over a smaller one.  The bits are the same either way.
 *
 * Checks (CLV_ERR_INVALID, the message names the call and the vector index): no pointer array is NULL and no entry is NULL, except the
 * whole `t` array of the fused call; r[j] != x[j] and t[j] != x[j]; t[j] is neither r[j] nor u[j]; no output range overlaps any input
 * range of any vector of the call, nor the matrix; no two outputs overlap.  The one exception is the in-place form r[j] == u[j].
 * Repeated INPUT pointers are allowed.
 *
 * The calls allocate nothing and capture into a hipGraph (clv_f16_threshold_batch in REFERENCE mode and beyond one workgroup's 32768
 * elements: as clv_f16_threshold_mode with a NULL workspace does).
 */
#ifndef CLOVER_HIP_BATCH_F16_H
#define CLOVER_HIP_BATCH_F16_H

#include "clover_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* r[j] = f16(A x[j]), j = 0 .. nvec - 1: clm_f16_mvm per vector, in order. */
int  clm_f16_mvm_batch(const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t nvec,
                       const uint16_t *const *x, uint16_t *const *r, void *stream);
/* t[j] = f16(A x[j]); r[j] = f16(fma(f32(t[j]), a, f32(u[j]))): clm_f16_mvm_scale_and_add per vector, in order.  t may be NULL (the mvm
 * result is not stored); r[j] may be u[j] (in place). */
int  clm_f16_mvm_scale_and_add_batch(const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t nvec,
                                     const uint16_t *const *x, const uint16_t *const *u, float a,
                                     uint16_t *const *t /* NULL: t is not stored */, uint16_t *const *r, void *stream);
/* CloverVector16::threshold(k) on nvec vectors of n elements (n_pad with padding, a multiple of 128): clv_f16_threshold_mode per vector,
 * in order.  CLV_THRESHOLD_FAST with n_pad <= 32768: one launch per 64 vectors, workgroup j on vector j; CLV_THRESHOLD_REFERENCE and
 * larger vectors: the single calls.  The h[j] do not overlap. */
int  clv_f16_threshold_batch(uint16_t *const *h, uint64_t nvec, uint64_t n, uint64_t n_pad, uint64_t k, int mode, void *stream);
/* Q_IHT / Q_GD for nvec signals with one Phi (m x n) and its stored transpose PhiT (n x m): clm_f16_iht per signal, in order.  Every x[j]
 * is cleared; then per iteration and group t1 = Phi x, t2 = y - t1 and t3 = PhiT t2, x += mu t3 (the fused call above, twice) and the
 * threshold on the first x_len elements (clv_f16_threshold_batch; 0 = none, 1 = FAST, 2 = REFERENCE).  m and n are multiples of 128,
 * x_len <= n; the matrices, x[j] and t2[j] are 16-byte aligned.  x[j] and t3[j] have n elements, y[j], t1[j] and t2[j] m. */
int  clm_f16_iht_batch(const uint16_t *Phi, const uint16_t *PhiT, uint64_t m, uint64_t n, uint64_t nvec,
                       uint16_t *const *x, uint64_t x_len, const uint16_t *const *y,
                       uint16_t *const *t1, uint16_t *const *t2, uint16_t *const *t3,
                       uint64_t iterations, uint64_t K, float mu, int threshold, void *stream);

#ifdef __cplusplus
}
#endif

#endif
