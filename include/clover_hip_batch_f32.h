/*
 * clover_hip_batch_f32.h -- C ABI of libclover_hip.so for the batched fp32-VECTOR mvm of the quantized matrices: r[j] = A x[j] for several
 * CloverVector32 with one CloverMatrix4 (clm4_) or one CloverMatrix8 (clm8_) in ONE pass over the matrix, the fused mvm + scaleAndAdd for
 * several vectors, and the two-matrix IHT / GD loop of <CloverMatrix4 / CloverMatrix8, CloverVector32> for several signals.
 *
 * A header of its own beside clover_hip.h, whose conventions hold unchanged: plain C99, every data pointer a DEVICE pointer, `stream` a
 * hipStream_t as void* (NULL = the default stream), every call only enqueues, returns CLV_OK or a negative CLV_ERR_* code with the text in
 * clv_last_error(), and checks its arguments before anything touches the device.  Pointer ARRAYS (x, u, t, r, ...) are HOST arrays of
 * nvec device pointers, read during the call, nothing kept.  Vectors are plain fp32; a matrix is the image clm4_mvm_f32 / clm8_mvm_f32
 * take, with the grid sA of (rows / 64) x (cols / 64) tile scales.
 *
 * Contract.  Each call is bit-identical to the sequence of single calls made for vector 0, then 1, and so on, on the same stream:
 * clm4_mvm_f32 / clm8_mvm_f32, their fused form and the two-matrix loop of clover_hip_m4_f32.h / clover_hip_m8_f32.h.  The identity includes t1 .. t3, subnormal
 * results and the single-rounding fma of the fused step.
 *
 * Sizes and groups.  rows is a multiple of 64 (a row shard), cols of 128, as for the single calls.  x[j] has `cols` values; r[j], u[j],
 * t[j] and r2[j] have `rows`.  A and every x[j] are 16-byte aligned, the other pointers 4-byte.  nvec == 0, rows == 0 or cols == 0 returns
 * CLV_OK with checked arguments and does nothing; nvec == 1 is the single call; groups of at most CLM4_MVM_BATCH_MAX vectors run one
 * matrix pass each, a remainder group of one vector is the single call.
 *
 * Dispatch.  CLV_MVM_BATCH=1 / 0 in the environment (read per call) forces every group of two or more to run batched / forwards every
 * group to the single calls; batched launches count in clv_mvm_batch_launches().  Unset, a group runs batched where the batched launch
 * was measured faster than the single calls by more than their spread ("Several fp32 vectors, one pass"): CloverMatrix4 --
 * groups of 8 over a matrix of 16 MiB or more, groups of 2 and of 4 over one of 2 GiB or more; CloverMatrix8 -- every group over a matrix
 * of 1 GiB or more.  The bits
 * are the same either way.
 *
 * Checks (CLV_ERR_INVALID, the message names the call and the vector index): no pointer array is NULL and no entry is NULL, except the
 * `t` array of the fused call and its entries; no output range overlaps any input range of any vector of the call, nor the matrix or
 * its scales; no two outputs overlap.  The one exception is the in-place form r2[j] == u[j].  Repeated INPUT pointers are allowed.
 *
 * The product calls take no workspace, keep no state, allocate nothing and capture into a hipGraph; the loop where the single loop does.
 */
#ifndef CLOVER_HIP_BATCH_F32_H
#define CLOVER_HIP_BATCH_F32_H

#include "clover_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* columns of every x[j] staged in LDS per pass of the batched kernel, both widths (the tests take their two-chunk shape from it) */
#define CLMQ_F32_BATCH_CHUNK 1024

/* r[j] = A x[j], j = 0 .. nvec - 1: clm4_mvm_f32 / clm8_mvm_f32 per vector, in order. */
int  clm4_mvm_f32_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec,
                        const float *const *x, float *const *r, void *stream);
int  clm8_mvm_f32_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec,
                        const float *const *x, float *const *r, void *stream);
/* d = A x[j]; t[j] = d where t and t[j] are given; r2[j] = fma(d, a, u[j]): the single fused call per vector, in order.
 * r2[j] may be u[j] (in place). */
int  clm4_mvm_f32_scale_and_add_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec,
                                      const float *const *x, const float *const *u, float a,
                                      float *const *t /* NULL or entries NULL: not stored */, float *const *r2, void *stream);
int  clm8_mvm_f32_scale_and_add_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec,
                                      const float *const *x, const float *const *u, float a,
                                      float *const *t /* NULL or entries NULL: not stored */, float *const *r2, void *stream);
/* Q_IHT / Q_GD for nvec signals with one Phi (m x n) and its stored transpose PhiT (n x m): the single loop per signal, in order.
 * Every x[j] is cleared; then per iteration and group t1 = Phi x, t2 = y - t1 and t3 = PhiT t2, x += mu t3 (the fused call above,
 * twice) and clv_f32_threshold_mode per vector on the first x_len elements (0 = none, 1 = FAST, 2 = REFERENCE).  m and n are
 * multiples of 128, x_len <= n; the matrices, x[j] and t2[j] are 16-byte aligned.  x[j] and t3[j] have n values, y[j], t1[j] and t2[j] m. */
int  clm4_iht_f32_batch(const int8_t *Phi, const float *sPhi, const int8_t *PhiT, const float *sPhiT, uint64_t m, uint64_t n,
                        uint64_t nvec, float *const *x, uint64_t x_len, const float *const *y,
                        float *const *t1, float *const *t2, float *const *t3,
                        uint64_t iterations, uint64_t K, float mu, int threshold, void *stream);
int  clm8_iht_f32_batch(const int8_t *Phi, const float *sPhi, const int8_t *PhiT, const float *sPhiT, uint64_t m, uint64_t n,
                        uint64_t nvec, float *const *x, uint64_t x_len, const float *const *y,
                        float *const *t1, float *const *t2, float *const *t3,
                        uint64_t iterations, uint64_t K, float mu, int threshold, void *stream);

#ifdef __cplusplus
}
#endif

#endif
