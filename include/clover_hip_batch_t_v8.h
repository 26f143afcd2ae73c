/*
 * clover_hip_batch_t_v8.h -- C ABI of libclover_hip.so for the batched TRANSPOSED mixed mvm: r[j] = quantize8(A' x[j]) for several
 * CloverVector8 with one CloverMatrix4, straight from A's own 4-bit bytes, and the mixed IHT / GD loop for several signals that holds
 * ONE matrix (the configuration the reference publishes as "4-bit", 02_bit04.cpp:140, without a stored transpose).
 *
 * A header of its own beside clover_hip.h, clover_hip_batch_t.h and clover_hip_batch_t8.h, whose conventions hold unchanged: plain C99,
 * every data pointer a DEVICE pointer, `stream` a hipStream_t as void* (NULL = the default stream), every call only enqueues, returns
 * CLV_OK or a negative CLV_ERR_* code with the text in clv_last_error(), and checks its arguments before anything touches the device.
 * Pointer ARRAYS (x, sx, r, ...) are HOST arrays of nvec device pointers, read during the call, nothing kept -- exactly as in the
 * clm4_*_v8_batch family of clover_hip.h.
 *
 * Contract.  Each call is bit-identical to the sequence of single calls made for vector 0, then 1, and so on, on the same stream:
 * clm4_mvm_v8_transposed, clm4_mvm_v8_transposed_scale_and_add and clm4_iht_v8_one_matrix.  The identity includes t1 .. t3 and, with an
 * rng, the XORShift state left behind.  Because the single calls are defined through the stored transpose, each call is also
 * bit-identical to clm4_mvm_v8_batch, clm4_mvm_v8_scale_and_add_batch or clm4_iht_v8_batch on clm4_transpose(A).
 *
 * Sizes and groups.  A is rows x cols nibbles (rows * cols / 2 bytes) with its (rows / 64) x (cols / 64) scale grid sA.  x[j] has `rows`
 * int8 elements and rows / 64 scales; r[j], qu[j] and t[j] have `cols` elements.  rows and cols are multiples of 128, rows / 64 and
 * cols / 64 <= 2^31 - 1.  nvec == 0 or an empty matrix returns CLV_OK and does nothing; nvec == 1 forwards to the single call; groups of
 * at most CLM4_MVM_BATCH_MAX vectors run one matrix pass each.
 *
 * Dispatch.  CLV_MVM_BATCH=1 / 0 in the environment forces / forbids the batched kernel, as for the other batched families; batched
 * launches count in clv_mvm_batch_launches().  With CLV_MVM_BATCH unset a group runs batched where the batched launch was measured
 * faster than the single calls by more than the spread of both; a deterministic group of one forwards to the single call.
 * The bits are the same either way.  The positioned call (clm4_mvm_v8_transposed_batch_at) with an rng always runs the batched kernel.
 *
 * Draws.  G = cols / 64 is the number of output blocks.  Within a vector's window output block cb takes draws 2 cb and 2 cb + 1; fused,
 * it also takes 2 G + 2 cb and 2 G + 2 cb + 1.  In the contiguous calls vector j's window follows vector j - 1's: a plain call draws 2 G
 * per vector, a fused call 4 G.
 *
 * Checks (CLV_ERR_INVALID, the message names the call and the vector index): no pointer array is NULL and no entry is NULL; t and st are
 * both given or both NULL; no output range overlaps any input range of any vector of the call, nor the matrix; no two outputs overlap.
 * The one exception is the in-place form r[j] == qu[j] with sr[j] == su[j].  Repeated INPUT pointers are allowed.
 *
 * Deterministic calls allocate nothing and capture into a hipGraph; stochastic calls capture under clv_rng_graph_mode, as
 * clm4_mvm_v8_batch does.
 */
#ifndef CLOVER_HIP_BATCH_T_V8_H
#define CLOVER_HIP_BATCH_T_V8_H

#include "clover_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* r[j] = quantize8(A' x[j]), j = 0 .. nvec - 1: clm4_mvm_v8_transposed per vector, in order. */
int  clm4_mvm_v8_transposed_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec,
                                  const int8_t *const *x, const float *const *sx, int8_t *const *r, float *const *sr,
                                  uint64_t *rng_state_dev, void *stream);
/* The same with the draws of vector j placed at draw_base + j * draw_stride draws behind the state the call finds, across the groups of
 * CLM4_MVM_BATCH_MAX too: vector j gets what clm4_mvm_v8_transposed gives from the state moved that far.  The state is advanced by
 * commit_draws; with commit_draws == 0 it is left untouched.  Every window (2 G draws) and commit_draws stay below 2^55.  With an rng the
 * batched kernel runs always, for nvec == 1 too; without one the call is clm4_mvm_v8_transposed_batch and the positions are unused. */
int  clm4_mvm_v8_transposed_batch_at(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec,
                                     const int8_t *const *x, const float *const *sx, int8_t *const *r, float *const *sr,
                                     uint64_t *rng_state_dev, uint64_t draw_base, uint64_t draw_stride, uint64_t commit_draws, void *stream);
/* t[j] = quantize8(A' x[j]); r[j] = quantize8(qu[j] + a * t[j]): clm4_mvm_v8_transposed_scale_and_add per vector, in order.  t / st may
 * both be NULL (the mvm result is not stored); r[j] may be qu[j] with sr[j] == su[j] (in place). */
int  clm4_mvm_v8_transposed_scale_and_add_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec,
                                                const int8_t *const *x, const float *const *sx, const int8_t *const *qu,
                                                const float *const *su, float a, int8_t *const *t, float *const *st,
                                                int8_t *const *r, float *const *sr, uint64_t *rng_state_dev, void *stream);
/* Q_IHT / Q_GD for nvec CloverVector8 signals with ONE CloverMatrix4 Phi (m x n): clm4_iht_v8_one_matrix per signal, in order -- the
 * arguments of clm4_iht_v8_batch without PhiT / sPhiT.  Per iteration and group: t1 = Phi x, t2 = y - t1
 * (clm4_mvm_v8_scale_and_add_batch); t3 = Phi' t2, x += mu t3 (the fused call above, from Phi's own bytes); the threshold
 * (clv8_threshold_batch; 0 = none, 1 = FAST, 2 = REFERENCE).  The draws lie where the single calls have them: one iteration of one
 * signal draws P = 4 (m / 64) + 4 (n / 64). */
int  clm4_iht_v8_batch_one_matrix(const int8_t *Phi, const float *sPhi, uint64_t m, uint64_t n, uint64_t nvec,
                                  int8_t *const *x, float *const *sx, uint64_t x_len, const int8_t *const *y, const float *const *sy,
                                  int8_t *const *t1, float *const *st1, int8_t *const *t2, float *const *st2,
                                  int8_t *const *t3, float *const *st3, uint64_t iterations, uint64_t K, float mu, int threshold,
                                  uint64_t *rng_state_dev, void *stream);

#ifdef __cplusplus
}
#endif

#endif
