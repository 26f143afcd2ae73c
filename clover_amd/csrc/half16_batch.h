// half16_batch.h -- what the one-matrix half-precision loop (clm_f16_iht_batch_one_matrix, half16_t_batch.hip) needs of the batched
// row-major family: the vectors of a call and the launch of one group.  The kernel and the launches are in half16_batch.hip; the loop runs
// step 1 (t1 = Phi x, t2 = y - t1) on them and step 2 on the transposed kernel of its own file.
#pragma once

#include "half16_device.h"

// the vectors of a call (host arrays of device pointers).  u == NULL: the plain mvm, r[j] = f16(A x[j]).  Else the fused form: t[j] =
// f16(A x[j]) (t == NULL: not stored), r[j] = f16(fma(f32(t[j]), a, f32(u[j])))
struct F16BatchVectors {
    const uint16_t *const *x;
    const uint16_t *const *u;
    float a;
    uint16_t *const *t;
    uint16_t *const *r;
    F16BatchVectors from(uint64_t j0) const { return {x + j0, u ? u + j0 : nullptr, a, t ? t + j0 : nullptr, r + j0}; }
};

// one batched launch (counted) of k_f16_mvm_batch for the first g <= CLM4_MVM_BATCH_MAX vectors of v, on the smallest instantiation that
// holds them; the arguments have been checked
int f16_batch_launch_group(const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t g, const F16BatchVectors &v, hipStream_t st);
