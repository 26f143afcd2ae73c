/* fake_clv_batch.c -- host-memory stand-ins for the 24 batched entry points of the C ABI (and the scaleAndAdd calls the stochastic build
 * of the classes issues behind them), so that the marshalling of include/clover_batch.h -- which pointer of which vector lands in which
 * slot of which call -- can be recorded without a GPU (tests/cpp/batch_marshal_trace.cpp, linked with tests/cpp/fake_clv.c for the calls of
 * clover_hip::Mirror).  TEST DOUBLE ONLY: every call prints its name and every scalar argument, then "plays the kernel": into the first
 * value and the first scale of every output it writes a number computed from the first value and scale of that vector's inputs, each input
 * slot with a weight of its own, so that a swapped slot, a swapped index or a wrong matrix changes what the host reads afterwards.  No
 * address is printed. */
#include <stdio.h>

#include "clover_hip.h"
#include "clover_hip_batch_t.h"
#include "clover_hip_batch_t8.h"
#include "clover_hip_batch_t_v8.h"

typedef unsigned long long ull;

static int8_t q8(int v) { return (int8_t)(unsigned char)(v & 0xFF); }
static const char *null_or_set(const void *p) { return p ? "set" : "NULL"; }

static int fake_mvm(const char *fn, const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                    const float *const *sx, int8_t *const *r, float *const *sr, uint64_t *rng, const uint64_t *draws, void *stream)
{
    printf("%s rows=%llu cols=%llu nvec=%llu", fn, (ull)rows, (ull)cols, (ull)nvec);
    if (draws) printf(" draw_base=%llu draw_stride=%llu commit_draws=%llu", (ull)draws[0], (ull)draws[1], (ull)draws[2]);
    printf(" rng=%s stream=%s\n", null_or_set(rng), null_or_set(stream));
    for (uint64_t j = 0; j < nvec; j++) {
        const int8_t v = q8(3 * A[0] + 5 * x[j][0] + 1);
        const float s = sA[0] + 2.0f * sx[j][0] + 0.25f;
        r[j][0] = v;
        sr[j][0] = s;
    }
    return CLV_OK;
}

static int fake_fused(const char *fn, const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                      const float *const *sx, const int8_t *const *qu, const float *const *su, float a, int8_t *const *t, float *const *st,
                      int8_t *const *r, float *const *sr, uint64_t *rng, void *stream)
{
    printf("%s rows=%llu cols=%llu nvec=%llu a=%.4f t=%s rng=%s stream=%s\n", fn, (ull)rows, (ull)cols, (ull)nvec, a, null_or_set(t),
           null_or_set(rng), null_or_set(stream));
    for (uint64_t j = 0; j < nvec; j++) {
        printf("  vector %llu: r==qu %d sr==su %d\n", (ull)j, (int)((const void *)r[j] == (const void *)qu[j]),
               (int)((const void *)sr[j] == (const void *)su[j]));
        const int8_t tv = q8(3 * A[0] + 5 * x[j][0] + 1), rv = q8(7 * A[0] + 11 * x[j][0] + 13 * qu[j][0] + 2);
        const float ts = sA[0] + 2.0f * sx[j][0] + 0.25f, rs = 0.5f * sA[0] + 3.0f * sx[j][0] + 5.0f * su[j][0] + a;
        if (t) {
            t[j][0] = tv;
            st[j][0] = ts;
        }
        r[j][0] = rv;
        sr[j][0] = rs;
    }
    return CLV_OK;
}

/* PhiT == NULL: the one-matrix loop */
static int fake_iht(const char *fn, const int8_t *Phi, const float *sPhi, const int8_t *PhiT, const float *sPhiT, uint64_t m, uint64_t n,
                    uint64_t nvec, int8_t *const *x, float *const *sx, uint64_t x_len, const int8_t *const *y, const float *const *sy,
                    int8_t *const *t1, float *const *st1, int8_t *const *t2, float *const *st2, int8_t *const *t3, float *const *st3,
                    uint64_t iterations, uint64_t K, float mu, int threshold, uint64_t *rng, void *stream)
{
    printf("%s rows=%llu cols=%llu nvec=%llu x_len=%llu iterations=%llu K=%llu mu=%.4f threshold=%d rng=%s stream=%s\n", fn, (ull)m, (ull)n,
           (ull)nvec, (ull)x_len, (ull)iterations, (ull)K, mu, threshold, null_or_set(rng), null_or_set(stream));
    for (uint64_t j = 0; j < nvec; j++) {
        const int xv = 17 * Phi[0] + (PhiT ? 19 * PhiT[0] : 0) + 23 * y[j][0] + 3;
        const float xs = sPhi[0] + (PhiT ? 2.0f * sPhiT[0] : 0.0f) + 3.0f * sy[j][0] + 0.5f;
        x[j][0] = q8(xv);
        sx[j][0] = xs;
        t1[j][0] = q8(xv + 29);
        st1[j][0] = xs + 1.0f;
        t2[j][0] = q8(xv + 58);
        st2[j][0] = xs + 2.0f;
        t3[j][0] = q8(xv + 87);
        st3[j][0] = xs + 3.0f;
    }
    return CLV_OK;
}

/* the six families: plain, positioned, fused, and the loop -- with the stored transpose in the forward families, without in the others */
#define FAKE_MVM_CALLS(prefix)                                                                                                          \
    int prefix##_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,           \
                       const float *const *sx, int8_t *const *r, float *const *sr, uint64_t *rng, void *stream)                         \
    {                                                                                                                                   \
        return fake_mvm(#prefix "_batch", A, sA, rows, cols, nvec, x, sx, r, sr, rng, NULL, stream);                                    \
    }                                                                                                                                   \
    int prefix##_batch_at(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,        \
                          const float *const *sx, int8_t *const *r, float *const *sr, uint64_t *rng, uint64_t draw_base,                \
                          uint64_t draw_stride, uint64_t commit_draws, void *stream)                                                    \
    {                                                                                                                                   \
        const uint64_t draws[3] = {draw_base, draw_stride, commit_draws};                                                               \
        return fake_mvm(#prefix "_batch_at", A, sA, rows, cols, nvec, x, sx, r, sr, rng, draws, stream);                                \
    }                                                                                                                                   \
    int prefix##_scale_and_add_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec,                     \
                                     const int8_t *const *x, const float *const *sx, const int8_t *const *qu, const float *const *su,   \
                                     float a, int8_t *const *t, float *const *st, int8_t *const *r, float *const *sr, uint64_t *rng,    \
                                     void *stream)                                                                                      \
    {                                                                                                                                   \
        return fake_fused(#prefix "_scale_and_add_batch", A, sA, rows, cols, nvec, x, sx, qu, su, a, t, st, r, sr, rng, stream);        \
    }
#define FAKE_IHT_CALLS(name)                                                                                                            \
    int name(const int8_t *Phi, const float *sPhi, const int8_t *PhiT, const float *sPhiT, uint64_t m, uint64_t n, uint64_t nvec,       \
             int8_t *const *x, float *const *sx, uint64_t x_len, const int8_t *const *y, const float *const *sy, int8_t *const *t1,     \
             float *const *st1, int8_t *const *t2, float *const *st2, int8_t *const *t3, float *const *st3, uint64_t iterations,        \
             uint64_t K, float mu, int threshold, uint64_t *rng, void *stream)                                                          \
    {                                                                                                                                   \
        return fake_iht(#name, Phi, sPhi, PhiT, sPhiT, m, n, nvec, x, sx, x_len, y, sy, t1, st1, t2, st2, t3, st3, iterations, K, mu,   \
                        threshold, rng, stream);                                                                                        \
    }                                                                                                                                   \
    int name##_one_matrix(const int8_t *Phi, const float *sPhi, uint64_t m, uint64_t n, uint64_t nvec, int8_t *const *x,                \
                          float *const *sx, uint64_t x_len, const int8_t *const *y, const float *const *sy, int8_t *const *t1,          \
                          float *const *st1, int8_t *const *t2, float *const *st2, int8_t *const *t3, float *const *st3,                \
                          uint64_t iterations, uint64_t K, float mu, int threshold, uint64_t *rng, void *stream)                        \
    {                                                                                                                                   \
        return fake_iht(#name "_one_matrix", Phi, sPhi, NULL, NULL, m, n, nvec, x, sx, x_len, y, sy, t1, st1, t2, st2, t3, st3,         \
                        iterations, K, mu, threshold, rng, stream);                                                                     \
    }

FAKE_MVM_CALLS(clm4_mvm)
FAKE_MVM_CALLS(clm4_mvm_transposed)
FAKE_IHT_CALLS(clm4_iht_batch)
FAKE_MVM_CALLS(clm4_mvm_v8)
FAKE_MVM_CALLS(clm4_mvm_v8_transposed)
FAKE_IHT_CALLS(clm4_iht_v8_batch)
FAKE_MVM_CALLS(clm8_mvm)
FAKE_MVM_CALLS(clm8_mvm_transposed)
FAKE_IHT_CALLS(clm8_iht_batch)

/* ~CloverMatrix4 names it; no test matrix holds a cached GEMM operand */
int clm4_gemm_release(clm4_gemm_operand *op) { (void)op; return CLV_OK; }

/* what the stochastic build of the fused batch methods issues per vector behind its one mvm batch call */
static int fake_scale_and_add(const char *fn, const int8_t *qu, const float *su, const int8_t *qv, const float *sv, float a, uint64_t n_pad,
                              int8_t *r, float *sr, uint64_t *rng, void *stream)
{
    printf("%s n_pad=%llu a=%.4f r==qu %d sr==su %d rng=%s stream=%s\n", fn, (ull)n_pad, a, (int)((const void *)r == (const void *)qu),
           (int)((const void *)sr == (const void *)su), null_or_set(rng), null_or_set(stream));
    const int8_t v = q8(31 * qu[0] + 37 * qv[0] + 5);
    const float s = su[0] + 2.0f * sv[0] + a;
    r[0] = v;
    sr[0] = s;
    return CLV_OK;
}
int clv4_scale_and_add(const int8_t *qu, const float *su, const int8_t *qv, const float *sv, float a, uint64_t n_pad, int8_t *r, float *sr,
                       uint64_t *rng, void *stream)
{
    return fake_scale_and_add("clv4_scale_and_add", qu, su, qv, sv, a, n_pad, r, sr, rng, stream);
}
int clv8_scale_and_add(const int8_t *qu, const float *su, const int8_t *qv, const float *sv, float a, uint64_t n_pad, int8_t *r, float *sr,
                       uint64_t *rng, void *stream)
{
    return fake_scale_and_add("clv8_scale_and_add", qu, su, qv, sv, a, n_pad, r, sr, rng, stream);
}
