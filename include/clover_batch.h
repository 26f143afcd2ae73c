/*
 * clover_batch.h -- what the batch methods of CloverMatrix4 and CloverMatrix8 do to carry a caller's vectors into the batched C calls,
 * written once: check the sizes, map the inputs read-only and then the outputs write-only (read-write for the in-place form), fill the
 * parallel arrays of value and scale pointers, call the family's entry point through clover_hip::check, commit the outputs.
 *
 * A family is a matrix class, a vector class and a direction (this * x[j] or this' * x[j]); BatchAbi names its four entry points.  The
 * four bodies of Batch<M, D> are what the public methods of the two classes call, one statement each.  Errors follow the convention of
 * clover_device.h: a message on stdout and exit(1).
 */
#ifndef CLOVER_BATCH_H
#define CLOVER_BATCH_H

#include <vector>

#include "clover_device.h"
#include "clover_hip_batch_t.h"    /* the batched transposed calls: headers of their own beside clover_hip.h */
#include "clover_hip_batch_t8.h"
#include "clover_hip_batch_t_v8.h"

class CloverMatrix4;
class CloverMatrix8;
class CloverVector4;
class CloverVector8;

namespace clover_hip {

enum BatchDirection { BATCH_FORWARD, BATCH_TRANSPOSED };

/* a matrix as the bodies take it: its device pointers (mapped read-only by the caller) and its padded shape */
struct BatchMatrix {
    const int8_t *q;
    const float *s;
    uint64_t rows, cols;
};
/* what the one-matrix loop passes for the stored transpose it does not have */
inline BatchMatrix no_transpose()
{
    const BatchMatrix none = {nullptr, nullptr, 0, 0};
    return none;
}

/* the device pointers of `count` vectors as the batch calls take them: values and scales.  The pointers of inputs are stored without
 * their const and handed on as const again (int8_t ** converts to const int8_t *const *) */
struct DevArrays {
    std::vector<int8_t *> q;
    std::vector<float *> s;
};
template <class V>
DevArrays dev_inputs(const V *const *v, uint64_t count)
{
    DevArrays a;
    for (uint64_t j = 0; j < count; j++) {
        a.q.push_back(const_cast<int8_t *>(v[j]->dev_values_ro()));
        a.s.push_back(const_cast<float *>(v[j]->dev_scales_ro()));
    }
    return a;
}
template <class V>
DevArrays dev_outputs(V *const *v, uint64_t count, bool read_too)
{
    DevArrays a;
    for (uint64_t j = 0; j < count; j++) {
        a.q.push_back(read_too ? v[j]->dev_values_rw() : v[j]->dev_values_wo());
        a.s.push_back(read_too ? v[j]->dev_scales_rw() : v[j]->dev_scales_wo());
    }
    return a;
}

/* The entry points of a family: plain, positioned, fused and the loop.  The six families share the signatures of the first three; the
 * loop of a forward family takes the stored transpose, the loop of a transposed one (the one-matrix loop) does not.  Each entry point is
 * returned from a function, not stored in a member: a client that never calls a method then never references its symbol. */
typedef decltype(&clm4_mvm_batch) batch_mvm_fn;
typedef decltype(&clm4_mvm_batch_at) batch_mvm_at_fn;
typedef decltype(&clm4_mvm_scale_and_add_batch) batch_fused_fn;
typedef decltype(&clm4_iht_batch) batch_loop_fn;
typedef decltype(&clm4_iht_batch_one_matrix) batch_loop_one_matrix_fn;

template <class M, class V, BatchDirection D> struct BatchAbi;
template <> struct BatchAbi<CloverMatrix4, CloverVector4, BATCH_FORWARD> {
    static batch_mvm_fn mvm() { return clm4_mvm_batch; }
    static batch_mvm_at_fn mvm_at() { return clm4_mvm_batch_at; }
    static batch_fused_fn fused() { return clm4_mvm_scale_and_add_batch; }
    static batch_loop_fn loop() { return clm4_iht_batch; }
};
template <> struct BatchAbi<CloverMatrix4, CloverVector4, BATCH_TRANSPOSED> {
    static batch_mvm_fn mvm() { return clm4_mvm_transposed_batch; }
    static batch_mvm_at_fn mvm_at() { return clm4_mvm_transposed_batch_at; }
    static batch_fused_fn fused() { return clm4_mvm_transposed_scale_and_add_batch; }
    static batch_loop_one_matrix_fn loop() { return clm4_iht_batch_one_matrix; }
};
template <> struct BatchAbi<CloverMatrix4, CloverVector8, BATCH_FORWARD> {
    static batch_mvm_fn mvm() { return clm4_mvm_v8_batch; }
    static batch_mvm_at_fn mvm_at() { return clm4_mvm_v8_batch_at; }
    static batch_fused_fn fused() { return clm4_mvm_v8_scale_and_add_batch; }
    static batch_loop_fn loop() { return clm4_iht_v8_batch; }
};
template <> struct BatchAbi<CloverMatrix4, CloverVector8, BATCH_TRANSPOSED> {
    static batch_mvm_fn mvm() { return clm4_mvm_v8_transposed_batch; }
    static batch_mvm_at_fn mvm_at() { return clm4_mvm_v8_transposed_batch_at; }
    static batch_fused_fn fused() { return clm4_mvm_v8_transposed_scale_and_add_batch; }
    static batch_loop_one_matrix_fn loop() { return clm4_iht_v8_batch_one_matrix; }
};
template <> struct BatchAbi<CloverMatrix8, CloverVector8, BATCH_FORWARD> {
    static batch_mvm_fn mvm() { return clm8_mvm_batch; }
    static batch_mvm_at_fn mvm_at() { return clm8_mvm_batch_at; }
    static batch_fused_fn fused() { return clm8_mvm_scale_and_add_batch; }
    static batch_loop_fn loop() { return clm8_iht_batch; }
};
template <> struct BatchAbi<CloverMatrix8, CloverVector8, BATCH_TRANSPOSED> {
    static batch_mvm_fn mvm() { return clm8_mvm_transposed_batch; }
    static batch_mvm_at_fn mvm_at() { return clm8_mvm_transposed_batch_at; }
    static batch_fused_fn fused() { return clm8_mvm_transposed_scale_and_add_batch; }
    static batch_loop_one_matrix_fn loop() { return clm8_iht_batch_one_matrix; }
};

inline void batch_exit(const char *message)
{
    std::cout << message << std::endl;
    exit(1);
}

/* The size rules of the fused forms for `count` vectors, vector by vector in the order of the single methods: x has x_len elements, t, u
 * and r have r_len.  r == NULL: the in-place form, or a caller that leaves r to scaleAndAdd. */
template <class V>
void batch_check_fused(uint64_t x_len, uint64_t r_len, const V *const *x, const V *const *u, V *const *t, V *const *r, uint64_t count)
{
    for (uint64_t j = 0; j < count; j++) {
        if (x[j]->size() != x_len || t[j]->size_pad() != r_len) batch_exit("MVM can not be performed. Exiting ...");
        if (u[j]->size_pad() != r_len || (r && r[j]->size_pad() != r_len)) batch_exit("Vectors do not have the same size. Exiting ...");
    }
}

/* the loop call of either shape: the forward families' takes the stored transpose, the one-matrix loop has none to take */
template <class... Rest>
int batch_loop_call(batch_loop_fn loop, const BatchMatrix &A, const BatchMatrix &AT, Rest... rest)
{
    return loop(A.q, A.s, AT.q, AT.s, A.rows, A.cols, rest...);
}
template <class... Rest>
int batch_loop_call(batch_loop_one_matrix_fn loop, const BatchMatrix &A, const BatchMatrix &, Rest... rest)
{
    return loop(A.q, A.s, A.rows, A.cols, rest...);
}

/* The bodies of the batch methods of matrix class M in direction D, for either vector class V.  `what` names the method to
 * clover_hip::check. */
template <class M, BatchDirection D>
struct Batch {
    /* which dimension sizes x and which the result: r = A x has `rows` elements and x `cols`, r = A' x the other way round */
    static uint64_t x_len(const BatchMatrix &A) { return D == BATCH_FORWARD ? A.cols : A.rows; }
    static uint64_t r_len(const BatchMatrix &A) { return D == BATCH_FORWARD ? A.rows : A.cols; }

    /* r[j] = A x[j] (A' x[j]).  positioned: the place of every vector's draws is the caller's; else the launcher may forward groups to
     * the single calls where those were measured faster, and the three numbers are unused */
    template <class V>
    static void mvm(const BatchMatrix &A, const V *const *x, V *const *r, uint64_t count, uint64_t *rng, bool positioned, uint64_t draw_base,
                    uint64_t draw_stride, uint64_t commit_draws, const char *what)
    {
        for (uint64_t j = 0; j < count; j++)
            if (x[j]->size() != x_len(A) || r[j]->size_pad() != r_len(A)) batch_exit("MVM can not be performed. Exiting ...");
        const DevArrays px = dev_inputs(x, count), pr = dev_outputs(r, count, false);
        if (positioned)
            check(BatchAbi<M, V, D>::mvm_at()(A.q, A.s, A.rows, A.cols, count, px.q.data(), px.s.data(), pr.q.data(), pr.s.data(), rng, draw_base,
                                              draw_stride, commit_draws, nullptr), what);
        else
            check(BatchAbi<M, V, D>::mvm()(A.q, A.s, A.rows, A.cols, count, px.q.data(), px.s.data(), pr.q.data(), pr.s.data(), rng, nullptr), what);
        for (uint64_t j = 0; j < count; j++) r[j]->commit();
    }

    /* t[j] = A x[j] (A' x[j]), r[j] = quantize(u[j] + a * t[j]): rounding disabled only */
    template <class V>
    static void fused(const BatchMatrix &A, const V *const *x, const V *const *u, float a, V *const *t, V *const *r, uint64_t count, const char *what)
    {
        batch_check_fused<V>(x_len(A), r_len(A), x, u, t, r, count);
        const DevArrays px = dev_inputs(x, count), pu = dev_inputs(u, count), pt = dev_outputs(t, count, false), pr = dev_outputs(r, count, false);
        check(BatchAbi<M, V, D>::fused()(A.q, A.s, A.rows, A.cols, count, px.q.data(), px.s.data(), pu.q.data(), pu.s.data(), a, pt.q.data(),
                                         pt.s.data(), pr.q.data(), pr.s.data(), nullptr, nullptr), what);
        for (uint64_t j = 0; j < count; j++) { t[j]->commit(); r[j]->commit(); }
    }

    /* in place: u[j] = quantize(u[j] + a * t[j]); u[j] is mapped read-write and is both the call's qu / su and its r / sr */
    template <class V>
    static void fused_in_place(const BatchMatrix &A, const V *const *x, V *const *u, float a, V *const *t, uint64_t count, const char *what)
    {
        batch_check_fused<V>(x_len(A), r_len(A), x, u, t, nullptr, count);
        const DevArrays px = dev_inputs(x, count), pu = dev_outputs(u, count, true), pt = dev_outputs(t, count, false);
        check(BatchAbi<M, V, D>::fused()(A.q, A.s, A.rows, A.cols, count, px.q.data(), px.s.data(), pu.q.data(), pu.s.data(), a, pt.q.data(),
                                         pt.s.data(), pu.q.data(), pu.s.data(), nullptr, nullptr), what);
        for (uint64_t j = 0; j < count; j++) { t[j]->commit(); u[j]->commit(); }
    }

    /* The IHT / GD loop for `count` signals with A as Phi.  AT: the stored transpose of a forward family; no_transpose() in the one-matrix
     * loop, which is the loop of a transposed family (step 2 reads A's own bytes).  x and t3 have `cols` elements, y, t1 and t2 `rows`, in
     * either.  Rounding disabled only. */
    template <class V>
    static void iht_loop(const BatchMatrix &A, const BatchMatrix &AT, V *const *x, const V *const *y, V *const *t1, V *const *t2, V *const *t3,
                         uint64_t count, uint64_t iterations, uint64_t K, float mu, bool with_threshold, const char *what)
    {
        for (uint64_t j = 0; j < count; j++)
            if ((D == BATCH_FORWARD && (AT.rows != A.cols || AT.cols != A.rows)) || x[j]->size_pad() != A.cols || y[j]->size_pad() != A.rows ||
                t1[j]->size_pad() != A.rows || t2[j]->size_pad() != A.rows || t3[j]->size_pad() != A.cols || x[j]->size() != x[0]->size())
                batch_exit("MVM can not be performed. Exiting ...");
        const DevArrays py = dev_inputs(y, count), px = dev_outputs(x, count, false), p1 = dev_outputs(t1, count, false),
                        p2 = dev_outputs(t2, count, false), p3 = dev_outputs(t3, count, false);
        const int thr = !with_threshold ? 0 : (threshold_mode() == CLV_THRESHOLD_FAST ? 1 : 2);
        check(batch_loop_call(BatchAbi<M, V, D>::loop(), A, AT, count, px.q.data(), px.s.data(), count ? x[0]->size() : 0, py.q.data(),
                              py.s.data(), p1.q.data(), p1.s.data(), p2.q.data(), p2.s.data(), p3.q.data(), p3.s.data(), iterations, K, mu, thr,
                              (uint64_t *)nullptr, (void *)nullptr), what);
        for (uint64_t j = 0; j < count; j++) {
            x[j]->commit();
            if (iterations) { t1[j]->commit(); t2[j]->commit(); t3[j]->commit(); }
        }
    }
};

}      /* namespace clover_hip */

#endif
