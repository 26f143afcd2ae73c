/*
 * CloverIHT.h -- the two application loops that call the 4-bit hot path in the reference:
 * quantized Iterative Hard Thresholding and quantized Gradient Descent
 * (test/performance/01_measure.h:923-946 and :999-1021).
 *
 * Same function names, argument order and step sequence as the reference's templates.  With the containers
 * of this directory every step is a kernel on the device mirrors and nothing is copied back between steps:
 * Phi, PhiT, x, y and the temporaries stay in HBM for the whole loop (the reference re-streams them from
 * DRAM through the caches every iteration).
 */
#ifndef CLOVER_IHT_H
#define CLOVER_IHT_H

#include "CloverMatrix4.h"
#include "CloverMatrix8.h"       /* Q_IHT<CloverMatrix8, CloverVector8> / Q_GD<...>: the specialisations at the end */
#include "CloverMatrix16.h"      /* Q_IHT<CloverMatrix16, CloverVector16> / Q_GD<...>: the specialisations at the end */
#include "CloverVector4.h"

/* Generic forms, for any container pair with the reference's method names (the five steps of 01_measure.h:930-944):
 * residual r = y - Phi x, gradient g = Phi' r, step x += mu g, then (IHT only) keep the K largest entries. */
template <class QMatrix, class QVector>
inline void Q_IHT(QMatrix &Phi, QMatrix &PhiT, QVector &x, QVector &y, QVector &t1, QVector &t2, QVector &t3,
                  const uint64_t iterations, const uint64_t K, const float mu)
{
    x.clear();
    for (uint64_t it = 0; it < iterations; ++it) {
        Phi.mvm_parallel(x, t1);
        y.scaleAndAdd_parallel(t1, -1.0f, t2);
        PhiT.mvm_parallel(t2, t3);
        x.scaleAndAdd_parallel(t3, mu);
        x.threshold_parallel(K);
    }
}

template <class QMatrix, class QVector>
inline void Q_GD(QMatrix &Phi, QMatrix &PhiT, QVector &x, QVector &y, QVector &t1, QVector &t2, QVector &t3,
                 const uint64_t iterations, const float mu)
{
    x.clear();
    for (uint64_t it = 0; it < iterations; ++it) {
        Phi.mvm_parallel(x, t1);
        y.scaleAndAdd_parallel(t1, -1.0f, t2);
        PhiT.mvm_parallel(t2, t3);
        x.scaleAndAdd_parallel(t3, mu);
    }
}


/* The 4-bit containers of this directory run the whole loop in ONE call when rounding is deterministic (CloverMatrix4::iht_loop ->
 * clm4_iht: a persistent launch with Phi and PhiT resident in LDS for the sizes the reference publishes, 9 us per iteration at
 * N = 8192), and otherwise pair every scaleAndAdd with the mvm before it (CloverMatrix4::mvm_scaleAndAdd: one launch instead of two);
 * identical results either way, so the same calls -- Q_IHT(Phi, PhiT, x, y, t1, t2, t3, ...) -- pick these overloads. */
inline void Q_IHT(CloverMatrix4 &Phi, CloverMatrix4 &PhiT, CloverVector4 &x, CloverVector4 &y, CloverVector4 &t1, CloverVector4 &t2,
                  CloverVector4 &t3, const uint64_t iterations, const uint64_t K, const float mu)
{
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
    Phi.iht_loop(PhiT, x, y, t1, t2, t3, iterations, K, mu, true);
    return;
#endif
    x.clear();
    for (uint64_t i = 0; i < iterations; i += 1) {
        Phi.mvm_scaleAndAdd(x, y, -1.0f, t1, t2);      /* residual:  t1 = Phi x,  t2 = y - t1   (one launch) */
        PhiT.mvm_scaleAndAdd(t2, x, mu, t3);           /* gradient step:  t3 = Phi' t2,  x += mu t3   (one launch) */
        x.threshold_parallel(K);                       /* keep the K largest magnitudes */
    }
}

inline void Q_GD(CloverMatrix4 &Phi, CloverMatrix4 &PhiT, CloverVector4 &x, CloverVector4 &y, CloverVector4 &t1, CloverVector4 &t2,
                 CloverVector4 &t3, const uint64_t iterations, const float mu)
{
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
    Phi.iht_loop(PhiT, x, y, t1, t2, t3, iterations, 0, mu, false);
    return;
#endif
    x.clear();
    for (uint64_t i = 0; i < iterations; i += 1) {
        Phi.mvm_scaleAndAdd(x, y, -1.0f, t1, t2);
        PhiT.mvm_scaleAndAdd(t2, x, mu, t3);
    }
}


/* Not in the reference: the two loops above with ONE matrix -- the gradient step takes Phi' t2 straight from Phi
 * (CloverMatrix4::mvm_transposed_scaleAndAdd -> clm4_mvm_transposed_scale_and_add), so no PhiT is built, held or kept in step with Phi.
 * Rounding disabled: CloverMatrix4::iht_loop_one_matrix -> clm4_iht_one_matrix, the bits of Q_IHT / Q_GD with PhiT = transpose(Phi).
 * Stochastic: the same calls as above; the gradient step draws from Phi's generator, where the two-matrix loop draws from PhiT's.  The
 * two-matrix overloads stay the default: what one matrix costs per iteration is measured in DESIGN.md 3. */
inline void Q_IHT_one_matrix(CloverMatrix4 &Phi, CloverVector4 &x, CloverVector4 &y, CloverVector4 &t1, CloverVector4 &t2, CloverVector4 &t3,
                             const uint64_t iterations, const uint64_t K, const float mu)
{
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
    Phi.iht_loop_one_matrix(x, y, t1, t2, t3, iterations, K, mu, true);
    return;
#endif
    x.clear();
    for (uint64_t i = 0; i < iterations; i += 1) {
        Phi.mvm_scaleAndAdd(x, y, -1.0f, t1, t2);
        Phi.mvm_transposed_scaleAndAdd(t2, x, mu, t3);
        x.threshold_parallel(K);
    }
}

inline void Q_GD_one_matrix(CloverMatrix4 &Phi, CloverVector4 &x, CloverVector4 &y, CloverVector4 &t1, CloverVector4 &t2, CloverVector4 &t3,
                            const uint64_t iterations, const float mu)
{
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
    Phi.iht_loop_one_matrix(x, y, t1, t2, t3, iterations, 0, mu, false);
    return;
#endif
    x.clear();
    for (uint64_t i = 0; i < iterations; i += 1) {
        Phi.mvm_scaleAndAdd(x, y, -1.0f, t1, t2);
        Phi.mvm_transposed_scaleAndAdd(t2, x, mu, t3);
    }
}


/* Not in the reference: Q_IHT / Q_GD for `count` signals with ONE Phi: per iteration two passes over Phi / PhiT for every group of
 * CLM4_MVM_BATCH_MAX signals instead of two per signal.  x[j], t1[j], t2[j], t3[j] end as
 * Q_IHT(Phi, PhiT, *x[j], *y[j], *t1[j], *t2[j], *t3[j], ...) called for signal 0, then 1, ... leaves them, bit for bit, and so do the
 * generators of Phi and PhiT.  Rounding disabled: CloverMatrix4::iht_loop_batch -> clm4_iht_batch.  Stochastic: in that order of calls Phi's
 * generator serves all iterations of signal 0 first, 2 (m / 64) draws per mvm, so signal j's mvm of iteration `it` draws at
 * (j * iterations + it) * 2 (m / 64) -- which is where CloverMatrix4::mvm_batch_at places it while the loop below runs iteration by
 * iteration for all signals; the last iteration advances the generator by everything.  The scaleAndAdd steps draw from y[j]'s and x[j]'s
 * own generators and stay single calls. */
namespace clover_hip {
template <class QMatrix, class QVector>       /* CloverMatrix4 with CloverVector4 or CloverVector8, CloverMatrix8 with CloverVector8: every mvm draws 2 (rows / 64) */
inline void q_iht_batch_stochastic(QMatrix &Phi, QMatrix &PhiT, QVector *const *x, QVector *const *y, QVector *const *t1,
                                   QVector *const *t2, QVector *const *t3, const uint64_t count, const uint64_t iterations, const uint64_t K,
                                   const float mu, const bool with_threshold)
{
    for (uint64_t j = 0; j < count; j++) x[j]->clear();
    const uint64_t dm = 2 * (Phi.getRows() >> 6), dn = 2 * (PhiT.getRows() >> 6);       /* draws of one mvm with Phi, with PhiT */
    for (uint64_t it = 0; it < iterations; it++) {
        const bool last = it + 1 == iterations;
        Phi.mvm_batch_at(x, t1, count, it * dm, iterations * dm, last ? count * iterations * dm : 0);
        for (uint64_t j = 0; j < count; j++) y[j]->scaleAndAdd_parallel(*t1[j], -1.0f, *t2[j]);
        PhiT.mvm_batch_at(t2, t3, count, it * dn, iterations * dn, last ? count * iterations * dn : 0);
        for (uint64_t j = 0; j < count; j++) x[j]->scaleAndAdd_parallel(*t3[j], mu);
        if (with_threshold) QVector::threshold_batch(x, count, K);
    }
}
}

inline void Q_IHT_batch(CloverMatrix4 &Phi, CloverMatrix4 &PhiT, CloverVector4 *const *x, CloverVector4 *const *y, CloverVector4 *const *t1,
                        CloverVector4 *const *t2, CloverVector4 *const *t3, const uint64_t count, const uint64_t iterations, const uint64_t K,
                        const float mu)
{
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
    Phi.iht_loop_batch(PhiT, x, y, t1, t2, t3, count, iterations, K, mu, true);
#else
    clover_hip::q_iht_batch_stochastic(Phi, PhiT, x, y, t1, t2, t3, count, iterations, K, mu, true);
#endif
}

inline void Q_GD_batch(CloverMatrix4 &Phi, CloverMatrix4 &PhiT, CloverVector4 *const *x, CloverVector4 *const *y, CloverVector4 *const *t1,
                       CloverVector4 *const *t2, CloverVector4 *const *t3, const uint64_t count, const uint64_t iterations, const float mu)
{
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
    Phi.iht_loop_batch(PhiT, x, y, t1, t2, t3, count, iterations, 0, mu, false);
#else
    clover_hip::q_iht_batch_stochastic(Phi, PhiT, x, y, t1, t2, t3, count, iterations, 0, mu, false);
#endif
}


/* Not in the reference: Q_IHT_batch / Q_GD_batch with ONE matrix -- the gradient step of every group takes Phi' t2[j] straight from Phi
 * (CloverMatrix4::mvm_transposed_batch_at -> clm4_mvm_transposed_batch_at, clover_hip_batch_t.h), so no PhiT is built or held.  x[j],
 * t1[j], t2[j], t3[j] end as Q_IHT_one_matrix(Phi, *x[j], *y[j], ...) called for signal 0, then 1, ... leaves them, bit for bit, and so does
 * Phi's generator.  Rounding disabled: CloverMatrix4::iht_loop_batch_one_matrix -> clm4_iht_batch_one_matrix.  Stochastic: BOTH products
 * draw from Phi's generator, as in Q_IHT_one_matrix: with dm = 2 (m / 64) and dn = 2 (n / 64) signal j's iteration `it` has its Phi window
 * at (j * iterations + it) * (dm + dn) and its Phi' window dm further on; the last iteration advances the generator by everything. */
namespace clover_hip {
template <class QMatrix, class QVector>       /* CloverMatrix4 with CloverVector4 or CloverVector8, CloverMatrix8 with CloverVector8: the products draw 2 (m / 64) and 2 (n / 64) */
inline void q_iht_batch_one_matrix_stochastic(QMatrix &Phi, QVector *const *x, QVector *const *y, QVector *const *t1, QVector *const *t2,
                                              QVector *const *t3, const uint64_t count, const uint64_t iterations, const uint64_t K, const float mu,
                                              const bool with_threshold)
{
    for (uint64_t j = 0; j < count; j++) x[j]->clear();
    const uint64_t dm = 2 * (Phi.getRows() >> 6), dn = 2 * (Phi.getCols() >> 6), P = dm + dn;
    for (uint64_t it = 0; it < iterations; it++) {
        const bool last = it + 1 == iterations;
        Phi.mvm_batch_at(x, t1, count, it * P, iterations * P, 0);
        for (uint64_t j = 0; j < count; j++) y[j]->scaleAndAdd_parallel(*t1[j], -1.0f, *t2[j]);
        Phi.mvm_transposed_batch_at(t2, t3, count, it * P + dm, iterations * P, last ? count * iterations * P : 0);
        for (uint64_t j = 0; j < count; j++) x[j]->scaleAndAdd_parallel(*t3[j], mu);
        if (with_threshold) QVector::threshold_batch(x, count, K);
    }
}
}

inline void Q_IHT_batch_one_matrix(CloverMatrix4 &Phi, CloverVector4 *const *x, CloverVector4 *const *y, CloverVector4 *const *t1,
                                   CloverVector4 *const *t2, CloverVector4 *const *t3, const uint64_t count, const uint64_t iterations,
                                   const uint64_t K, const float mu)
{
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
    Phi.iht_loop_batch_one_matrix(x, y, t1, t2, t3, count, iterations, K, mu, true);
#else
    clover_hip::q_iht_batch_one_matrix_stochastic(Phi, x, y, t1, t2, t3, count, iterations, K, mu, true);
#endif
}

inline void Q_GD_batch_one_matrix(CloverMatrix4 &Phi, CloverVector4 *const *x, CloverVector4 *const *y, CloverVector4 *const *t1,
                                  CloverVector4 *const *t2, CloverVector4 *const *t3, const uint64_t count, const uint64_t iterations, const float mu)
{
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
    Phi.iht_loop_batch_one_matrix(x, y, t1, t2, t3, count, iterations, 0, mu, false);
#else
    clover_hip::q_iht_batch_one_matrix_stochastic(Phi, x, y, t1, t2, t3, count, iterations, 0, mu, false);
#endif
}

/* the same for `count` CloverVector8 signals with ONE CloverMatrix4 Phi and no PhiT -- the published "4-bit" configuration
 * (clm4_iht_v8_batch_one_matrix, clover_hip_batch_t_v8.h; stochastic: the CloverVector8 overloads of CloverMatrix4::mvm_batch_at and
 * mvm_transposed_batch_at per step, both on Phi's generator): bit-identical to calling the CloverVector8 overloads of Q_IHT_one_matrix /
 * Q_GD_one_matrix signal after signal, Phi's generator included */
inline void Q_IHT_batch_one_matrix(CloverMatrix4 &Phi, CloverVector8 *const *x, CloverVector8 *const *y, CloverVector8 *const *t1,
                                   CloverVector8 *const *t2, CloverVector8 *const *t3, const uint64_t count, const uint64_t iterations,
                                   const uint64_t K, const float mu)
{
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
    Phi.iht_loop_batch_one_matrix(x, y, t1, t2, t3, count, iterations, K, mu, true);
#else
    clover_hip::q_iht_batch_one_matrix_stochastic(Phi, x, y, t1, t2, t3, count, iterations, K, mu, true);
#endif
}

inline void Q_GD_batch_one_matrix(CloverMatrix4 &Phi, CloverVector8 *const *x, CloverVector8 *const *y, CloverVector8 *const *t1,
                                  CloverVector8 *const *t2, CloverVector8 *const *t3, const uint64_t count, const uint64_t iterations, const float mu)
{
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
    Phi.iht_loop_batch_one_matrix(x, y, t1, t2, t3, count, iterations, 0, mu, false);
#else
    clover_hip::q_iht_batch_one_matrix_stochastic(Phi, x, y, t1, t2, t3, count, iterations, 0, mu, false);
#endif
}



/* CloverMatrix4 with CloverVector8 vectors: the configuration the reference measures and publishes as the 4-bit IHT / GD
 * (test/performance/02_bit04.cpp:140; "the 4-bit version uses the mixed precision MVM", doc/results/performance.txt:597-606) */
inline void Q_IHT(CloverMatrix4 &Phi, CloverMatrix4 &PhiT, CloverVector8 &x, CloverVector8 &y, CloverVector8 &t1, CloverVector8 &t2,
                  CloverVector8 &t3, const uint64_t iterations, const uint64_t K, const float mu)
{
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
    Phi.iht_loop(PhiT, x, y, t1, t2, t3, iterations, K, mu, true);
    return;
#endif
    x.clear();
    for (uint64_t i = 0; i < iterations; i += 1) {
        Phi.mvm_scaleAndAdd(x, y, -1.0f, t1, t2);
        PhiT.mvm_scaleAndAdd(t2, x, mu, t3);
        x.threshold_parallel(K);
    }
}

inline void Q_GD(CloverMatrix4 &Phi, CloverMatrix4 &PhiT, CloverVector8 &x, CloverVector8 &y, CloverVector8 &t1, CloverVector8 &t2,
                 CloverVector8 &t3, const uint64_t iterations, const float mu)
{
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
    Phi.iht_loop(PhiT, x, y, t1, t2, t3, iterations, 0, mu, false);
    return;
#endif
    x.clear();
    for (uint64_t i = 0; i < iterations; i += 1) {
        Phi.mvm_scaleAndAdd(x, y, -1.0f, t1, t2);
        PhiT.mvm_scaleAndAdd(t2, x, mu, t3);
    }
}

/* Not in the reference: the two loops above with ONE matrix (CloverMatrix4::mvm_transposed_scaleAndAdd on CloverVector8 ->
 * clm4_mvm_v8_transposed_scale_and_add; rounding disabled: iht_loop_one_matrix -> clm4_iht_v8_one_matrix), the bits of Q_IHT / Q_GD with
 * PhiT = transpose(Phi).  Stochastic: the gradient step draws from Phi's generator, where the two-matrix loop draws from PhiT's.  The
 * two-matrix overloads stay the default. */
inline void Q_IHT_one_matrix(CloverMatrix4 &Phi, CloverVector8 &x, CloverVector8 &y, CloverVector8 &t1, CloverVector8 &t2, CloverVector8 &t3,
                             const uint64_t iterations, const uint64_t K, const float mu)
{
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
    Phi.iht_loop_one_matrix(x, y, t1, t2, t3, iterations, K, mu, true);
    return;
#endif
    x.clear();
    for (uint64_t i = 0; i < iterations; i += 1) {
        Phi.mvm_scaleAndAdd(x, y, -1.0f, t1, t2);
        Phi.mvm_transposed_scaleAndAdd(t2, x, mu, t3);
        x.threshold_parallel(K);
    }
}

inline void Q_GD_one_matrix(CloverMatrix4 &Phi, CloverVector8 &x, CloverVector8 &y, CloverVector8 &t1, CloverVector8 &t2, CloverVector8 &t3,
                            const uint64_t iterations, const float mu)
{
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
    Phi.iht_loop_one_matrix(x, y, t1, t2, t3, iterations, 0, mu, false);
    return;
#endif
    x.clear();
    for (uint64_t i = 0; i < iterations; i += 1) {
        Phi.mvm_scaleAndAdd(x, y, -1.0f, t1, t2);
        Phi.mvm_transposed_scaleAndAdd(t2, x, mu, t3);
    }
}

/* the same for `count` signals with ONE Phi (clm4_iht_v8_batch; stochastic: CloverMatrix4::mvm_batch_at per step): bit-identical to
 * calling Q_IHT / Q_GD above signal after signal, the generators of Phi and PhiT included */
inline void Q_IHT_batch(CloverMatrix4 &Phi, CloverMatrix4 &PhiT, CloverVector8 *const *x, CloverVector8 *const *y, CloverVector8 *const *t1,
                        CloverVector8 *const *t2, CloverVector8 *const *t3, const uint64_t count, const uint64_t iterations, const uint64_t K,
                        const float mu)
{
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
    Phi.iht_loop_batch(PhiT, x, y, t1, t2, t3, count, iterations, K, mu, true);
#else
    clover_hip::q_iht_batch_stochastic(Phi, PhiT, x, y, t1, t2, t3, count, iterations, K, mu, true);
#endif
}

inline void Q_GD_batch(CloverMatrix4 &Phi, CloverMatrix4 &PhiT, CloverVector8 *const *x, CloverVector8 *const *y, CloverVector8 *const *t1,
                       CloverVector8 *const *t2, CloverVector8 *const *t3, const uint64_t count, const uint64_t iterations, const float mu)
{
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
    Phi.iht_loop_batch(PhiT, x, y, t1, t2, t3, count, iterations, 0, mu, false);
#else
    clover_hip::q_iht_batch_stochastic(Phi, PhiT, x, y, t1, t2, t3, count, iterations, 0, mu, false);
#endif
}


/* CloverMatrix8 with CloverVector8 vectors: the reference's pure 8-bit configuration (test/performance/02_bit08.cpp).  Explicit
 * specialisations of the generic templates, not overloads: callers that spell the template arguments out --
 * Q_IHT<CloverMatrix8, CloverVector8>(Phi, ...) -- reach them as well as those that let them be deduced.  The whole loop in one call
 * (CloverMatrix8::iht_loop -> clm8_iht, three launches per iteration) when rounding is deterministic, else every scaleAndAdd paired with
 * the mvm before it; identical results either way. */
template <>
inline void Q_IHT<CloverMatrix8, CloverVector8>(CloverMatrix8 &Phi, CloverMatrix8 &PhiT, CloverVector8 &x, CloverVector8 &y, CloverVector8 &t1,
                                                CloverVector8 &t2, CloverVector8 &t3, const uint64_t iterations, const uint64_t K, const float mu)
{
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
    Phi.iht_loop(PhiT, x, y, t1, t2, t3, iterations, K, mu, true);
    return;
#endif
    x.clear();
    for (uint64_t i = 0; i < iterations; i += 1) {
        Phi.mvm_scaleAndAdd(x, y, -1.0f, t1, t2);
        PhiT.mvm_scaleAndAdd(t2, x, mu, t3);
        x.threshold_parallel(K);
    }
}

template <>
inline void Q_GD<CloverMatrix8, CloverVector8>(CloverMatrix8 &Phi, CloverMatrix8 &PhiT, CloverVector8 &x, CloverVector8 &y, CloverVector8 &t1,
                                               CloverVector8 &t2, CloverVector8 &t3, const uint64_t iterations, const float mu)
{
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
    Phi.iht_loop(PhiT, x, y, t1, t2, t3, iterations, 0, mu, false);
    return;
#endif
    x.clear();
    for (uint64_t i = 0; i < iterations; i += 1) {
        Phi.mvm_scaleAndAdd(x, y, -1.0f, t1, t2);
        PhiT.mvm_scaleAndAdd(t2, x, mu, t3);
    }
}

/* Not in the reference: the two loops above with ONE matrix (CloverMatrix8::mvm_transposed_scaleAndAdd -> clm8_mvm_transposed_scale_and_add;
 * rounding disabled: iht_loop_one_matrix -> clm8_iht_one_matrix), the bits of Q_IHT / Q_GD with PhiT = transpose(Phi).  Stochastic: the
 * gradient step draws from Phi's generator, where the two-matrix loop draws from PhiT's.  The two-matrix forms stay the default. */
inline void Q_IHT_one_matrix(CloverMatrix8 &Phi, CloverVector8 &x, CloverVector8 &y, CloverVector8 &t1, CloverVector8 &t2, CloverVector8 &t3,
                             const uint64_t iterations, const uint64_t K, const float mu)
{
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
    Phi.iht_loop_one_matrix(x, y, t1, t2, t3, iterations, K, mu, true);
    return;
#endif
    x.clear();
    for (uint64_t i = 0; i < iterations; i += 1) {
        Phi.mvm_scaleAndAdd(x, y, -1.0f, t1, t2);
        Phi.mvm_transposed_scaleAndAdd(t2, x, mu, t3);
        x.threshold_parallel(K);
    }
}

inline void Q_GD_one_matrix(CloverMatrix8 &Phi, CloverVector8 &x, CloverVector8 &y, CloverVector8 &t1, CloverVector8 &t2, CloverVector8 &t3,
                            const uint64_t iterations, const float mu)
{
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
    Phi.iht_loop_one_matrix(x, y, t1, t2, t3, iterations, 0, mu, false);
    return;
#endif
    x.clear();
    for (uint64_t i = 0; i < iterations; i += 1) {
        Phi.mvm_scaleAndAdd(x, y, -1.0f, t1, t2);
        Phi.mvm_transposed_scaleAndAdd(t2, x, mu, t3);
    }
}

/* the same for `count` signals with ONE 8-bit Phi (clm8_iht_batch; stochastic: CloverMatrix8::mvm_batch_at per step): bit-identical to
 * calling Q_IHT / Q_GD above signal after signal, the generators of Phi and PhiT included */
inline void Q_IHT_batch(CloverMatrix8 &Phi, CloverMatrix8 &PhiT, CloverVector8 *const *x, CloverVector8 *const *y, CloverVector8 *const *t1,
                        CloverVector8 *const *t2, CloverVector8 *const *t3, const uint64_t count, const uint64_t iterations, const uint64_t K,
                        const float mu)
{
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
    Phi.iht_loop_batch(PhiT, x, y, t1, t2, t3, count, iterations, K, mu, true);
#else
    clover_hip::q_iht_batch_stochastic(Phi, PhiT, x, y, t1, t2, t3, count, iterations, K, mu, true);
#endif
}

inline void Q_GD_batch(CloverMatrix8 &Phi, CloverMatrix8 &PhiT, CloverVector8 *const *x, CloverVector8 *const *y, CloverVector8 *const *t1,
                       CloverVector8 *const *t2, CloverVector8 *const *t3, const uint64_t count, const uint64_t iterations, const float mu)
{
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
    Phi.iht_loop_batch(PhiT, x, y, t1, t2, t3, count, iterations, 0, mu, false);
#else
    clover_hip::q_iht_batch_stochastic(Phi, PhiT, x, y, t1, t2, t3, count, iterations, 0, mu, false);
#endif
}

/* the one-matrix loops for `count` signals with ONE 8-bit Phi and no PhiT (clm8_iht_batch_one_matrix, clover_hip_batch_t8.h; stochastic:
 * CloverMatrix8::mvm_batch_at and mvm_transposed_batch_at per step, both on Phi's generator): bit-identical to calling Q_IHT_one_matrix /
 * Q_GD_one_matrix above signal after signal, Phi's generator included */
inline void Q_IHT_batch_one_matrix(CloverMatrix8 &Phi, CloverVector8 *const *x, CloverVector8 *const *y, CloverVector8 *const *t1,
                                   CloverVector8 *const *t2, CloverVector8 *const *t3, const uint64_t count, const uint64_t iterations,
                                   const uint64_t K, const float mu)
{
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
    Phi.iht_loop_batch_one_matrix(x, y, t1, t2, t3, count, iterations, K, mu, true);
#else
    clover_hip::q_iht_batch_one_matrix_stochastic(Phi, x, y, t1, t2, t3, count, iterations, K, mu, true);
#endif
}

inline void Q_GD_batch_one_matrix(CloverMatrix8 &Phi, CloverVector8 *const *x, CloverVector8 *const *y, CloverVector8 *const *t1,
                                  CloverVector8 *const *t2, CloverVector8 *const *t3, const uint64_t count, const uint64_t iterations, const float mu)
{
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
    Phi.iht_loop_batch_one_matrix(x, y, t1, t2, t3, count, iterations, 0, mu, false);
#else
    clover_hip::q_iht_batch_one_matrix_stochastic(Phi, x, y, t1, t2, t3, count, iterations, 0, mu, false);
#endif
}

/* CloverMatrix16 with CloverVector16 vectors: the half-precision loop the reference measures in test/performance/02_bit16.cpp:112-117.
 * Explicit specialisations again, so that the explicit and the deduced spelling both reach them, and unconditional: the 16-bit classes
 * have no stochastic rounding.  The whole loop in one call (CloverMatrix16::iht_loop -> clm_f16_iht): three launches per iteration, two
 * for Q_GD, the bits of the generic templates' five method calls. */
template <>
inline void Q_IHT<CloverMatrix16, CloverVector16>(CloverMatrix16 &Phi, CloverMatrix16 &PhiT, CloverVector16 &x, CloverVector16 &y, CloverVector16 &t1,
                                                  CloverVector16 &t2, CloverVector16 &t3, const uint64_t iterations, const uint64_t K, const float mu)
{
    Phi.iht_loop(PhiT, x, y, t1, t2, t3, iterations, K, mu, true);
}

template <>
inline void Q_GD<CloverMatrix16, CloverVector16>(CloverMatrix16 &Phi, CloverMatrix16 &PhiT, CloverVector16 &x, CloverVector16 &y, CloverVector16 &t1,
                                                 CloverVector16 &t2, CloverVector16 &t3, const uint64_t iterations, const float mu)
{
    Phi.iht_loop(PhiT, x, y, t1, t2, t3, iterations, 0, mu, false);
}

/* Q_IHT / Q_GD on this pair holding ONE matrix: Phi' t2 comes straight from Phi's own bytes (CloverMatrix16::iht_loop_one_matrix ->
 * clm_f16_iht_one_matrix, clover_hip_f16_t.h), the bits of Q_IHT / Q_GD above with PhiT = transpose(Phi) and the same launches per
 * iteration.  Opt-in by name: Q_IHT / Q_GD themselves keep two matrices. */
inline void Q_IHT_one_matrix(CloverMatrix16 &Phi, CloverVector16 &x, CloverVector16 &y, CloverVector16 &t1, CloverVector16 &t2, CloverVector16 &t3,
                             const uint64_t iterations, const uint64_t K, const float mu)
{
    Phi.iht_loop_one_matrix(x, y, t1, t2, t3, iterations, K, mu, true);
}

inline void Q_GD_one_matrix(CloverMatrix16 &Phi, CloverVector16 &x, CloverVector16 &y, CloverVector16 &t1, CloverVector16 &t2, CloverVector16 &t3,
                            const uint64_t iterations, const float mu)
{
    Phi.iht_loop_one_matrix(x, y, t1, t2, t3, iterations, 0, mu, false);
}

/* the same for `count` signals with ONE half-precision Phi (CloverMatrix16::iht_loop_batch -> clm_f16_iht_batch, clover_hip_batch_f16.h): per
 * iteration two fused launches and one threshold for a group of signals; bit-identical to calling Q_IHT / Q_GD above signal after signal.
 * Unconditional, as those: the 16-bit classes have no stochastic rounding; the threshold follows the exactness switch (FAST under
 * -DCLOVER_FAST, the reference's survivors by default). */
inline void Q_IHT_batch(CloverMatrix16 &Phi, CloverMatrix16 &PhiT, CloverVector16 *const *x, CloverVector16 *const *y, CloverVector16 *const *t1,
                        CloverVector16 *const *t2, CloverVector16 *const *t3, const uint64_t count, const uint64_t iterations, const uint64_t K,
                        const float mu)
{
    Phi.iht_loop_batch(PhiT, x, y, t1, t2, t3, count, iterations, K, mu, true);
}

inline void Q_GD_batch(CloverMatrix16 &Phi, CloverMatrix16 &PhiT, CloverVector16 *const *x, CloverVector16 *const *y, CloverVector16 *const *t1,
                       CloverVector16 *const *t2, CloverVector16 *const *t3, const uint64_t count, const uint64_t iterations, const float mu)
{
    Phi.iht_loop_batch(PhiT, x, y, t1, t2, t3, count, iterations, 0, mu, false);
}

/* `count` signals holding ONE half-precision matrix: both of the above at once (CloverMatrix16::iht_loop_batch_one_matrix ->
 * clm_f16_iht_batch_one_matrix, clover_hip_batch_f16_t.h).  Bit-identical to Q_IHT_one_matrix / Q_GD_one_matrix signal after signal, and
 * through those to Q_IHT_batch / Q_GD_batch with PhiT = transpose(Phi).  Opt-in by name. */
inline void Q_IHT_batch_one_matrix(CloverMatrix16 &Phi, CloverVector16 *const *x, CloverVector16 *const *y, CloverVector16 *const *t1,
                                   CloverVector16 *const *t2, CloverVector16 *const *t3, const uint64_t count, const uint64_t iterations,
                                   const uint64_t K, const float mu)
{
    Phi.iht_loop_batch_one_matrix(x, y, t1, t2, t3, count, iterations, K, mu, true);
}

inline void Q_GD_batch_one_matrix(CloverMatrix16 &Phi, CloverVector16 *const *x, CloverVector16 *const *y, CloverVector16 *const *t1,
                                  CloverVector16 *const *t2, CloverVector16 *const *t3, const uint64_t count, const uint64_t iterations,
                                  const float mu)
{
    Phi.iht_loop_batch_one_matrix(x, y, t1, t2, t3, count, iterations, 0, mu, false);
}

#ifdef CLOVER_FP32_ON_DEVICE
/* CloverMatrix32 with CloverVector32 vectors under -DCLOVER_FP32_ON_DEVICE: the fp32 baseline of every table of the reference, on the
 * device.  The whole loop in one call (CloverMatrix32::iht_loop -> clm_f32_iht): three launches per iteration, two for Q_GD, the bits of
 * the generic templates' five method calls.  Without the switch the generic templates run the host methods, as before. */
template <>
inline void Q_IHT<CloverMatrix32, CloverVector32>(CloverMatrix32 &Phi, CloverMatrix32 &PhiT, CloverVector32 &x, CloverVector32 &y, CloverVector32 &t1,
                                                  CloverVector32 &t2, CloverVector32 &t3, const uint64_t iterations, const uint64_t K, const float mu)
{
    Phi.iht_loop(PhiT, x, y, t1, t2, t3, iterations, K, mu, true);
}
template <>
inline void Q_GD<CloverMatrix32, CloverVector32>(CloverMatrix32 &Phi, CloverMatrix32 &PhiT, CloverVector32 &x, CloverVector32 &y, CloverVector32 &t1,
                                                 CloverVector32 &t2, CloverVector32 &t3, const uint64_t iterations, const float mu)
{
    Phi.iht_loop(PhiT, x, y, t1, t2, t3, iterations, 0, mu, false);
}

/* CloverMatrix4 with CloverVector32 vectors (the reference's Q_IHT<CloverMatrix4, CloverVector32>: the matrix carries the bytes, the iterate
 * keeps fp32) under the same switch, which puts CloverVector32's scaleAndAdd and threshold on the device: the whole loop in one call
 * (CloverMatrix4::iht_loop -> clm4_iht_f32, clover_hip_m4_f32.h), one fused launch per product plus the threshold, the bits of the generic
 * templates' five method calls.  Overloads, as for the other vector widths of CloverMatrix4; without the switch the generic templates
 * run one device product and the host methods, as before. */
inline void Q_IHT(CloverMatrix4 &Phi, CloverMatrix4 &PhiT, CloverVector32 &x, CloverVector32 &y, CloverVector32 &t1, CloverVector32 &t2,
                  CloverVector32 &t3, const uint64_t iterations, const uint64_t K, const float mu)
{
    Phi.iht_loop(PhiT, x, y, t1, t2, t3, iterations, K, mu, true);
}
inline void Q_GD(CloverMatrix4 &Phi, CloverMatrix4 &PhiT, CloverVector32 &x, CloverVector32 &y, CloverVector32 &t1, CloverVector32 &t2,
                 CloverVector32 &t3, const uint64_t iterations, const float mu)
{
    Phi.iht_loop(PhiT, x, y, t1, t2, t3, iterations, 0, mu, false);
}
/* the same holding ONE matrix: Phi' t2 comes straight from Phi's own bytes (CloverMatrix4::iht_loop_one_matrix -> clm4_iht_f32_one_matrix),
 * the bits of the two above with PhiT = transpose(Phi).  Opt-in by name. */
inline void Q_IHT_one_matrix(CloverMatrix4 &Phi, CloverVector32 &x, CloverVector32 &y, CloverVector32 &t1, CloverVector32 &t2, CloverVector32 &t3,
                             const uint64_t iterations, const uint64_t K, const float mu)
{
    Phi.iht_loop_one_matrix(x, y, t1, t2, t3, iterations, K, mu, true);
}
inline void Q_GD_one_matrix(CloverMatrix4 &Phi, CloverVector32 &x, CloverVector32 &y, CloverVector32 &t1, CloverVector32 &t2, CloverVector32 &t3,
                            const uint64_t iterations, const float mu)
{
    Phi.iht_loop_one_matrix(x, y, t1, t2, t3, iterations, 0, mu, false);
}

/* CloverMatrix8 with CloverVector32 vectors (the reference's Q_IHT<CloverMatrix8, CloverVector32>), the same column under the same switch:
 * CloverMatrix8::iht_loop -> clm8_iht_f32, iht_loop_one_matrix -> clm8_iht_f32_one_matrix (clover_hip_m8_f32.h).  Overloads; without the
 * switch the generic templates run one device product and the host methods, as before. */
inline void Q_IHT(CloverMatrix8 &Phi, CloverMatrix8 &PhiT, CloverVector32 &x, CloverVector32 &y, CloverVector32 &t1, CloverVector32 &t2,
                  CloverVector32 &t3, const uint64_t iterations, const uint64_t K, const float mu)
{
    Phi.iht_loop(PhiT, x, y, t1, t2, t3, iterations, K, mu, true);
}
inline void Q_GD(CloverMatrix8 &Phi, CloverMatrix8 &PhiT, CloverVector32 &x, CloverVector32 &y, CloverVector32 &t1, CloverVector32 &t2,
                 CloverVector32 &t3, const uint64_t iterations, const float mu)
{
    Phi.iht_loop(PhiT, x, y, t1, t2, t3, iterations, 0, mu, false);
}
inline void Q_IHT_one_matrix(CloverMatrix8 &Phi, CloverVector32 &x, CloverVector32 &y, CloverVector32 &t1, CloverVector32 &t2, CloverVector32 &t3,
                             const uint64_t iterations, const uint64_t K, const float mu)
{
    Phi.iht_loop_one_matrix(x, y, t1, t2, t3, iterations, K, mu, true);
}
inline void Q_GD_one_matrix(CloverMatrix8 &Phi, CloverVector32 &x, CloverVector32 &y, CloverVector32 &t1, CloverVector32 &t2, CloverVector32 &t3,
                            const uint64_t iterations, const float mu)
{
    Phi.iht_loop_one_matrix(x, y, t1, t2, t3, iterations, 0, mu, false);
}
#endif

#endif
