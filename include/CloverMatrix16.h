/*
 * CloverMatrix16.h -- half-precision matrix, MI355X-backed.
 *
 * Drop-in for the reference's include/CloverMatrix16.h: same class name, constructor, method names and data format (row-major raw IEEE
 * binary16 bit patterns, rows / cols padded to multiples of 128, no scales; :36-66).  Hot methods call libclover_hip.so:
 *
 *   quantize                             -> clm_f16_quantize   (CloverMatrix16.h:383-410)
 *   mvm / mvm_parallel (CloverVector16)  -> clm_f16_mvm        (:230-308, :133-228)
 *   mvm / mvm_parallel (CloverVector32)  -> clm_f16_mvm_f32    (:321-381)
 *   transpose / transpose_parallel       -> clm_f16_transpose  (:441-474)
 *   *_scalar                             -> plain host loops in the reference's scalar order: quantize_scalar (:412-421), mvm_scalar
 *                                           (:98-131: one running fp32 sum per row; for fp32 vectors a double accumulation, :310-319),
 *                                           transpose_scalar (:424-439)
 *
 *   mvm_scaleAndAdd                      -> clm_f16_mvm_scale_and_add  (not in the reference: mvm + the scaleAndAdd behind it, one launch)
 *   iht_loop                             -> clm_f16_iht        (the whole Q_IHT / Q_GD loop of 01_measure.h:923-946, 999-1021 in one call)
 *   mvm_transposed / mvm_transposed_scaleAndAdd / iht_loop_one_matrix
 *                                        -> clm_f16_mvm_transposed, clm_f16_mvm_f32_transposed, clm_f16_mvm_transposed_scale_and_add,
 *                                           clm_f16_iht_one_matrix (clover_hip_f16_t.h; not in the reference: this' * x straight from this
 *                                           matrix's own bytes, no stored transpose, bit-identical to transpose() + the methods above)
 *   mvm_batch / mvm_scaleAndAdd_batch / iht_loop_batch
 *                                        -> clm_f16_mvm_batch, clm_f16_mvm_scale_and_add_batch, clm_f16_iht_batch (clover_hip_batch_f16.h;
 *                                           not in the reference: the same for several vectors in ONE pass over the matrix per group of
 *                                           CLM4_MVM_BATCH_MAX, bit-identical to the single methods vector after vector)
 *   mvm_transposed_batch / mvm_transposed_scaleAndAdd_batch / iht_loop_batch_one_matrix
 *                                        -> clm_f16_mvm_transposed_batch, clm_f16_mvm_transposed_scale_and_add_batch,
 *                                           clm_f16_iht_batch_one_matrix (clover_hip_batch_f16_t.h; not in the reference: this' * x[j] for
 *                                           several vectors in ONE pass over this matrix's own bytes, bit-identical to the single
 *                                           transposed methods vector after vector)
 *
 * Q_IHT<CloverMatrix16, CloverVector16> and Q_GD<...> are specialised in CloverIHT.h (which includes this header) and call iht_loop: every
 * step is a kernel on the device mirrors, nothing is copied back between steps.
 */
#ifndef CLOVER_MATRIX16_H
#define CLOVER_MATRIX16_H

#include <sstream>
#include <string>
#include <vector>

#include "CloverMatrix32.h"
#include "CloverVector16.h"
#include "CloverVector32.h"
#include "clover_hip_batch_f16.h"  /* the batched half-precision calls: a header of their own beside clover_hip.h */
#include "clover_hip_f16_t.h"      /* the transposed half-precision calls: likewise */
#include "clover_hip_batch_f16_t.h" /* the batched transposed half-precision calls: likewise */

class CloverMatrix16 {
protected:
    const uint64_t rows;
    const uint64_t cols;
    mutable clover_hip::Mirror mem;            /* rows * cols uint16_t */

    const uint16_t *dev_values() const { return reinterpret_cast<const uint16_t *>(mem.dev_ro()); }
    const uint16_t *values_ro() const { return reinterpret_cast<const uint16_t *>(mem.host_ro()); }
    uint16_t *values_rw() const { return reinterpret_cast<uint16_t *>(mem.host_rw()); }

    void check_same_size(const CloverMatrix32 &m) const
    {
        if (m.getRows() != rows || m.getCols() != cols) {
            std::cout << "Matrices do not have the same size. Exiting ..." << std::endl;
            exit(1);
        }
    }
    template <class V, class R>
    void check_mvm(const V &productVector, const R &resultVector) const
    {
        if (productVector.size_pad() != getCols() || resultVector.size_pad() != getRows()) {
            std::cout << "MVM can not be performed. Exiting ..." << std::endl;
            exit(1);
        }
    }
    /* the sizes of this' * x: x has as many elements as this has rows, the result as many as it has columns */
    template <class V, class R>
    void check_mvm_transposed(const V &productVector, const R &resultVector) const
    {
        if (productVector.size_pad() != getRows() || resultVector.size_pad() != getCols()) {
            std::cout << "MVM can not be performed. Exiting ..." << std::endl;
            exit(1);
        }
    }
    /* The batch methods carry a caller's vectors into the batched C calls as the batch methods of CloverMatrix4 / 8 do (clover_batch.h),
     * without the scale arrays those have: inputs are mapped read-only first, then the outputs write-only (read-write for the in-place
     * form).  The pointers of inputs are stored without their const and handed on as const again. */
    typedef std::vector<uint16_t *> DevArray;
    static DevArray dev_inputs(const CloverVector16 *const *v, uint64_t count)
    {
        DevArray a;
        for (uint64_t j = 0; j < count; j++) a.push_back(const_cast<uint16_t *>(v[j]->dev_values_ro()));
        return a;
    }
    static DevArray dev_outputs(CloverVector16 *const *v, uint64_t count, bool read_too)
    {
        DevArray a;
        for (uint64_t j = 0; j < count; j++) a.push_back(read_too ? v[j]->dev_values_rw() : v[j]->dev_values_wo());
        return a;
    }
    static void batch_exit(const char *message)
    {
        std::cout << message << std::endl;
        exit(1);
    }
    /* the size rules of mvm_scaleAndAdd, vector by vector; r == NULL: the in-place form */
    void check_fused_batch(const CloverVector16 *const *x, const CloverVector16 *const *u, CloverVector16 *const *t, CloverVector16 *const *r,
                           uint64_t count) const
    {
        for (uint64_t j = 0; j < count; j++) {
            if (x[j]->size_pad() != getCols() || t[j]->size_pad() != getRows()) batch_exit("MVM can not be performed. Exiting ...");
            if (u[j]->size_pad() != getRows() || (r && r[j]->size_pad() != getRows())) batch_exit("Vectors do not have the same size. Exiting ...");
        }
    }
    void check_transpose(const CloverMatrix16 &other) const
    {
        if (other.rows != cols || other.cols != rows) {
            std::cout << "Matrix can not be transposed. Exiting ..." << std::endl;
            exit(1);
        }
    }

public:
    CloverMatrix16(uint64_t h, uint64_t w)
        : rows(clover_hip::round_up(h, CLOVER_VECTOR_SIZE_PAD)), cols(clover_hip::round_up(w, CLOVER_VECTOR_SIZE_PAD))
    {
        mem.allocate(rows * cols * sizeof(uint16_t));
    }

    uint64_t getRows() const { return rows; }
    uint64_t getCols() const { return cols; }
    uint64_t size() const { return rows * cols; }
    uint64_t getBitsLength() const { return 16; }
    uint64_t getBytes() const { return rows * cols * sizeof(uint16_t); }

    /* explicit residency, as CloverMatrix4 (clover_device.h, -DCLOVER_HIP_EXPLICIT_SYNC) */
    void toDevice() const { (void)mem.dev_ro(); }
    void toHost() const { (void)mem.host_ro(); }
    uint16_t *getData() const { return reinterpret_cast<uint16_t *>(mem.host_ptr()); }

    /* :88-96 */
    float get(uint64_t i, uint64_t j) const { return clover_hip::half::to_f32(values_ro()[i * cols + j]); }
    void set(uint64_t i, uint64_t j, float value) { values_rw()[i * cols + j] = clover_hip::half::from_f32(value); }
    void clear() { memset(values_rw(), 0, getBytes()); }
    /* :74-86: the raw bit patterns row by row */
    std::string toString() const
    {
        const uint16_t *v = values_ro();
        std::stringstream sout;
        for (uint64_t i = 0; i < rows; i++) {
            for (uint64_t j = 0; j < cols; j++) sout << v[i * cols + j] << " ";
            sout << ";" << std::endl;
        }
        return sout.str();
    }

    void quantize(const CloverMatrix32 &m)
    {
        check_same_size(m);
        clover_hip::check(clm_f16_quantize(m.device_ro(), rows, cols, reinterpret_cast<uint16_t *>(mem.dev_wo()), nullptr),
                          "CloverMatrix16::quantize");
    }
    void quantize_parallel(const CloverMatrix32 &m) { quantize(m); }
    void quantize_scalar(const CloverMatrix32 &m)
    {
        check_same_size(m);
        const float *u = m.host_ro();
        uint16_t *r = values_rw();
        for (uint64_t i = 0; i < rows * cols; i++) r[i] = clover_hip::half::from_f32(u[i]);
    }

    /* f16 vector in, f16 vector out */
    void mvm(const CloverVector16 &productVector, CloverVector16 &resultVector) const
    {
        check_mvm(productVector, resultVector);
        clover_hip::check(clm_f16_mvm(dev_values(), rows, cols, productVector.dev_values_ro(), resultVector.dev_values_wo(), nullptr),
                          "CloverMatrix16::mvm");
        resultVector.commit();
    }
    void mvm_parallel(const CloverVector16 &productVector, CloverVector16 &resultVector) const { mvm(productVector, resultVector); }
    /* Not in the reference: t = this * x immediately followed by r = f16(u + a * t), the pair of steps the IHT / GD loops repeat
     * (01_measure.h:940-941, :942-943), as CloverMatrix8::mvm_scaleAndAdd: one launch, the bits of mvm(x, t); u.scaleAndAdd(t, a, r). */
    void mvm_scaleAndAdd(const CloverVector16 &x, const CloverVector16 &u, float a, CloverVector16 &t, CloverVector16 &r) const
    {
        check_mvm(x, t);
        if (u.size_pad() != getRows() || r.size_pad() != getRows()) { std::cout << "Vectors do not have the same size. Exiting ..." << std::endl; exit(1); }
        clover_hip::check(clm_f16_mvm_scale_and_add(dev_values(), rows, cols, x.dev_values_ro(), u.dev_values_ro(), a, t.dev_values_wo(),
                                                    r.dev_values_wo(), nullptr), "CloverMatrix16::mvm_scaleAndAdd");
        t.commit();
        r.commit();
    }
    /* in place: u = f16(u + a * (this * x)) */
    void mvm_scaleAndAdd(const CloverVector16 &x, CloverVector16 &u, float a, CloverVector16 &t) const
    {
        check_mvm(x, t);
        if (u.size_pad() != getRows()) { std::cout << "Vectors do not have the same size. Exiting ..." << std::endl; exit(1); }
        uint16_t *du = u.dev_values_rw();
        clover_hip::check(clm_f16_mvm_scale_and_add(dev_values(), rows, cols, x.dev_values_ro(), du, a, t.dev_values_wo(), du, nullptr),
                          "CloverMatrix16::mvm_scaleAndAdd");
        t.commit();
        u.commit();
    }
    /* The WHOLE IHT / GD loop of 01_measure.h:923-946, 999-1021 with this matrix as Phi, in one call (clm_f16_iht): x.clear(), then
     * `iterations` times t1 = Phi x; t2 = y - t1; t3 = PhiT t2; x += mu t3; [threshold(K)] -- three launches per iteration (two without
     * threshold), the bits of the five method calls.  The threshold is the one x.threshold_parallel(K) would take under the exactness
     * switch (default: the reference's survivors). */
    void iht_loop(const CloverMatrix16 &PhiT, CloverVector16 &x, const CloverVector16 &y, CloverVector16 &t1, CloverVector16 &t2,
                  CloverVector16 &t3, uint64_t iterations, uint64_t K, float mu, bool with_threshold) const
    {
        if (PhiT.getRows() != getCols() || PhiT.getCols() != getRows() || x.size_pad() != getCols() || y.size_pad() != getRows() ||
            t1.size_pad() != getRows() || t2.size_pad() != getRows() || t3.size_pad() != getCols()) {
            std::cout << "MVM can not be performed. Exiting ..." << std::endl;
            exit(1);
        }
        const int thr = !with_threshold ? 0 : (clover_hip::threshold_mode() == CLV_THRESHOLD_FAST ? 1 : 2);
        clover_hip::check(clm_f16_iht(dev_values(), PhiT.dev_values(), rows, cols, x.dev_values_wo(), x.size(), y.dev_values_ro(),
                                      t1.dev_values_wo(), t2.dev_values_wo(), t3.dev_values_wo(), iterations, K, mu, thr, nullptr),
                          "CloverMatrix16::iht_loop");
        x.commit();
        if (iterations) { t1.commit(); t2.commit(); t3.commit(); }
    }
    /* Not in the reference: resultVector = this' * productVector from this matrix's own bytes (clm_f16_mvm_transposed), bit for bit what
     * transpose(T); T.mvm(productVector, resultVector) gives, without the second matrix. */
    void mvm_transposed(const CloverVector16 &productVector, CloverVector16 &resultVector) const
    {
        check_mvm_transposed(productVector, resultVector);
        clover_hip::check(clm_f16_mvm_transposed(dev_values(), rows, cols, productVector.dev_values_ro(), resultVector.dev_values_wo(), nullptr),
                          "CloverMatrix16::mvm_transposed");
        resultVector.commit();
    }
    /* fp32 vector in, fp32 vector out (clm_f16_mvm_f32_transposed): the bits of transpose(T); T.mvm(productVector, resultVector) */
    void mvm_transposed(const CloverVector32 &productVector, CloverVector32 &resultVector) const
    {
        check_mvm_transposed(productVector, resultVector);
        clover_hip::check(clm_f16_mvm_f32_transposed(dev_values(), rows, cols, productVector.device_ro(), resultVector.device_wo(), nullptr),
                          "CloverMatrix16::mvm_transposed");
        resultVector.commit();
    }
    /* t = this' * x immediately followed by r = f16(u + a * t) (clm_f16_mvm_transposed_scale_and_add): one launch, the bits of
     * transpose(T); T.mvm_scaleAndAdd(x, u, a, t, r) */
    void mvm_transposed_scaleAndAdd(const CloverVector16 &x, const CloverVector16 &u, float a, CloverVector16 &t, CloverVector16 &r) const
    {
        check_mvm_transposed(x, t);
        if (u.size_pad() != getCols() || r.size_pad() != getCols()) { std::cout << "Vectors do not have the same size. Exiting ..." << std::endl; exit(1); }
        clover_hip::check(clm_f16_mvm_transposed_scale_and_add(dev_values(), rows, cols, x.dev_values_ro(), u.dev_values_ro(), a, t.dev_values_wo(),
                                                               r.dev_values_wo(), nullptr), "CloverMatrix16::mvm_transposed_scaleAndAdd");
        t.commit();
        r.commit();
    }
    /* in place: u = f16(u + a * (this' * x)) */
    void mvm_transposed_scaleAndAdd(const CloverVector16 &x, CloverVector16 &u, float a, CloverVector16 &t) const
    {
        check_mvm_transposed(x, t);
        if (u.size_pad() != getCols()) { std::cout << "Vectors do not have the same size. Exiting ..." << std::endl; exit(1); }
        uint16_t *du = u.dev_values_rw();
        clover_hip::check(clm_f16_mvm_transposed_scale_and_add(dev_values(), rows, cols, x.dev_values_ro(), du, a, t.dev_values_wo(), du, nullptr),
                          "CloverMatrix16::mvm_transposed_scaleAndAdd");
        t.commit();
        u.commit();
    }
    /* iht_loop with no PhiT (clm_f16_iht_one_matrix): the bits of iht_loop with PhiT = transpose of this, the same three launches per
     * iteration (two without threshold), half the resident matrix bytes; DESIGN.md 3 has what that costs per iteration. */
    void iht_loop_one_matrix(CloverVector16 &x, const CloverVector16 &y, CloverVector16 &t1, CloverVector16 &t2, CloverVector16 &t3,
                             uint64_t iterations, uint64_t K, float mu, bool with_threshold) const
    {
        if (x.size_pad() != getCols() || y.size_pad() != getRows() || t1.size_pad() != getRows() || t2.size_pad() != getRows() ||
            t3.size_pad() != getCols()) {
            std::cout << "MVM can not be performed. Exiting ..." << std::endl;
            exit(1);
        }
        const int thr = !with_threshold ? 0 : (clover_hip::threshold_mode() == CLV_THRESHOLD_FAST ? 1 : 2);
        clover_hip::check(clm_f16_iht_one_matrix(dev_values(), rows, cols, x.dev_values_wo(), x.size(), y.dev_values_ro(), t1.dev_values_wo(),
                                                 t2.dev_values_wo(), t3.dev_values_wo(), iterations, K, mu, thr, nullptr),
                          "CloverMatrix16::iht_loop_one_matrix");
        x.commit();
        if (iterations) { t1.commit(); t2.commit(); t3.commit(); }
    }
    /* Not in the reference: this * x[j] for `count` vectors in ONE pass over the matrix per group of CLM4_MVM_BATCH_MAX (clm_f16_mvm_batch);
     * r[j] equals what mvm(*x[j], *r[j]) gives, bit for bit.  The x[j] may repeat; the r[j] are distinct and none of them is an x. */
    void mvm_batch(const CloverVector16 *const *x, CloverVector16 *const *r, uint64_t count) const
    {
        for (uint64_t j = 0; j < count; j++)
            if (x[j]->size_pad() != getCols() || r[j]->size_pad() != getRows()) batch_exit("MVM can not be performed. Exiting ...");
        const DevArray px = dev_inputs(x, count), pr = dev_outputs(r, count, false);
        clover_hip::check(clm_f16_mvm_batch(dev_values(), rows, cols, count, px.data(), pr.data(), nullptr), "CloverMatrix16::mvm_batch");
        for (uint64_t j = 0; j < count; j++) r[j]->commit();
    }
    /* mvm_scaleAndAdd for `count` vectors: t[j] = this * x[j], r[j] = f16(u[j] + a * t[j]), the matrix read once per group
     * (clm_f16_mvm_scale_and_add_batch); the bits of the loop of mvm_scaleAndAdd. */
    void mvm_scaleAndAdd_batch(const CloverVector16 *const *x, const CloverVector16 *const *u, float a, CloverVector16 *const *t,
                               CloverVector16 *const *r, uint64_t count) const
    {
        check_fused_batch(x, u, t, r, count);
        const DevArray px = dev_inputs(x, count), pu = dev_inputs(u, count), pt = dev_outputs(t, count, false), pr = dev_outputs(r, count, false);
        clover_hip::check(clm_f16_mvm_scale_and_add_batch(dev_values(), rows, cols, count, px.data(), pu.data(), a, pt.data(), pr.data(), nullptr),
                          "CloverMatrix16::mvm_scaleAndAdd_batch");
        for (uint64_t j = 0; j < count; j++) { t[j]->commit(); r[j]->commit(); }
    }
    /* in place: u[j] = f16(u[j] + a * (this * x[j])); u[j] is mapped read-write and is both the call's u and its r */
    void mvm_scaleAndAdd_batch(const CloverVector16 *const *x, CloverVector16 *const *u, float a, CloverVector16 *const *t, uint64_t count) const
    {
        check_fused_batch(x, u, t, nullptr, count);
        const DevArray px = dev_inputs(x, count), pu = dev_outputs(u, count, true), pt = dev_outputs(t, count, false);
        clover_hip::check(clm_f16_mvm_scale_and_add_batch(dev_values(), rows, cols, count, px.data(), pu.data(), a, pt.data(), pu.data(), nullptr),
                          "CloverMatrix16::mvm_scaleAndAdd_batch");
        for (uint64_t j = 0; j < count; j++) { t[j]->commit(); u[j]->commit(); }
    }
    /* iht_loop for `count` signals with this matrix as Phi (clm_f16_iht_batch): per iteration every step runs once for a group of signals;
     * x[j], t1[j], t2[j], t3[j] end as iht_loop(PhiT, *x[j], *y[j], ...) leaves them, bit for bit.  All x[j] have one size(). */
    void iht_loop_batch(const CloverMatrix16 &PhiT, CloverVector16 *const *x, const CloverVector16 *const *y, CloverVector16 *const *t1,
                        CloverVector16 *const *t2, CloverVector16 *const *t3, uint64_t count, uint64_t iterations, uint64_t K, float mu,
                        bool with_threshold) const
    {
        for (uint64_t j = 0; j < count; j++)
            if (PhiT.getRows() != getCols() || PhiT.getCols() != getRows() || x[j]->size_pad() != getCols() || y[j]->size_pad() != getRows() ||
                t1[j]->size_pad() != getRows() || t2[j]->size_pad() != getRows() || t3[j]->size_pad() != getCols() || x[j]->size() != x[0]->size())
                batch_exit("MVM can not be performed. Exiting ...");
        const DevArray py = dev_inputs(y, count), px = dev_outputs(x, count, false), p1 = dev_outputs(t1, count, false),
                       p2 = dev_outputs(t2, count, false), p3 = dev_outputs(t3, count, false);
        const int thr = !with_threshold ? 0 : (clover_hip::threshold_mode() == CLV_THRESHOLD_FAST ? 1 : 2);
        clover_hip::check(clm_f16_iht_batch(dev_values(), PhiT.dev_values(), rows, cols, count, px.data(), count ? x[0]->size() : 0, py.data(),
                                            p1.data(), p2.data(), p3.data(), iterations, K, mu, thr, nullptr), "CloverMatrix16::iht_loop_batch");
        for (uint64_t j = 0; j < count; j++) {
            x[j]->commit();
            if (iterations) { t1[j]->commit(); t2[j]->commit(); t3[j]->commit(); }
        }
    }
    /* the size rules of mvm_transposed_scaleAndAdd, vector by vector; r == NULL: the in-place form */
    void check_fused_transposed_batch(const CloverVector16 *const *x, const CloverVector16 *const *u, CloverVector16 *const *t,
                                      CloverVector16 *const *r, uint64_t count) const
    {
        for (uint64_t j = 0; j < count; j++) {
            check_mvm_transposed(*x[j], *t[j]);
            if (u[j]->size_pad() != getCols() || (r && r[j]->size_pad() != getCols())) batch_exit("Vectors do not have the same size. Exiting ...");
        }
    }
    /* Not in the reference: this' * x[j] for `count` vectors in ONE pass over this matrix's own bytes per group of CLM4_MVM_BATCH_MAX
     * (clm_f16_mvm_transposed_batch); r[j] equals what mvm_transposed(*x[j], *r[j]) gives, bit for bit.  The x[j] may repeat; the r[j]
     * are distinct and none of them is an x. */
    void mvm_transposed_batch(const CloverVector16 *const *x, CloverVector16 *const *r, uint64_t count) const
    {
        for (uint64_t j = 0; j < count; j++) check_mvm_transposed(*x[j], *r[j]);
        const DevArray px = dev_inputs(x, count), pr = dev_outputs(r, count, false);
        clover_hip::check(clm_f16_mvm_transposed_batch(dev_values(), rows, cols, count, px.data(), pr.data(), nullptr),
                          "CloverMatrix16::mvm_transposed_batch");
        for (uint64_t j = 0; j < count; j++) r[j]->commit();
    }
    /* mvm_transposed_scaleAndAdd for `count` vectors: t[j] = this' * x[j], r[j] = f16(u[j] + a * t[j]), the matrix read once per group
     * (clm_f16_mvm_transposed_scale_and_add_batch); the bits of the loop of mvm_transposed_scaleAndAdd. */
    void mvm_transposed_scaleAndAdd_batch(const CloverVector16 *const *x, const CloverVector16 *const *u, float a, CloverVector16 *const *t,
                                          CloverVector16 *const *r, uint64_t count) const
    {
        check_fused_transposed_batch(x, u, t, r, count);
        const DevArray px = dev_inputs(x, count), pu = dev_inputs(u, count), pt = dev_outputs(t, count, false), pr = dev_outputs(r, count, false);
        clover_hip::check(clm_f16_mvm_transposed_scale_and_add_batch(dev_values(), rows, cols, count, px.data(), pu.data(), a, pt.data(), pr.data(),
                                                                     nullptr), "CloverMatrix16::mvm_transposed_scaleAndAdd_batch");
        for (uint64_t j = 0; j < count; j++) { t[j]->commit(); r[j]->commit(); }
    }
    /* in place: u[j] = f16(u[j] + a * (this' * x[j])); u[j] is mapped read-write and is both the call's u and its r */
    void mvm_transposed_scaleAndAdd_batch(const CloverVector16 *const *x, CloverVector16 *const *u, float a, CloverVector16 *const *t,
                                          uint64_t count) const
    {
        check_fused_transposed_batch(x, u, t, nullptr, count);
        const DevArray px = dev_inputs(x, count), pu = dev_outputs(u, count, true), pt = dev_outputs(t, count, false);
        clover_hip::check(clm_f16_mvm_transposed_scale_and_add_batch(dev_values(), rows, cols, count, px.data(), pu.data(), a, pt.data(), pu.data(),
                                                                     nullptr), "CloverMatrix16::mvm_transposed_scaleAndAdd_batch");
        for (uint64_t j = 0; j < count; j++) { t[j]->commit(); u[j]->commit(); }
    }
    /* iht_loop_batch with no PhiT (clm_f16_iht_batch_one_matrix): x[j], t1[j], t2[j], t3[j] end as iht_loop_one_matrix(*x[j], *y[j], ...)
     * leaves them, bit for bit; half the resident matrix bytes.  All x[j] have one size(). */
    void iht_loop_batch_one_matrix(CloverVector16 *const *x, const CloverVector16 *const *y, CloverVector16 *const *t1, CloverVector16 *const *t2,
                                   CloverVector16 *const *t3, uint64_t count, uint64_t iterations, uint64_t K, float mu, bool with_threshold) const
    {
        for (uint64_t j = 0; j < count; j++)
            if (x[j]->size_pad() != getCols() || y[j]->size_pad() != getRows() || t1[j]->size_pad() != getRows() || t2[j]->size_pad() != getRows() ||
                t3[j]->size_pad() != getCols() || x[j]->size() != x[0]->size())
                batch_exit("MVM can not be performed. Exiting ...");
        const DevArray py = dev_inputs(y, count), px = dev_outputs(x, count, false), p1 = dev_outputs(t1, count, false),
                       p2 = dev_outputs(t2, count, false), p3 = dev_outputs(t3, count, false);
        const int thr = !with_threshold ? 0 : (clover_hip::threshold_mode() == CLV_THRESHOLD_FAST ? 1 : 2);
        clover_hip::check(clm_f16_iht_batch_one_matrix(dev_values(), rows, cols, count, px.data(), count ? x[0]->size() : 0, py.data(), p1.data(),
                                                       p2.data(), p3.data(), iterations, K, mu, thr, nullptr),
                          "CloverMatrix16::iht_loop_batch_one_matrix");
        for (uint64_t j = 0; j < count; j++) {
            x[j]->commit();
            if (iterations) { t1[j]->commit(); t2[j]->commit(); t3[j]->commit(); }
        }
    }
    /* :98-131: one running fp32 sum of separately rounded products per row, rounded to f16 */
    void mvm_scalar(const CloverVector16 &productVector, CloverVector16 &resultVector) const
    {
        check_mvm(productVector, resultVector);
        const uint16_t *A = values_ro(), *x = productVector.values_ro();
        uint16_t *y = resultVector.values_rw();
        for (uint64_t i = 0; i < rows; i++) {
            float y_i = 0;
            for (uint64_t j = 0; j < cols; j++) y_i += clover_hip::half::to_f32(A[i * cols + j]) * clover_hip::half::to_f32(x[j]);
            y[i] = clover_hip::half::from_f32(y_i);
        }
    }

    /* fp32 vector in, fp32 vector out */
    void mvm(const CloverVector32 &productVector, CloverVector32 &resultVector) const
    {
        check_mvm(productVector, resultVector);
        clover_hip::check(clm_f16_mvm_f32(dev_values(), rows, cols, productVector.device_ro(), resultVector.device_wo(), nullptr),
                          "CloverMatrix16::mvm");
        resultVector.commit();
    }
    void mvm_parallel(const CloverVector32 &productVector, CloverVector32 &resultVector) const { mvm(productVector, resultVector); }
    /* :310-319: double accumulation on the host */
    void mvm_scalar(const CloverVector32 &productVector, CloverVector32 &resultVector) const
    {
        check_mvm(productVector, resultVector);
        for (uint64_t i = 0; i < rows; i++) {
            double sum = 0;
            for (uint64_t j = 0; j < cols; j++) sum += (double)get(i, j) * (double)productVector.get(j);
            resultVector.set(i, (float)sum);
        }
    }

    /* other = this^T */
    void transpose(CloverMatrix16 &other) const
    {
        check_transpose(other);
        clover_hip::check(clm_f16_transpose(dev_values(), rows, cols, reinterpret_cast<uint16_t *>(other.mem.dev_wo()), nullptr),
                          "CloverMatrix16::transpose");
    }
    void transpose_parallel(CloverMatrix16 &other) const { transpose(other); }
    void transpose_scalar(CloverMatrix16 &other) const
    {
        check_transpose(other);
        const uint16_t *u = values_ro();
        uint16_t *v = other.values_rw();
        for (uint64_t i = 0; i < rows; i++)
            for (uint64_t j = 0; j < cols; j++) v[j * rows + i] = u[i * cols + j];
    }
};

#endif
