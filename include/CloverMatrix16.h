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
 *
 * Q_IHT<CloverMatrix16, CloverVector16> and Q_GD<...> are specialised in CloverIHT.h (which includes this header) and call iht_loop: every
 * step is a kernel on the device mirrors, nothing is copied back between steps.
 */
#ifndef CLOVER_MATRIX16_H
#define CLOVER_MATRIX16_H

#include <sstream>
#include <string>

#include "CloverMatrix32.h"
#include "CloverVector16.h"
#include "CloverVector32.h"

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
