/*
 * CloverMatrix32.h -- fp32 row-major matrix container: the input of CloverMatrix4::quantize and the
 * output of CloverMatrix4::gemm.  Mirrors the storage part of the reference's include/CloverMatrix32.h
 * (:43-73; rows and cols padded to multiples of 128 by CloverMatrix.h:48-53, contents uninitialised).
 * The class's own fp32 arithmetic -- mvm (MKL sgemv there), transpose (IPP / MKL there), quantize = copy -- is by default provided on
 * the HOST (clover_fp32.h): the baseline the 4-bit results are compared with.
 *
 * -DCLOVER_FP32_ON_DEVICE (opt-in, see CloverVector32.h) routes it to the device with the bits of the host loops:
 *   mvm / mvm_parallel              -> clm_f32_mvm
 *   transpose / transpose_parallel  -> clm_f32_transpose
 *   mvm_scaleAndAdd                 -> clm_f32_mvm_scale_and_add  (not in the reference: mvm + the scaleAndAdd behind it, one launch)
 *   iht_loop                        -> clm_f32_iht  (the whole Q_IHT / Q_GD loop of 01_measure.h:923-946, 999-1021 in one call)
 * Q_IHT<CloverMatrix32, CloverVector32> and Q_GD<...> are then specialised in CloverIHT.h and call iht_loop.  mvm_scalar,
 * transpose_scalar, quantize, clear and the random fills stay host code.
 */
#ifndef CLOVER_MATRIX32_H
#define CLOVER_MATRIX32_H

#include <iomanip>
#include <iostream>
#include <sstream>
#include <string>

#include "CloverVector32.h"

class CloverMatrix32 {
protected:
    const uint64_t rows;
    const uint64_t cols;
    mutable clover_hip::Mirror mem;

public:
    CloverMatrix32(uint64_t h, uint64_t w)
        : rows(clover_hip::round_up(h, CLOVER_VECTOR_SIZE_PAD)), cols(clover_hip::round_up(w, CLOVER_VECTOR_SIZE_PAD))
    {
        mem.allocate(rows * cols * sizeof(float));
    }

    uint64_t getRows() const { return rows; }
    uint64_t getCols() const { return cols; }
    uint64_t size() const { return rows * cols; }
    uint64_t getBitsLength() const { return 32; }
    uint64_t getBytes() const { return rows * cols * sizeof(float); }

    /* Explicit residency (clover_device.h, -DCLOVER_HIP_EXPLICIT_SYNC): move the bytes NOW instead of at the next use.  toDevice(): upload
     * if the host copy is the newer one; toHost(): bring a device result back.  Optional in every build (the default build's page tracking
     * and all accessors synchronise by themselves); not in the reference, which has one copy. */
    void toDevice() const { (void)mem.dev_ro(); }
    void toHost() const { (void)mem.host_ro(); }
    float *getData() const { return reinterpret_cast<float *>(mem.host_ptr()); }      /* stays valid and current (clover_device.h) */
    float get(uint64_t i, uint64_t j) const { return reinterpret_cast<const float *>(mem.host_ro())[i * cols + j]; }
    void set(uint64_t i, uint64_t j, float v) { reinterpret_cast<float *>(mem.host_rw())[i * cols + j] = v; }
    void clear() { memset(mem.host_rw(), 0, rows * cols * sizeof(float)); }

    /* ---- fp32 arithmetic (clover_fp32.h on the host; CloverMatrix32.h:90-215) ---- */
    /* result = A * productVector; shape mismatch: message + exit(1) as the reference (:109-113) */
#ifdef CLOVER_FP32_ON_DEVICE
    void mvm(const CloverVector32 &productVector, CloverVector32 &result) const
    {
        check_mvm(productVector, result);
        clover_hip::check(clm_f32_mvm(device_ro(), rows, cols, productVector.device_ro(), result.device_wo(), nullptr), "CloverMatrix32::mvm");
        result.commit();
    }
    void mvm_parallel(const CloverVector32 &productVector, CloverVector32 &result) const { mvm(productVector, result); }
    /* Not in the reference: t = this * x immediately followed by r = u + a * t, the pair of steps the IHT / GD loops repeat
     * (01_measure.h:940-941, :942-943), as CloverMatrix16::mvm_scaleAndAdd: one launch, the bits of mvm(x, t); u.scaleAndAdd(t, a, r). */
    void mvm_scaleAndAdd(const CloverVector32 &x, const CloverVector32 &u, float a, CloverVector32 &t, CloverVector32 &r) const
    {
        check_mvm(x, t);
        if (u.size_pad() != rows || r.size_pad() != rows) { std::cout << "Vectors do not have the same size. Exiting ..." << std::endl; exit(1); }
        clover_hip::check(clm_f32_mvm_scale_and_add(device_ro(), rows, cols, x.device_ro(), u.device_ro(), a, t.device_wo(), r.device_wo(), nullptr),
                          "CloverMatrix32::mvm_scaleAndAdd");
        t.commit();
        r.commit();
    }
    /* in place: u = u + a * (this * x) */
    void mvm_scaleAndAdd(const CloverVector32 &x, CloverVector32 &u, float a, CloverVector32 &t) const
    {
        check_mvm(x, t);
        if (u.size_pad() != rows) { std::cout << "Vectors do not have the same size. Exiting ..." << std::endl; exit(1); }
        float *du = u.device_rw();
        clover_hip::check(clm_f32_mvm_scale_and_add(device_ro(), rows, cols, x.device_ro(), du, a, t.device_wo(), du, nullptr),
                          "CloverMatrix32::mvm_scaleAndAdd");
        t.commit();
        u.commit();
    }
    /* The WHOLE IHT / GD loop of 01_measure.h:923-946, 999-1021 with this matrix as Phi, in one call (clm_f32_iht): x.clear(), then
     * `iterations` times t1 = Phi x; t2 = y - t1; t3 = PhiT t2; x += mu t3; [threshold(K)] -- three launches per iteration (two without
     * threshold), the bits of the five method calls.  The threshold is the one x.threshold_parallel(K) would take under the exactness
     * switch (default: the reference's survivors). */
    void iht_loop(const CloverMatrix32 &PhiT, CloverVector32 &x, const CloverVector32 &y, CloverVector32 &t1, CloverVector32 &t2,
                  CloverVector32 &t3, uint64_t iterations, uint64_t K, float mu, bool with_threshold) const
    {
        if (PhiT.rows != cols || PhiT.cols != rows || x.size_pad() != cols || y.size_pad() != rows || t1.size_pad() != rows ||
            t2.size_pad() != rows || t3.size_pad() != cols) {
            std::cout << "MVM can not be performed. Exiting ..." << std::endl;
            exit(1);
        }
        const int thr = !with_threshold ? 0 : (clover_hip::threshold_mode() == CLV_THRESHOLD_FAST ? 1 : 2);
        clover_hip::check(clm_f32_iht(device_ro(), PhiT.device_ro(), rows, cols, x.device_wo(), x.size(), y.device_ro(), t1.device_wo(),
                                      t2.device_wo(), t3.device_wo(), iterations, K, mu, thr, nullptr), "CloverMatrix32::iht_loop");
        x.commit();
        if (iterations) { t1.commit(); t2.commit(); t3.commit(); }
    }
    /* other (cols x rows) = this transposed */
    void transpose(CloverMatrix32 &other) const
    {
        if (other.rows != cols || other.cols != rows) { std::cout << "Matrices do not have transposed shapes. Exiting ..." << std::endl; exit(1); }
        clover_hip::check(clm_f32_transpose(device_ro(), rows, cols, other.device_wo(), nullptr), "CloverMatrix32::transpose");
        other.mem.commit();
    }
    void transpose_parallel(CloverMatrix32 &other) const { transpose(other); }
#else
    void mvm(const CloverVector32 &productVector, CloverVector32 &result) const { mvm_host(productVector, result, false); }
    void mvm_parallel(const CloverVector32 &productVector, CloverVector32 &result) const { mvm_host(productVector, result, true); }
    /* other (cols x rows) = this transposed */
    void transpose(CloverMatrix32 &other) const { clover_fp32::transpose(host_ro(), rows, cols, other.host_rw(), false); }
    void transpose_parallel(CloverMatrix32 &other) const { clover_fp32::transpose(host_ro(), rows, cols, other.host_rw(), true); }
#endif
    void mvm_scalar(const CloverVector32 &productVector, CloverVector32 &result) const { mvm_host(productVector, result, false); }
    void quantize(const CloverMatrix32 &other) { memcpy(mem.host_rw(), other.mem.host_ro(), rows * cols * sizeof(float)); }
    void transpose_scalar(CloverMatrix32 &other) const { clover_fp32::transpose(host_ro(), rows, cols, other.host_rw(), false); }
    void setRandomFloats(float min_value, float max_value, uint64_t seed = 0x9E3779B97F4A7C15ull)
    {
        clover_fp32::fill_uniform(reinterpret_cast<float *>(mem.host_rw()), rows * cols, min_value, max_value, seed);
    }

    void setRandomInteger(float max_value, uint64_t seed = 0x9E3779B97F4A7C15ull)
    {
        CloverVector32 view(rows * cols, reinterpret_cast<float *>(mem.host_rw()));      /* non-owning view over the same buffer */
        view.setRandomInteger(max_value, seed);
    }

    std::string toString() const
    {
        std::stringstream sout;
        for (uint64_t i = 0; i < rows; i++) {
            for (uint64_t j = 0; j < cols; j++) sout << std::setw(7) << std::setprecision(2) << get(i, j) << " ";
            sout << ";" << std::endl;
        }
        return sout.str();
    }

    /* host access for the scalar validation twins (clover_scalar.h) */
    const float *host_ro() const { return reinterpret_cast<const float *>(mem.host_ro()); }
    float *host_rw() { return reinterpret_cast<float *>(mem.host_rw()); }
    const float *device_ro() const { return reinterpret_cast<const float *>(mem.dev_ro()); }
    float *device_wo() { return reinterpret_cast<float *>(mem.dev_wo()); }

private:
#ifdef CLOVER_FP32_ON_DEVICE
    void check_mvm(const CloverVector32 &x, const CloverVector32 &result) const
    {
        if (x.size() != cols || result.size_pad() != rows) {
            std::cout << "Can't perform MVM: " << rows << " x " << cols << " Matrix times a " << x.size() << " vector to update a "
                      << result.size() << " vector. Exiting..." << std::endl;
            exit(1);
        }
    }
#endif
    void mvm_host(const CloverVector32 &x, CloverVector32 &result, bool team) const
    {
        if (x.size() != cols) {
            std::cout << "Can't perform MVM: " << rows << " x " << cols << " Matrix times a " << x.size() << " vector to update a "
                      << result.size() << " vector. Exiting..." << std::endl;
            exit(1);
        }
        clover_fp32::mvm_rows(host_ro(), rows, cols, x.host_ro(), result.host_rw(), team);
    }
};

#endif
