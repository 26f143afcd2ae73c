/*
 * CloverMatrix8.h -- 8-bit quantized matrix, MI355X-backed.
 *
 * Drop-in for the reference's include/CloverMatrix8.h: same class name, constructor, method names and data format (row-major int8
 * values followed by a row-major grid of fp32 scales, one per 64x64 tile, value = q * scale / 127; rows/cols padded to multiples of
 * 128; :36-90).  Hot methods call libclover_hip.so:
 *
 *   quantize / quantize_parallel       -> clm8_quantize   (CloverMatrix8.h:203-480)
 *   restore                            -> clm8_restore    (get, :117-131; the reference has only restore_scalar, :1300-1309)
 *   mvm / mvm_parallel (CloverVector8) -> clm8_mvm        (:1002-1299, :664-998)
 *   mvm / mvm_parallel (CloverVector32)-> clm8_mvm_f32    (:558-662)
 *   transpose / transpose_parallel     -> clm8_transpose  (:1312-1386)
 *   *_scalar                           -> scalar HOST code, the reference's validation partners: quantize_scalar (:144-201),
 *                                         restore_scalar, mvm_scalar (:480-556: row views + CloverVector8::dot, then the scalar
 *                                         quantiser; for fp32 vectors a double accumulation), transpose_scalar (:1312-1340).  With
 *                                         rounding disabled mvm == mvm_parallel == mvm_scalar bit for bit, as in the reference.
 *
 *   mvm_scaleAndAdd                    -> clm8_mvm_scale_and_add  (not in the reference: mvm + the scaleAndAdd behind it, one launch)
 *   iht_loop                           -> clm8_iht        (the whole Q_IHT / Q_GD loop of 01_measure.h:923-946, 999-1021 in one call)
 *   mvm_transposed / mvm_transposed_scaleAndAdd / iht_loop_one_matrix
 *                                      -> clm8_mvm_transposed, clm8_mvm_transposed_scale_and_add, clm8_iht_one_matrix (not in the reference:
 *                                         this' * x from this matrix's own bytes, and the loop with no stored transpose)
 *   mvm_batch / mvm_batch_at / mvm_scaleAndAdd_batch / iht_loop_batch
 *                                      -> clm8_mvm_batch, clm8_mvm_batch_at, clm8_mvm_scale_and_add_batch, clm8_iht_batch (not in the
 *                                         reference: several vectors, ONE pass over the matrix per group of CLM4_MVM_BATCH_MAX)
 *   mvm_transposed_batch / mvm_transposed_batch_at / mvm_transposed_scaleAndAdd_batch / iht_loop_batch_one_matrix
 *                                      -> clm8_mvm_transposed_batch, clm8_mvm_transposed_batch_at, clm8_mvm_transposed_scale_and_add_batch,
 *                                         clm8_iht_batch_one_matrix (clover_hip_batch_t8.h; not in the reference: this' * x[j] for several
 *                                         vectors from this matrix's own bytes, and the batched loop with no stored transpose)
 *   gemm                               -> clm8_gemm       (not in the reference, which has no GEMM; semantics in DESIGN.md 6)
 *   mvm_transposed (CloverVector32)    -> clm8_mvm_f32_transposed (clover_hip_m8_f32.h; not in the reference: this' * x straight from this
 *                                         matrix's own bytes); under -DCLOVER_FP32_ON_DEVICE also mvm_scaleAndAdd,
 *                                         mvm_transposed_scaleAndAdd, iht_loop and iht_loop_one_matrix for CloverVector32 vectors
 *                                         (clm8_mvm_f32_scale_and_add, clm8_mvm_f32_transposed_scale_and_add, clm8_iht_f32,
 *                                         clm8_iht_f32_one_matrix)
 *
 * Q_IHT<CloverMatrix8, CloverVector8> and Q_GD<...> are specialised in CloverIHT.h (which includes this header): iht_loop when rounding is
 * deterministic, the mvm_scaleAndAdd pairs otherwise; every step is a kernel on the device mirrors, nothing is copied back between steps.
 */
#ifndef CLOVER_MATRIX8_H
#define CLOVER_MATRIX8_H

#include <cmath>
#include <iomanip>
#include <sstream>
#include <string>
#include <vector>

#include "CloverMatrix32.h"
#include "CloverVector32.h"
#include "CloverVector8.h"
#include "clover_batch.h"          /* what the batch methods share with CloverMatrix4's: the marshalling into the batched C calls */
#include "clover_hip_m8_f32.h"     /* this matrix on fp32 vectors: the fused step, this' * x, the fp32-vector IHT / GD loop */

class CloverMatrix4;

class CloverMatrix8 {
    friend class CloverMatrix4;                /* CloverMatrix4::gemm(const CloverMatrix8 &, ...) reads the device image */
protected:
    const uint64_t rows;
    const uint64_t cols;
    mutable clover_hip::Mirror mem;            /* [rows*cols value bytes][(rows/64)*(cols/64) scales] */
    mutable clover_hip::RandomState random;
    uint64_t value_bytes;

    const int8_t *dev_values() const { return reinterpret_cast<const int8_t *>(mem.dev_ro()); }
    const float *dev_scales() const { return reinterpret_cast<const float *>(mem.dev_ro() + value_bytes); }
    /* the bodies of the batch methods (clover_batch.h) and this matrix as they take it */
    typedef clover_hip::Batch<CloverMatrix8, clover_hip::BATCH_FORWARD> BatchForward;
    typedef clover_hip::Batch<CloverMatrix8, clover_hip::BATCH_TRANSPOSED> BatchTransposed;
    clover_hip::BatchMatrix batch_view() const
    {
        const clover_hip::BatchMatrix m = {dev_values(), dev_scales(), rows, cols};
        return m;
    }

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
        if (productVector.size() != getCols() || resultVector.size_pad() != getRows()) {
            std::cout << "MVM can not be performed. Exiting ..." << std::endl;
            exit(1);
        }
    }
    void check_transpose(const CloverMatrix8 &other) const
    {
        if (other.rows != cols || other.cols != rows) {
            std::cout << "Matrix can not be transposed. Exiting ..." << std::endl;
            exit(1);
        }
    }

public:
    CloverMatrix8(uint64_t h, uint64_t w)
        : rows(clover_hip::round_up(h, CLOVER_VECTOR_SIZE_PAD)), cols(clover_hip::round_up(w, CLOVER_VECTOR_SIZE_PAD))
    {
        value_bytes = rows * cols;
        mem.allocate(value_bytes + (rows >> 6) * (cols >> 6) * sizeof(float));
    }

    uint64_t getRows() const { return rows; }
    uint64_t getCols() const { return cols; }
    uint64_t size() const { return rows * cols; }
    uint64_t getBitsLength() const { return 8; }
    uint64_t getBytes() const { return value_bytes + (rows >> 6) * (cols >> 6) * sizeof(float); }

    /* explicit residency, as CloverMatrix4 (clover_device.h, -DCLOVER_HIP_EXPLICIT_SYNC) */
    void toDevice() const { (void)mem.dev_ro(); }
    void toHost() const { (void)mem.host_ro(); }
    /* host views of the values and of the tile scales (protected in the reference; exposed for interop) */
    int8_t *getData() const { return reinterpret_cast<int8_t *>(mem.host_ptr()); }
    float *getScales() const { return reinterpret_cast<float *>(mem.host_ptr() + value_bytes); }

    /* :117-131 */
    float get(uint64_t i, uint64_t j) const
    {
        const uint8_t *h = mem.host_ro();
        const float *s = reinterpret_cast<const float *>(h + value_bytes);
        const float scale = s[(i >> 6) * (cols >> 6) + (j >> 6)] / 127.0f;
        return scale * (float)(int8_t)h[i * cols + j];
    }

    /* :1388-1411: the restored elements row by row, then the grid of tile scales */
    std::string toString() const
    {
        const uint8_t *h = mem.host_ro();
        const float *s = reinterpret_cast<const float *>(h + value_bytes);
        const uint64_t v_blocks = rows >> 6, h_blocks = cols >> 6;
        std::stringstream sout;
        for (uint64_t i = 0; i < rows; i++) {
            for (uint64_t j = 0; j < cols; j++) sout << std::setw(7) << std::fixed << std::setprecision(2) << get(i, j) << " ";
            sout << ";" << std::endl;
        }
        for (uint64_t i = 0; i < v_blocks; i++) {
            for (uint64_t j = 0; j < h_blocks; j++) sout << std::setw(7) << std::fixed << std::setprecision(2) << s[i * h_blocks + j] << " ";
            sout << ";" << std::endl;
        }
        return sout.str();
    }

    void setRandomKeys(const uint64_t key1[4], const uint64_t key2[4]) { random.set(key1, key2); }
#ifdef CLOVER_HIP_M256_KEYS
    void setRandomKeys(__m256i key1, __m256i key2) { clover_hip::set_keys_m256(random, key1, key2); }   /* CloverRandom.h:90-94 */
#endif
    void seedRandomKeys(uint64_t key1, uint64_t key2) { random.seed(key1, key2); }
    /* the generator's present keys, read back from the device (for tests: as CloverMatrix4::getRandomKeys) */
    void getRandomKeys(uint64_t key1[4], uint64_t key2[4]) const { random.get(key1, key2); }

    void quantize(const CloverMatrix32 &m)
    {
        check_same_size(m);
        uint8_t *d = mem.dev_wo();
        clover_hip::check(clm8_quantize(m.device_ro(), rows, cols, reinterpret_cast<int8_t *>(d), reinterpret_cast<float *>(d + value_bytes),
                                        clover_hip::rng_or_null(random), nullptr), "CloverMatrix8::quantize");
    }
    void quantize_parallel(const CloverMatrix32 &m) { quantize(m); }
    /* the reference's scalar twin (:144-201), on the host: tiles column-block outer, maximum over the 64 x 64 tile */
    void quantize_scalar(const CloverMatrix32 &m)
    {
        check_same_size(m);
        const float *u = m.host_ro();
        uint8_t *h = mem.host_rw();
        int8_t *r = reinterpret_cast<int8_t *>(h);
        float *sr = reinterpret_cast<float *>(h + value_bytes);
        const uint64_t hb = cols >> 6, vb = rows >> 6;
        for (uint64_t bj = 0; bj < hb; bj++)
            for (uint64_t bi = 0; bi < vb; bi++) {
                const uint64_t off = (bi << 6) * cols + (bj << 6);
                float mx = 0.0f;
                for (uint64_t i = 0; i < 64; i++)
                    for (uint64_t j = 0; j < 64; j++) { const float a = std::fabs(u[off + i * cols + j]); if (a > mx) mx = a; }
                if (mx == 0.0f) mx = 1.0f;                         /* the SIMD contract (:262-270); the scalar code divides by zero */
                sr[bi * hb + bj] = mx;
                const float k = 127.0f / mx;
                for (uint64_t i = 0; i < 64; i++)
                    for (uint64_t j = 0; j < 64; j++) {
                        const float x = u[off + i * cols + j];
                        const float mag = std::floor(std::fma(std::fabs(x), k, clover_hip::scalar::noise()));
                        r[off + i * cols + j] = (int8_t)(std::signbit(x) ? -(int)mag : (int)mag);
                    }
            }
    }

    void restore(CloverMatrix32 &other) const
    {
        check_same_size(other);
        clover_hip::check(clm8_restore(dev_values(), dev_scales(), rows, cols, other.device_wo(), nullptr), "CloverMatrix8::restore");
    }
    void restore_scalar(CloverMatrix32 &other) const
    {
        check_same_size(other);
        float *out = other.host_rw();
        for (uint64_t i = 0; i < rows; i++)
            for (uint64_t j = 0; j < cols; j++) out[i * cols + j] = get(i, j);
    }

    /* 8-bit vector in, 8-bit vector out */
    void mvm(const CloverVector8 &productVector, CloverVector8 &resultVector)
    {
        check_mvm(productVector, resultVector);
        clover_hip::check(clm8_mvm(dev_values(), dev_scales(), rows, cols, productVector.dev_values_ro(), productVector.dev_scales_ro(),
                                   resultVector.dev_values_wo(), resultVector.dev_scales_wo(), clover_hip::rng_or_null(random), nullptr),
                          "CloverMatrix8::mvm");
        resultVector.commit();
    }
    void mvm_parallel(const CloverVector8 &productVector, CloverVector8 &resultVector) { mvm(productVector, resultVector); }
    /* Not in the reference: t = this * x immediately followed by r = quantize(u + a * t), the pair of steps the IHT / GD loops repeat
     * (01_measure.h:940-941, :942-943), as CloverMatrix4::mvm_scaleAndAdd.  One launch when rounding is deterministic; with stochastic
     * rounding the two steps draw from two objects' generators (the matrix's, then u's), as they do in the reference, and are issued as
     * the two calls.  Results are identical to mvm(x, t); u.scaleAndAdd(t, a, r) either way. */
    void mvm_scaleAndAdd(const CloverVector8 &x, const CloverVector8 &u, float a, CloverVector8 &t, CloverVector8 &r)
    {
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
        if (x.size() != getCols() || t.size_pad() != getRows()) { std::cout << "MVM can not be performed. Exiting ..." << std::endl; exit(1); }
        if (u.size_pad() != getRows() || r.size_pad() != getRows()) { std::cout << "Vectors do not have the same size. Exiting ..." << std::endl; exit(1); }
        clover_hip::check(clm8_mvm_scale_and_add(dev_values(), dev_scales(), rows, cols, x.dev_values_ro(), x.dev_scales_ro(),
                                                 u.dev_values_ro(), u.dev_scales_ro(), a, t.dev_values_wo(), t.dev_scales_wo(),
                                                 r.dev_values_wo(), r.dev_scales_wo(), nullptr, nullptr), "CloverMatrix8::mvm_scaleAndAdd");
        t.commit();
        r.commit();
#else
        mvm(x, t);
        const_cast<CloverVector8 &>(u).scaleAndAdd(t, a, r);
#endif
    }
    /* in place: u = quantize(u + a * (this * x)) */
    void mvm_scaleAndAdd(const CloverVector8 &x, CloverVector8 &u, float a, CloverVector8 &t)
    {
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
        if (x.size() != getCols() || t.size_pad() != getRows()) { std::cout << "MVM can not be performed. Exiting ..." << std::endl; exit(1); }
        if (u.size_pad() != getRows()) { std::cout << "Vectors do not have the same size. Exiting ..." << std::endl; exit(1); }
        int8_t *qu = u.dev_values_rw();
        float *su = u.dev_scales_rw();
        clover_hip::check(clm8_mvm_scale_and_add(dev_values(), dev_scales(), rows, cols, x.dev_values_ro(), x.dev_scales_ro(), qu, su, a,
                                                 t.dev_values_wo(), t.dev_scales_wo(), qu, su, nullptr, nullptr),
                          "CloverMatrix8::mvm_scaleAndAdd");
        t.commit();
        u.commit();
#else
        mvm(x, t);
        u.scaleAndAdd(t, a);
#endif
    }
    /* The WHOLE quantized IHT / GD loop of 01_measure.h:923-946, 999-1021 with this matrix as Phi, in one call (clm8_iht): x.clear(), then
     * `iterations` times t1 = Phi x; t2 = y - t1; t3 = PhiT t2; x += mu t3; [threshold(K)] -- three launches per iteration, same bits as
     * the five method calls.  Deterministic rounding only (each step of a stochastic loop draws from its own object's generator:
     * CloverIHT.h keeps the calls apart there). */
    void iht_loop(CloverMatrix8 &PhiT, CloverVector8 &x, const CloverVector8 &y, CloverVector8 &t1, CloverVector8 &t2, CloverVector8 &t3,
                  uint64_t iterations, uint64_t K, float mu, bool with_threshold)
    {
        if (PhiT.getRows() != getCols() || PhiT.getCols() != getRows() || x.size_pad() != getCols() || y.size_pad() != getRows() ||
            t1.size_pad() != getRows() || t2.size_pad() != getRows() || t3.size_pad() != getCols()) {
            std::cout << "MVM can not be performed. Exiting ..." << std::endl;
            exit(1);
        }
        const int thr = !with_threshold ? 0 : (clover_hip::threshold_mode() == CLV_THRESHOLD_FAST ? 1 : 2);
        clover_hip::check(clm8_iht(dev_values(), dev_scales(), PhiT.dev_values(), PhiT.dev_scales(), rows, cols, x.dev_values_wo(), x.dev_scales_wo(),
                                   x.size(), y.dev_values_ro(), y.dev_scales_ro(), t1.dev_values_wo(), t1.dev_scales_wo(), t2.dev_values_wo(),
                                   t2.dev_scales_wo(), t3.dev_values_wo(), t3.dev_scales_wo(), iterations, K, mu, thr, nullptr, nullptr),
                          "CloverMatrix8::iht_loop");
        x.commit();
        if (iterations) { t1.commit(); t2.commit(); t3.commit(); }
    }
    /* Not in the reference: mvm_transposed and its fused forms (clm8_mvm_transposed, clm8_mvm_transposed_scale_and_add): resultVector =
     * this' * productVector from this matrix's own bytes, bit for bit what transpose(T); T.mvm(productVector, resultVector) gives, with
     * stochastic rounding the draws from THIS matrix's generator included. */
    void mvm_transposed(const CloverVector8 &productVector, CloverVector8 &resultVector)
    {
        if (productVector.size() != getRows() || resultVector.size_pad() != getCols()) {
            std::cout << "MVM can not be performed. Exiting ..." << std::endl;
            exit(1);
        }
        clover_hip::check(clm8_mvm_transposed(dev_values(), dev_scales(), rows, cols, productVector.dev_values_ro(), productVector.dev_scales_ro(),
                                              resultVector.dev_values_wo(), resultVector.dev_scales_wo(), clover_hip::rng_or_null(random), nullptr),
                          "CloverMatrix8::mvm_transposed");
        resultVector.commit();
    }
    void check_fused_transposed(const CloverVector8 &x, const CloverVector8 &u, const CloverVector8 &t) const
    {
        if (x.size() != getRows() || t.size_pad() != getCols()) { std::cout << "MVM can not be performed. Exiting ..." << std::endl; exit(1); }
        if (u.size_pad() != getCols()) { std::cout << "Vectors do not have the same size. Exiting ..." << std::endl; exit(1); }
    }
    void mvm_transposed_scaleAndAdd(const CloverVector8 &x, const CloverVector8 &u, float a, CloverVector8 &t, CloverVector8 &r)
    {
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
        check_fused_transposed(x, u, t);
        if (r.size_pad() != getCols()) { std::cout << "Vectors do not have the same size. Exiting ..." << std::endl; exit(1); }
        clover_hip::check(clm8_mvm_transposed_scale_and_add(dev_values(), dev_scales(), rows, cols, x.dev_values_ro(), x.dev_scales_ro(),
                                                            u.dev_values_ro(), u.dev_scales_ro(), a, t.dev_values_wo(), t.dev_scales_wo(),
                                                            r.dev_values_wo(), r.dev_scales_wo(), nullptr, nullptr),
                          "CloverMatrix8::mvm_transposed_scaleAndAdd");
        t.commit();
        r.commit();
#else
        mvm_transposed(x, t);
        const_cast<CloverVector8 &>(u).scaleAndAdd(t, a, r);
#endif
    }
    /* in place: u = quantize(u + a * (this' * x)) */
    void mvm_transposed_scaleAndAdd(const CloverVector8 &x, CloverVector8 &u, float a, CloverVector8 &t)
    {
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
        check_fused_transposed(x, u, t);
        int8_t *qu = u.dev_values_rw();
        float *su = u.dev_scales_rw();
        clover_hip::check(clm8_mvm_transposed_scale_and_add(dev_values(), dev_scales(), rows, cols, x.dev_values_ro(), x.dev_scales_ro(), qu, su, a,
                                                            t.dev_values_wo(), t.dev_scales_wo(), qu, su, nullptr, nullptr),
                          "CloverMatrix8::mvm_transposed_scaleAndAdd");
        t.commit();
        u.commit();
#else
        mvm_transposed(x, t);
        u.scaleAndAdd(t, a);
#endif
    }
    /* iht_loop with no PhiT (clm8_iht_one_matrix): the bits of iht_loop with PhiT = transpose of this, the same three launches per
     * iteration.  Half the resident matrix bytes; DESIGN.md 3 has what that costs per iteration.  Deterministic rounding only, as iht_loop. */
    void iht_loop_one_matrix(CloverVector8 &x, const CloverVector8 &y, CloverVector8 &t1, CloverVector8 &t2, CloverVector8 &t3,
                             uint64_t iterations, uint64_t K, float mu, bool with_threshold)
    {
        if (x.size_pad() != getCols() || y.size_pad() != getRows() || t1.size_pad() != getRows() || t2.size_pad() != getRows() ||
            t3.size_pad() != getCols()) {
            std::cout << "MVM can not be performed. Exiting ..." << std::endl;
            exit(1);
        }
        const int thr = !with_threshold ? 0 : (clover_hip::threshold_mode() == CLV_THRESHOLD_FAST ? 1 : 2);
        clover_hip::check(clm8_iht_one_matrix(dev_values(), dev_scales(), rows, cols, x.dev_values_wo(), x.dev_scales_wo(), x.size(),
                                              y.dev_values_ro(), y.dev_scales_ro(), t1.dev_values_wo(), t1.dev_scales_wo(), t2.dev_values_wo(),
                                              t2.dev_scales_wo(), t3.dev_values_wo(), t3.dev_scales_wo(), iterations, K, mu, thr, nullptr, nullptr),
                          "CloverMatrix8::iht_loop_one_matrix");
        x.commit();
        if (iterations) { t1.commit(); t2.commit(); t3.commit(); }
    }
    /* Not in the reference: this * x[j] for `count` vectors in ONE pass over the matrix per group of CLM4_MVM_BATCH_MAX (clm8_mvm_batch);
     * r[j] equals what mvm(*x[j], *r[j]) gives, bit for bit.  The x[j] may repeat; the r[j] are distinct vectors, none of them an x.  With
     * stochastic rounding enabled the vectors draw from the matrix's generator one after another, as the single calls in order do -- still
     * one pass: the kernel jumps to every vector's place in the stream -- and the generator ends where those calls leave it. */
    void mvm_batch(const CloverVector8 *const *x, CloverVector8 *const *r, uint64_t count)
    {
        BatchForward::mvm(batch_view(), x, r, count, clover_hip::rng_or_null(random), false, 0, 0, 0, "CloverMatrix8::mvm_batch");
    }
    /* mvm_batch with the place of every vector's draws chosen by the caller (clm8_mvm_batch_at), counted in draws -- mvm consumes
     * 2 (rows / 64) -- from where the matrix's generator stands: vector j draws from draw_base + j * draw_stride on, and the generator is
     * advanced by commit_draws afterwards (0: left as it is).  For callers whose stream order is not vector after vector (Q_IHT_batch,
     * CloverIHT.h).  With rounding disabled the three numbers are ignored. */
    void mvm_batch_at(const CloverVector8 *const *x, CloverVector8 *const *r, uint64_t count, uint64_t draw_base, uint64_t draw_stride,
                      uint64_t commit_draws)
    {
        BatchForward::mvm(batch_view(), x, r, count, clover_hip::rng_or_null(random), true, draw_base, draw_stride, commit_draws,
                          "CloverMatrix8::mvm_batch_at");
    }
    /* mvm_scaleAndAdd for `count` vectors: t[j] = this * x[j], r[j] = quantize(u[j] + a * t[j]).  Rounding disabled: one launch per group
     * (clm8_mvm_scale_and_add_batch).  Stochastic: the mvm draws from the matrix's generator and every scaleAndAdd from its u[j]'s own, so
     * it is one mvm_batch and the scaleAndAdd calls -- the bits of the loop of mvm_scaleAndAdd, the matrix read once per group. */
    void mvm_scaleAndAdd_batch(const CloverVector8 *const *x, const CloverVector8 *const *u, float a, CloverVector8 *const *t,
                               CloverVector8 *const *r, uint64_t count)
    {
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
        BatchForward::fused(batch_view(), x, u, a, t, r, count, "CloverMatrix8::mvm_scaleAndAdd_batch");
#else
        clover_hip::batch_check_fused<CloverVector8>(cols, rows, x, u, t, r, count);
        mvm_batch(x, t, count);
        for (uint64_t j = 0; j < count; j++) const_cast<CloverVector8 *>(u[j])->scaleAndAdd(*t[j], a, *r[j]);
#endif
    }
    /* in place: u[j] = quantize(u[j] + a * (this * x[j])) */
    void mvm_scaleAndAdd_batch(const CloverVector8 *const *x, CloverVector8 *const *u, float a, CloverVector8 *const *t, uint64_t count)
    {
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
        BatchForward::fused_in_place(batch_view(), x, u, a, t, count, "CloverMatrix8::mvm_scaleAndAdd_batch");
#else
        clover_hip::batch_check_fused<CloverVector8>(cols, rows, x, u, t, nullptr, count);
        mvm_batch(x, t, count);
        for (uint64_t j = 0; j < count; j++) u[j]->scaleAndAdd(*t[j], a);
#endif
    }
    /* iht_loop for `count` signals with this matrix as Phi (clm8_iht_batch): per iteration every step runs once for a group of signals;
     * x[j], t1[j], t2[j], t3[j] end as iht_loop(PhiT, *x[j], *y[j], ...) leaves them.  Deterministic rounding only, as iht_loop. */
    void iht_loop_batch(CloverMatrix8 &PhiT, CloverVector8 *const *x, const CloverVector8 *const *y, CloverVector8 *const *t1,
                        CloverVector8 *const *t2, CloverVector8 *const *t3, uint64_t count, uint64_t iterations, uint64_t K, float mu,
                        bool with_threshold)
    {
        BatchForward::iht_loop(batch_view(), PhiT.batch_view(), x, y, t1, t2, t3, count, iterations, K, mu, with_threshold,
                               "CloverMatrix8::iht_loop_batch");
    }
    /* Not in the reference: this' * x[j] for `count` vectors in ONE pass over this matrix's own bytes per group of CLM4_MVM_BATCH_MAX
     * (clm8_mvm_transposed_batch, clover_hip_batch_t8.h); r[j] equals what mvm_transposed(*x[j], *r[j]) gives, bit for bit.  The x[j] may
     * repeat; the r[j] are distinct vectors, none of them an x.  With stochastic rounding enabled the vectors draw from the matrix's
     * generator one after another, as the single calls in order do, and the generator ends where those calls leave it. */
    void mvm_transposed_batch(const CloverVector8 *const *x, CloverVector8 *const *r, uint64_t count)
    {
        BatchTransposed::mvm(batch_view(), x, r, count, clover_hip::rng_or_null(random), false, 0, 0, 0, "CloverMatrix8::mvm_transposed_batch");
    }
    /* mvm_transposed_batch with the place of every vector's draws chosen by the caller (clm8_mvm_transposed_batch_at), counted in draws --
     * mvm_transposed consumes 2 (cols / 64) -- from where the matrix's generator stands: vector j draws from draw_base + j * draw_stride on,
     * and the generator is advanced by commit_draws afterwards (0: left as it is).  For callers whose stream order is not vector after
     * vector (Q_IHT_batch_one_matrix, CloverIHT.h).  With rounding disabled the three numbers are ignored. */
    void mvm_transposed_batch_at(const CloverVector8 *const *x, CloverVector8 *const *r, uint64_t count, uint64_t draw_base, uint64_t draw_stride,
                                 uint64_t commit_draws)
    {
        BatchTransposed::mvm(batch_view(), x, r, count, clover_hip::rng_or_null(random), true, draw_base, draw_stride, commit_draws,
                             "CloverMatrix8::mvm_transposed_batch_at");
    }
    /* mvm_transposed_scaleAndAdd for `count` vectors: t[j] = this' * x[j], r[j] = quantize(u[j] + a * t[j]).  Rounding disabled: one launch
     * per group (clm8_mvm_transposed_scale_and_add_batch).  Stochastic: one mvm_transposed_batch and the scaleAndAdd calls, which draw from
     * their u[j]'s own generators -- the bits of the loop of mvm_transposed_scaleAndAdd. */
    void mvm_transposed_scaleAndAdd_batch(const CloverVector8 *const *x, const CloverVector8 *const *u, float a, CloverVector8 *const *t,
                                          CloverVector8 *const *r, uint64_t count)
    {
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
        BatchTransposed::fused(batch_view(), x, u, a, t, r, count, "CloverMatrix8::mvm_transposed_scaleAndAdd_batch");
#else
        clover_hip::batch_check_fused<CloverVector8>(rows, cols, x, u, t, r, count);
        mvm_transposed_batch(x, t, count);
        for (uint64_t j = 0; j < count; j++) const_cast<CloverVector8 *>(u[j])->scaleAndAdd(*t[j], a, *r[j]);
#endif
    }
    /* in place: u[j] = quantize(u[j] + a * (this' * x[j])) */
    void mvm_transposed_scaleAndAdd_batch(const CloverVector8 *const *x, CloverVector8 *const *u, float a, CloverVector8 *const *t, uint64_t count)
    {
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
        BatchTransposed::fused_in_place(batch_view(), x, u, a, t, count, "CloverMatrix8::mvm_transposed_scaleAndAdd_batch");
#else
        clover_hip::batch_check_fused<CloverVector8>(rows, cols, x, u, t, nullptr, count);
        mvm_transposed_batch(x, t, count);
        for (uint64_t j = 0; j < count; j++) u[j]->scaleAndAdd(*t[j], a);
#endif
    }
    /* iht_loop_one_matrix for `count` signals with this matrix as Phi and no PhiT (clm8_iht_batch_one_matrix): per iteration every step
     * runs once for a group of signals, t3 = Phi' t2 from this matrix's own bytes; x[j], t1[j], t2[j], t3[j] end as
     * iht_loop_one_matrix(*x[j], *y[j], ...) leaves them.  Deterministic rounding only, as iht_loop_one_matrix. */
    void iht_loop_batch_one_matrix(CloverVector8 *const *x, const CloverVector8 *const *y, CloverVector8 *const *t1, CloverVector8 *const *t2,
                                   CloverVector8 *const *t3, uint64_t count, uint64_t iterations, uint64_t K, float mu, bool with_threshold)
    {
        BatchTransposed::iht_loop(batch_view(), clover_hip::no_transpose(), x, y, t1, t2, t3, count, iterations, K, mu, with_threshold,
                                  "CloverMatrix8::iht_loop_batch_one_matrix");
    }

    /* :480-548: every row wrapped in a non-owning CloverVector8 view over the matrix's own memory and multiplied with dot() (the
     * reference's order), then 64 results at a time quantised by scalar code -- an implementation independent of the mvm kernel */
    void mvm_scalar(const CloverVector8 &productVector, CloverVector8 &resultVector)
    {
        check_mvm(productVector, resultVector);
        int8_t *vals = getData();
        float *scs = getScales();
        int8_t *r = resultVector.getData();
        float *sr = resultVector.getScales();
        const uint64_t hb = cols >> 6;
        for (uint64_t bi = 0; bi < (rows >> 6); bi++) {
            float block[64];
            for (uint64_t i = 0; i < 64; i++) {
                CloverVector8 rowVector(cols, vals + ((bi << 6) + i) * cols, scs + bi * hb);
                block[i] = rowVector.dot(productVector);
            }
            sr[bi] = clover_hip::scalar::quantize_block8(block, r + 64 * bi);
        }
    }

    /* fp32 vector in, fp32 vector out */
    void mvm(const CloverVector32 &productVector, CloverVector32 &resultVector)
    {
        check_mvm(productVector, resultVector);
        clover_hip::check(clm8_mvm_f32(dev_values(), dev_scales(), rows, cols, productVector.device_ro(), resultVector.device_wo(), nullptr),
                          "CloverMatrix8::mvm");
        resultVector.commit();
    }
    void mvm_parallel(const CloverVector32 &productVector, CloverVector32 &resultVector) { mvm(productVector, resultVector); }
    /* Not in the reference: resultVector = this' * productVector for fp32 vectors straight from this matrix's own bytes
     * (clm8_mvm_f32_transposed, clover_hip_m8_f32.h), bit for bit what transpose(T); T.mvm(productVector, resultVector) gives. */
    void mvm_transposed(const CloverVector32 &productVector, CloverVector32 &resultVector)
    {
        if (productVector.size() != getRows() || resultVector.size_pad() != getCols()) {
            std::cout << "MVM can not be performed. Exiting ..." << std::endl;
            exit(1);
        }
        clover_hip::check(clm8_mvm_f32_transposed(dev_values(), dev_scales(), rows, cols, productVector.device_ro(), resultVector.device_wo(), nullptr),
                          "CloverMatrix8::mvm_transposed");
        resultVector.commit();
    }
    void mvm_transposed_parallel(const CloverVector32 &productVector, CloverVector32 &resultVector) { mvm_transposed(productVector, resultVector); }
#ifdef CLOVER_FP32_ON_DEVICE
    /* Not in the reference, and only where CloverVector32's own arithmetic runs on the device: t = this * x immediately followed by
     * r = u + a * t, the pair of steps the IHT / GD loops repeat, as for the other widths -- one launch (clm8_mvm_f32_scale_and_add), the
     * bits of mvm(x, t); u.scaleAndAdd(t, a, r). */
    void mvm_scaleAndAdd(const CloverVector32 &x, const CloverVector32 &u, float a, CloverVector32 &t, CloverVector32 &r)
    {
        if (x.size() != getCols() || t.size_pad() != getRows()) { std::cout << "MVM can not be performed. Exiting ..." << std::endl; exit(1); }
        if (u.size_pad() != getRows() || r.size_pad() != getRows()) { std::cout << "Vectors do not have the same size. Exiting ..." << std::endl; exit(1); }
        clover_hip::check(clm8_mvm_f32_scale_and_add(dev_values(), dev_scales(), rows, cols, x.device_ro(), u.device_ro(), a, t.device_wo(),
                                                     r.device_wo(), nullptr), "CloverMatrix8::mvm_scaleAndAdd");
        t.commit();
        r.commit();
    }
    /* in place: u = u + a * (this * x) */
    void mvm_scaleAndAdd(const CloverVector32 &x, CloverVector32 &u, float a, CloverVector32 &t)
    {
        if (x.size() != getCols() || t.size_pad() != getRows()) { std::cout << "MVM can not be performed. Exiting ..." << std::endl; exit(1); }
        if (u.size_pad() != getRows()) { std::cout << "Vectors do not have the same size. Exiting ..." << std::endl; exit(1); }
        float *du = u.device_rw();
        clover_hip::check(clm8_mvm_f32_scale_and_add(dev_values(), dev_scales(), rows, cols, x.device_ro(), du, a, t.device_wo(), du, nullptr),
                          "CloverMatrix8::mvm_scaleAndAdd");
        t.commit();
        u.commit();
    }
    /* the same on this' * x (clm8_mvm_f32_transposed_scale_and_add): the bits of mvm_transposed(x, t); u.scaleAndAdd(t, a, r) */
    void mvm_transposed_scaleAndAdd(const CloverVector32 &x, const CloverVector32 &u, float a, CloverVector32 &t, CloverVector32 &r)
    {
        if (x.size() != getRows() || t.size_pad() != getCols()) { std::cout << "MVM can not be performed. Exiting ..." << std::endl; exit(1); }
        if (u.size_pad() != getCols() || r.size_pad() != getCols()) { std::cout << "Vectors do not have the same size. Exiting ..." << std::endl; exit(1); }
        clover_hip::check(clm8_mvm_f32_transposed_scale_and_add(dev_values(), dev_scales(), rows, cols, x.device_ro(), u.device_ro(), a, t.device_wo(),
                                                                r.device_wo(), nullptr), "CloverMatrix8::mvm_transposed_scaleAndAdd");
        t.commit();
        r.commit();
    }
    void mvm_transposed_scaleAndAdd(const CloverVector32 &x, CloverVector32 &u, float a, CloverVector32 &t)
    {
        if (x.size() != getRows() || t.size_pad() != getCols()) { std::cout << "MVM can not be performed. Exiting ..." << std::endl; exit(1); }
        if (u.size_pad() != getCols()) { std::cout << "Vectors do not have the same size. Exiting ..." << std::endl; exit(1); }
        float *du = u.device_rw();
        clover_hip::check(clm8_mvm_f32_transposed_scale_and_add(dev_values(), dev_scales(), rows, cols, x.device_ro(), du, a, t.device_wo(), du, nullptr),
                          "CloverMatrix8::mvm_transposed_scaleAndAdd");
        t.commit();
        u.commit();
    }
    /* The reference's Q_IHT / Q_GD loop (01_measure.h:923-946, 999-1021) on <CloverMatrix8, CloverVector32> with this matrix as Phi, in one
     * call (clm8_iht_f32): x.clear(), then `iterations` times t1 = Phi x; t2 = y - t1; t3 = PhiT t2; x += mu t3; [threshold(K)] -- one
     * fused launch per product plus the threshold, the bits of the five method calls.  The threshold is the one x.threshold_parallel(K)
     * would take under the exactness switch (default: the reference's survivors). */
    void iht_loop(CloverMatrix8 &PhiT, CloverVector32 &x, const CloverVector32 &y, CloverVector32 &t1, CloverVector32 &t2, CloverVector32 &t3,
                  uint64_t iterations, uint64_t K, float mu, bool with_threshold)
    {
        if (PhiT.rows != cols || PhiT.cols != rows || x.size_pad() != getCols() || y.size_pad() != getRows() || t1.size_pad() != getRows() ||
            t2.size_pad() != getRows() || t3.size_pad() != getCols()) {
            std::cout << "MVM can not be performed. Exiting ..." << std::endl;
            exit(1);
        }
        const int thr = !with_threshold ? 0 : (clover_hip::threshold_mode() == CLV_THRESHOLD_FAST ? 1 : 2);
        clover_hip::check(clm8_iht_f32(dev_values(), dev_scales(), PhiT.dev_values(), PhiT.dev_scales(), rows, cols, x.device_wo(), x.size(),
                                       y.device_ro(), t1.device_wo(), t2.device_wo(), t3.device_wo(), iterations, K, mu, thr, nullptr),
                          "CloverMatrix8::iht_loop");
        x.commit();
        if (iterations) { t1.commit(); t2.commit(); t3.commit(); }
    }
    /* iht_loop without PhiT (clm8_iht_f32_one_matrix): t3 = Phi' t2 comes from this matrix; the bits of iht_loop with PhiT = transpose of
     * this.  Half the resident matrix bytes; DESIGN.md 3 has what that costs per iteration. */
    void iht_loop_one_matrix(CloverVector32 &x, const CloverVector32 &y, CloverVector32 &t1, CloverVector32 &t2, CloverVector32 &t3,
                             uint64_t iterations, uint64_t K, float mu, bool with_threshold)
    {
        if (x.size_pad() != getCols() || y.size_pad() != getRows() || t1.size_pad() != getRows() || t2.size_pad() != getRows() ||
            t3.size_pad() != getCols()) {
            std::cout << "MVM can not be performed. Exiting ..." << std::endl;
            exit(1);
        }
        const int thr = !with_threshold ? 0 : (clover_hip::threshold_mode() == CLV_THRESHOLD_FAST ? 1 : 2);
        clover_hip::check(clm8_iht_f32_one_matrix(dev_values(), dev_scales(), rows, cols, x.device_wo(), x.size(), y.device_ro(), t1.device_wo(),
                                                  t2.device_wo(), t3.device_wo(), iterations, K, mu, thr, nullptr),
                          "CloverMatrix8::iht_loop_one_matrix");
        x.commit();
        if (iterations) { t1.commit(); t2.commit(); t3.commit(); }
    }
#endif
    /* :550-556: double accumulation on the host */
    void mvm_scalar(const CloverVector32 &productVector, CloverVector32 &resultVector)
    {
        check_mvm(productVector, resultVector);
        for (uint64_t i = 0; i < rows; i++) {
            double sum = 0;
            for (uint64_t j = 0; j < cols; j++) sum += (double)get(i, j) * (double)productVector.get(j);
            resultVector.set(i, (float)sum);
        }
    }

    /* other = this^T, values and tile scales */
    void transpose(CloverMatrix8 &other) const
    {
        check_transpose(other);
        uint8_t *d = other.mem.dev_wo();
        clover_hip::check(clm8_transpose(dev_values(), dev_scales(), rows, cols, reinterpret_cast<int8_t *>(d),
                                         reinterpret_cast<float *>(d + other.value_bytes), nullptr), "CloverMatrix8::transpose");
    }
    void transpose_parallel(CloverMatrix8 &other) const { transpose(other); }

    /* C = this * B^T, fp32: this is M x K, B is N x K, C is M x N (build-defined like CloverMatrix4::gemm).  One launch
     * on the int8 matrix cores, nothing is re-coded and no scratch is used. */
    void gemm(const CloverMatrix8 &B, CloverMatrix32 &C) const
    {
        if (B.cols != cols || C.getRows() != rows || C.getCols() != B.rows) {
            std::cout << "GEMM can not be performed. Exiting ..." << std::endl;
            exit(1);
        }
        clover_hip::check(clm8_gemm(dev_values(), dev_scales(), rows, cols, B.dev_values(), B.dev_scales(), B.rows, C.device_wo(), nullptr),
                          "CloverMatrix8::gemm");
    }
    void transpose_scalar(CloverMatrix8 &other) const
    {
        check_transpose(other);
        const uint8_t *h = mem.host_ro();
        uint8_t *o = other.mem.host_rw();
        const float *s = reinterpret_cast<const float *>(h + value_bytes);
        float *so = reinterpret_cast<float *>(o + other.value_bytes);
        for (uint64_t i = 0; i < rows; i++)
            for (uint64_t j = 0; j < cols; j++) o[j * rows + i] = h[i * cols + j];
        for (uint64_t bi = 0; bi < (rows >> 6); bi++)
            for (uint64_t bj = 0; bj < (cols >> 6); bj++) so[bj * (rows >> 6) + bi] = s[bi * (cols >> 6) + bj];
    }
};

#endif
