/*
 * CloverVector16.h -- half-precision vector, MI355X-backed.
 *
 * Same class name, constructors, data format and element accessors as the reference's include/CloverVector16.h: length_pad raw IEEE
 * binary16 bit patterns in uint16_t (padded to a multiple of 128, the padding zero), no scales (:35-66).  Methods:
 *
 *   quantize / quantize_parallel            -> clv_f16_quantize       (CloverVector16.h:212-277)
 *   restore                                 -> clv_f16_restore        (:279-307)
 *   scaleAndAdd / _parallel (both forms)    -> clv_f16_scale_and_add  (:309-470)
 *   dot / dot_parallel                      -> clv_f16_dot EXACT / FAST (:473-610; the exactness switch, clover_device.h)
 *   threshold / threshold_parallel          -> clv_f16_threshold_mode (:612-626; tie rule by the exactness switch)
 *   threshold_min_heap / _parallel          -> clv_f16_threshold_heap (:628-768)
 *   *_scalar                                -> plain host loops in the reference's scalar order (:143-206), f16 conversion in integer
 *                                              arithmetic (clover_half.h): no F16C needed on the build machine
 */
#ifndef CLOVER_VECTOR16_H
#define CLOVER_VECTOR16_H

#include <cmath>

#include "CloverVector32.h"
#include "clover_half.h"

class CloverVector16 {
    friend class CloverMatrix16;               /* mvm_scalar reads and writes the host copy */
protected:
    const uint64_t length;
    const uint64_t length_pad;
    mutable clover_hip::Mirror mem;            /* length_pad uint16_t */

    void allocate()
    {
        mem.allocate(length_pad * sizeof(uint16_t));
        uint16_t *v = values_rw();
        for (uint64_t i = length; i < length_pad; i++) v[i] = 0;                /* zeroed padding */
    }

public:
    typedef clover_hip::idx_t idx_t;

    explicit CloverVector16(uint64_t s) : length(s), length_pad(clover_hip::round_up(s, CLOVER_VECTOR_SIZE_PAD)) { allocate(); }

    /* non-owning view (CloverVector16.h:67-71): reads and writes go to the caller's memory */
    CloverVector16(uint64_t s, uint16_t *data) : length(s), length_pad(clover_hip::round_up(s, CLOVER_VECTOR_SIZE_PAD))
    {
        mem.adopt(data, length_pad * sizeof(uint16_t));
    }

    explicit CloverVector16(const CloverVector32 &other) : length(other.size()), length_pad(other.size_pad())
    {
        allocate();
        quantize(other);
    }

    CloverVector16(const CloverVector16 &other) : length(other.length), length_pad(other.length_pad)
    {
        allocate();
        memcpy(values_rw(), other.values_ro(), length_pad * sizeof(uint16_t));
    }

    uint64_t size() const { return length; }
    uint64_t size_pad() const { return length_pad; }
    uint64_t getBitsLength() const { return 16; }
    uint64_t getBytes() const { return length_pad * sizeof(uint16_t); }

    /* explicit residency (clover_device.h, -DCLOVER_HIP_EXPLICIT_SYNC); optional in every build */
    void toDevice() const { (void)mem.dev_ro(); }
    void toHost() const { (void)mem.host_ro(); }
    /* raw pointer as in the reference: valid for the life of the object and always current (clover_device.h) */
    uint16_t *getData() const { return reinterpret_cast<uint16_t *>(mem.host_ptr()); }

    /* :91-117 */
    float get(uint64_t i) const { return clover_hip::half::to_f32(values_ro()[i]); }
    float getAbs(uint64_t i) const { return clover_hip::half::to_f32((uint16_t)(values_ro()[i] & 0x7FFFu)); }
    void set(uint64_t i, float v) { values_rw()[i] = clover_hip::half::from_f32(v); }
    uint16_t getBits(uint64_t i) const { return values_ro()[i]; }
    void setBits(uint64_t i, uint16_t bits) { values_rw()[i] = bits; }
    void clear() { memset(values_rw(), 0, length_pad * sizeof(uint16_t)); }
    /* :136-141 */
    std::string toString() const
    {
        CloverVector32 tmp(size());
        restore(tmp);
        return tmp.toString();
    }

    void quantize(const CloverVector32 &other)
    {
        if (other.size_pad() != length_pad) {
            std::cout << "Vectors do not have the same size. Exiting ..." << std::endl;
            exit(1);
        }
        clover_hip::check(clv_f16_quantize(other.device_ro(), length_pad, dev_values_wo(), nullptr), "CloverVector16::quantize");
        commit();
    }
    void quantize_parallel(const CloverVector32 &other) { quantize(other); }
    void quantize_scalar(const CloverVector32 &other)      /* :143-151 */
    {
        const float *u = other.host_ro();
        uint16_t *r = values_rw();
        for (uint64_t i = 0; i < length_pad; i++) r[i] = clover_hip::half::from_f32(u[i]);
    }

    void restore(CloverVector32 &other) const
    {
        if (other.size_pad() != length_pad) {
            std::cout << "Vectors do not have the same size. Exiting ..." << std::endl;
            exit(1);
        }
        clover_hip::check(clv_f16_restore(dev_values_ro(), length_pad, other.device_wo(), nullptr), "CloverVector16::restore");
        other.commit();
    }
    void restore_scalar(CloverVector32 &other) const      /* :153-161 */
    {
        const uint16_t *u = values_ro();
        float *r = other.host_rw();
        for (uint64_t i = 0; i < length_pad; i++) r[i] = clover_hip::half::to_f32(u[i]);
    }

    /* this = f16(fma(other, a, this))   (:309-320) */
    void scaleAndAdd(const CloverVector16 &other, float a)
    {
        same_size(other);
        const uint16_t *v = other.dev_values_ro();
        uint16_t *u = dev_values_rw();
        clover_hip::check(clv_f16_scale_and_add(u, v, a, length_pad, u, nullptr), "CloverVector16::scaleAndAdd");
        commit();
    }
    /* result = f16(fma(other, a, this)) (:322-333) */
    void scaleAndAdd(const CloverVector16 &other, float a, CloverVector16 &result) const
    {
        same_size(other);
        same_size(result);
        clover_hip::check(clv_f16_scale_and_add(dev_values_ro(), other.dev_values_ro(), a, length_pad, result.dev_values_wo(), nullptr),
                          "CloverVector16::scaleAndAdd");
        result.commit();
    }
    void scaleAndAdd_parallel(const CloverVector16 &other, float a) { scaleAndAdd(other, a); }
    void scaleAndAdd_parallel(const CloverVector16 &other, float a, CloverVector16 &result) const { scaleAndAdd(other, a, result); }
    void scaleAndAdd_scalar(const CloverVector16 &other, float a)      /* :163-175 */
    {
        same_size(other);
        const uint16_t *v = other.values_ro();
        uint16_t *u = values_rw();
        for (uint64_t i = 0; i < length_pad; i++)
            u[i] = clover_hip::half::from_f32(std::fma(clover_hip::half::to_f32(v[i]), a, clover_hip::half::to_f32(u[i])));
    }
    void scaleAndAdd_scalar(const CloverVector16 &other, float a, CloverVector16 &result) const      /* :177-190 */
    {
        same_size(other);
        same_size(result);
        const uint16_t *u = values_ro(), *v = other.values_ro();
        uint16_t *r = result.values_rw();
        for (uint64_t i = 0; i < length_pad; i++)
            r[i] = clover_hip::half::from_f32(std::fma(clover_hip::half::to_f32(v[i]), a, clover_hip::half::to_f32(u[i])));
    }

    /* dot(): by default the reference's order, bit for bit -- 32 sequential fma chains of n / 32 steps (:473-530): latency-bound by that
     * definition.  Under -DCLOVER_FAST / clover_hip::set_exactness(FAST) the one-launch tree order.  dot_parallel(): always the fast order
     * (the reference's own is "any order", :532-610); dot_exact(): always the reference's. */
    float dot(const CloverVector16 &other) const { return dot_mode(other, clover_hip::dot_mode()); }
    float dot_exact(const CloverVector16 &other) const { return dot_mode(other, CLV_DOT_EXACT); }
    float dot_parallel(const CloverVector16 &other) const { return dot_mode(other, CLV_DOT_FAST); }
    float dot_fast(const CloverVector16 &other) const { return dot_mode(other, CLV_DOT_FAST); }
    /* :193-206, on the host: one running fp32 sum of separately rounded products */
    float dot_scalar(const CloverVector16 &other) const
    {
        same_size(other);
        const uint16_t *u = values_ro(), *v = other.values_ro();
        float dot_product = 0;
        for (uint64_t i = 0; i < length_pad; i++) dot_product += clover_hip::half::to_f32(u[i]) * clover_hip::half::to_f32(v[i]);
        return dot_product;
    }

    /* keep the k largest magnitudes, the other elements below size() become 0x0000 (:612-673) */
    void threshold(uint64_t k)
    {
        clover_hip::check(clv_f16_threshold_mode(dev_values_rw(), length, length_pad, k, clover_hip::threshold_mode(), nullptr, nullptr),
                          "CloverVector16::threshold");
        commit();
    }
    void threshold_parallel(uint64_t k) { threshold(k); }
    /* threshold with the caller's own heap memory (:628-673): the reference's walk, its heap left in min_heap entry for entry */
    void threshold_min_heap(idx_t *min_heap, uint64_t k)
    {
        if (k == 0 || k > length) { std::cout << "threshold_min_heap: k must lie in 1 .. size(). Exiting ..." << std::endl; exit(1); }
        const uint16_t *before = values_ro();
        uint16_t *bits = static_cast<uint16_t *>(malloc(length * sizeof(uint16_t)));
        if (!bits) { std::cout << "We ran out of memory, while allocating thresholding memory. Exiting ..." << std::endl; exit(1); }
        memcpy(bits, before, length * sizeof(uint16_t));
        void *heap_dev = nullptr;
        clover_hip::check(clv_malloc(&heap_dev, k * 8), "CloverVector16::threshold_min_heap");
        const int rc = clv_f16_threshold_heap(dev_values_rw(), length, length_pad, k, heap_dev, nullptr, nullptr);
        if (rc) { clv_free(heap_dev); free(bits); clover_hip::check(rc, "CloverVector16::threshold_min_heap"); }
        uint32_t *pairs = static_cast<uint32_t *>(malloc(k * 8));
        if (!pairs) { std::cout << "We ran out of memory, while allocating thresholding memory. Exiting ..." << std::endl; exit(1); }
        clover_hip::check(clv_memcpy_d2h(pairs, heap_dev, k * 8, nullptr), "CloverVector16::threshold_min_heap");
        clv_free(heap_dev);
        commit();
        for (uint64_t i = 0; i < k; i++) {
            memcpy(&min_heap[i].value, &pairs[2 * i], 4);
            min_heap[i].idx = pairs[2 * i + 1];
            min_heap[i].bits.i = bits[pairs[2 * i + 1]];
        }
        free(pairs);
        free(bits);
    }
    void threshold_min_heap_parallel(idx_t *min_heaps, uint64_t k) { threshold_min_heap(min_heaps, k); }

    /* ---- device views, used by CloverMatrix16 ----------------------------------------------------- */
    const uint16_t *dev_values_ro() const { return reinterpret_cast<const uint16_t *>(mem.dev_ro()); }
    uint16_t *dev_values_wo() { return reinterpret_cast<uint16_t *>(mem.dev_wo()); }
    uint16_t *dev_values_rw() { return reinterpret_cast<uint16_t *>(mem.dev_rw()); }
    /* after a launch that wrote through dev_values_wo() / dev_values_rw(): a view copies the result into the caller's memory now */
    void commit() { mem.commit(); }

private:
    float dot_mode(const CloverVector16 &other, int mode) const
    {
        same_size(other);
        clover_hip::ResultSlot &slot = clover_hip::result_slot();          /* per-thread device word + pinned host word */
        clover_hip::check(clv_f16_dot(dev_values_ro(), other.dev_values_ro(), length_pad, mode, slot.device(), nullptr, nullptr),
                          "CloverVector16::dot");
        return slot.fetch();
    }
    void same_size(const CloverVector16 &other) const
    {
        if (other.length_pad != length_pad) {
            std::cout << "Vectors do not have the same size. Exiting ..." << std::endl;
            exit(1);
        }
    }
    uint16_t *values_rw() const { return reinterpret_cast<uint16_t *>(mem.host_rw()); }
    const uint16_t *values_ro() const { return reinterpret_cast<const uint16_t *>(mem.host_ro()); }
};

#endif
