/*
 * ref_containers.cpp -- harness around the REFERENCE's own containers (TEST INFRASTRUCTURE ONLY).
 *
 * Contains no reference code: it #includes the eight container headers from where they lie (the Makefile passes
 * -I$(REFERENCE)/include) and calls their sequential methods behind a plain C ABI, host pointers in and out.
 * include/CloverBase.h includes Intel ipp.h / mkl.h; ref_shim/ declares those names and defines only library start-up
 * (no-ops) -- every Intel function that would compute aborts, so no value that leaves this file was computed by a
 * stand-in.  Methods that end in such a call (every transpose, CloverMatrix32::mvm) are not wrapped.
 *
 * Built three times by oracle/Makefile:
 *   _ref/libclover_ref.so        the reference's default: stochastic rounding
 *   _ref/libclover_ref_norng.so  -DCLOVER_STOCHASTIC_ROUNDING_DISABLED (the reference's compile-time switch)
 *   _ref/clover_ref_gen          -DREF_CONTAINERS_MAIN: includes no reference header; dlopen()s the two libraries and
 *                                writes the fixtures tests/golden/ref_*.json from the case list and input bytes that
 *                                tests/ref_fixture_cases.py lays down.  It never generates data.
 *
 * Generator state `st`: 8 x uint64 = random_key1 lanes then random_key2 lanes (the convention of ref_xorshift.cpp),
 * loaded into the object whose generator the method draws from before the call and stored back after it.  The
 * constructors seed from RDRAND, so a stochastic call without `st` is not reproducible; st == NULL is for the calls
 * that draw nothing.
 *
 * Three facts about the reference's objects that shape this file:
 *   - the base constructor prints banners to stdout; nothing here writes a result to stdout.
 *   - threshold() takes its heap from malloc (CloverVector.h:74) and the destructor releases it with delete[] (:111).
 *     A container that has been thresholded is therefore allocated with new and never destroyed (leaked on purpose).
 *   - threshold(0) reads min_heap[0] of a heap that was never allocated (CloverVector4.h:1957 with a null pointer from
 *     CloverVector.h:67-82), so k = 0 is not a case; cref_*_threshold refuses it.
 * Every buffer is copied into 64-byte aligned memory first: CloverVector8::restore stores with aligned instructions.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* the C ABI (both libraries export all of it) */
extern "C" {
int cref_stochastic(void);
void cref_v4_quantize(const float *x, uint64_t n, int8_t *q, float *s, uint64_t *st);
void cref_v4_restore(const int8_t *q, const float *s, uint64_t n, float *x);
float cref_v4_dot(const int8_t *qu, const float *su, const int8_t *qv, const float *sv, uint64_t n);
void cref_v4_scale_and_add(const int8_t *qu, const float *su, const int8_t *qv, const float *sv, float a, uint64_t n, int8_t *qr, float *sr, uint64_t *st, int in_place);
int cref_v4_threshold(int8_t *q, const float *s, uint64_t n, uint64_t k);
void cref_v8_quantize(const float *x, uint64_t n, int8_t *q, float *s, uint64_t *st);
void cref_v8_restore(const int8_t *q, const float *s, uint64_t n, float *x);
float cref_v8_dot(const int8_t *qu, const float *su, const int8_t *qv, const float *sv, uint64_t n);
void cref_v8_scale_and_add(const int8_t *qu, const float *su, const int8_t *qv, const float *sv, float a, uint64_t n, int8_t *qr, float *sr, uint64_t *st, int in_place);
int cref_v8_threshold(int8_t *q, const float *s, uint64_t n, uint64_t k);
void cref_v16_quantize(const float *x, uint64_t n, uint16_t *h);
void cref_v16_restore(const uint16_t *h, uint64_t n, float *x);
float cref_v16_dot(const uint16_t *hu, const uint16_t *hv, uint64_t n);
void cref_v16_scale_and_add(const uint16_t *hu, const uint16_t *hv, float a, uint64_t n, uint16_t *hr, int in_place);
int cref_v16_threshold(uint16_t *h, uint64_t n, uint64_t k);
float cref_v32_dot(const float *xu, const float *xv, uint64_t n);
void cref_v32_scale_and_add(const float *xu, const float *xv, float a, uint64_t n, float *xr, int in_place);
int cref_v32_threshold(float *x, uint64_t n, uint64_t k);
void cref_m4_quantize(const float *A, uint64_t rows, uint64_t cols, int8_t *q, float *s, uint64_t *st);
void cref_m4_mvm(const int8_t *qA, const float *sA, uint64_t rows, uint64_t cols, const int8_t *qx, const float *sx, int8_t *qr, float *sr, uint64_t *st);
void cref_m4_mvm_v8(const int8_t *qA, const float *sA, uint64_t rows, uint64_t cols, const int8_t *qx, const float *sx, int8_t *qr, float *sr, uint64_t *st);
void cref_m4_mvm_f32(const int8_t *qA, const float *sA, uint64_t rows, uint64_t cols, const float *x, float *r);
void cref_m8_quantize(const float *A, uint64_t rows, uint64_t cols, int8_t *q, float *s, uint64_t *st);
void cref_m8_restore(const int8_t *q, const float *s, uint64_t rows, uint64_t cols, float *A);
void cref_m8_mvm(const int8_t *qA, const float *sA, uint64_t rows, uint64_t cols, const int8_t *qx, const float *sx, int8_t *qr, float *sr, uint64_t *st);
void cref_m8_mvm_f32(const int8_t *qA, const float *sA, uint64_t rows, uint64_t cols, const float *x, float *r);
void cref_m16_quantize(const float *A, uint64_t rows, uint64_t cols, uint16_t *h);
void cref_m16_mvm(const uint16_t *hA, uint64_t rows, uint64_t cols, const uint16_t *hx, uint16_t *hr);
void cref_m16_mvm_f32(const uint16_t *hA, uint64_t rows, uint64_t cols, const float *x, float *r);
void cref_loop_m4v4(const int8_t *qPhi, const float *sPhi, const int8_t *qPhiT, const float *sPhiT, uint64_t m, uint64_t n, const int8_t *qy, const float *sy, uint64_t iterations, uint64_t K, float mu, int8_t *out_q, float *out_s, uint64_t *st);
void cref_loop_m4v8(const int8_t *qPhi, const float *sPhi, const int8_t *qPhiT, const float *sPhiT, uint64_t m, uint64_t n, const int8_t *qy, const float *sy, uint64_t iterations, uint64_t K, float mu, int8_t *out_q, float *out_s, uint64_t *st);
void cref_loop_m8v8(const int8_t *qPhi, const float *sPhi, const int8_t *qPhiT, const float *sPhiT, uint64_t m, uint64_t n, const int8_t *qy, const float *sy, uint64_t iterations, uint64_t K, float mu, int8_t *out_q, float *out_s, uint64_t *st);
void cref_loop_m16v16(const uint16_t *hPhi, const uint16_t *hPhiT, uint64_t m, uint64_t n, const uint16_t *hy, uint64_t iterations, uint64_t K, float mu, uint16_t *out_h);
}

#ifndef REF_CONTAINERS_MAIN

#include "CloverVector4.h"
#include "CloverVector8.h"
#include "CloverVector16.h"
#include "CloverVector32.h"
#include "CloverMatrix4.h"
#include "CloverMatrix8.h"
#include "CloverMatrix16.h"
#include "CloverMatrix32.h"

namespace {

/* aligned copy of a caller's buffer; out() copies it back */
template <class T> struct Al {
    T *p;
    size_t n;
    Al(const T *src, size_t count) : p(NULL), n(count) {
        void *m = NULL;
        if (posix_memalign(&m, 64, n * sizeof(T) + 64) != 0) abort();
        p = (T *)m;
        if (src) memcpy(p, src, n * sizeof(T)); else memset(p, 0, n * sizeof(T));
    }
    ~Al() { free(p); }
    void out(T *dst) const { memcpy(dst, p, n * sizeof(T)); }
private:
    Al(const Al &);
    Al &operator=(const Al &);
};

/* opens the protected generator keys (and, for matrices, the storage) of a container */
template <class T> struct Keyed : T {
    template <class A> explicit Keyed(A a) : T(a) {}
    template <class A, class B> Keyed(A a, B b) : T(a, b) {}
    template <class A, class B, class D> Keyed(A a, B b, D d) : T(a, b, d) {}
    void load(const uint64_t *st) {
        if (!st) return;
        this->random_key1 = _mm256_loadu_si256((const __m256i *)st);
        this->random_key2 = _mm256_loadu_si256((const __m256i *)(st + 4));
    }
    void store(uint64_t *st) const {
        if (!st) return;
        _mm256_storeu_si256((__m256i *)st, this->random_key1);
        _mm256_storeu_si256((__m256i *)(st + 4), this->random_key2);
    }
};

template <class T> struct Mat : Keyed<T> {
    Mat(uint64_t r, uint64_t c) : Keyed<T>(r, c) {}
    void put(const int8_t *q, const float *s) {
        memcpy(this->values, q, this->getBytes() - nscales() * sizeof(float));
        memcpy(this->scales, s, nscales() * sizeof(float));
    }
    void take(int8_t *q, float *s) const {
        memcpy(q, this->values, this->getBytes() - nscales() * sizeof(float));
        memcpy(s, this->scales, nscales() * sizeof(float));
    }
    size_t nscales() const { return (size_t)(this->rows >> 6) * (size_t)(this->cols >> 6); }
};

typedef Keyed<CloverVector4> V4;
typedef Keyed<CloverVector8> V8;
typedef Keyed<CloverVector16> V16;
typedef Keyed<CloverVector32> V32;
typedef Mat<CloverMatrix4> M4;
typedef Mat<CloverMatrix8> M8;

struct M16 : CloverMatrix16 {
    M16(uint64_t r, uint64_t c) : CloverMatrix16(r, c) {}
};

void fill32(CloverMatrix32 &m, const float *A, uint64_t rows, uint64_t cols) { memcpy(m.getData(), A, rows * cols * sizeof(float)); }

}  /* namespace */

extern "C" {

int cref_stochastic(void) {
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
    return 0;
#else
    return 1;
#endif
}

/* ================================================================ CloverVector4 (n/2 bytes, n/64 scales) */
void cref_v4_quantize(const float *x, uint64_t n, int8_t *q, float *s, uint64_t *st) {
    Al<float> ax(x, n); Al<int8_t> aq(NULL, n / 2); Al<float> as(NULL, n / 64);
    CloverVector32 v(n, ax.p);
    V4 r(n, aq.p, as.p);
    r.load(st); r.quantize(v); r.store(st);
    aq.out(q); as.out(s);
}

void cref_v4_restore(const int8_t *q, const float *s, uint64_t n, float *x) {
    Al<int8_t> aq(q, n / 2); Al<float> as(s, n / 64); Al<float> ax(NULL, n);
    CloverVector32 v(n, ax.p);
    V4 u(n, aq.p, as.p);
    u.restore(v);
    ax.out(x);
}

float cref_v4_dot(const int8_t *qu, const float *su, const int8_t *qv, const float *sv, uint64_t n) {
    Al<int8_t> au(qu, n / 2), av(qv, n / 2); Al<float> asu(su, n / 64), asv(sv, n / 64);
    V4 u(n, au.p, asu.p), v(n, av.p, asv.p);
    return u.dot(v);
}

/* in_place: u.scaleAndAdd(v, a), the result is u's storage afterwards; else u.scaleAndAdd(v, a, r).  Draws from u. */
void cref_v4_scale_and_add(const int8_t *qu, const float *su, const int8_t *qv, const float *sv, float a, uint64_t n, int8_t *qr,
                           float *sr, uint64_t *st, int in_place) {
    Al<int8_t> au(qu, n / 2), av(qv, n / 2), ar(NULL, n / 2); Al<float> asu(su, n / 64), asv(sv, n / 64), asr(NULL, n / 64);
    V4 u(n, au.p, asu.p), v(n, av.p, asv.p), r(n, ar.p, asr.p);
    u.load(st);
    if (in_place) { u.scaleAndAdd(v, a); au.out(qr); asu.out(sr); }
    else { u.scaleAndAdd(v, a, r); ar.out(qr); asr.out(sr); }
    u.store(st);
}

int cref_v4_threshold(int8_t *q, const float *s, uint64_t n, uint64_t k) {
    if (k == 0 || k > n) return 1;
    Al<int8_t> aq(q, n / 2); Al<float> as(s, n / 64);
    V4 *u = new V4(n, aq.p, as.p);       /* never destroyed: malloc / delete[] mismatch in the reference, see the header */
    u->threshold(k);
    aq.out(q);
    return 0;
}

/* ================================================================ CloverVector8 (n bytes, n/64 scales) */
void cref_v8_quantize(const float *x, uint64_t n, int8_t *q, float *s, uint64_t *st) {
    Al<float> ax(x, n); Al<int8_t> aq(NULL, n); Al<float> as(NULL, n / 64);
    CloverVector32 v(n, ax.p);
    V8 r(n, aq.p, as.p);
    r.load(st); r.quantize(v); r.store(st);
    aq.out(q); as.out(s);
}

void cref_v8_restore(const int8_t *q, const float *s, uint64_t n, float *x) {
    Al<int8_t> aq(q, n); Al<float> as(s, n / 64); Al<float> ax(NULL, n);
    CloverVector32 v(n, ax.p);
    V8 u(n, aq.p, as.p);
    u.restore(v);
    ax.out(x);
}

float cref_v8_dot(const int8_t *qu, const float *su, const int8_t *qv, const float *sv, uint64_t n) {
    Al<int8_t> au(qu, n), av(qv, n); Al<float> asu(su, n / 64), asv(sv, n / 64);
    V8 u(n, au.p, asu.p), v(n, av.p, asv.p);
    return u.dot(v);
}

void cref_v8_scale_and_add(const int8_t *qu, const float *su, const int8_t *qv, const float *sv, float a, uint64_t n, int8_t *qr,
                           float *sr, uint64_t *st, int in_place) {
    Al<int8_t> au(qu, n), av(qv, n), ar(NULL, n); Al<float> asu(su, n / 64), asv(sv, n / 64), asr(NULL, n / 64);
    V8 u(n, au.p, asu.p), v(n, av.p, asv.p), r(n, ar.p, asr.p);
    u.load(st);
    if (in_place) { u.scaleAndAdd(v, a); au.out(qr); asu.out(sr); }
    else { u.scaleAndAdd(v, a, r); ar.out(qr); asr.out(sr); }
    u.store(st);
}

int cref_v8_threshold(int8_t *q, const float *s, uint64_t n, uint64_t k) {
    if (k == 0 || k > n) return 1;
    Al<int8_t> aq(q, n); Al<float> as(s, n / 64);
    V8 *u = new V8(n, aq.p, as.p);       /* never destroyed, see the header */
    u->threshold(k);
    aq.out(q);
    return 0;
}

/* ================================================================ CloverVector16 (n half-precision bit patterns) */
void cref_v16_quantize(const float *x, uint64_t n, uint16_t *h) {
    Al<float> ax(x, n); Al<uint16_t> ah(NULL, n);
    CloverVector32 v(n, ax.p);
    V16 r(n, ah.p);
    r.quantize(v);
    ah.out(h);
}

void cref_v16_restore(const uint16_t *h, uint64_t n, float *x) {
    Al<uint16_t> ah(h, n); Al<float> ax(NULL, n);
    CloverVector32 v(n, ax.p);
    V16 u(n, ah.p);
    u.restore(v);
    ax.out(x);
}

float cref_v16_dot(const uint16_t *hu, const uint16_t *hv, uint64_t n) {
    Al<uint16_t> au(hu, n), av(hv, n);
    V16 u(n, au.p), v(n, av.p);
    return u.dot(v);
}

void cref_v16_scale_and_add(const uint16_t *hu, const uint16_t *hv, float a, uint64_t n, uint16_t *hr, int in_place) {
    Al<uint16_t> au(hu, n), av(hv, n), ar(NULL, n);
    V16 u(n, au.p), v(n, av.p), r(n, ar.p);
    if (in_place) { u.scaleAndAdd(v, a); au.out(hr); }
    else { u.scaleAndAdd(v, a, r); ar.out(hr); }
}

int cref_v16_threshold(uint16_t *h, uint64_t n, uint64_t k) {
    if (k == 0 || k > n) return 1;
    Al<uint16_t> ah(h, n);
    V16 *u = new V16(n, ah.p);           /* never destroyed, see the header */
    u->threshold(k);
    ah.out(h);
    return 0;
}

/* ================================================================ CloverVector32 */
float cref_v32_dot(const float *xu, const float *xv, uint64_t n) {
    Al<float> au(xu, n), av(xv, n);
    V32 u(n, au.p), v(n, av.p);
    return u.dot(v);
}

void cref_v32_scale_and_add(const float *xu, const float *xv, float a, uint64_t n, float *xr, int in_place) {
    Al<float> au(xu, n), av(xv, n), ar(NULL, n);
    V32 u(n, au.p), v(n, av.p), r(n, ar.p);
    if (in_place) { u.scaleAndAdd(v, a); au.out(xr); }
    else { u.scaleAndAdd(v, a, r); ar.out(xr); }
}

int cref_v32_threshold(float *x, uint64_t n, uint64_t k) {
    if (k == 0 || k > n) return 1;
    Al<float> ax(x, n);
    V32 *u = new V32(n, ax.p);           /* never destroyed, see the header */
    u->threshold(k);
    ax.out(x);
    return 0;
}

/* ================================================================ CloverMatrix4 (rows*cols/2 bytes, (rows/64)(cols/64) scales) */
void cref_m4_quantize(const float *A, uint64_t rows, uint64_t cols, int8_t *q, float *s, uint64_t *st) {
    CloverMatrix32 F(rows, cols);
    fill32(F, A, rows, cols);
    M4 m(rows, cols);
    m.load(st); m.quantize(F); m.store(st);
    m.take(q, s);
}

/* the three mvm forms draw from the matrix's generator */
void cref_m4_mvm(const int8_t *qA, const float *sA, uint64_t rows, uint64_t cols, const int8_t *qx, const float *sx, int8_t *qr, float *sr,
                 uint64_t *st) {
    M4 m(rows, cols);
    m.put(qA, sA);
    Al<int8_t> ax(qx, cols / 2), ar(NULL, rows / 2); Al<float> asx(sx, cols / 64), asr(NULL, rows / 64);
    V4 x(cols, ax.p, asx.p), r(rows, ar.p, asr.p);
    m.load(st); m.mvm(x, r); m.store(st);
    ar.out(qr); asr.out(sr);
}

void cref_m4_mvm_v8(const int8_t *qA, const float *sA, uint64_t rows, uint64_t cols, const int8_t *qx, const float *sx, int8_t *qr,
                    float *sr, uint64_t *st) {
    M4 m(rows, cols);
    m.put(qA, sA);
    Al<int8_t> ax(qx, cols), ar(NULL, rows); Al<float> asx(sx, cols / 64), asr(NULL, rows / 64);
    V8 x(cols, ax.p, asx.p), r(rows, ar.p, asr.p);
    m.load(st); m.mvm(x, r); m.store(st);
    ar.out(qr); asr.out(sr);
}

void cref_m4_mvm_f32(const int8_t *qA, const float *sA, uint64_t rows, uint64_t cols, const float *x, float *r) {
    M4 m(rows, cols);
    m.put(qA, sA);
    Al<float> ax(x, cols), ar(NULL, rows);
    V32 vx(cols, ax.p), vr(rows, ar.p);
    m.mvm(vx, vr);
    ar.out(r);
}

/* ================================================================ CloverMatrix8 (rows*cols bytes) */
void cref_m8_quantize(const float *A, uint64_t rows, uint64_t cols, int8_t *q, float *s, uint64_t *st) {
    CloverMatrix32 F(rows, cols);
    fill32(F, A, rows, cols);
    M8 m(rows, cols);
    m.load(st); m.quantize(F); m.store(st);
    m.take(q, s);
}

/* The reference has no restore() for this class, and its restore_scalar cannot run: the inner loop of CloverMatrix8.h:1304 advances i
 * instead of j and walks off the matrix.  What that loop means to store is get(i, j) (:117-129), the reference's own arithmetic for one
 * element; this calls it for every element. */
void cref_m8_restore(const int8_t *q, const float *s, uint64_t rows, uint64_t cols, float *A) {
    M8 m(rows, cols);
    m.put(q, s);
    for (uint64_t i = 0; i < rows; ++i)
        for (uint64_t j = 0; j < cols; ++j) A[i * cols + j] = m.get(i, j);
}

void cref_m8_mvm(const int8_t *qA, const float *sA, uint64_t rows, uint64_t cols, const int8_t *qx, const float *sx, int8_t *qr, float *sr,
                 uint64_t *st) {
    M8 m(rows, cols);
    m.put(qA, sA);
    Al<int8_t> ax(qx, cols), ar(NULL, rows); Al<float> asx(sx, cols / 64), asr(NULL, rows / 64);
    V8 x(cols, ax.p, asx.p), r(rows, ar.p, asr.p);
    m.load(st); m.mvm(x, r); m.store(st);
    ar.out(qr); asr.out(sr);
}

void cref_m8_mvm_f32(const int8_t *qA, const float *sA, uint64_t rows, uint64_t cols, const float *x, float *r) {
    M8 m(rows, cols);
    m.put(qA, sA);
    Al<float> ax(x, cols), ar(NULL, rows);
    V32 vx(cols, ax.p), vr(rows, ar.p);
    m.mvm(vx, vr);
    ar.out(r);
}

/* ================================================================ CloverMatrix16 (no restore method in the reference) */
void cref_m16_quantize(const float *A, uint64_t rows, uint64_t cols, uint16_t *h) {
    CloverMatrix32 F(rows, cols);
    fill32(F, A, rows, cols);
    M16 m(rows, cols);
    m.quantize(F);
    memcpy(h, m.getData(), rows * cols * sizeof(uint16_t));
}

void cref_m16_mvm(const uint16_t *hA, uint64_t rows, uint64_t cols, const uint16_t *hx, uint16_t *hr) {
    M16 m(rows, cols);
    memcpy(m.getData(), hA, rows * cols * sizeof(uint16_t));
    Al<uint16_t> ax(hx, cols), ar(NULL, rows);
    V16 x(cols, ax.p), r(rows, ar.p);
    m.mvm(x, r);
    ar.out(hr);
}

void cref_m16_mvm_f32(const uint16_t *hA, uint64_t rows, uint64_t cols, const float *x, float *r) {
    M16 m(rows, cols);
    memcpy(m.getData(), hA, rows * cols * sizeof(uint16_t));
    Al<float> ax(x, cols), ar(NULL, rows);
    V32 vx(cols, ax.p), vr(rows, ar.p);
    m.mvm(vx, vr);
    ar.out(r);
}


/* ================================================================ the IHT / GD loop, composed from the sequential methods in the order
 * the application loops document (residual, gradient, step, threshold): K = 0 runs GD (no threshold).  After every iteration x, t1, t2, t3
 * are appended to out_q / out_s (values / scales, in that order).  st: four generator states, for Phi, PhiT, x and y -- mvm draws from its
 * matrix, scaleAndAdd from the vector it is called on. */
}  /* extern "C" */

namespace {
template <class V> struct Bytes;
template <> struct Bytes<V4> { static size_t of(uint64_t n) { return n / 2; } };
template <> struct Bytes<V8> { static size_t of(uint64_t n) { return n; } };

template <class V> struct Held {
    Al<int8_t> q; Al<float> s; V *v;      /* v is never destroyed: x is thresholded, see the header */
    Held(const int8_t *q0, const float *s0, uint64_t n) : q(q0, Bytes<V>::of(n)), s(s0, n / 64), v(new V(n, q.p, s.p)) {}
    void append(int8_t *&oq, float *&os) const { memcpy(oq, q.p, q.n); oq += q.n; memcpy(os, s.p, s.n * sizeof(float)); os += s.n; }
};

template <class M, class V>
void run_loop(const int8_t *qPhi, const float *sPhi, const int8_t *qPhiT, const float *sPhiT, uint64_t m, uint64_t n, const int8_t *qy,
              const float *sy, uint64_t iterations, uint64_t K, float mu, int8_t *out_q, float *out_s, uint64_t *st) {
    M Phi(m, n), PhiT(n, m);
    Phi.put(qPhi, sPhi); PhiT.put(qPhiT, sPhiT);
    Held<V> x(NULL, NULL, n), y(qy, sy, m), t1(NULL, NULL, m), t2(NULL, NULL, m), t3(NULL, NULL, n);
    if (st) { Phi.load(st); PhiT.load(st + 8); x.v->load(st + 16); y.v->load(st + 24); }
    x.v->clear();
    for (uint64_t it = 0; it < iterations; ++it) {
        Phi.mvm(*x.v, *t1.v);
        y.v->scaleAndAdd(*t1.v, -1.0f, *t2.v);
        PhiT.mvm(*t2.v, *t3.v);
        x.v->scaleAndAdd(*t3.v, mu);
        if (K) x.v->threshold(K);
        x.append(out_q, out_s); t1.append(out_q, out_s); t2.append(out_q, out_s); t3.append(out_q, out_s);
    }
    if (st) { Phi.store(st); PhiT.store(st + 8); x.v->store(st + 16); y.v->store(st + 24); }
}
}  /* namespace */

extern "C" {

void cref_loop_m4v4(const int8_t *qPhi, const float *sPhi, const int8_t *qPhiT, const float *sPhiT, uint64_t m, uint64_t n, const int8_t *qy, const float *sy, uint64_t iterations, uint64_t K, float mu, int8_t *out_q, float *out_s, uint64_t *st) {
    run_loop<M4, V4>(qPhi, sPhi, qPhiT, sPhiT, m, n, qy, sy, iterations, K, mu, out_q, out_s, st);
}

void cref_loop_m4v8(const int8_t *qPhi, const float *sPhi, const int8_t *qPhiT, const float *sPhiT, uint64_t m, uint64_t n, const int8_t *qy, const float *sy, uint64_t iterations, uint64_t K, float mu, int8_t *out_q, float *out_s, uint64_t *st) {
    run_loop<M4, V8>(qPhi, sPhi, qPhiT, sPhiT, m, n, qy, sy, iterations, K, mu, out_q, out_s, st);
}

void cref_loop_m8v8(const int8_t *qPhi, const float *sPhi, const int8_t *qPhiT, const float *sPhiT, uint64_t m, uint64_t n, const int8_t *qy, const float *sy, uint64_t iterations, uint64_t K, float mu, int8_t *out_q, float *out_s, uint64_t *st) {
    run_loop<M8, V8>(qPhi, sPhi, qPhiT, sPhiT, m, n, qy, sy, iterations, K, mu, out_q, out_s, st);
}

/* half precision: no scales, no generator; out_h receives x, t1, t2, t3 after every iteration */
void cref_loop_m16v16(const uint16_t *hPhi, const uint16_t *hPhiT, uint64_t m, uint64_t n, const uint16_t *hy, uint64_t iterations, uint64_t K, float mu, uint16_t *out_h) {
    M16 Phi(m, n), PhiT(n, m);
    memcpy(Phi.getData(), hPhi, m * n * sizeof(uint16_t));
    memcpy(PhiT.getData(), hPhiT, m * n * sizeof(uint16_t));
    Al<uint16_t> ax(NULL, n), ay(hy, m), a1(NULL, m), a2(NULL, m), a3(NULL, n);
    V16 *x = new V16(n, ax.p);           /* never destroyed, see the header */
    V16 y(m, ay.p), t1(m, a1.p), t2(m, a2.p), t3(n, a3.p);
    x->clear();
    for (uint64_t it = 0; it < iterations; ++it) {
        Phi.mvm(*x, t1);
        y.scaleAndAdd(t1, -1.0f, t2);
        PhiT.mvm(t2, t3);
        x->scaleAndAdd(t3, mu);
        if (K) x->threshold(K);
        ax.out(out_h); out_h += n; a1.out(out_h); out_h += m; a2.out(out_h); out_h += m; a3.out(out_h); out_h += n;
    }
}

}  /* extern "C" */

#else  /* REF_CONTAINERS_MAIN */
/* ---------------------------------------------------------------------------------------------------------------------
 * clover_ref_gen <case directory> <golden directory>
 *
 * Reads <case directory>/manifest.txt (written by tests/ref_fixture_cases.py, with the input bytes next to it), runs every case through
 * the two libraries next to this program and writes the fixture files.  One manifest line per case:
 *     input <file> <name>      (what the case list calls the bytes in <file>)
 *     case <family> <op> <stochastic 0|1> <n> <rows> <cols> <k> <a bits, hex> <key1> <key2> <in_place> <iterations> <count> <input files> | <group> <case id, JSON string>
 * plus `file <name>` (start a fixture file) and `header <JSON members>` (copied into its head).  Quantised operands come from the
 * deterministic library's quantize of the float inputs; their digests are recorded so that a test knows it feeds the same bytes.
 *
 * A case's record is the SHA-256 of all its outputs in order (values before scales) followed, for stochastic rounding, by the generator
 * lanes afterwards -- or those bytes themselves in hex when there are at most 16 (a dot's float).  A fixture file holds "groups": {group:
 * SHA-256 of the records of its cases, in case order} (a group: one operation at one shape and one kind of rounding, over all data kinds),
 * "values": the records that are stored whole, "inputs_sha256": one digest over the digests of all input files in the order of their
 * names, and "operands_sha256": the same over the quantised operands (values then scales), named "<v|m><bits>:<input name>". */
#include <dlfcn.h>

#include <map>
#include <string>
#include <vector>

#include "simdxorshift128plus.h"      /* the reference's own seeding, from its generator header (compiled alone, as in ref_xorshift.cpp) */

#ifndef REF_FLAGS
#define REF_FLAGS "unknown"
#endif

namespace {

/* SHA-256 (FIPS 180-4) */
struct Sha256 {
    uint32_t h[8]; uint8_t buf[64]; uint64_t len; size_t fill;
    static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
    Sha256() : len(0), fill(0) {
        static const uint32_t init[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
        memcpy(h, init, sizeof h);
    }
    void block(const uint8_t *p) {
        static const uint32_t K[64] = {
            0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
            0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
            0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
            0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
            0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
            0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
        uint32_t w[64], a[8];
        for (int i = 0; i < 16; ++i) w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
        for (int i = 16; i < 64; ++i) {
            const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
            const uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
            w[i] = w[i - 16] + s0 + w[i - 7] + s1;
        }
        memcpy(a, h, sizeof a);
        for (int i = 0; i < 64; ++i) {
            const uint32_t S1 = rotr(a[4], 6) ^ rotr(a[4], 11) ^ rotr(a[4], 25), ch = (a[4] & a[5]) ^ (~a[4] & a[6]);
            const uint32_t t1 = a[7] + S1 + ch + K[i] + w[i];
            const uint32_t S0 = rotr(a[0], 2) ^ rotr(a[0], 13) ^ rotr(a[0], 22), mj = (a[0] & a[1]) ^ (a[0] & a[2]) ^ (a[1] & a[2]);
            const uint32_t t2 = S0 + mj;
            a[7] = a[6]; a[6] = a[5]; a[5] = a[4]; a[4] = a[3] + t1; a[3] = a[2]; a[2] = a[1]; a[1] = a[0]; a[0] = t1 + t2;
        }
        for (int i = 0; i < 8; ++i) h[i] += a[i];
    }
    void update(const uint8_t *p, size_t n) {
        len += n;
        while (n) {
            const size_t take = n < 64 - fill ? n : 64 - fill;
            memcpy(buf + fill, p, take); fill += take; p += take; n -= take;
            if (fill == 64) { block(buf); fill = 0; }
        }
    }
    std::string hex() {
        const uint64_t bits = len * 8;
        const uint8_t one = 0x80, zero = 0;
        update(&one, 1);
        while (fill != 56) update(&zero, 1);
        uint8_t be[8];
        for (int i = 0; i < 8; ++i) be[i] = (uint8_t)(bits >> (56 - 8 * i));
        update(be, 8);
        char out[65];
        for (int i = 0; i < 8; ++i) snprintf(out + 8 * i, 9, "%08x", h[i]);
        return std::string(out, 64);
    }
};

typedef std::vector<uint8_t> Bytes;
struct Blob { std::string name; Bytes b; };

std::string sha(const Bytes &b) { Sha256 s; s.update(b.data(), b.size()); return s.hex(); }

std::string hexs(const uint8_t *p, size_t n) {
    static const char d[] = "0123456789abcdef";
    std::string o(2 * n, '0');
    for (size_t i = 0; i < n; ++i) { o[2 * i] = d[p[i] >> 4]; o[2 * i + 1] = d[p[i] & 15]; }
    return o;
}

enum { WHOLE_MAX = 16 };      /* outputs of at most this many bytes (a dot's float) are stored whole, everything else as SHA-256 */

template <class T> Blob blob(const char *name, const std::vector<T> &v) {
    Blob b; b.name = name;
    b.b.assign((const uint8_t *)v.data(), (const uint8_t *)(v.data() + v.size()));
    return b;
}

Bytes read_file(const std::string &path) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) { fprintf(stderr, "clover_ref_gen: cannot read %s\n", path.c_str()); exit(2); }
    Bytes b;
    uint8_t tmp[1 << 16];
    size_t got;
    while ((got = fread(tmp, 1, sizeof tmp, f)) > 0) b.insert(b.end(), tmp, tmp + got);
    fclose(f);
    return b;
}

/* every function of the C ABI, once */
#define CREF_FUNCTIONS(X) \
    X(cref_stochastic) X(cref_v4_quantize) X(cref_v4_restore) X(cref_v4_dot) X(cref_v4_scale_and_add) X(cref_v4_threshold) \
    X(cref_v8_quantize) X(cref_v8_restore) X(cref_v8_dot) X(cref_v8_scale_and_add) X(cref_v8_threshold) \
    X(cref_v16_quantize) X(cref_v16_restore) X(cref_v16_dot) X(cref_v16_scale_and_add) X(cref_v16_threshold) \
    X(cref_v32_dot) X(cref_v32_scale_and_add) X(cref_v32_threshold) \
    X(cref_m4_quantize) X(cref_m4_mvm) X(cref_m4_mvm_v8) X(cref_m4_mvm_f32) \
    X(cref_m8_quantize) X(cref_m8_restore) X(cref_m8_mvm) X(cref_m8_mvm_f32) \
    X(cref_m16_quantize) X(cref_m16_mvm) X(cref_m16_mvm_f32) \
    X(cref_loop_m4v4) X(cref_loop_m4v8) X(cref_loop_m8v8) X(cref_loop_m16v16)

struct Lib {
    void *h;
#define CREF_MEMBER(name) decltype(&::name) name;
    CREF_FUNCTIONS(CREF_MEMBER)
#undef CREF_MEMBER
    explicit Lib(const std::string &path) {
        h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (!h) { fprintf(stderr, "clover_ref_gen: %s\n", dlerror()); exit(2); }
#define CREF_LOAD(name) name = (decltype(&::name))dlsym(h, #name); if (!name) { fprintf(stderr, "clover_ref_gen: %s lacks %s\n", path.c_str(), #name); exit(2); }
        CREF_FUNCTIONS(CREF_LOAD)
#undef CREF_LOAD
    }
};

typedef std::vector<float> F;
typedef std::vector<int8_t> I8;
typedef std::vector<uint16_t> H;

F as_floats(const Bytes &b) { F v(b.size() / 4); memcpy(v.data(), b.data(), v.size() * 4); return v; }

/* a quantised vector or matrix: values and scales (half precision: h) */
struct Q { I8 q; F s; H h; };

struct Case {
    std::string family, op, meta;
    int stochastic, in_place;
    uint64_t n, rows, cols, k, key1, key2, iterations;
    float a;
    std::vector<Bytes> in;
    std::vector<std::string> in_key;      /* what tests/ref_fixture_cases.py calls each input */
};

struct Result { std::vector<Blob> operands, outputs; std::vector<uint64_t> state; };

/* records a quantised operand under "<v|m><bits>:<input>": its values followed by its scales */
void operand(Result &r, const Case &c, int input, char kind, int bits, const Q &v) {
    char head[16];
    snprintf(head, sizeof head, "%c%d:", kind, bits);
    Blob b = v.h.empty() ? blob("", v.q) : blob("", v.h);
    b.b.insert(b.b.end(), (const uint8_t *)v.s.data(), (const uint8_t *)(v.s.data() + v.s.size()));
    b.name = head + c.in_key[input];
    r.operands.push_back(b);
}

/* deterministic quantize of a float input into the family's vector / matrix format */
Q quant_vec(const Lib &det, int bits, const F &x) {
    Q v; const uint64_t n = x.size();
    if (bits == 4) { v.q.resize(n / 2); v.s.resize(n / 64); det.cref_v4_quantize(x.data(), n, v.q.data(), v.s.data(), NULL); }
    else if (bits == 8) { v.q.resize(n); v.s.resize(n / 64); det.cref_v8_quantize(x.data(), n, v.q.data(), v.s.data(), NULL); }
    else { v.h.resize(n); det.cref_v16_quantize(x.data(), n, v.h.data()); }
    return v;
}

Q quant_mat(const Lib &det, int bits, const F &A, uint64_t rows, uint64_t cols) {
    Q m;
    if (bits == 4) { m.q.resize(rows * cols / 2); m.s.resize((rows / 64) * (cols / 64)); det.cref_m4_quantize(A.data(), rows, cols, m.q.data(), m.s.data(), NULL); }
    else if (bits == 8) { m.q.resize(rows * cols); m.s.resize((rows / 64) * (cols / 64)); det.cref_m8_quantize(A.data(), rows, cols, m.q.data(), m.s.data(), NULL); }
    else { m.h.resize(rows * cols); det.cref_m16_quantize(A.data(), rows, cols, m.h.data()); }
    return m;
}

void fail(const Case &c) { fprintf(stderr, "clover_ref_gen: no such case: %s %s\n", c.family.c_str(), c.op.c_str()); exit(2); }

Result run(const Lib &det, const Lib &L, const Case &c) {
    Result r;
    uint64_t *st = NULL;
    if (c.stochastic) {       /* up to four generators (the loops use all four); generator g is seeded (key1 + g, key2 + g) by the reference's own init */
        r.state.resize(32);
        st = r.state.data();
        for (int g = 0; g < 4; ++g) {
            __m256i p1, p2;
            avx_xorshift128plus_init(c.key1 + g, c.key2 + g, p1, p2);
            _mm256_storeu_si256((__m256i *)(st + 8 * g), p1);
            _mm256_storeu_si256((__m256i *)(st + 8 * g + 4), p2);
        }
    }
    const std::string &fam = c.family, &op = c.op;
    const int vbits = fam == "v4" ? 4 : fam == "v8" ? 8 : fam == "v16" ? 16 : fam == "v32" ? 32 : 0;
    const uint64_t n = c.n, rows = c.rows, cols = c.cols;
    if (vbits == 4 || vbits == 8) {
        const bool four = vbits == 4;
        const size_t vb = four ? n / 2 : n;
        if (op == "quantize") {
            const F x = as_floats(c.in[0]);
            I8 q(vb); F s(n / 64);
            (four ? L.cref_v4_quantize : L.cref_v8_quantize)(x.data(), n, q.data(), s.data(), st);
            r.outputs.push_back(blob("q", q)); r.outputs.push_back(blob("s", s));
            return r;
        }
        const Q u = quant_vec(det, vbits, as_floats(c.in[0]));
        operand(r, c, 0, 'v', vbits, u);
        if (op == "restore") {
            F x(n);
            (four ? L.cref_v4_restore : L.cref_v8_restore)(u.q.data(), u.s.data(), n, x.data());
            r.outputs.push_back(blob("x", x));
        } else if (op == "threshold") {
            I8 q = u.q;
            if ((four ? L.cref_v4_threshold : L.cref_v8_threshold)(q.data(), u.s.data(), n, c.k)) fail(c);
            r.outputs.push_back(blob("q", q));
        } else if (op == "dot" || op == "scale_and_add") {
            const Q v = quant_vec(det, vbits, as_floats(c.in[1]));
            operand(r, c, 1, 'v', vbits, v);
            if (op == "dot") {
                F d(1, (four ? L.cref_v4_dot : L.cref_v8_dot)(u.q.data(), u.s.data(), v.q.data(), v.s.data(), n));
                r.outputs.push_back(blob("dot", d));
            } else {
                I8 q(vb); F s(n / 64);
                (four ? L.cref_v4_scale_and_add : L.cref_v8_scale_and_add)(u.q.data(), u.s.data(), v.q.data(), v.s.data(), c.a, n, q.data(), s.data(), st, c.in_place);
                r.outputs.push_back(blob("q", q)); r.outputs.push_back(blob("s", s));
            }
        } else fail(c);
        return r;
    }
    if (vbits == 16) {
        if (op == "quantize") {
            const F x = as_floats(c.in[0]);
            H h(n);
            L.cref_v16_quantize(x.data(), n, h.data());
            r.outputs.push_back(blob("h", h));
            return r;
        }
        const Q u = quant_vec(det, 16, as_floats(c.in[0]));
        operand(r, c, 0, 'v', 16, u);
        if (op == "restore") { F x(n); L.cref_v16_restore(u.h.data(), n, x.data()); r.outputs.push_back(blob("x", x)); }
        else if (op == "threshold") { H h = u.h; if (L.cref_v16_threshold(h.data(), n, c.k)) fail(c); r.outputs.push_back(blob("h", h)); }
        else if (op == "dot" || op == "scale_and_add") {
            const Q v = quant_vec(det, 16, as_floats(c.in[1]));
            operand(r, c, 1, 'v', 16, v);
            if (op == "dot") { F d(1, L.cref_v16_dot(u.h.data(), v.h.data(), n)); r.outputs.push_back(blob("dot", d)); }
            else { H h(n); L.cref_v16_scale_and_add(u.h.data(), v.h.data(), c.a, n, h.data(), c.in_place); r.outputs.push_back(blob("h", h)); }
        } else fail(c);
        return r;
    }
    if (vbits == 32) {
        const F u = as_floats(c.in[0]);
        if (op == "threshold") { F x = u; if (L.cref_v32_threshold(x.data(), n, c.k)) fail(c); r.outputs.push_back(blob("x", x)); return r; }
        const F v = as_floats(c.in[1]);
        if (op == "dot") { F d(1, L.cref_v32_dot(u.data(), v.data(), n)); r.outputs.push_back(blob("dot", d)); }
        else if (op == "scale_and_add") { F x(n); L.cref_v32_scale_and_add(u.data(), v.data(), c.a, n, x.data(), c.in_place); r.outputs.push_back(blob("x", x)); }
        else fail(c);
        return r;
    }
    const int mbits = fam == "m4" ? 4 : fam == "m8" ? 8 : fam == "m16" ? 16 : 0;
    if (mbits) {
        const F A = as_floats(c.in[0]);
        if (op == "quantize") {
            if (mbits == 16) { H h(rows * cols); L.cref_m16_quantize(A.data(), rows, cols, h.data()); r.outputs.push_back(blob("h", h)); return r; }
            I8 q(mbits == 4 ? rows * cols / 2 : rows * cols); F s((rows / 64) * (cols / 64));
            (mbits == 4 ? L.cref_m4_quantize : L.cref_m8_quantize)(A.data(), rows, cols, q.data(), s.data(), st);
            r.outputs.push_back(blob("q", q)); r.outputs.push_back(blob("s", s));
            return r;
        }
        const Q m = quant_mat(det, mbits, A, rows, cols);
        operand(r, c, 0, 'm', mbits, m);
        if (op == "restore" && mbits == 8) {
            F B(rows * cols);
            L.cref_m8_restore(m.q.data(), m.s.data(), rows, cols, B.data());
            r.outputs.push_back(blob("A", B));
            return r;
        }
        const F xf = as_floats(c.in[1]);
        if (op == "mvm_f32") {
            F y(rows);
            if (mbits == 4) L.cref_m4_mvm_f32(m.q.data(), m.s.data(), rows, cols, xf.data(), y.data());
            else if (mbits == 8) L.cref_m8_mvm_f32(m.q.data(), m.s.data(), rows, cols, xf.data(), y.data());
            else L.cref_m16_mvm_f32(m.h.data(), rows, cols, xf.data(), y.data());
            r.outputs.push_back(blob("r", y));
            return r;
        }
        if (op == "mvm" && mbits == 16) {
            const Q x = quant_vec(det, 16, xf);
            operand(r, c, 1, 'v', 16, x);
            H y(rows);
            L.cref_m16_mvm(m.h.data(), rows, cols, x.h.data(), y.data());
            r.outputs.push_back(blob("h", y));
            return r;
        }
        const int xbits = op == "mvm" ? mbits : op == "mvm_v8" && mbits == 4 ? 8 : 0;
        if (!xbits) fail(c);
        const Q x = quant_vec(det, xbits, xf);
        operand(r, c, 1, 'v', xbits, x);
        I8 q(xbits == 4 ? rows / 2 : rows); F s(rows / 64);
        (mbits == 8 ? L.cref_m8_mvm : xbits == 4 ? L.cref_m4_mvm : L.cref_m4_mvm_v8)(m.q.data(), m.s.data(), rows, cols, x.q.data(), x.s.data(), q.data(), s.data(), st);
        r.outputs.push_back(blob("q", q)); r.outputs.push_back(blob("s", s));
        return r;
    }
    if (fam == "loop") {       /* inputs: Phi (rows x cols), its transpose (transposed as floats by the case list), y (rows) */
        const int mb = op == "m8v8" ? 8 : op == "m16v16" ? 16 : 4, vb = op == "m4v4" ? 4 : op == "m16v16" ? 16 : 8;
        const Q Phi = quant_mat(det, mb, as_floats(c.in[0]), rows, cols), PhiT = quant_mat(det, mb, as_floats(c.in[1]), cols, rows);
        const Q y = quant_vec(det, vb, as_floats(c.in[2]));
        operand(r, c, 0, 'm', mb, Phi); operand(r, c, 1, 'm', mb, PhiT); operand(r, c, 2, 'v', vb, y);
        const uint64_t elems = 2 * (rows + cols) * c.iterations;
        if (vb == 16) {
            H out(elems);
            L.cref_loop_m16v16(Phi.h.data(), PhiT.h.data(), rows, cols, y.h.data(), c.iterations, c.k, c.a, out.data());
            r.outputs.push_back(blob("trace.h", out));
            return r;
        }
        I8 oq(vb == 4 ? elems / 2 : elems); F os(elems / 64);
        (op == "m4v4" ? L.cref_loop_m4v4 : op == "m4v8" ? L.cref_loop_m4v8 : op == "m8v8" ? L.cref_loop_m8v8 : (fail(c), L.cref_loop_m8v8))(
            Phi.q.data(), Phi.s.data(), PhiT.q.data(), PhiT.s.data(), rows, cols, y.q.data(), y.s.data(), c.iterations, c.k, c.a, oq.data(), os.data(), st);
        r.outputs.push_back(blob("trace.q", oq)); r.outputs.push_back(blob("trace.s", os));
        return r;
    }
    fail(c);
    return r;
}

}  /* namespace */

/* one fixture file: one digest over all inputs, one over all quantised operands, one per group of cases, and the small records whole */
struct Out {
    FILE *f;
    std::map<std::string, std::string> inputs, operands, values;
    std::vector<std::string> order;
    std::map<std::string, std::string> group;      /* group -> its cases' records, concatenated in case order */
    Out() : f(NULL) {}
    static std::string over(const std::map<std::string, std::string> &t) {      /* the digests of a table, in the order of its names */
        std::string all;
        for (std::map<std::string, std::string>::const_iterator i = t.begin(); i != t.end(); ++i) all += i->second;
        return sha(Bytes(all.begin(), all.end()));
    }
    void close() {
        if (!f) return;
        for (size_t i = 0; i < order.size(); ++i) {
            const std::string &g = group[order[i]];
            fprintf(f, "%s\n  \"%s\": \"%s\"", i ? "," : "", order[i].c_str(), sha(Bytes(g.begin(), g.end())).c_str());
        }
        fprintf(f, "\n },\n \"values\": {");
        for (std::map<std::string, std::string>::const_iterator i = values.begin(); i != values.end(); ++i)
            fprintf(f, "%s\n  %s: \"%s\"", i == values.begin() ? "" : ",", i->first.c_str(), i->second.c_str());
        fprintf(f, "\n },\n \"inputs_sha256\": \"%s\",\n \"operands_sha256\": \"%s\"\n}\n", over(inputs).c_str(), over(operands).c_str());
        fclose(f);
        *this = Out();
    }
};

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <case directory> <golden directory>\n", argv[0]); return 2; }
    const std::string dir = argv[1], out_dir = argv[2];
    std::string self = argv[0];
    const size_t slash = self.rfind('/');
    const std::string here = slash == std::string::npos ? std::string(".") : self.substr(0, slash);
    const Lib det(here + "/libclover_ref_norng.so"), sto(here + "/libclover_ref.so");
    if (det.cref_stochastic() || !sto.cref_stochastic()) { fprintf(stderr, "clover_ref_gen: the two libraries are not the two roundings\n"); return 2; }

    FILE *man = fopen((dir + "/manifest.txt").c_str(), "r");
    if (!man) { fprintf(stderr, "clover_ref_gen: no manifest in %s\n", dir.c_str()); return 2; }
    Out out;
    std::map<std::string, std::string> key_of;      /* input file -> its name in the case list */
    std::vector<char> line(1 << 16);
    while (fgets(line.data(), (int)line.size(), man)) {
        std::string l(line.data());
        while (!l.empty() && (l[l.size() - 1] == '\n' || l[l.size() - 1] == '\r')) l.erase(l.size() - 1);
        if (l.compare(0, 5, "file ") == 0) {
            out.close();
            out.f = fopen((out_dir + "/" + l.substr(5)).c_str(), "w");
            if (!out.f) { fprintf(stderr, "clover_ref_gen: cannot write %s\n", l.substr(5).c_str()); return 2; }
        } else if (l.compare(0, 6, "input ") == 0) {
            const size_t sp = l.find(' ', 6);
            key_of[l.substr(6, sp - 6)] = l.substr(sp + 1);
        } else if (l.compare(0, 7, "header ") == 0 && out.f) {
            fprintf(out.f, "{\n \"generator\": \"oracle/ref_containers.cpp over the reference's include/Clover*.h (make -C oracle ref-fixtures)\",\n"
                           " \"flags\": \"%s\",\n \"whole_max\": %d,\n %s,\n \"groups\": {", REF_FLAGS, (int)WHOLE_MAX, l.substr(7).c_str());
        } else if (l.compare(0, 5, "case ") == 0 && out.f) {
            Case c;
            char fam[32], op[32];
            unsigned abits;
            int used = 0, count = 0;
            unsigned long long n, rows, cols, k, key1, key2, iters;
            if (sscanf(l.c_str(), "case %31s %31s %d %llu %llu %llu %llu %x %llu %llu %d %llu %d%n", fam, op, &c.stochastic, &n, &rows, &cols, &k, &abits,
                       &key1, &key2, &c.in_place, &iters, &count, &used) != 13) { fprintf(stderr, "clover_ref_gen: bad line: %s\n", l.c_str()); return 2; }
            c.family = fam; c.op = op; c.n = n; c.rows = rows; c.cols = cols; c.k = k; c.key1 = key1; c.key2 = key2; c.iterations = iters;
            memcpy(&c.a, &abits, 4);
            const size_t bar = l.find(" | ", used);
            if (bar == std::string::npos) { fprintf(stderr, "clover_ref_gen: bad line: %s\n", l.c_str()); return 2; }
            c.meta = l.substr(bar + 3);                                   /* <group> <case id as a JSON string> */
            const std::string grp = c.meta.substr(0, c.meta.find(' ')), id = c.meta.substr(c.meta.find(' ') + 1);
            std::string files = l.substr(used, bar - used);
            for (int i = 0; i < count; ++i) {
                const size_t b = files.find_first_not_of(' '), e = files.find(' ', b);
                const std::string file = files.substr(b, e == std::string::npos ? e : e - b);
                c.in.push_back(read_file(dir + "/" + file));
                c.in_key.push_back(key_of[file]);
                if (!out.inputs.count(c.in_key.back())) out.inputs[c.in_key.back()] = sha(c.in.back());
                files = e == std::string::npos ? std::string() : files.substr(e);
            }
            const Result r = run(det, c.stochastic ? sto : det, c);
            for (size_t i = 0; i < r.operands.size(); ++i)
                if (!out.operands.count(r.operands[i].name)) out.operands[r.operands[i].name] = sha(r.operands[i].b);
            /* the record: every output in order, then the generator lanes afterwards (one generator; the loops: all four) */
            Bytes all;
            for (size_t i = 0; i < r.outputs.size(); ++i) all.insert(all.end(), r.outputs[i].b.begin(), r.outputs[i].b.end());
            if (c.stochastic) {
                const uint8_t *st = (const uint8_t *)r.state.data();
                all.insert(all.end(), st, st + 8 * (c.family == "loop" ? 32 : 8));
            }
            const std::string rec = all.size() <= WHOLE_MAX ? hexs(all.data(), all.size()) : sha(all);
            if (!out.group.count(grp)) out.order.push_back(grp);
            out.group[grp] += rec;
            if (all.size() <= WHOLE_MAX) out.values[id] = rec;
        }
    }
    out.close();
    fclose(man);
    return 0;
}
#endif
