// fp32_restate.cpp -- the CPU reference of the fp32 device tests: extern "C" wrappers around the functions of include/clover_fp32.h (which
// tests/test_fp32_baseline.py pins), plus the float64 sums the FAST dot is bounded against and the IHT / GD loop made of those functions.
// Built twice by tests/fp32_helpers.py: -O2 -ffp-contract=off -fno-fast-math, and the same with -mfma -fopenmp (at most 16 threads).
#include "clover_fp32.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#if defined(_OPENMP)
#include <omp.h>
namespace {
struct ThreadCap {
    ThreadCap() { if (omp_get_max_threads() > 16) omp_set_num_threads(16); }
} thread_cap;
}
#endif

extern "C" {

float rf_dot(const float *u, const float *v, uint64_t n) { return clover_fp32::dot_chains32(u, v, n); }
float rf_dot_sequential(const float *u, const float *v, uint64_t n) { return clover_fp32::dot_sequential(u, v, n); }

// float64: a product of two fp32 values is exact (48 bits); the sums carry a relative error of n 2^-53, nothing beside the 2^-24 bounds
void rf_dot64(const float *u, const float *v, uint64_t n, double *exact, double *absum)
{
    double e = 0.0, a = 0.0;
    for (uint64_t i = 0; i < n; i++) {
        const double p = (double)u[i] * (double)v[i];
        e += p;
        a += std::fabs(p);
    }
    *exact = e;
    *absum = a;
}

void rf_scale_and_add(const float *u, const float *v, float s, float *r, uint64_t n) { clover_fp32::axpy_fma(u, v, s, r, n, true); }
void rf_mvm(const float *A, uint64_t rows, uint64_t cols, const float *x, float *y) { clover_fp32::mvm_rows(A, rows, cols, x, y, true); }
void rf_mvm_sequential(const float *A, uint64_t rows, uint64_t cols, const float *x, float *y)
{
    for (uint64_t i = 0; i < rows; i++) y[i] = clover_fp32::dot_sequential(A + i * cols, x, cols);
}
void rf_transpose(const float *in, uint64_t rows, uint64_t cols, float *out) { clover_fp32::transpose(in, rows, cols, out, true); }
void rf_threshold(float *x, uint64_t n, uint64_t k) { clover_fp32::keep_top_k(x, n, k); }

// Q_IHT / Q_GD on the host, one shim function per step: x.clear(); t1 = Phi x; t2 = y - t1; t3 = PhiT t2; x += mu t3; threshold(K) over the
// first x_len elements when `threshold` is set.  zeroed[it] = how many non-zero elements iteration it's threshold cleared.
void rf_iht(const float *Phi, const float *PhiT, uint64_t m, uint64_t n, float *x, uint64_t x_len, const float *y, float *t1, float *t2, float *t3,
            uint64_t iterations, uint64_t K, float mu, int threshold, uint64_t *zeroed)
{
    std::memset(x, 0, n * sizeof(float));
    for (uint64_t it = 0; it < iterations; it++) {
        clover_fp32::mvm_rows(Phi, m, n, x, t1, true);
        clover_fp32::axpy_fma(y, t1, -1.0f, t2, m, true);
        clover_fp32::mvm_rows(PhiT, n, m, t2, t3, true);
        clover_fp32::axpy_fma(x, t3, mu, x, n, true);
        if (threshold) {
            uint64_t before = 0, after = 0;
            for (uint64_t i = 0; i < x_len; i++) before += x[i] != 0.0f;
            clover_fp32::keep_top_k(x, x_len, K);
            for (uint64_t i = 0; i < x_len; i++) after += x[i] != 0.0f;
            if (zeroed) zeroed[it] = before - after;
        }
    }
}

}  // extern "C"
