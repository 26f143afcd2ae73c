/* matrix8_exact64.c -- float64 definitions of CloverMatrix8's two mvm forms, for the error bounds of tests/test_matrix8_scale.py and
 * tests/test_matrix8.py.  They share nothing with tests/matrix8_restate.c: no chain order, no fp32 rounding.  Per row they return
 * the value itself and the sum of the magnitudes of its terms, the quantity a rounding-error bound is proportional to.
 *
 *   x64_mvm8:    sum over blocks b of (su_b / 127) (sv_b / 127) * sum_{j in b} q_j x_j          (the 64 byte products exactly)
 *   x64_mvm_f32: sum over j of x_j (s_b(j) / 127) q_j
 *
 * The integer block sums are exact, and each float64 operation is good to 2^-53, far below the fp32 bounds being checked.
 * Built with  cc -O2 -fopenmp  (at most 16 threads) by tests/matrix8_helpers.py. */
#include <stdint.h>
#include <stdlib.h>
#ifdef _OPENMP
#include <omp.h>
#endif

static inline int x64_threads(void)
{
#ifdef _OPENMP
    const int n = omp_get_max_threads();
    return n < 16 ? n : 16;
#else
    return 1;
#endif
}

void x64_mvm8(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const int8_t *x, const float *sx, double *exact,
              double *absum)
{
    const uint64_t hb = cols >> 6;
#pragma omp parallel for num_threads(x64_threads())
    for (uint64_t i = 0; i < rows; i++) {
        const int8_t *u = A + i * cols;
        const float *su = sA + (i >> 6) * hb;
        double e = 0.0, a = 0.0;
        for (uint64_t b = 0; b < hb; b++) {
            int64_t d = 0, ad = 0;
            for (uint64_t j = 64 * b; j < 64 * b + 64; j++) {
                const int32_t p = (int32_t)u[j] * (int32_t)x[j];
                d += p;
                ad += p < 0 ? -p : p;
            }
            const double c = ((double)su[b] / 127.0) * ((double)sx[b] / 127.0);
            e += c * (double)d;
            a += c * (double)ad;
        }
        exact[i] = e;
        absum[i] = a;
    }
}

void x64_mvm_f32(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, double *exact, double *absum)
{
    const uint64_t hb = cols >> 6;
#pragma omp parallel for num_threads(x64_threads())
    for (uint64_t i = 0; i < rows; i++) {
        const int8_t *u = A + i * cols;
        const float *su = sA + (i >> 6) * hb;
        double e = 0.0, a = 0.0;
        for (uint64_t b = 0; b < hb; b++) {
            const double f = (double)su[b] / 127.0;
            double eb = 0.0, ab = 0.0;
            for (uint64_t j = 64 * b; j < 64 * b + 64; j++) {
                const double t = (double)x[j] * (double)u[j];
                eb += t;
                ab += t < 0 ? -t : t;
            }
            e += f * eb;
            a += f * ab;
        }
        exact[i] = e;
        absum[i] = a;
    }
}
