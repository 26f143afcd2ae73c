/*
 * mkl.h -- declarations only (TEST INFRASTRUCTURE, own text).  See ipp.h in this directory for the rule.
 */
#ifndef CLOVER_REF_SHIM_MKL_H
#define CLOVER_REF_SHIM_MKL_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { CblasRowMajor = 101, CblasColMajor = 102 } CBLAS_LAYOUT;
typedef enum { CblasNoTrans = 111, CblasTrans = 112 } CBLAS_TRANSPOSE;

/* library start-up (shim.cpp: no-ops) */
void mkl_get_version_string(char *buf, int len);
void mkl_set_num_threads(int n);

/* computing functions (shim.cpp: abort) */
void cblas_sgemv(CBLAS_LAYOUT layout, CBLAS_TRANSPOSE trans, int m, int n, float alpha, const float *a, int lda,
                 const float *x, int incx, float beta, float *y, int incy);
void mkl_somatcopy(char ordering, char trans, size_t rows, size_t cols, float alpha, const float *a, size_t lda,
                   float *b, size_t ldb);

#ifdef __cplusplus
}
#endif

#endif /* CLOVER_REF_SHIM_MKL_H */
