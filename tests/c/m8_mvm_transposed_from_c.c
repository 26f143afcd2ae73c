/* A C99 client of clm8_mvm_transposed, clm8_mvm_transposed_scale_and_add and clm8_iht_one_matrix (include/clover_hip.h): compiles with
 * -pedantic, links, and asks the argument checks, which answer before any device work -- the addresses below are never dereferenced. */
#include <stdio.h>
#include <string.h>

#include "clover_hip.h"

#define AT(i) (0x10000000u + ((unsigned)(i) << 20))

int main(void)
{
    const int8_t *A = (const int8_t *)AT(0), *x = (const int8_t *)AT(2), *qu = (const int8_t *)AT(4);
    const float *sA = (const float *)AT(1), *sx = (const float *)AT(3), *su = (const float *)AT(5);
    int8_t *t = (int8_t *)AT(6), *r = (int8_t *)AT(8);
    float *st = (float *)AT(7), *sr = (float *)AT(9);
    int ok = 1, rc;
    rc = clm8_mvm_transposed(A, sA, 128, 192, x, sx, r, sr, NULL, NULL);
    ok = ok && rc == CLV_ERR_INVALID && strstr(clv_last_error(), "clm8_mvm_transposed:") != NULL;
    rc = clm8_mvm_transposed(A, sA, 128, 128, x, sx, (int8_t *)(AT(2) + 127), sr, NULL, NULL);           /* r meets the last byte of x */
    ok = ok && rc == CLV_ERR_INVALID && strstr(clv_last_error(), "overlaps") != NULL;
    rc = clm8_mvm_transposed(A, sA, 128, 128, x, sx, (int8_t *)(AT(0) + 128 * 128 - 1), sr, NULL, NULL); /* r meets the last byte of A */
    ok = ok && rc == CLV_ERR_INVALID && strstr(clv_last_error(), "overlaps") != NULL;
    rc = clm8_mvm_transposed_scale_and_add(A, sA, 128, 128, x, sx, qu, su, 0.5f, t, NULL, r, sr, NULL, NULL);
    ok = ok && rc == CLV_ERR_INVALID && strstr(clv_last_error(), "clm8_mvm_transposed_scale_and_add") != NULL;
    rc = clm8_iht_one_matrix(A, sA, 128, 128, r, sr, 128, x, sx, t, st, (int8_t *)AT(10), (float *)AT(11), (int8_t *)AT(12), NULL, 3, 8, 0.5f, 1,
                             NULL, NULL);
    ok = ok && rc == CLV_ERR_INVALID && strstr(clv_last_error(), "clm8_iht_one_matrix") != NULL;
    rc = clm8_mvm_transposed(A, sA, 0, 128, x, sx, r, sr, NULL, NULL);                                   /* rows == 0: checked, nothing runs */
    ok = ok && rc == CLV_OK;
    rc = clm8_mvm_transposed_scale_and_add(A, sA, 128, 0, x, sx, qu, su, 0.5f, NULL, NULL, r, sr, NULL, NULL);
    ok = ok && rc == CLV_OK;
    printf("ok=%d\n", ok);
    return ok ? 0 : 1;
}
