/* A C99 client of the batched transposed mixed calls (CloverMatrix4 x CloverVector8) (include/clover_hip_batch_t_v8.h): compiles with -pedantic, links, and asks the
 * argument checks, which answer before any device work -- the addresses below are never dereferenced. */
#include <stdio.h>
#include <string.h>

#include "clover_hip_batch_t_v8.h"

int main(void)
{
    const int8_t *x[2], *qu[2];
    const float *sx[2], *su[2];
    int8_t *r[2], *t[2];
    float *sr[2], *st[2];
    const int8_t *A = (const int8_t *)0x10000000;
    const float *sA = (const float *)0x10100000;
    uint64_t *rng = (uint64_t *)0x10900000;
    uint64_t before = clv_mvm_batch_launches();
    int ok = 1, rc;
    x[0] = (const int8_t *)0x10200000; x[1] = (const int8_t *)0x10300000;
    sx[0] = (const float *)0x10400000; sx[1] = (const float *)0x10500000;
    r[0] = (int8_t *)0x10600000; r[1] = NULL;
    sr[0] = (float *)0x10700000; sr[1] = (float *)0x10800000;
    qu[0] = (const int8_t *)0x10a00000; qu[1] = (const int8_t *)0x10b00000;
    su[0] = (const float *)0x10c00000; su[1] = (const float *)0x10d00000;
    t[0] = (int8_t *)0x10e00000; t[1] = (int8_t *)0x10f00000;
    st[0] = (float *)0x11000000; st[1] = (float *)0x11100000;
    rc = clm4_mvm_v8_transposed_batch(A, sA, 128, 256, 2, x, sx, r, sr, NULL, NULL);
    ok = ok && rc == CLV_ERR_INVALID && strstr(clv_last_error(), "clm4_mvm_v8_transposed_batch") != NULL && strstr(clv_last_error(), "vector 1") != NULL;
    r[1] = (int8_t *)0x10680000;
    rc = clm4_mvm_v8_transposed_batch_at(A, sA, 128, 256, 2, x, sx, r, sr, rng, (uint64_t)1 << 55, 8, 16, NULL);
    ok = ok && rc == CLV_ERR_INVALID && strstr(clv_last_error(), "2^55") != NULL;
    rc = clm4_mvm_v8_transposed_scale_and_add_batch(A, sA, 128, 256, 2, x, sx, qu, su, 0.5f, t, NULL, r, sr, NULL, NULL);
    ok = ok && rc == CLV_ERR_INVALID && strstr(clv_last_error(), "t and st") != NULL;
    r[1] = (int8_t *)0x10200000 + 127;                                                /* the last byte of x[0]: 128 rows = 128 bytes */
    rc = clm4_mvm_v8_transposed_scale_and_add_batch(A, sA, 128, 256, 2, x, sx, qu, su, 0.5f, t, st, r, sr, NULL, NULL);
    ok = ok && rc == CLV_ERR_INVALID && strstr(clv_last_error(), "overlaps") != NULL;
    r[1] = (int8_t *)0x10680000;
    rc = clm4_iht_v8_batch_one_matrix(A, sA, 64, 128, 2, r, sr, 128, x, sx, t, st, t, st, t, st, 3, 8, 0.5f, 1, NULL, NULL);
    ok = ok && rc == CLV_ERR_INVALID && strstr(clv_last_error(), "clm4_iht_v8_batch_one_matrix") != NULL;
    rc = clm4_mvm_v8_transposed_batch_at(A, sA, 0, 256, 2, x, sx, r, sr, rng, 0, 8, 16, NULL);   /* rows == 0: checked, nothing runs */
    ok = ok && rc == CLV_OK && clv_mvm_batch_launches() == before;
    printf("ok=%d\n", ok);
    return ok ? 0 : 1;
}
