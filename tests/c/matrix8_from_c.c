/* matrix8_from_c.c -- the CloverMatrix8 calls from C99 (gcc, not g++) against include/clover_hip.h alone.
 * With a GPU: a 128 x 128 matrix of 2.0f and a vector of 1.0f are quantized (clm8_quantize, clv8_quantize), multiplied
 * (clm8_mvm, clm8_mvm_f32), transposed and restored; every row value is 2 * 128 = 256 up to fp32 rounding, which the program prints.  A bad shape
 * returns CLV_ERR_INVALID with a message.  Without a device it reports the status text and exits 0. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "clover_hip.h"

#define CHECK(call)                                                                       \
    do {                                                                                  \
        if ((call) != CLV_OK) {                                                           \
            printf("error %s: %s\n", #call, clv_last_error());                            \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

int main(void)
{
    int count = 0;
    if (clv_device_count(&count) != CLV_OK || count < 1) {
        printf("no_device status_text=%s\n", clv_last_error());
        return 0;
    }
    enum { N = 128 };
    static float hA[N * N], hx[N], hr[N], hback[N * N];
    signed char hq[N];
    float hs[N / 64];
    void *A, *x, *qA, *sA, *qT, *sT, *qx, *sx, *r, *sr, *rf, *back;
    for (int i = 0; i < N * N; i++) hA[i] = 2.0f;
    for (int i = 0; i < N; i++) hx[i] = 1.0f;
    CHECK(clv_malloc(&A, sizeof hA));
    CHECK(clv_malloc(&x, sizeof hx));
    CHECK(clv_malloc(&qA, N * N));
    CHECK(clv_malloc(&sA, 4 * sizeof(float)));
    CHECK(clv_malloc(&qT, N * N));
    CHECK(clv_malloc(&sT, 4 * sizeof(float)));
    CHECK(clv_malloc(&qx, N));
    CHECK(clv_malloc(&sx, (N / 64) * sizeof(float)));
    CHECK(clv_malloc(&r, N));
    CHECK(clv_malloc(&sr, (N / 64) * sizeof(float)));
    CHECK(clv_malloc(&rf, N * sizeof(float)));
    CHECK(clv_malloc(&back, sizeof hback));
    CHECK(clv_memcpy_h2d(A, hA, sizeof hA, NULL));
    CHECK(clv_memcpy_h2d(x, hx, sizeof hx, NULL));
    CHECK(clm8_quantize((const float *)A, N, N, (int8_t *)qA, (float *)sA, NULL, NULL));
    CHECK(clv8_quantize((const float *)x, N, (int8_t *)qx, (float *)sx, NULL, NULL));
    CHECK(clm8_transpose((const int8_t *)qA, (const float *)sA, N, N, (int8_t *)qT, (float *)sT, NULL));
    CHECK(clm8_mvm((const int8_t *)qT, (const float *)sT, N, N, (const int8_t *)qx, (const float *)sx, (int8_t *)r, (float *)sr, NULL, NULL));
    CHECK(clm8_mvm_f32((const int8_t *)qA, (const float *)sA, N, N, (const float *)x, (float *)rf, NULL));
    CHECK(clm8_restore((const int8_t *)qA, (const float *)sA, N, N, (float *)back, NULL));
    CHECK(clv_memcpy_d2h(hr, rf, sizeof hr, NULL));
    CHECK(clv_memcpy_d2h(hq, r, sizeof hq, NULL));
    CHECK(clv_memcpy_d2h(hs, sr, sizeof hs, NULL));
    CHECK(clv_memcpy_d2h(hback, back, sizeof hback, NULL));
    CHECK(clv_device_sync());
    int ok = hq[0] == 127 && hq[N - 1] == 127 && fabsf(hs[0] - 256.0f) < 1e-3f && fabsf(hback[0] - 2.0f) < 1e-6f &&
             fabsf(hback[N * N - 1] - 2.0f) < 1e-6f;
    for (int i = 0; i < N; i++) ok = ok && fabsf(hr[i] - 256.0f) < 1e-3f;
    const int bad = clm8_quantize((const float *)A, 100, N, (int8_t *)qA, (float *)sA, NULL, NULL);
    printf("mvm=%.1f ok=%d bad_shape=%d msg=%s\n", hr[0], ok, bad, clv_last_error());
    void *bufs[] = {A, x, qA, sA, qT, sT, qx, sx, r, sr, rf, back};
    for (unsigned i = 0; i < sizeof bufs / sizeof bufs[0]; i++) clv_free(bufs[i]);
    return ok && bad == CLV_ERR_INVALID ? 0 : 1;
}
