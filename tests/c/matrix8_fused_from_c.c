/* matrix8_fused_from_c.c -- clm8_mvm_scale_and_add and clm8_iht from C99 (gcc, not g++) against include/clover_hip.h alone.
 * With a GPU: A = 128 x 128 of 2.0f, x = u = 1.0f (quantized by clm8_quantize / clv8_quantize).  t = quantize8(A x) has every byte at the top of
 * the range and scale 256; r = quantize8(u - t) every byte at the bottom and scale 255; the in-place form with t = NULL leaves the same r in u.  clm8_iht
 * with 0 iterations clears x (bytes 0, scales 1.0) and leaves t1 alone.  A bad shape returns CLV_ERR_INVALID with a message.  Without a
 * device the program reports the status text and exits 0. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
    enum { N = 128, NS = N / 64 };
    static float hA[N * N], hx[N];
    signed char ht[N], hr[N], hu[N], hxc[N], ht1[N];
    float hst[NS], hsr[NS], hsu[NS], hsx[NS];
    void *A, *x, *qA, *sA, *qx, *sx, *qu, *su, *t, *st, *r, *sr, *t1, *st1, *t2, *st2, *t3, *st3, *xi, *sxi;
    for (int i = 0; i < N * N; i++) hA[i] = 2.0f;
    for (int i = 0; i < N; i++) hx[i] = 1.0f;
    CHECK(clv_malloc(&A, sizeof hA));
    CHECK(clv_malloc(&x, sizeof hx));
    CHECK(clv_malloc(&qA, N * N));
    CHECK(clv_malloc(&sA, NS * NS * sizeof(float)));
    void **vecs[] = {&qx, &qu, &t, &r, &t1, &t2, &t3, &xi}, **scales[] = {&sx, &su, &st, &sr, &st1, &st2, &st3, &sxi};
    for (unsigned i = 0; i < sizeof vecs / sizeof vecs[0]; i++) {
        CHECK(clv_malloc(vecs[i], N));
        CHECK(clv_malloc(scales[i], NS * sizeof(float)));
        CHECK(clv_memset(*vecs[i], 0x55, N, NULL));
    }
    CHECK(clv_memcpy_h2d(A, hA, sizeof hA, NULL));
    CHECK(clv_memcpy_h2d(x, hx, sizeof hx, NULL));
    CHECK(clm8_quantize((const float *)A, N, N, (int8_t *)qA, (float *)sA, NULL, NULL));
    CHECK(clv8_quantize((const float *)x, N, (int8_t *)qx, (float *)sx, NULL, NULL));
    CHECK(clv8_quantize((const float *)x, N, (int8_t *)qu, (float *)su, NULL, NULL));
    CHECK(clm8_mvm_scale_and_add((const int8_t *)qA, (const float *)sA, N, N, (const int8_t *)qx, (const float *)sx, (const int8_t *)qu,
                                 (const float *)su, -1.0f, (int8_t *)t, (float *)st, (int8_t *)r, (float *)sr, NULL, NULL));
    CHECK(clm8_mvm_scale_and_add((const int8_t *)qA, (const float *)sA, N, N, (const int8_t *)qx, (const float *)sx, (const int8_t *)qu,
                                 (const float *)su, -1.0f, NULL, NULL, (int8_t *)qu, (float *)su, NULL, NULL));
    CHECK(clm8_iht((const int8_t *)qA, (const float *)sA, (const int8_t *)qA, (const float *)sA, N, N, (int8_t *)xi, (float *)sxi, N,
                   (const int8_t *)qx, (const float *)sx, (int8_t *)t1, (float *)st1, (int8_t *)t2, (float *)st2, (int8_t *)t3, (float *)st3, 0, 16,
                   0.5f, 1, NULL, NULL));
    CHECK(clv_memcpy_d2h(ht, t, sizeof ht, NULL));
    CHECK(clv_memcpy_d2h(hst, st, sizeof hst, NULL));
    CHECK(clv_memcpy_d2h(hr, r, sizeof hr, NULL));
    CHECK(clv_memcpy_d2h(hsr, sr, sizeof hsr, NULL));
    CHECK(clv_memcpy_d2h(hu, qu, sizeof hu, NULL));
    CHECK(clv_memcpy_d2h(hsu, su, sizeof hsu, NULL));
    CHECK(clv_memcpy_d2h(hxc, xi, sizeof hxc, NULL));
    CHECK(clv_memcpy_d2h(hsx, sxi, sizeof hsx, NULL));
    CHECK(clv_memcpy_d2h(ht1, t1, sizeof ht1, NULL));
    CHECK(clv_device_sync());
    int ok = !memcmp(hr, hu, sizeof hr) && !memcmp(hsr, hsu, sizeof hsr);
    for (int i = 0; i < N; i++) ok = ok && ht[i] >= 126 && hr[i] <= -126 && hxc[i] == 0 && ht1[i] == 0x55;
    for (int i = 0; i < NS; i++) ok = ok && fabsf(hst[i] - 256.0f) < 1e-3f && fabsf(hsr[i] - 255.0f) < 1e-3f && hsx[i] == 1.0f;
    const int bad = clm8_mvm_scale_and_add((const int8_t *)qA, (const float *)sA, 96, N, (const int8_t *)qx, (const float *)sx, (const int8_t *)qu,
                                           (const float *)su, -1.0f, NULL, NULL, (int8_t *)r, (float *)sr, NULL, NULL);
    printf("t=%d st=%.1f r=%d sr=%.1f ok=%d bad_shape=%d msg=%s\n", ht[0], hst[0], hr[0], hsr[0], ok, bad, clv_last_error());
    for (unsigned i = 0; i < sizeof vecs / sizeof vecs[0]; i++) {
        clv_free(*vecs[i]);
        clv_free(*scales[i]);
    }
    clv_free(A);
    clv_free(x);
    clv_free(qA);
    clv_free(sA);
    return ok && bad == CLV_ERR_INVALID ? 0 : 1;
}
