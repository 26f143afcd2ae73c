/* half16_fused_from_c.c -- clm_f16_mvm_scale_and_add and clm_f16_iht from C99 (gcc, not g++) against include/clover_hip.h alone.
 * With a GPU: A = 128 x 128 of 0.5, x = u = 1.0 (quantized by clm_f16_quantize / clv_f16_quantize).  t = f16(A x) is 64.0 (0x5400) in every
 * row and r = f16(u - t) is -63.0 (0xD3E0); the in-place form with t = NULL leaves the same r in u.  clm_f16_iht with 0 iterations
 * clears x and leaves t1 alone.  A bad shape returns CLV_ERR_INVALID with a message.  Without a device the program reports the status
 * text and exits 0. */
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
    enum { N = 128 };
    static float hA[N * N], hx[N];
    uint16_t ht[N], hr[N], hu[N], hxc[N], ht1[N];
    void *A, *x, *hAq, *xq, *u, *t, *r, *t1, *t2, *t3, *xi;
    for (int i = 0; i < N * N; i++) hA[i] = 0.5f;
    for (int i = 0; i < N; i++) hx[i] = 1.0f;
    CHECK(clv_malloc(&A, sizeof hA));
    CHECK(clv_malloc(&x, sizeof hx));
    CHECK(clv_malloc(&hAq, N * N * sizeof(uint16_t)));
    void **vecs[] = {&xq, &u, &t, &r, &t1, &t2, &t3, &xi};
    for (unsigned i = 0; i < sizeof vecs / sizeof vecs[0]; i++) {
        CHECK(clv_malloc(vecs[i], N * sizeof(uint16_t)));
        CHECK(clv_memset(*vecs[i], 0x55, N * sizeof(uint16_t), NULL));
    }
    CHECK(clv_memcpy_h2d(A, hA, sizeof hA, NULL));
    CHECK(clv_memcpy_h2d(x, hx, sizeof hx, NULL));
    CHECK(clm_f16_quantize((const float *)A, N, N, (uint16_t *)hAq, NULL));
    CHECK(clv_f16_quantize((const float *)x, N, (uint16_t *)xq, NULL));
    CHECK(clv_f16_quantize((const float *)x, N, (uint16_t *)u, NULL));
    CHECK(clm_f16_mvm_scale_and_add((const uint16_t *)hAq, N, N, (const uint16_t *)xq, (const uint16_t *)u, -1.0f, (uint16_t *)t, (uint16_t *)r,
                                    NULL));
    CHECK(clm_f16_mvm_scale_and_add((const uint16_t *)hAq, N, N, (const uint16_t *)xq, (const uint16_t *)u, -1.0f, NULL, (uint16_t *)u, NULL));
    CHECK(clm_f16_iht((const uint16_t *)hAq, (const uint16_t *)hAq, N, N, (uint16_t *)xi, N, (const uint16_t *)xq, (uint16_t *)t1, (uint16_t *)t2,
                      (uint16_t *)t3, 0, 16, 0.5f, 1, NULL));
    CHECK(clv_memcpy_d2h(ht, t, sizeof ht, NULL));
    CHECK(clv_memcpy_d2h(hr, r, sizeof hr, NULL));
    CHECK(clv_memcpy_d2h(hu, u, sizeof hu, NULL));
    CHECK(clv_memcpy_d2h(hxc, xi, sizeof hxc, NULL));
    CHECK(clv_memcpy_d2h(ht1, t1, sizeof ht1, NULL));
    CHECK(clv_device_sync());
    int ok = !memcmp(hr, hu, sizeof hr);
    for (int i = 0; i < N; i++) ok = ok && ht[i] == 0x5400 && hr[i] == 0xD3E0 && hxc[i] == 0 && ht1[i] == 0x5555;
    const int bad = clm_f16_mvm_scale_and_add((const uint16_t *)hAq, N, 100, (const uint16_t *)xq, (const uint16_t *)u, -1.0f, NULL, (uint16_t *)r,
                                              NULL);
    printf("t=%04x r=%04x ok=%d bad_shape=%d msg=%s\n", (unsigned)ht[0], (unsigned)hr[0], ok, bad, clv_last_error());
    for (unsigned i = 0; i < sizeof vecs / sizeof vecs[0]; i++) clv_free(*vecs[i]);
    clv_free(A);
    clv_free(x);
    clv_free(hAq);
    return ok && bad == CLV_ERR_INVALID ? 0 : 1;
}
