/* A C99 client of the half-precision entry points of include/clover_hip.h: compiles with -pedantic, links, and -- on a machine with a
 * device -- quantizes 128 ones and takes their dot product (128.0).  Without a device the argument checks still answer. */
#include <stdio.h>
#include <string.h>

#include "clover_hip.h"

int main(void)
{
    int n = 0;
    float x[128], d = -1.0f;
    void *dx = NULL, *dh = NULL, *dout = NULL;
    int i;

    /* argument checks come before any device work */
    if (clv_f16_quantize(NULL, 128, NULL, NULL) != CLV_ERR_INVALID || !strstr(clv_last_error(), "null")) return 2;
    if (clv_f16_dot((const uint16_t *)16, (const uint16_t *)16, 100, CLV_DOT_EXACT, &d, NULL, NULL) != CLV_ERR_INVALID) return 3;
    if (clm_f16_mvm((const uint16_t *)16, 64, 100, (const uint16_t *)16, (uint16_t *)32, NULL) != CLV_ERR_INVALID) return 4;
    if (clv_f16_dot_workspace_bytes(128) != 0) return 5;
    if (clv_f16_threshold_workspace_bytes(128) == 0) return 6;

    if (clv_device_count(&n) != CLV_OK || n < 1) {
        printf("no_device\n");
        return 0;
    }
    for (i = 0; i < 128; i++) x[i] = 1.0f;
    if (clv_malloc(&dx, sizeof x) || clv_malloc(&dh, 256) || clv_malloc(&dout, 4)) return 7;
    if (clv_memcpy_h2d(dx, x, sizeof x, NULL)) return 8;
    if (clv_f16_quantize((const float *)dx, 128, (uint16_t *)dh, NULL)) return 9;
    if (clv_f16_dot((const uint16_t *)dh, (const uint16_t *)dh, 128, CLV_DOT_EXACT, (float *)dout, NULL, NULL)) return 10;
    if (clv_memcpy_d2h(&d, dout, 4, NULL) || clv_device_sync()) return 11;
    printf("dot=%.1f\n", d);
    clv_free(dx);
    clv_free(dh);
    clv_free(dout);
    return d == 128.0f ? 0 : 12;
}
