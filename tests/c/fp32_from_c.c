/* A C99 client of include/clover_hip_fp32.h: compiles with -pedantic, links, and -- on a machine with a device -- takes the dot product of
 * 128 ones with themselves (128.0).  Without a device the argument checks still answer. */
#include <stdio.h>
#include <string.h>

#include "clover_hip_fp32.h"

int main(void)
{
    int n = 0;
    float x[128], d = -1.0f;
    void *dx = NULL, *dout = NULL;
    int i;

    /* argument checks come before any device work */
    if (clv_f32_scale_and_add(NULL, NULL, 1.0f, 128, NULL, NULL) != CLV_ERR_INVALID || !strstr(clv_last_error(), "null")) return 2;
    if (clv_f32_dot((const float *)16, (const float *)16, 100, CLV_DOT_EXACT, (float *)16, NULL, NULL) != CLV_ERR_INVALID) return 3;
    if (clm_f32_mvm((const float *)16, 128, 100, (const float *)16, (float *)32, NULL) != CLV_ERR_INVALID) return 4;
    if (clv_f32_dot_workspace_bytes(128) != 0) return 5;
    if (clv_f32_threshold_workspace_bytes(128) == 0) return 6;
    if (clm_f32_iht((const float *)16, (const float *)16, 128, 128, (float *)16, 129, (const float *)16, (float *)16, (float *)16, (float *)16, 1, 1,
                    1.0f, CLV_THRESHOLD_FAST, NULL) != CLV_ERR_INVALID) return 7;

    if (clv_device_count(&n) != CLV_OK || n < 1) {
        printf("no_device\n");
        return 0;
    }
    for (i = 0; i < 128; i++) x[i] = 1.0f;
    if (clv_malloc(&dx, sizeof x) || clv_malloc(&dout, 4)) return 8;
    if (clv_memcpy_h2d(dx, x, sizeof x, NULL)) return 9;
    if (clv_f32_dot((const float *)dx, (const float *)dx, 128, CLV_DOT_EXACT, (float *)dout, NULL, NULL)) return 10;
    if (clv_memcpy_d2h(&d, dout, 4, NULL) || clv_device_sync()) return 11;
    printf("dot=%.1f\n", d);
    clv_free(dx);
    clv_free(dout);
    return d == 128.0f ? 0 : 12;
}
