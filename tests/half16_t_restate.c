/* half16_t_restate.c -- the transposed half-precision mvm (include/clover_hip_f16_t.h) restated in plain C as a COLUMN WALK of the stated
 * definition: the checker of tests/test_f16_mvm_transposed*.py.  It is not a transpose followed by a row dot; the tests hold it to
 * rh_transpose + rh_mvm / rh_mvm_f32 / rh_scale_and_add of half16_restate.c (included below for the two conversions), bit for bit.
 *
 *   column j     32 sequential fp32 chains, row i on chain i mod 32 in increasing i, each from +0.0f, one step
 *                acc = fmaf(f32(x[i]), f32(A[i][j]), acc);  s[l] = (acc[l] + acc[8 + l]) + (acc[16 + l] + acc[24 + l]);
 *                t[k] = s[k + 4] + s[k];  d = (t0 + t2) + (t1 + t3)
 *   f16 vectors  r[j] = f16(d);  fused: t[j] = f16(d), r[j] = f16(fmaf(f32(t[j]), a, f32(u[j])))
 *   fp32 vectors x used as fp32, r[j] = d
 *
 * `order` selects the walk.  RT_RIGHT is the definition.  The other three are WRONG ON PURPOSE and exist only so that the tests can show
 * that their data tells the orders apart: RT_ENDS_LEFT_TO_RIGHT (the 32 chains, their ends summed 0, 1, .. 31), RT_ONE_CHAIN (one
 * running sum over all rows), RT_16_CHAINS (row i on chain i mod 16; s[l] = acc[l] + acc[8 + l], then the same t and d). */
#include "half16_restate.c"

enum { RT_RIGHT = 0, RT_ENDS_LEFT_TO_RIGHT = 1, RT_ONE_CHAIN = 2, RT_16_CHAINS = 3 };

/* xf: x widened (or given) as fp32, `rows` values */
static float rt_column(const float *T, const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t j, const float *xf, int order)
{
    float acc[32], s[8], t[4];
    const uint64_t nch = order == RT_ONE_CHAIN ? 1 : order == RT_16_CHAINS ? 16 : 32;
    for (int c = 0; c < 32; c++) acc[c] = 0.0f;
    for (uint64_t i = 0; i < rows; i++) acc[i % nch] = fmaf(xf[i], T[A[i * cols + j]], acc[i % nch]);
    if (order == RT_ONE_CHAIN) return acc[0];
    if (order == RT_ENDS_LEFT_TO_RIGHT) {
        float d = acc[0];
        for (int c = 1; c < 32; c++) d = d + acc[c];
        return d;
    }
    for (int l = 0; l < 8; l++) s[l] = order == RT_16_CHAINS ? acc[l] + acc[8 + l] : (acc[l] + acc[8 + l]) + (acc[16 + l] + acc[24 + l]);
    for (int k = 0; k < 4; k++) t[k] = s[k + 4] + s[k];
    return (t[0] + t[2]) + (t[1] + t[3]);
}

/* d[j]: the fp32 column values of the f16-vector forms, before any rounding to f16 */
void rt_columns(const uint16_t *A, uint64_t rows, uint64_t cols, const uint16_t *x, int order, float *d)
{
    const float *T = rh_table();
    float *xf = (float *)malloc((rows ? rows : 1) * sizeof(float));
    for (uint64_t i = 0; i < rows; i++) xf[i] = T[x[i]];
    for (uint64_t j = 0; j < cols; j++) d[j] = rt_column(T, A, rows, cols, j, xf, order);
    free(xf);
}

void rt_mvm_transposed(const uint16_t *A, uint64_t rows, uint64_t cols, const uint16_t *x, int order, uint16_t *r)
{
    float *d = (float *)malloc((cols ? cols : 1) * sizeof(float));
    rt_columns(A, rows, cols, x, order, d);
    for (uint64_t j = 0; j < cols; j++) r[j] = rh_f32_to_f16(d[j]);
    free(d);
}

void rt_mvm_f32_transposed(const uint16_t *A, uint64_t rows, uint64_t cols, const float *x, int order, float *r)
{
    const float *T = rh_table();
    for (uint64_t j = 0; j < cols; j++) r[j] = rt_column(T, A, rows, cols, j, x, order);
}

/* t (never NULL here) and r of the fused form; r is computed from the ROUNDED t widened again */
void rt_mvm_transposed_scale_and_add(const uint16_t *A, uint64_t rows, uint64_t cols, const uint16_t *x, const uint16_t *u, float a, int order,
                                     uint16_t *t, uint16_t *r)
{
    const float *T = rh_table();
    rt_mvm_transposed(A, rows, cols, x, order, t);
    for (uint64_t j = 0; j < cols; j++) r[j] = rh_f32_to_f16(fmaf(T[t[j]], a, T[u[j]]));
}
