/* m8_f32_t_restate.c -- the transposed CloverMatrix8 x fp32-vector product (include/clover_hip_m8_f32.h: clm8_mvm_f32_transposed) restated
 * in plain C as a COLUMN WALK of the stated definition.  It walks down the columns of A and never builds A': output column c is 32
 * sequential fma chains, row i of A on chain i mod 32 in increasing i, each from +0.0f,
 *     acc = fma(f32(x[i] * f32(sA[i / 64][c / 64] / 127.0f)), (float)q(i, c), acc)
 * with the scale read from A's own grid -- it multiplies x, not q; then (acc1 + acc2) + (acc3 + acc4) per AVX lane l = chain mod 8
 * (accumulator = chain / 8) and the _mm256_haddf32_ps tree t[k] = s[k + 4] + s[k], (t0 + t2) + (t1 + t3).
 *
 * Build with -ffp-contract=off: every product is rounded on its own and the only fused operation is the explicit fmaf.
 *
 * A: rows x cols signed bytes, row-major (-128 is a legal byte); sA: (rows / 64) x (cols / 64) tile scales, row-major.
 * `chains` is 32 for the definition; another count (16, 8, 64) gives a wrong-order variant for the tests that show the data tells the
 * orders apart: chain i mod chains, the ends summed pairwise in the same shape as far as it applies (see below). */
#include <math.h>
#include <stdint.h>

/* the 32 chain ends of one column -> the value */
static float tree32(const float *acc)
{
    float s[8], t[4];
    int l;
    for (l = 0; l < 8; l++) s[l] = (acc[l] + acc[8 + l]) + (acc[16 + l] + acc[24 + l]);
    for (l = 0; l < 4; l++) t[l] = s[l + 4] + s[l];
    return (t[0] + t[2]) + (t[1] + t[3]);
}

void m8rt_mvm_f32_transposed(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, float *r, int chains)
{
    uint64_t c, i;
    int k;
    for (c = 0; c < cols; c++) {
        float acc[64], full[32];
        for (k = 0; k < 64; k++) acc[k] = 0.0f;
        for (i = 0; i < rows; i++) {
            const float f = sA[(i / 64) * (cols / 64) + c / 64] / 127.0f;
            const float t = x[i] * f;
            acc[i % (uint64_t)chains] = fmaf(t, (float)A[i * cols + c], acc[i % (uint64_t)chains]);
        }
        /* wrong-order variants: fewer chains leave the other ends +0; 64 chains are folded to 32 first */
        for (k = 0; k < 32; k++) full[k] = chains == 64 ? acc[k] + acc[32 + k] : acc[k];
        r[c] = tree32(full);
    }
}
