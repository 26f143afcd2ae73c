/* m4_f32_t_restate.c -- the transposed CloverMatrix4 x fp32-vector product (include/clover_hip_m4_f32.h: clm4_mvm_f32_transposed) restated
 * in plain C as a COLUMN WALK of the stated definition.  It walks down the columns of A and never builds A': output column c is 32
 * sequential fma chains, row i of A on chain i mod 32 in increasing i, each from +0.0f,
 *     acc = fma(x[i], f32((float)q(i, c) * f32(sA[i / 64][c / 64] / 7)), acc)
 * with the scale read from A's own grid; then (acc1 + acc2) + (acc3 + acc4) per AVX lane j = chain mod 8 (accumulator = chain / 8) and the
 * _mm256_haddf32_ps tree t[k] = s[k + 4] + s[k], (t0 + t2) + (t1 + t3).
 *
 * Build with -ffp-contract=off: every product is rounded on its own and the only fused operation is the explicit fmaf.
 *
 * A: rows x cols nibbles, row-major, cols / 2 bytes per row, even elements in the HIGH nibble of their byte (two's complement);
 * sA: (rows / 64) x (cols / 64) tile scales, row-major.
 * `chains` is 32 for the definition; another count (16, 8, 64) gives a wrong-order variant for the tests that show the data tells the
 * orders apart: chain i mod chains, the ends summed pairwise in the same shape as far as it applies (see below). */
#include <math.h>
#include <stdint.h>

static int nibble(const uint8_t *A, uint64_t cols, uint64_t i, uint64_t c)
{
    const uint8_t b = A[(i * cols + c) / 2];
    const int v = (c & 1) ? (b & 0xF) : (b >> 4);
    return v >= 8 ? v - 16 : v;
}

/* the 32 chain ends of one column -> the value */
static float tree32(const float *acc)
{
    float s[8], t[4];
    int j;
    for (j = 0; j < 8; j++) s[j] = (acc[j] + acc[8 + j]) + (acc[16 + j] + acc[24 + j]);
    for (j = 0; j < 4; j++) t[j] = s[j + 4] + s[j];
    return (t[0] + t[2]) + (t[1] + t[3]);
}

void m4rt_mvm_f32_transposed(const uint8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, float *r, int chains)
{
    uint64_t c, i;
    int k;
    for (c = 0; c < cols; c++) {
        float acc[64], full[32];
        for (k = 0; k < 64; k++) acc[k] = 0.0f;
        for (i = 0; i < rows; i++) {
            const float f = sA[(i / 64) * (cols / 64) + c / 64] / 7.0f;
            const float a = (float)nibble(A, cols, i, c) * f;
            acc[i % (uint64_t)chains] = fmaf(x[i], a, acc[i % (uint64_t)chains]);
        }
        /* wrong-order variants: fewer chains leave the other ends +0; 64 chains are folded to 32 first */
        for (k = 0; k < 32; k++) full[k] = chains == 64 ? acc[k] + acc[32 + k] : acc[k];
        r[c] = tree32(full);
    }
}
