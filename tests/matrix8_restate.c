/* matrix8_restate.c -- plain-C restatement of CloverMatrix8 (the reference's include/CloverMatrix8.h) in its SIMD order, the
 * checker of the CloverMatrix8 tests.  Built by tests/matrix8_helpers.py with  cc -O2 -ffp-contract=off -fno-fast-math  and linked
 * against the oracle (oracle/liboracle.so) for the XORShift stream: every draw is orc_rng_draw, the generator of the other
 * restatements.  Every fused multiply-add is an explicit fmaf(); every other operation is a separately rounded fp32 operation.
 *
 * The same file is built a second time with  -mfma -fopenmp  for the large shapes: fmaf() becomes one instruction (same result), and
 * the loops whose iterations are independent -- the row dots, rm8_mvm_f32, rm8_transpose and the deterministic quantize -- run on at
 * most 16 threads.  Everything that draws from the stream stays sequential and in the reference's order.
 *
 * Layout: rows*cols int8 values row-major, then (rows/64)*(cols/64) fp32 tile scales row-major; value = q * (s / 127). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

/* threads of the -fopenmp build: never more than 16 (the CPUs one command may use) */
static inline int rm8_threads(void)
{
#ifdef _OPENMP
    const int n = omp_get_max_threads();
    return n < 16 ? n : 16;
#else
    return 1;
#endif
}

typedef struct { uint64_t s0[4]; uint64_t s1[4]; } orc_rng;      /* oracle/clover4_oracle.h */
void orc_rng_draw(orc_rng *r, uint32_t W[8]);

static float absf_bits(float x)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    u &= 0x7FFFFFFFu;
    memcpy(&x, &u, 4);
    return x;
}

/* the noise of one byte field: (W & 0x7F7F7F7F) << 8 sh as int32, converted (round to nearest), times 2^-31
 * (CloverMatrix8.h:345-400: rnd_i8_1 .. rnd_i8_4) */
static float noise_of(uint32_t W, int sh)
{
    const int32_t v = (int32_t)((W & 0x7F7F7F7Fu) << (8 * sh));
    return (float)v * (1.0f / 2147483648.0f);
}

/* the 64 noises of one 64-element row from two draws: element e takes draw e >> 5, word e & 7, byte (e >> 3) & 3 */
static void row_noise(orc_rng *rng, float n[64])
{
    uint32_t W[2][8];
    if (!rng) {
        for (int e = 0; e < 64; e++) n[e] = 0.0f;
        return;
    }
    orc_rng_draw(rng, W[0]);
    orc_rng_draw(rng, W[1]);
    for (int e = 0; e < 64; e++) n[e] = noise_of(W[e >> 5][e & 7], (e >> 3) & 3);
}

/* one element: trunc(fma(|x|, k, noise)) with the sign of x (cvttps_epi32 + sign_epi32; the low byte is stored).  cvttps of an
 * out-of-range or NaN value is 0x80000000 (low byte 0). */
static int8_t quant1(float x, float k, float noise)
{
    const float p = fmaf(absf_bits(x), k, noise);
    int32_t t;
    if (!(p > -2147483648.0f && p < 2147483648.0f)) t = INT32_MIN;
    else t = (int32_t)p;
    uint32_t xb;
    memcpy(&xb, &x, 4);
    if (xb & 0x80000000u) t = (int32_t)(0u - (uint32_t)t);
    else if (xb == 0u) t = 0;               /* sign_epi32 with a zero sign source */
    return (int8_t)(uint8_t)(uint32_t)t;
}

/* max -> stored scale: 0 becomes 1.0 (the isZero / cndOne add) */
static float fix_zero(float m)
{
    uint32_t u;
    memcpy(&u, &m, 4);
    return u == 0u ? m + 1.0f : m;
}

/* CloverMatrix8::quantize (:203-480) */
void rm8_quantize(const float *A, uint64_t rows, uint64_t cols, int8_t *q, float *s, orc_rng *rng)
{
    const uint64_t h_blocks = cols >> 6, v_blocks = rows >> 6;
    /* with a generator the tiles draw in this loop order: sequential */
#pragma omp parallel for collapse(2) num_threads(rm8_threads()) if (!rng)
    for (uint64_t b_j = 0; b_j < h_blocks; b_j++)
        for (uint64_t b_i = 0; b_i < v_blocks; b_i++) {
            const uint64_t off = (b_i << 6) * cols + (b_j << 6);
            float m = 0.0f;
            for (uint64_t i = 0; i < 64; i++)
                for (uint64_t j = 0; j < 64; j++) {
                    const float a = absf_bits(A[off + i * cols + j]);
                    if (a > m) m = a;
                }
            m = fix_zero(m);
            const float k = 127.0f / m;
            s[b_i * h_blocks + b_j] = m;
            for (uint64_t i = 0; i < 64; i++) {
                float n[64];
                row_noise(rng, n);
                for (uint64_t j = 0; j < 64; j++) q[off + i * cols + j] = quant1(A[off + i * cols + j], k, n[j]);
            }
        }
}

/* CloverMatrix8::get (:117-131) for every element */
void rm8_restore(const int8_t *q, const float *s, uint64_t rows, uint64_t cols, float *A)
{
    const uint64_t h_blocks = cols >> 6;
    for (uint64_t i = 0; i < rows; i++)
        for (uint64_t j = 0; j < cols; j++) {
            const float f = s[(i >> 6) * h_blocks + (j >> 6)] / 127.0f;
            A[i * cols + j] = f * (float)q[i * cols + j];
        }
}

/* the row value of CloverMatrix8::mvm(CloverVector8) (:1020-1085): 8 lanes, lane k = exact sum of bytes {4k..4k+3} and
 * {32+4k..32+4k+3} of the block, one fma chain per lane, then the extractf128 / movehl / shuffle(0x55) tree */
static float row_dot8(const int8_t *u, const float *su, const int8_t *v, const float *sv, uint64_t h_blocks)
{
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint64_t b = 0; b < h_blocks; b++) {
        const float scale = (su[b] * (1.0f / 127.0f)) * (sv[b] * (1.0f / 127.0f));
        for (int k = 0; k < 8; k++) {
            int32_t d = 0;
            for (int t = 0; t < 4; t++) {
                d += (int32_t)u[64 * b + 4 * k + t] * (int32_t)v[64 * b + 4 * k + t];
                d += (int32_t)u[64 * b + 32 + 4 * k + t] * (int32_t)v[64 * b + 32 + 4 * k + t];
            }
            acc[k] = fmaf(scale, (float)d, acc[k]);
        }
    }
    float t[4];
    for (int k = 0; k < 4; k++) t[k] = acc[k + 4] + acc[k];
    const float h0 = t[0] + t[2], h1 = t[1] + t[3];
    return h0 + h1;
}

/* the re-quantisation of 64 row values (:1140-1299 = CloverVector8::quantize of one block) */
static void requant64(const float d[64], int8_t r[64], float *sr, orc_rng *rng)
{
    float m = 0.0f;
    for (int l = 0; l < 64; l++) {
        const float a = absf_bits(d[l]);
        m = a > m ? a : m;                  /* _mm_max_ss(habs, max_ss) */
    }
    m = fix_zero(m);
    const float k = 127.0f / m;
    *sr = m;
    float n[64];
    row_noise(rng, n);
    for (int l = 0; l < 64; l++) r[l] = quant1(d[l], k, n[l]);
}

/* the fp32 row values of CloverMatrix8::mvm (before re-quantisation) */
void rm8_rowdots(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const int8_t *x, const float *sx, float *d)
{
    const uint64_t h_blocks = cols >> 6;
#pragma omp parallel for num_threads(rm8_threads())
    for (uint64_t i = 0; i < rows; i++) d[i] = row_dot8(A + i * cols, sA + (i >> 6) * h_blocks, x, sx, h_blocks);
}

/* CloverMatrix8::mvm(const CloverVector8 &, CloverVector8 &) (:1002-1299): every row dot first, then the row groups re-quantised in
 * order (with a generator, row group rb takes the stream's draws 2 rb, 2 rb + 1) */
void rm8_mvm(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const int8_t *x, const float *sx, int8_t *r, float *sr,
             orc_rng *rng)
{
    float *d = (float *)malloc((rows ? rows : 1) * sizeof(float));
    if (!d) abort();
    rm8_rowdots(A, sA, rows, cols, x, sx, d);
    for (uint64_t rb = 0; rb < rows / 64; rb++) requant64(d + rb * 64, r + rb * 64, sr + rb, rng);
    free(d);
}

/* CloverMatrix8::mvm(const CloverVector32 &, CloverVector32 &) (:558-662): element 8j + l of a block -> accumulator j mod 4, lane l
 * (the restore_perm shuffles give the natural order), fma(f32(v * f32(s / 127)), q, acc), j = 0..3 before j = 4..7; then
 * (acc1 + acc2) + (acc3 + acc4) and _mm256_haddf32_ps (CloverBase.h:149-157) */
void rm8_mvm_f32(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, float *r)
{
    const uint64_t h_blocks = cols >> 6;
#pragma omp parallel for num_threads(rm8_threads())
    for (uint64_t i = 0; i < rows; i++) {
        const int8_t *u = A + i * cols;
        const float *su = sA + (i >> 6) * h_blocks;
        float acc[4][8];
        memset(acc, 0, sizeof acc);
        for (uint64_t b = 0; b < h_blocks; b++) {
            const float scale = su[b] / 127.0f;
            for (int j = 0; j < 8; j++)
                for (int l = 0; l < 8; l++) {
                    const uint64_t e = 64 * b + 8 * j + l;
                    const float t = x[e] * scale;
                    acc[j & 3][l] = fmaf(t, (float)u[e], acc[j & 3][l]);
                }
        }
        float sum[8];
        for (int l = 0; l < 8; l++) sum[l] = (acc[0][l] + acc[1][l]) + (acc[2][l] + acc[3][l]);
        float x128[4];
        for (int l = 0; l < 4; l++) x128[l] = sum[l + 4] + sum[l];
        r[i] = (x128[0] + x128[2]) + (x128[1] + x128[3]);
    }
}

/* CloverMatrix8::transpose (:1312-1386): values and the tile scale grid */
void rm8_transpose(const int8_t *q, const float *s, uint64_t rows, uint64_t cols, int8_t *qt, float *st)
{
    const uint64_t v_blocks = rows >> 6, h_blocks = cols >> 6;
    /* 64 x 64 tiles at a time: the same bytes, without a cache miss per byte at 65536 columns */
#pragma omp parallel for collapse(2) num_threads(rm8_threads())
    for (uint64_t bi = 0; bi < v_blocks; bi++)
        for (uint64_t bj = 0; bj < h_blocks; bj++)
            for (uint64_t i = 64 * bi; i < 64 * bi + 64; i++)
                for (uint64_t j = 64 * bj; j < 64 * bj + 64; j++) qt[j * rows + i] = q[i * cols + j];
    for (uint64_t bi = 0; bi < v_blocks; bi++)
        for (uint64_t bj = 0; bj < h_blocks; bj++) st[bj * v_blocks + bi] = s[bi * h_blocks + bj];
}
