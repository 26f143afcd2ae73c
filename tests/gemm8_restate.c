/* gemm8_restate.c -- plain-C restatement of the three GEMM definitions with 8-bit operands (include/clover_hip.h: clm8_gemm,
 * clm8_gemm_i32, clm4_gemm_m8), written from their text and from nothing else: no oracle link, the quantized images are
 * taken as given.
 *
 *   A is M x K, B is N x K, C = A * B^T, M x N row-major.  Per element (i, j) and K-block b (64 elements):
 *     S_b     = the exact integer sum of the 64 products
 *     C[i][j] = one sequential chain over b = 0, 1, 2, ... from C = 0:  C = fmaf(c_b, (float)S_b, C)
 *     8 x 8:  c_b = f32( f32(sA[i>>6][b] * R127) * f32(sB[j>>6][b] * R127) ),  R127 = 1.0f / 127.0f
 *     4 x 8:  c_b = f32( f32(sA[i>>6][b] * (1.0f / 7.0f)) * f32(sB[j>>6][b] * R127) );  A holds nibbles: byte p of a row holds element 2p in
 *             its high nibble and 2p + 1 in its low nibble, two's complement (-8 .. 7)
 *   the integer form: S[i][j] = sum of S_b over the K-blocks [kb_begin, kb_begin + kb_count), int32.
 *
 * Build: cc -O2 -ffp-contract=off -fno-fast-math (every product above is rounded on its own, fmaf is the fused operation), optionally
 * -fopenmp: the loops over i then run on at most 16 threads. */
#include <math.h>
#include <stdint.h>
#ifdef _OPENMP
#include <omp.h>
#endif

static int rg8_threads(void)
{
#ifdef _OPENMP
    const int n = omp_get_max_threads();
    return n < 16 ? n : 16;
#else
    return 1;
#endif
}

static inline int nibble(const uint8_t *row, uint64_t e)
{
    const uint8_t byte = row[e >> 1];
    const int v = (e & 1) ? (byte & 0xF) : (byte >> 4);
    return v >= 8 ? v - 16 : v;
}

static inline int32_t block_sum8(const int8_t *a, const int8_t *b)
{
    int32_t s = 0;
    for (int k = 0; k < 64; k++) s += (int32_t)a[k] * (int32_t)b[k];
    return s;
}

static inline int32_t block_sum48(const uint8_t *arow, uint64_t blk, const int8_t *b)
{
    int32_t s = 0;
    for (int k = 0; k < 64; k++) s += (int32_t)nibble(arow, 64 * blk + k) * (int32_t)b[k];
    return s;
}

static inline float factor8(float sa, float sb)
{
    const float r127 = 1.0f / 127.0f;
    const float fa = sa * r127, fb = sb * r127;
    return fa * fb;
}

static inline float factor48(float sa, float sb)
{
    const float fa = sa * (1.0f / 7.0f), fb = sb * (1.0f / 127.0f);
    return fa * fb;
}

void rg8_gemm(const int8_t *A, const float *sA, uint64_t M, uint64_t K, const int8_t *B, const float *sB, uint64_t N, float *C)
{
    const uint64_t nb = K / 64;
    const int64_t rows = (int64_t)M;
#pragma omp parallel for schedule(static) num_threads(rg8_threads())
    for (int64_t i = 0; i < rows; i++)
        for (uint64_t j = 0; j < N; j++) {
            float c = 0.0f;
            for (uint64_t b = 0; b < nb; b++) {
                const int32_t S = block_sum8(A + (uint64_t)i * K + 64 * b, B + j * K + 64 * b);
                c = fmaf(factor8(sA[((uint64_t)i >> 6) * nb + b], sB[(j >> 6) * nb + b]), (float)S, c);
            }
            C[(uint64_t)i * N + j] = c;
        }
}

void rg8_gemm_i32(const int8_t *A, uint64_t M, uint64_t K, const int8_t *B, uint64_t N, uint64_t kb_begin, uint64_t kb_count, int32_t *S)
{
    const int64_t rows = (int64_t)M;
#pragma omp parallel for schedule(static) num_threads(rg8_threads())
    for (int64_t i = 0; i < rows; i++)
        for (uint64_t j = 0; j < N; j++) {
            int32_t s = 0;
            for (uint64_t b = kb_begin; b < kb_begin + kb_count; b++) s += block_sum8(A + (uint64_t)i * K + 64 * b, B + j * K + 64 * b);
            S[(uint64_t)i * N + j] = s;
        }
}

void rg8_gemm_m8(const uint8_t *A4, const float *sA, uint64_t M, uint64_t K, const int8_t *B8, const float *sB, uint64_t N, float *C)
{
    const uint64_t nb = K / 64;
    const int64_t rows = (int64_t)M;
#pragma omp parallel for schedule(static) num_threads(rg8_threads())
    for (int64_t i = 0; i < rows; i++)
        for (uint64_t j = 0; j < N; j++) {
            float c = 0.0f;
            for (uint64_t b = 0; b < nb; b++) {
                const int32_t S = block_sum48(A4 + (uint64_t)i * (K / 2), b, B8 + j * K + 64 * b);
                c = fmaf(factor48(sA[((uint64_t)i >> 6) * nb + b], sB[(j >> 6) * nb + b]), (float)S, c);
            }
            C[(uint64_t)i * N + j] = c;
        }
}

/* the integer sums of the mixed form over a K-block range (no ABI call returns them; the CPU tests check the nibble decoding with them) */
void rg8_gemm_m8_i32(const uint8_t *A4, uint64_t M, uint64_t K, const int8_t *B8, uint64_t N, uint64_t kb_begin, uint64_t kb_count, int32_t *S)
{
    const int64_t rows = (int64_t)M;
#pragma omp parallel for schedule(static) num_threads(rg8_threads())
    for (int64_t i = 0; i < rows; i++)
        for (uint64_t j = 0; j < N; j++) {
            int32_t s = 0;
            for (uint64_t b = kb_begin; b < kb_begin + kb_count; b++) s += block_sum48(A4 + (uint64_t)i * (K / 2), b, B8 + j * K + 64 * b);
            S[(uint64_t)i * N + j] = s;
        }
}

/* one step of the 8 x 8 chain on given block sums: C = fmaf(c_b, (float)S_b, C) for K-block b, all elements */
void rg8_fold_step(const int32_t *Sb, const float *sA, const float *sB, uint64_t M, uint64_t N, uint64_t K, uint64_t b, float *C)
{
    const uint64_t nb = K / 64;
    for (uint64_t i = 0; i < M; i++)
        for (uint64_t j = 0; j < N; j++)
            C[i * N + j] = fmaf(factor8(sA[(i >> 6) * nb + b], sB[(j >> 6) * nb + b]), (float)Sb[i * N + j], C[i * N + j]);
}
