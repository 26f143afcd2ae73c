/* half16_restate.c -- the CloverVector16 / CloverMatrix16 semantics restated in plain C: the checker of tests/test_half16*.py.
 *
 * Written from the stated semantics, no intrinsics:
 *   storage      raw IEEE binary16 bit patterns in uint16_t, no scales
 *   quantize     fp32 -> f16, round to nearest even, subnormal results kept (rh_f32_to_f16, integer arithmetic only)
 *   restore      the exact widening (rh_f16_to_f32)
 *   scaleAndAdd  r = f16(fma(f32(v), s, f32(u))), one fused fp32 fma
 *   dot          32 sequential fp32 fma chains, element j in chain j mod 32 = 8 c + l (accumulator c, lane l), each step
 *                fma(f32(v_j), f32(u_j), acc);  s[l] = (acc0[l] + acc1[l]) + (acc2[l] + acc3[l]);  t[i] = s[i + 4] + s[i];
 *                (t0 + t2) + (t1 + t3)
 *   mvm          every row is that dot against x; f16 vectors: the fp32 row value rounded to f16; fp32 vectors: x used as fp32, fp32 result
 *   transpose    element transpose
 *   threshold    the K-entry min-heap walk over |f32(h)|: std::make_heap under (a > b || isnan(a)) restated (libstdc++'s bottom-up
 *                adjust + push), every later element strictly larger than the root replaces it and sifts down (left child on ties)
 * Two builds: serial, and -fopenmp (at most 16 threads) for the large shapes; the tests check that they agree bit for bit.
 * rh_*64: float64 evaluations (value and sum of |terms|) for the error bounds. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

static int rh_threads(void)
{
#ifdef _OPENMP
    const int m = omp_get_max_threads();
    return m < 16 ? m : 16;
#else
    return 1;
#endif
}

static uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

float rh_f16_to_f32(uint16_t h)
{
    const uint32_t s = (uint32_t)(h & 0x8000u) << 16;
    uint32_t e = (h >> 10) & 31u, m = h & 0x3FFu;
    if (e == 31u) return u2f(s | 0x7F800000u | (m << 13));           /* inf, NaN (payload kept) */
    if (e == 0u) {
        if (m == 0u) return u2f(s);
        e = 113u;                                                    /* subnormal: m * 2^-24, normalise */
        while (!(m & 0x400u)) { m <<= 1; e--; }
        return u2f(s | (e << 23) | ((m & 0x3FFu) << 13));
    }
    return u2f(s | ((e + 112u) << 23) | (m << 13));
}

uint16_t rh_f32_to_f16(float f)
{
    const uint32_t u = f2u(f);
    const uint16_t s = (uint16_t)((u >> 16) & 0x8000u);
    const uint32_t e = (u >> 23) & 0xFFu, m = u & 0x7FFFFFu;
    if (e == 0xFFu) return (uint16_t)(s | 0x7C00u | (m ? (0x200u | (m >> 13)) : 0u));    /* inf; NaN quieted, top payload bits kept */
    if (e == 0u) return s;                                           /* fp32 zero / subnormal: far below half of 2^-24 */
    const uint32_t sig = 0x800000u | m;                              /* value = sig * 2^(e - 150) */
    if (e >= 143u) return (uint16_t)(s | 0x7C00u);                   /* >= 2^16 */
    /* f16 normal (e >= 113): 11 significant bits, drop 13; below: the unit is 2^-24, drop 126 - e */
    const uint32_t drop = e >= 113u ? 13u : 126u - e;
    if (drop >= 25u) return s;                                       /* below half of the smallest subnormal */
    uint32_t q = sig >> drop;
    const uint32_t rem = sig & ((1u << drop) - 1u), half = 1u << (drop - 1u);
    if (rem > half || (rem == half && (q & 1u))) q++;                /* nearest, ties to even */
    /* normal: q carries the hidden bit (0x400 .. 0x800), so (e - 113) << 10 plus q is the pattern, a carry moving into the exponent
     * (up to 0x7C00 = inf); subnormal: q itself (0x400 = the smallest normal) */
    return (uint16_t)(s | (e >= 113u ? ((e - 113u) << 10) + q : q));
}

static float *rh_table(void)
{
    static float *T = NULL;
    if (!T) {
        float *t = (float *)malloc(65536 * sizeof(float));
        for (uint32_t h = 0; h < 65536u; h++) t[h] = rh_f16_to_f32((uint16_t)h);
        T = t;
    }
    return T;
}

void rh_widen_all(float *out) { for (uint32_t h = 0; h < 65536u; h++) out[h] = rh_f16_to_f32((uint16_t)h); }

void rh_quantize(const float *x, uint64_t n, uint16_t *h)
{
#pragma omp parallel for schedule(static) num_threads(rh_threads())
    for (uint64_t i = 0; i < n; i++) h[i] = rh_f32_to_f16(x[i]);
}

void rh_restore(const uint16_t *h, uint64_t n, float *x)
{
    const float *T = rh_table();
#pragma omp parallel for schedule(static) num_threads(rh_threads())
    for (uint64_t i = 0; i < n; i++) x[i] = T[h[i]];
}

void rh_scale_and_add(const uint16_t *u, const uint16_t *v, float s, uint64_t n, uint16_t *r)
{
    const float *T = rh_table();
#pragma omp parallel for schedule(static) num_threads(rh_threads())
    for (uint64_t i = 0; i < n; i++) r[i] = rh_f32_to_f16(fmaf(T[v[i]], s, T[u[i]]));
}

static float rh_tree(const float acc[32])
{
    float s[8], t[4];
    for (int l = 0; l < 8; l++) s[l] = (acc[l] + acc[8 + l]) + (acc[16 + l] + acc[24 + l]);
    for (int i = 0; i < 4; i++) t[i] = s[i + 4] + s[i];
    return (t[0] + t[2]) + (t[1] + t[3]);
}

static float rh_dot_row(const float *T, const uint16_t *u, const uint16_t *v, uint64_t n)
{
    float acc[32];
    for (int c = 0; c < 32; c++) acc[c] = 0.0f;
    for (uint64_t j = 0; j < n; j += 32)
        for (int c = 0; c < 32; c++) acc[c] = fmaf(T[v[j + c]], T[u[j + c]], acc[c]);
    return rh_tree(acc);
}

static float rh_dot_row_f32(const float *T, const uint16_t *a, const float *x, uint64_t n)
{
    float acc[32];
    for (int c = 0; c < 32; c++) acc[c] = 0.0f;
    for (uint64_t j = 0; j < n; j += 32)
        for (int c = 0; c < 32; c++) acc[c] = fmaf(x[j + c], T[a[j + c]], acc[c]);
    return rh_tree(acc);
}

float rh_dot(const uint16_t *u, const uint16_t *v, uint64_t n) { return rh_dot_row(rh_table(), u, v, n); }

void rh_mvm(const uint16_t *A, uint64_t rows, uint64_t cols, const uint16_t *x, uint16_t *r)
{
    const float *T = rh_table();
#pragma omp parallel for schedule(static) num_threads(rh_threads())
    for (uint64_t i = 0; i < rows; i++) r[i] = rh_f32_to_f16(rh_dot_row(T, A + i * cols, x, cols));
}

/* the fp32 row values of rh_mvm before the rounding to f16 */
void rh_rowdots(const uint16_t *A, uint64_t rows, uint64_t cols, const uint16_t *x, float *d)
{
    const float *T = rh_table();
#pragma omp parallel for schedule(static) num_threads(rh_threads())
    for (uint64_t i = 0; i < rows; i++) d[i] = rh_dot_row(T, A + i * cols, x, cols);
}

void rh_mvm_f32(const uint16_t *A, uint64_t rows, uint64_t cols, const float *x, float *r)
{
    const float *T = rh_table();
#pragma omp parallel for schedule(static) num_threads(rh_threads())
    for (uint64_t i = 0; i < rows; i++) r[i] = rh_dot_row_f32(T, A + i * cols, x, cols);
}

void rh_transpose(const uint16_t *h, uint64_t rows, uint64_t cols, uint16_t *ht)
{
    /* 64 x 64 tiles so that neither side strides through memory */
#pragma omp parallel for schedule(static) num_threads(rh_threads())
    for (uint64_t i0 = 0; i0 < rows; i0 += 64)
        for (uint64_t j0 = 0; j0 < cols; j0 += 64)
            for (uint64_t i = i0; i < i0 + 64 && i < rows; i++)
                for (uint64_t j = j0; j < j0 + 64 && j < cols; j++) ht[j * rows + i] = h[i * cols + j];
}

/* 1 if transposing h gives ht, without a second matrix */
int rh_is_transpose(const uint16_t *h, uint64_t rows, uint64_t cols, const uint16_t *ht)
{
    int ok = 1;
#pragma omp parallel for schedule(static) num_threads(rh_threads()) reduction(&& : ok)
    for (uint64_t i0 = 0; i0 < rows; i0 += 64)
        for (uint64_t j0 = 0; j0 < cols; j0 += 64)
            for (uint64_t i = i0; i < i0 + 64 && i < rows; i++)
                for (uint64_t j = j0; j < j0 + 64 && j < cols; j++) ok = ok && ht[j * rows + i] == h[i * cols + j];
    return ok;
}

/* ---- float64 evaluations: value and sum of |terms| ------------------------------------------------------------------ */
void rh_mvm64(const uint16_t *A, uint64_t rows, uint64_t cols, const uint16_t *x, double *exact, double *absum)
{
    const float *T = rh_table();
#pragma omp parallel for schedule(static) num_threads(rh_threads())
    for (uint64_t i = 0; i < rows; i++) {
        double e = 0.0, a = 0.0;
        for (uint64_t j = 0; j < cols; j++) {
            const double p = (double)T[A[i * cols + j]] * (double)T[x[j]];      /* 22 significant bits: exact */
            e += p;
            a += fabs(p);
        }
        exact[i] = e;
        absum[i] = a;
    }
}

void rh_mvm_f32_64(const uint16_t *A, uint64_t rows, uint64_t cols, const float *x, double *exact, double *absum)
{
    const float *T = rh_table();
#pragma omp parallel for schedule(static) num_threads(rh_threads())
    for (uint64_t i = 0; i < rows; i++) {
        double e = 0.0, a = 0.0;
        for (uint64_t j = 0; j < cols; j++) {
            const double p = (double)T[A[i * cols + j]] * (double)x[j];         /* 35 significant bits: exact */
            e += p;
            a += fabs(p);
        }
        exact[i] = e;
        absum[i] = a;
    }
}

/* ---- threshold: the reference's heap walk ------------------------------------------------------------------------------- */
typedef struct { float value; uint16_t bits; uint32_t idx; } rh_item;

static int rh_gt(const rh_item *a, const rh_item *b) { return (a->value > b->value) || isnan(a->value); }

/* libstdc++ std::make_heap(first, first + k, comp): for parent = (k - 2) / 2 down to 0, __adjust_heap(first, parent, k, first[parent]) --
 * the hole moves down to a leaf along the children that do NOT compare `comp(right, left)`-smaller, then the value is pushed back up */
static void rh_make_heap(rh_item *h, uint64_t k)
{
    if (k < 2) return;
    for (uint64_t parent = (k - 2) / 2 + 1; parent-- > 0;) {
        const rh_item v = h[parent];
        uint64_t hole = parent, child = parent;
        while (child < (k - 1) / 2) {
            child = 2 * (child + 1);
            if (rh_gt(&h[child], &h[child - 1])) child--;
            h[hole] = h[child];
            hole = child;
        }
        if ((k & 1) == 0 && child == (k - 2) / 2) {
            child = 2 * (child + 1);
            h[hole] = h[child - 1];
            hole = child - 1;
        }
        while (hole > parent) {
            const uint64_t par = (hole - 1) / 2;
            if (!rh_gt(&h[par], &v)) break;
            h[hole] = h[par];
            hole = par;
        }
        h[hole] = v;
    }
}

static void rh_min_heapify(rh_item *h, uint64_t pos, uint64_t k)
{
    for (;;) {
        const uint64_t l = 2 * pos + 1, r = 2 * pos + 2;
        uint64_t smallest = pos;
        if (l < k && h[l].value < h[smallest].value) smallest = l;
        if (r < k && h[r].value < h[smallest].value) smallest = r;
        if (smallest == pos) break;
        const rh_item t = h[pos];
        h[pos] = h[smallest];
        h[smallest] = t;
        pos = smallest;
    }
}

/* threshold_min_heap(heap, k) over the first n elements of h, 1 <= k <= n: survivors keep their bits, the rest of [0, n) becomes 0;
 * heap_value / heap_idx (k entries, may be NULL) receive the heap as the walk leaves it */
void rh_threshold_heap(uint16_t *h, uint64_t n, uint64_t k, float *heap_value, uint32_t *heap_idx)
{
    const float *T = rh_table();
    rh_item *heap = (rh_item *)malloc((size_t)k * sizeof(rh_item));
    for (uint64_t i = 0; i < k; i++) {
        heap[i].value = T[h[i] & 0x7FFFu];
        heap[i].bits = h[i];
        heap[i].idx = (uint32_t)i;
        h[i] = 0;
    }
    rh_make_heap(heap, k);
    for (uint64_t i = k; i < n; i++) {
        const float value = T[h[i] & 0x7FFFu];
        if (value > heap[0].value) {
            heap[0].value = value;
            heap[0].bits = h[i];
            heap[0].idx = (uint32_t)i;
            rh_min_heapify(heap, 0, k);
        }
        h[i] = 0;
    }
    for (uint64_t i = 0; i < k; i++) {
        h[heap[i].idx] = heap[i].bits;
        if (heap_value) heap_value[i] = heap[i].value;
        if (heap_idx) heap_idx[i] = heap[i].idx;
    }
    free(heap);
}

/* the heap rh_make_heap builds from `values` (k entries): heap_value / heap_idx in array order -- what a test compares with std::make_heap */
void rh_make_heap_of(const float *values, uint64_t k, float *heap_value, uint32_t *heap_idx)
{
    rh_item *heap = (rh_item *)malloc((size_t)(k ? k : 1) * sizeof(rh_item));
    for (uint64_t i = 0; i < k; i++) { heap[i].value = values[i]; heap[i].bits = 0; heap[i].idx = (uint32_t)i; }
    rh_make_heap(heap, k);
    for (uint64_t i = 0; i < k; i++) { heap_value[i] = heap[i].value; heap_idx[i] = heap[i].idx; }
    free(heap);
}
