// mvm_f32_host.h -- the host side of the fp32-vector calls of the quantized matrices, written once: the argument and overlap check of the
// three products, the bodies of their entry points, and the IHT / GD loop in one call.  Included by mvm_f32_t.hip (CloverMatrix4,
// include/clover_hip_m4_f32.h) and matrix8_f32_t.hip (CloverMatrix8, include/clover_hip_m8_f32.h); fp32.hip (CloverMatrix32) includes it
// for f32_iht_loop() alone.  Each of the two defines its transposed kernel and a traits struct F with exactly what differs between the widths:
//   matrix_bytes(rows, cols)                  the bytes of a matrix, for the overlap check
//   max_elements                              the bound of rows * cols behind "matrix too large"
//   streaming(rows, cols)                     whether the matrix streams (NT): above the 256 MiB Infinity Cache
//   row_major_fused(...)                      the launch of the width's row-major kernel with the epilogue pack
//   transposed_launch<FUSE...>(...)           the grid, block and hipLaunchKernelGGL of the width's transposed kernel, defined beside it
//   scale_and_add, transposed_scale_and_add   the width's own fused calls, which the loop enqueues: their checks answer under their names
// The extern "C" entry points of a width forward to mvm_f32_fused_entry, mvm_f32_t_entry, mvm_f32_t_fused_entry and mvm_f32_iht (below) with
// their own names, which the messages quote.
#pragma once

#include "mvm_f32_device.h"
#include "clover_hip_fp32.h"

#define MVM_F32_ALIGNED16(p) (((uintptr_t)(p) & 15u) == 0)
#define MVM_F32_ALIGNED4(p) (((uintptr_t)(p) & 3u) == 0)

// every check of the three products, before any device work.  The plain transposed call has u == t == NULL and r2 = r; the row-major
// fused call has transposed == false.  Returns CLV_OK, CLV_ERR_INVALID, or 1: valid and nothing to do
template <class F>
static int mvm_f32_check_args(const char *fn, const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, bool transposed, bool fused,
                              const float *u, const float *t, const float *r2)
{
    const char *out = fused ? "r2" : "r";
    CLV_REQUIRE(A, "%s: A is NULL", fn);
    CLV_REQUIRE(sA, "%s: sA is NULL", fn);
    CLV_REQUIRE(x, "%s: x is NULL", fn);
    CLV_REQUIRE(!fused || u, "%s: u is NULL", fn);
    CLV_REQUIRE(r2, "%s: %s is NULL", fn, out);
    if (transposed)
        CLV_REQUIRE(rows % 128 == 0 && cols % 128 == 0, "%s: rows=%llu cols=%llu must be multiples of 128", fn, (unsigned long long)rows,
                    (unsigned long long)cols);
    else
        CLV_REQUIRE(rows % 64 == 0 && cols % 128 == 0, "%s: rows=%llu must be a multiple of 64 (a row shard) and cols=%llu of 128", fn,
                    (unsigned long long)rows, (unsigned long long)cols);
    CLV_REQUIRE(MVM_F32_ALIGNED16(A), "%s: A must be 16-byte aligned", fn);
    CLV_REQUIRE(MVM_F32_ALIGNED16(x), "%s: x must be 16-byte aligned", fn);
    CLV_REQUIRE(MVM_F32_ALIGNED4(sA) && MVM_F32_ALIGNED4(u) && MVM_F32_ALIGNED4(t) && MVM_F32_ALIGNED4(r2), "%s: sA%s and %s must be 4-byte aligned", fn,
                fused ? ", u, t" : "", out);
    CLV_REQUIRE(!cols || rows <= F::max_elements / cols, "%s: rows=%llu cols=%llu: matrix too large", fn, (unsigned long long)rows,
                (unsigned long long)cols);
    CLV_REQUIRE(rows / 32 <= 0x7FFFFFFFull && cols / 64 <= 0x7FFFFFFFull, "%s: rows=%llu cols=%llu: matrix too large", fn, (unsigned long long)rows,
                (unsigned long long)cols);
    const uint64_t nin = transposed ? rows : cols, nout = transposed ? cols : rows;
    std::vector<ClvRange> rg;
    rg.reserve(6);
    rg.push_back(clv_range(A, F::matrix_bytes(rows, cols), false, ~0ull, "A"));
    rg.push_back(clv_range(sA, (rows / 64) * (cols / 64) * 4, false, ~0ull, "sA"));
    rg.push_back(clv_range(x, nin * 4, false, 0, "x"));
    rg.push_back(clv_range(r2, nout * 4, true, 0, out));
    // the in-place form r2 == u: the result IS the input, only the lane that owns an element touches it in either
    if (fused && u != r2) rg.push_back(clv_range(u, nout * 4, false, 0, "u"));
    if (t) rg.push_back(clv_range(t, nout * 4, true, 0, "t"));
    const int rc = clv_internal_check_ranges(fn, rg);
    if (rc) return rc;
    return rows && cols ? CLV_OK : 1;
}

// ---- the bodies of a width's three extern "C" product entry points; fn = the name of the entry point that was called ---------------------
// *_mvm_f32_scale_and_add: t = A x (stored if t != NULL), r2 = u + a t
template <class F>
static int mvm_f32_fused_entry(const char *fn, const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, const float *u, float a,
                               float *t, float *r2, void *stream)
{
    const int rc = mvm_f32_check_args<F>(fn, A, sA, rows, cols, x, false, true, u, t, r2);
    if (rc) return rc > 0 ? CLV_OK : rc;
    return F::row_major_fused(A, sA, rows, cols, x, t, M4F32Fuse{u, a, r2}, as_stream(stream));
}

// *_mvm_f32_transposed: r = A' x straight from A
template <class F>
static int mvm_f32_t_entry(const char *fn, const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, float *r, void *stream)
{
    const int rc = mvm_f32_check_args<F>(fn, A, sA, rows, cols, x, true, false, nullptr, nullptr, r);
    if (rc) return rc > 0 ? CLV_OK : rc;
    return F::transposed_launch(A, sA, rows, cols, x, r, as_stream(stream));
}

// *_mvm_f32_transposed_scale_and_add: t = A' x (stored if t != NULL), r2 = u + a t
template <class F>
static int mvm_f32_t_fused_entry(const char *fn, const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, const float *u, float a,
                                 float *t, float *r2, void *stream)
{
    const int rc = mvm_f32_check_args<F>(fn, A, sA, rows, cols, x, true, true, u, t, r2);
    if (rc) return rc > 0 ? CLV_OK : rc;
    return F::transposed_launch(A, sA, rows, cols, x, t, as_stream(stream), M4F32Fuse{u, a, r2});
}

// The loop of Q_IHT / Q_GD (test/performance/01_measure.h:923-946, 999-1021) on CloverVector32 vectors, whatever the matrix: x.clear(),
// then per iteration forward() (t1 = Phi x; t2 = y - t1), backward() (t3 = Phi' t2; x += mu t3) and the threshold (0: none, Q_GD; 1: keep
// the K largest; 2: in the reference's survivor order).  Stops at the first error
template <class Forward, class Backward>
static int f32_iht_loop(float *x, uint64_t x_len, uint64_t n, uint64_t iterations, uint64_t K, int threshold, void *stream, Forward forward,
                        Backward backward)
{
    int rc = clv_internal_f32_clear(x, n, as_stream(stream));
    for (uint64_t it = 0; !rc && it < iterations; it++) {
        rc = forward();
        if (!rc) rc = backward();
        if (!rc && threshold)
            rc = clv_f32_threshold_mode(x, x_len, n, K, threshold == 2 ? CLV_THRESHOLD_REFERENCE : CLV_THRESHOLD_FAST, nullptr, stream);
    }
    return rc;
}

// Q_IHT / Q_GD over a quantized matrix with CloverVector32 vectors, the driver of clm_f32_iht (fp32.hip) with the width's matrices: one call
// enqueues all iterations, one fused launch per product plus the threshold, nothing copied back.  one_matrix (PhiT == NULL): the gradient
// step takes Phi' t2 straight from Phi.
template <class F>
static int mvm_f32_iht(const char *fn, const int8_t *Phi, const float *sPhi, const int8_t *PhiT, const float *sPhiT, bool one_matrix, uint64_t m,
                       uint64_t n, float *x, uint64_t x_len, const float *y, float *t1, float *t2, float *t3, uint64_t iterations, uint64_t K, float mu,
                       int threshold, void *stream)
{
    CLV_REQUIRE(Phi, "%s: Phi is NULL", fn);
    CLV_REQUIRE(sPhi, "%s: sPhi is NULL", fn);
    CLV_REQUIRE(one_matrix || PhiT, "%s: PhiT is NULL", fn);
    CLV_REQUIRE(one_matrix || sPhiT, "%s: sPhiT is NULL", fn);
    CLV_REQUIRE(x, "%s: x is NULL", fn);
    CLV_REQUIRE(y, "%s: y is NULL", fn);
    CLV_REQUIRE(t1, "%s: t1 is NULL", fn);
    CLV_REQUIRE(t2, "%s: t2 is NULL", fn);
    CLV_REQUIRE(t3, "%s: t3 is NULL", fn);
    CLV_REQUIRE(m % 128 == 0 && n % 128 == 0, "%s: m=%llu n=%llu must be multiples of 128", fn, (unsigned long long)m, (unsigned long long)n);
    CLV_REQUIRE(x_len <= n, "%s: x_len=%llu exceeds n=%llu", fn, (unsigned long long)x_len, (unsigned long long)n);
    CLV_REQUIRE(threshold >= 0 && threshold <= 2, "%s: unknown threshold %d", fn, threshold);
    CLV_REQUIRE(MVM_F32_ALIGNED16(Phi) && MVM_F32_ALIGNED16(PhiT), "%s: the matrices must be 16-byte aligned", fn);
    CLV_REQUIRE(MVM_F32_ALIGNED16(x), "%s: x must be 16-byte aligned", fn);
    CLV_REQUIRE(MVM_F32_ALIGNED16(t2), "%s: t2 must be 16-byte aligned", fn);
    CLV_REQUIRE(MVM_F32_ALIGNED4(sPhi) && MVM_F32_ALIGNED4(sPhiT) && MVM_F32_ALIGNED4(y) && MVM_F32_ALIGNED4(t1) && MVM_F32_ALIGNED4(t3),
                "%s: the scales, y, t1 and t3 must be 4-byte aligned", fn);
    CLV_REQUIRE(!n || m <= F::max_elements / n, "%s: m=%llu n=%llu: matrix too large", fn, (unsigned long long)m, (unsigned long long)n);
    {
        const uint64_t grid = (m / 64) * (n / 64) * 4;
        std::vector<ClvRange> rg;
        rg.reserve(9);
        rg.push_back(clv_range(Phi, F::matrix_bytes(m, n), false, ~0ull, "Phi"));
        rg.push_back(clv_range(sPhi, grid, false, ~0ull, "sPhi"));
        if (!one_matrix) {
            rg.push_back(clv_range(PhiT, F::matrix_bytes(m, n), false, ~0ull, "PhiT"));
            rg.push_back(clv_range(sPhiT, grid, false, ~0ull, "sPhiT"));
        }
        rg.push_back(clv_range(y, m * 4, false, 0, "y"));
        rg.push_back(clv_range(x, n * 4, true, 0, "x"));
        rg.push_back(clv_range(t1, m * 4, true, 0, "t1"));
        rg.push_back(clv_range(t2, m * 4, true, 0, "t2"));
        rg.push_back(clv_range(t3, n * 4, true, 0, "t3"));
        const int rc = clv_internal_check_ranges(fn, rg);
        if (rc) return rc;
    }
    return f32_iht_loop(
        x, x_len, n, iterations, K, threshold, stream, [&] { return F::scale_and_add(Phi, sPhi, m, n, x, y, -1.0f, t1, t2, stream); },
        [&] {
            return one_matrix ? F::transposed_scale_and_add(Phi, sPhi, m, n, t2, x, mu, t3, x, stream)
                              : F::scale_and_add(PhiT, sPhiT, n, m, t2, x, mu, t3, x, stream);
        });
}
