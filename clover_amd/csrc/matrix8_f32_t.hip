// matrix8_f32_t.hip -- CloverMatrix8 on fp32 vectors beyond the single product of matrix8.hip (include/clover_hip_m8_f32.h): the transposed
// product r = A' x straight from A's own bytes, the one argument-check layer of the three product calls, and the IHT / GD loop of
// <CloverMatrix8, CloverVector32> in one call, with two matrices or with one.
//
// Contract of the transposed product: bit for bit what clm8_transpose(A -> At) followed by clm8_mvm_f32(At, cols, rows, x -> r) gives.
// Output column c is row c of A' under the definition of k_m8_mvm_f32 (matrix8.hip): 32 sequential fp32 fma chains, row i of A on chain
// i mod 32 in increasing i, each from +0.0f, one step acc = fma(f32(x[i] * f32(s / 127.0f)), (float)q(i, c), acc) with s read from A's OWN
// scale grid at (row tile i / 64, column tile c / 64) -- the scale multiplies x, not q; then (acc1 + acc2) + (acc3 + acc4) per AVX lane and
// the _mm256_haddf32_ps tree, as the last lines of k_m8_mvm_f32.  tests/m8_f32_t_restate.c states the same walk on the CPU.
//
// This is the walk of k_m4_mvm_f32_t (mvm_f32_t.hip) over the bytes of k_m8_mvm_t (matrix8_t.hip): x is fp32 and every (column, chain) pair
// has a register of its own, so no byte is transposed and no sdot4 is used -- a lane converts the bytes of its own piece of a row and feeds
// each to its own accumulator.
// Mapping:
//   workgroup = a strip of M8FT_COLS columns = M8FT_COLS contiguous bytes of every row (128: one whole 128-byte line); it walks ALL rows (a
//               chain is ordered over the rows, so rows are never split between workgroups): cols / M8FT_COLS workgroups, all whole;
//   lane      = (piece p = tid % PIECES, chain k = tid / PIECES): ONE 16-byte load = 16 columns of row 32 b + k of every 32-row block b, one
//               accumulator per column: the lane's one chain is k.  32 * PIECES threads; a wave's load instruction reads 8 rows x 128 B;
//   per block = ONE x value (x[32 b + k]) and ONE factor f32(s / 127.0f) per lane -- the lane's 16 columns lie in one 64-column tile, the
//               block in one 64-row tile -- both staged in LDS per CLM8_F32_T_CHUNK rows: all loads first, then the LDS writes.  One
//               multiply t = x * f, then 16 converts and 16 fmas;
//   pipeline  = M8FT_U blocks of loads per register set, two sets that take turns: the set ahead is loaded -- unconditionally, clamped to
//               the last block -- before the arithmetic of the current one (m4ft_load, m8t_group);
//   bytes     = (float)(int8_t) of the stored byte: -128 is a legal byte and converts exactly;
//   epilogue  = the 32 chain ends of every column through LDS (stride M8FT_COLS + 1) to one lane per column: the tree and the fused
//               epilogue (m4f32_store, mvm_f32_device.h).  u[c] is fetched before the walk, so r2 may be u.
#include "mvm_f32_device.h"
#include "clover_hip_fp32.h"
#include "clover_hip_m8_f32.h"

#ifndef M8FT_COLS
#define M8FT_COLS 128       // columns = bytes of a row per workgroup (the maps measured: DESIGN.md 3)
#endif
#ifndef M8FT_U
#define M8FT_U 8            // 32-row blocks of matrix loads per register set = blocks issued ahead of the arithmetic
#endif
#ifndef M8FT_CVT
#define M8FT_CVT 0          // 0: sign-extending convert of the byte; 1: unsigned-byte convert of q ^ 0x80, minus 128 (both exact)
#endif
#define M8FT_CHUNK ((uint32_t)CLM8_F32_T_CHUNK)          // rows of x staged in LDS per pass
#define M8FT_PIECES (M8FT_COLS / 16)                     // lanes per row
#define M8FT_THREADS (32 * M8FT_PIECES)
#define M8FT_TILES ((M8FT_COLS + 63) / 64)               // column tiles (of A's scale grid) a strip touches
#define M8FT_PART_STRIDE (M8FT_COLS + 1)

static_assert(M8FT_COLS == 64 || M8FT_COLS == 128, "a strip is whole 64-column tiles and divides cols (a multiple of 128)");
static_assert(M8FT_THREADS >= M8FT_COLS && M8FT_THREADS <= 1024, "one lane per column in the epilogue");
static_assert((M8FT_CHUNK / 32) % (2 * M8FT_U) == 0 && M8FT_CHUNK % (4 * M8FT_THREADS) == 0, "a chunk is whole pairs of load groups and whole rounds of staging threads");
static_assert(32 * M8FT_PART_STRIDE <= M8FT_CHUNK + M8FT_CHUNK / 64 * M8FT_TILES, "the chain ends reuse the staging area");

template <bool NT> __device__ __forceinline__ u32x4 m8ft_ld(const u32x4 *p) { return NT ? __builtin_nontemporal_load(p) : *p; }

// stage x and the factors f32(s / 127.0f) of the chunk that starts at row r0: all loads first (one round trip), then the LDS writes
__device__ __forceinline__ void m8ft_stage(float *xs, float *cs, const float *__restrict__ x, const float *__restrict__ sA, uint64_t rows, uint64_t G,
                                           uint64_t tile0, uint64_t r0, int tid)
{
    constexpr int NX = M8FT_CHUNK / 4 / M8FT_THREADS;        // 16-byte pieces of x per thread
    constexpr int NC = (M8FT_CHUNK / 64 * M8FT_TILES + M8FT_THREADS - 1) / M8FT_THREADS;      // factors per thread
    const uint32_t ch = (uint32_t)((rows - r0) < M8FT_CHUNK ? (rows - r0) : M8FT_CHUNK);
    if (r0) __syncthreads();                                 // the previous chunk's x has been consumed
    const f32x4 *xg = reinterpret_cast<const f32x4 *>(x) + r0 / 4;
    const uint32_t nx = ch / 4, nc = ch / 64 * M8FT_TILES;
    f32x4 xr[NX];
#pragma unroll
    for (int j = 0; j < NX; j++) { const uint32_t i = tid + M8FT_THREADS * j; xr[j] = xg[i < nx ? i : 0]; }
    float c[NC];
#pragma unroll
    for (int j = 0; j < NC; j++) {
        const uint32_t i = tid + M8FT_THREADS * j, ci = i < nc ? i : 0;
        c[j] = sA[(r0 / 64 + ci / M8FT_TILES) * G + tile0 + ci % M8FT_TILES] / 127.0f;      // the expression of k_m8_mvm_f32
    }
#pragma unroll
    for (int j = 0; j < NX; j++) { const uint32_t i = tid + M8FT_THREADS * j; if (i < nx) reinterpret_cast<f32x4 *>(xs)[i] = xr[j]; }
#pragma unroll
    for (int j = 0; j < NC; j++) { const uint32_t i = tid + M8FT_THREADS * j; if (i < nc) cs[i] = c[j]; }
    __syncthreads();
}

// the loads of group g (U blocks) of the lane whose row of block 0 and piece Ap points at; blocks beyond the last read the last one again
template <int U, bool NT>
__device__ __forceinline__ void m8ft_load(const u32x4 *__restrict__ Ap, uint64_t stride, uint32_t g, uint32_t nblk, u32x4 (&a)[U])
{
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint32_t b = g * U + u, bc = b < nblk ? b : nblk - 1;
        a[u] = m8ft_ld<NT>(Ap + (uint64_t)bc * 32 * stride);
    }
}

// byte e (0..3) of a dword as a float, exactly, -128 included
__device__ __forceinline__ float m8ft_byte(uint32_t w, int e)
{
#if M8FT_CVT == 1
    return (float)(((w ^ 0x80808080u) >> (8 * e)) & 0xFFu) - 128.0f;
#else
    return (float)((int)(w << (24 - 8 * e)) >> 24);
#endif
}

// one chain step of the lane's 16 columns: t = f32(x of the lane's row * f32(s / 127.0f) of its tile)
__device__ __forceinline__ void m8ft_block(const u32x4 &a, float t, float (&acc)[16])
{
#pragma unroll
    for (int w = 0; w < 4; w++)
#pragma unroll
        for (int e = 0; e < 4; e++) acc[4 * w + e] = __builtin_fmaf(t, m8ft_byte(a[w], e), acc[4 * w + e]);
}

// group g of the walk from `cur` (loaded a group ago) while the next group's loads go to `nxt` -- issued UNCONDITIONALLY (beyond the last
// block: the last block again), so that the wait for `cur` lets them stay in flight.  xl = xs + the lane's chain, cl = cs + the lane's tile
template <int U, bool NT>
__device__ __forceinline__ void m8ft_group(const u32x4 (&cur)[U], u32x4 (&nxt)[U], const u32x4 *__restrict__ Ap, uint64_t stride, uint32_t g, uint32_t nblk,
                                           const float *xl, const float *cl, float (&acc)[16])
{
    constexpr uint32_t CB = M8FT_CHUNK / 32;             // blocks per chunk
    m8ft_load<U, NT>(Ap, stride, g + 1, nblk, nxt);
    const uint32_t b0 = g * U, lb = b0 % CB;             // a group never straddles a chunk
#pragma unroll
    for (int u = 0; u < U; u++)
        if (b0 + u < nblk) m8ft_block(cur[u], xl[32 * (lb + u)] * cl[M8FT_TILES * ((lb + u) >> 1)], acc);
}

// FUSE... = nothing or one M4F32Fuse, as k_m8_mvm_f32 (matrix8.hip).  r (t of the fused ABI) may be NULL under FUSE; fuse.r2 may be fuse.u
template <int U, bool NT, typename... FUSE>
__global__ __launch_bounds__(M8FT_THREADS) void k_m8_mvm_f32_t(const uint8_t *__restrict__ A, const float *__restrict__ sA, uint64_t rows, uint64_t cols,
                                                               const float *__restrict__ x, float *__restrict__ r, FUSE... fuse)
{
    __shared__ __attribute__((aligned(16))) float stage[M8FT_CHUNK + M8FT_CHUNK / 64 * M8FT_TILES];
    float *xs = stage;                                   // M8FT_CHUNK values of x
    float *cs = stage + M8FT_CHUNK;                      // [M8FT_CHUNK / 64][M8FT_TILES] factors
    float *part = stage;                                 // epilogue: [32 chains][M8FT_PART_STRIDE]
    constexpr bool FUSED = sizeof...(FUSE) != 0;

    const int tid = threadIdx.x, p = tid % M8FT_PIECES, k = tid / M8FT_PIECES;
    const uint64_t strip0 = (uint64_t)blockIdx.x * M8FT_COLS, G = cols / 64;
    // the epilogue's lane of column strip0 + tid: its element of u, fetched now so that the epilogue does not wait for it (and r2 may be u)
    const uint64_t col = strip0 + tid;
    const bool owner = tid < M8FT_COLS;
    float fuse_u = 0.0f;
    if (FUSED && owner) fuse_u = m4f32_fuse_load_u(col, fuse...);

    const uint64_t stride = cols / 16;                   // pieces per row
    const u32x4 *Ap = reinterpret_cast<const u32x4 *>(A) + strip0 / 16 + p + (uint64_t)k * stride;
    const float *xl = xs + k, *cl = cs + p / 4;

    float acc[16];
#pragma unroll
    for (int e = 0; e < 16; e++) acc[e] = 0.0f;

    // the walk over all rows in groups of U blocks; a chunk is a whole, even number of groups, so x is re-staged in front of an even group.
    // Two register sets take turns: no copies, and the loads of the group ahead stay in flight across the staging
    constexpr uint32_t CG = M8FT_CHUNK / 32 / U;
    const uint32_t nblk = (uint32_t)(rows / 32), ngroups = (nblk + U - 1) / U;
    u32x4 a[U], b[U];
    m8ft_load<U, NT>(Ap, stride, 0, nblk, a);
    uint32_t g = 0;
    for (; g + 1 < ngroups; g += 2) {
        if (g % CG == 0) m8ft_stage(xs, cs, x, sA, rows, G, strip0 / 64, (uint64_t)g * U * 32, tid);
        m8ft_group<U, NT>(a, b, Ap, stride, g, nblk, xl, cl, acc);
        m8ft_group<U, NT>(b, a, Ap, stride, g + 1, nblk, xl, cl, acc);
    }
    if (g < ngroups) {
        if (g % CG == 0) m8ft_stage(xs, cs, x, sA, rows, G, strip0 / 64, (uint64_t)g * U * 32, tid);
        m8ft_group<U, NT>(a, b, Ap, stride, g, nblk, xl, cl, acc);
    }

    // the 32 chain ends of every column meet in the column's lane
    __syncthreads();                                     // x and the factors have been consumed: the area is reused
#pragma unroll
    for (int e = 0; e < 16; e++) part[k * M8FT_PART_STRIDE + 16 * p + e] = acc[e];
    __syncthreads();
    if (owner) {
        const float *q = part + tid;
        float s[8];
#pragma unroll
        for (int l = 0; l < 8; l++)
            s[l] = (q[l * M8FT_PART_STRIDE] + q[(8 + l) * M8FT_PART_STRIDE]) + (q[(16 + l) * M8FT_PART_STRIDE] + q[(24 + l) * M8FT_PART_STRIDE]);
        const float t0 = s[4] + s[0], t1 = s[5] + s[1], t2 = s[6] + s[2], t3 = s[7] + s[3];
        m4f32_store(r, col, (t0 + t2) + (t1 + t3), fuse_u, fuse...);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
#define M8F32_ALIGNED16(p) (((uintptr_t)(p) & 15u) == 0)
#define M8F32_ALIGNED4(p) (((uintptr_t)(p) & 3u) == 0)

// every check of the three products, before any device work.  The plain transposed call has u == t == NULL and r2 = r; the row-major
// fused call has transposed == false.  Returns CLV_OK, CLV_ERR_INVALID, or 1: valid and nothing to do
static int m8f32_check_args(const char *fn, const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, bool transposed, bool fused,
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
    CLV_REQUIRE(M8F32_ALIGNED16(A), "%s: A must be 16-byte aligned", fn);
    CLV_REQUIRE(M8F32_ALIGNED16(x), "%s: x must be 16-byte aligned", fn);
    CLV_REQUIRE(M8F32_ALIGNED4(sA) && M8F32_ALIGNED4(u) && M8F32_ALIGNED4(t) && M8F32_ALIGNED4(r2), "%s: sA%s and %s must be 4-byte aligned", fn,
                fused ? ", u, t" : "", out);
    CLV_REQUIRE(!cols || rows <= 0x1000000000000ull / cols, "%s: rows=%llu cols=%llu: matrix too large", fn, (unsigned long long)rows,
                (unsigned long long)cols);
    CLV_REQUIRE(rows / 32 <= 0x7FFFFFFFull && cols / 64 <= 0x7FFFFFFFull, "%s: rows=%llu cols=%llu: matrix too large", fn, (unsigned long long)rows,
                (unsigned long long)cols);
    const uint64_t nin = transposed ? rows : cols, nout = transposed ? cols : rows;
    std::vector<ClvRange> rg;
    rg.reserve(6);
    rg.push_back(clv_range(A, rows * cols, false, ~0ull, "A"));
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

template <typename... FUSE>
static int m8f32_t_launch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, float *r, hipStream_t st, FUSE... fuse)
{
    const dim3 grid((unsigned)(cols / M8FT_COLS)), block(M8FT_THREADS);
    if (m8f32_streaming(rows, cols))
        hipLaunchKernelGGL((k_m8_mvm_f32_t<M8FT_U, true, FUSE...>), grid, block, 0, st, (const uint8_t *)A, sA, rows, cols, x, r, fuse...);
    else
        hipLaunchKernelGGL((k_m8_mvm_f32_t<M8FT_U, false, FUSE...>), grid, block, 0, st, (const uint8_t *)A, sA, rows, cols, x, r, fuse...);
    CLV_LAUNCH_CHECK();
    return CLV_OK;
}

extern "C" int clm8_mvm_f32_scale_and_add(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, const float *u, float a,
                                          float *t, float *r2, void *stream)
{
    const int rc = m8f32_check_args("clm8_mvm_f32_scale_and_add", A, sA, rows, cols, x, false, true, u, t, r2);
    if (rc) return rc > 0 ? CLV_OK : rc;
    return clv_internal_m8_mvm_f32_fused(A, sA, rows, cols, x, t, M4F32Fuse{u, a, r2}, as_stream(stream));
}

extern "C" int clm8_mvm_f32_transposed(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, float *r, void *stream)
{
    const int rc = m8f32_check_args("clm8_mvm_f32_transposed", A, sA, rows, cols, x, true, false, nullptr, nullptr, r);
    if (rc) return rc > 0 ? CLV_OK : rc;
    return m8f32_t_launch(A, sA, rows, cols, x, r, as_stream(stream));
}

extern "C" int clm8_mvm_f32_transposed_scale_and_add(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, const float *u,
                                                     float a, float *t, float *r2, void *stream)
{
    const int rc = m8f32_check_args("clm8_mvm_f32_transposed_scale_and_add", A, sA, rows, cols, x, true, true, u, t, r2);
    if (rc) return rc > 0 ? CLV_OK : rc;
    return m8f32_t_launch(A, sA, rows, cols, x, t, as_stream(stream), M4F32Fuse{u, a, r2});
}

// Q_IHT / Q_GD (test/performance/01_measure.h:923-946, 999-1021) over CloverMatrix8 with CloverVector32 vectors, the driver of clm4_iht_f32
// (mvm_f32_t.hip) with 8-bit matrices: one call enqueues all iterations, one fused launch per product plus the threshold, nothing copied
// back.  PhiT == NULL: the one-matrix form, whose gradient step takes Phi' t2 straight from Phi.
static int m8f32_iht(const char *fn, const int8_t *Phi, const float *sPhi, const int8_t *PhiT, const float *sPhiT, bool one_matrix, uint64_t m,
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
    CLV_REQUIRE(M8F32_ALIGNED16(Phi) && M8F32_ALIGNED16(PhiT), "%s: the matrices must be 16-byte aligned", fn);
    CLV_REQUIRE(M8F32_ALIGNED16(x), "%s: x must be 16-byte aligned", fn);
    CLV_REQUIRE(M8F32_ALIGNED16(t2), "%s: t2 must be 16-byte aligned", fn);
    CLV_REQUIRE(M8F32_ALIGNED4(sPhi) && M8F32_ALIGNED4(sPhiT) && M8F32_ALIGNED4(y) && M8F32_ALIGNED4(t1) && M8F32_ALIGNED4(t3),
                "%s: the scales, y, t1 and t3 must be 4-byte aligned", fn);
    CLV_REQUIRE(!n || m <= 0x1000000000000ull / n, "%s: m=%llu n=%llu: matrix too large", fn, (unsigned long long)m, (unsigned long long)n);
    {
        const uint64_t grid = (m / 64) * (n / 64) * 4;
        std::vector<ClvRange> rg;
        rg.reserve(9);
        rg.push_back(clv_range(Phi, m * n, false, ~0ull, "Phi"));
        rg.push_back(clv_range(sPhi, grid, false, ~0ull, "sPhi"));
        if (!one_matrix) {
            rg.push_back(clv_range(PhiT, m * n, false, ~0ull, "PhiT"));
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
    int rc = clv_internal_f32_clear(x, n, as_stream(stream));                                              // x.clear()
    for (uint64_t it = 0; !rc && it < iterations; it++) {
        rc = clm8_mvm_f32_scale_and_add(Phi, sPhi, m, n, x, y, -1.0f, t1, t2, stream);                     // t1 = Phi x; t2 = y - t1
        if (!rc)                                                                                           // t3 = Phi' t2; x += mu t3
            rc = one_matrix ? clm8_mvm_f32_transposed_scale_and_add(Phi, sPhi, m, n, t2, x, mu, t3, x, stream)
                            : clm8_mvm_f32_scale_and_add(PhiT, sPhiT, n, m, t2, x, mu, t3, x, stream);
        if (!rc && threshold)                                                          // keep the K largest (2: the reference's survivor order)
            rc = clv_f32_threshold_mode(x, x_len, n, K, threshold == 2 ? CLV_THRESHOLD_REFERENCE : CLV_THRESHOLD_FAST, nullptr, stream);
    }
    return rc;
}

extern "C" int clm8_iht_f32(const int8_t *Phi, const float *sPhi, const int8_t *PhiT, const float *sPhiT, uint64_t m, uint64_t n, float *x,
                            uint64_t x_len, const float *y, float *t1, float *t2, float *t3, uint64_t iterations, uint64_t K, float mu, int threshold,
                            void *stream)
{
    return m8f32_iht("clm8_iht_f32", Phi, sPhi, PhiT, sPhiT, false, m, n, x, x_len, y, t1, t2, t3, iterations, K, mu, threshold, stream);
}

extern "C" int clm8_iht_f32_one_matrix(const int8_t *Phi, const float *sPhi, uint64_t m, uint64_t n, float *x, uint64_t x_len, const float *y, float *t1,
                                       float *t2, float *t3, uint64_t iterations, uint64_t K, float mu, int threshold, void *stream)
{
    return m8f32_iht("clm8_iht_f32_one_matrix", Phi, sPhi, nullptr, nullptr, true, m, n, x, x_len, y, t1, t2, t3, iterations, K, mu, threshold, stream);
}
