// mvm_f32_t.hip -- CloverMatrix4 on fp32 vectors beyond the single product of mvm_f32.hip (include/clover_hip_m4_f32.h): the transposed
// product r = A' x straight from A's own bytes, the one argument-check layer of the three product calls, and the IHT / GD loop of
// <CloverMatrix4, CloverVector32> in one call, with two matrices or with one.
//
// Contract of the transposed product: bit for bit what clm4_transpose(A -> At) followed by clm4_mvm_f32(At, cols, rows, x -> r) gives.
// Output column c is row c of A' under the definition of k_m4_mvm_f32 (mvm_f32.hip): 32 sequential fp32 fma chains, row i of A on chain
// i mod 32 in increasing i, each from +0.0f, one step acc = fma(x[i], f32((float)q(i, c) * f32(s / 7)), acc) with s read from A's OWN
// scale grid at (row tile i / 64, column tile c / 64); then (acc1 + acc2) + (acc3 + acc4) per AVX lane and the _mm256_haddf32_ps tree, as
// the last lines of k_m4_mvm_f32.  tests/m4_f32_t_restate.c states the same walk on the CPU.
//
// x is fp32 and every (column, chain) pair has a register of its own, so -- unlike k_m4_mvm_t (mvm_t4.hip) -- NO nibble is transposed:
// a lane converts the nibbles of its own piece of a row and feeds each to its own accumulator.
// Mapping:
//   workgroup = a strip of M4FT_COLS columns = M4FT_COLS / 2 contiguous bytes of every row; it walks ALL rows (a chain is ordered over the
//               rows, so rows are never split between workgroups): ceil(cols / M4FT_COLS) workgroups.  A strip of 256 columns leaves the
//               last workgroup half outside when cols / 128 is odd: its lanes beyond `cols` read the strip's first piece (addresses stay
//               inside the matrix) and store nothing;
//   lane      = (piece p = tid % PIECES, chain k = tid / PIECES): M4FT_WORDS dwords = 8 M4FT_WORDS columns of row 32 b + k of every 32-row
//               block b, one accumulator per column: the lane's one chain is k.  32 * PIECES threads;
//   per block = ONE x value (x[32 b + k]) and ONE factor f32(s / 7) per lane -- the lane's columns lie in one 64-column tile, the block
//               in one 64-row tile -- both staged in LDS per CLM4_F32_T_CHUNK rows: all loads first, then the LDS writes;
//   pipeline  = M4FT_U blocks of loads per register set, two sets that take turns: the set ahead is loaded -- unconditionally, clamped to
//               the last block -- before the arithmetic of the current one (f16t_group, half16_t.hip);
//   (q / 16) (16 c): where every factor c of the strip's chunk survives 16 c (the barrier of the staging tells), the nibbles are taken as
//               q / 16 by v_cvt_off_f32_i4 (unpack8_16th, common.h) and the product rounds like q * c; otherwise the chunk takes the plain
//               conversion.  Same bits either way;
//   epilogue  = the 32 chain ends of every column through LDS (stride M4FT_COLS + 1) to one lane per column: the tree and the fused
//               epilogue (m4f32_store).  u[c] is fetched before the walk, so r2 may be u.
#include "mvm_f32_device.h"
#include "clover_hip_fp32.h"
#include "clover_hip_m4_f32.h"

#include <type_traits>

#ifndef M4FT_COLS
#define M4FT_COLS 128       // columns per workgroup (the maps measured: DESIGN.md 3)
#endif
#ifndef M4FT_WORDS
#define M4FT_WORDS 1        // dwords (8 columns each) per lane and row: 1, 2 or 4
#endif
#ifndef M4FT_U
#define M4FT_U 8            // 32-row blocks of matrix loads per register set = blocks issued ahead of the arithmetic
#endif
#define M4FT_CHUNK ((uint32_t)CLM4_F32_T_CHUNK)          // rows of x staged in LDS per pass
#define M4FT_PIECES (M4FT_COLS / (8 * M4FT_WORDS))       // lanes per row
#define M4FT_THREADS (32 * M4FT_PIECES)
#define M4FT_TILES ((M4FT_COLS + 63) / 64)               // column tiles (of A's scale grid) a strip touches
#define M4FT_PART_STRIDE (M4FT_COLS + 1)

static_assert(M4FT_COLS == 64 || M4FT_COLS == 128 || M4FT_COLS == 256, "a strip is whole 64-column tiles; 256 columns are 128 B of every row");
static_assert(M4FT_WORDS == 1 || M4FT_WORDS == 2 || M4FT_WORDS == 4, "a lane loads 4, 8 or 16 bytes");
static_assert(M4FT_THREADS >= M4FT_COLS && M4FT_THREADS <= 1024, "one lane per column in the epilogue");
static_assert((M4FT_CHUNK / 32) % (2 * M4FT_U) == 0 && M4FT_CHUNK % (4 * M4FT_THREADS) == 0, "a chunk is whole pairs of load groups and whole rounds of staging threads");
static_assert(32 * M4FT_PART_STRIDE <= M4FT_CHUNK + M4FT_CHUNK / 64 * M4FT_TILES, "the chain ends reuse the staging area");

template <int W> struct m4ft_words;
template <> struct m4ft_words<1> { typedef uint32_t type; };
template <> struct m4ft_words<2> { typedef u32x2 type; };
template <> struct m4ft_words<4> { typedef u32x4 type; };
typedef m4ft_words<M4FT_WORDS>::type m4ft_piece;

__device__ __forceinline__ uint32_t m4ft_word(uint32_t v, int) { return v; }
__device__ __forceinline__ uint32_t m4ft_word(const u32x2 &v, int i) { return v[i]; }
__device__ __forceinline__ uint32_t m4ft_word(const u32x4 &v, int i) { return v[i]; }

template <bool NT> __device__ __forceinline__ m4ft_piece m4ft_ld(const m4ft_piece *p) { return NT ? __builtin_nontemporal_load(p) : *p; }

// stage x and the factors f32(s / 7) of the chunk that starts at row r0: all loads first (one round trip), then the LDS writes.  Returns
// (to every thread) whether every factor of the chunk survives a multiplication by 16
__device__ __forceinline__ bool m4ft_stage(float *xs, float *cs, const float *__restrict__ x, const float *__restrict__ sA, uint64_t rows, uint64_t G,
                                           uint64_t tile0, uint64_t r0, int tid)
{
    constexpr int NX = M4FT_CHUNK / 4 / M4FT_THREADS;        // 16-byte pieces of x per thread
    constexpr int NC = (M4FT_CHUNK / 64 * M4FT_TILES + M4FT_THREADS - 1) / M4FT_THREADS;      // factors per thread
    const uint32_t ch = (uint32_t)((rows - r0) < M4FT_CHUNK ? (rows - r0) : M4FT_CHUNK);
    if (r0) __syncthreads();                                 // the previous chunk's x has been consumed
    const f32x4 *xg = reinterpret_cast<const f32x4 *>(x) + r0 / 4;
    const uint32_t nx = ch / 4, nc = ch / 64 * M4FT_TILES;
    f32x4 xr[NX];
#pragma unroll
    for (int j = 0; j < NX; j++) { const uint32_t i = tid + M4FT_THREADS * j; xr[j] = xg[i < nx ? i : 0]; }
    float c[NC];
#pragma unroll
    for (int j = 0; j < NC; j++) {
        const uint32_t i = tid + M4FT_THREADS * j, ci = i < nc ? i : 0;
        const uint64_t t = tile0 + ci % M4FT_TILES;          // a tile beyond the matrix (masked last strip): tile 0 of the same row tile
        c[j] = div7(sA[(r0 / 64 + ci / M4FT_TILES) * G + (t < G ? t : 0)]);
    }
#pragma unroll
    for (int j = 0; j < NX; j++) { const uint32_t i = tid + M4FT_THREADS * j; if (i < nx) reinterpret_cast<f32x4 *>(xs)[i] = xr[j]; }
    bool fast = true;
#pragma unroll
    for (int j = 0; j < NC; j++) {
        const uint32_t i = tid + M4FT_THREADS * j;
        if (i < nc) cs[i] = c[j];
        fast = fast && times16_is_finite(c[j]);              // a clamped index repeats a factor of the chunk
    }
    return __syncthreads_and(fast) != 0;
}

// the loads of group g (U blocks) of the lane whose row of block 0 and piece Ap points at; blocks beyond the last read the last one again
template <int U, bool NT>
__device__ __forceinline__ void m4ft_load(const m4ft_piece *__restrict__ Ap, uint64_t stride, uint32_t g, uint32_t nblk, m4ft_piece (&a)[U])
{
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint32_t b = g * U + u, bc = b < nblk ? b : nblk - 1;
        a[u] = m4ft_ld<NT>(Ap + (uint64_t)bc * 32 * stride);
    }
}

// one chain step of the lane's 8 M4FT_WORDS columns: xv = x of the lane's row, c = f32(s / 7) of its tile
template <bool FAST>
__device__ __forceinline__ void m4ft_block(const m4ft_piece &a, float xv, float c, float (&acc)[8 * M4FT_WORDS])
{
    const float c16 = c * 16.0f;
#pragma unroll
    for (int w = 0; w < M4FT_WORDS; w++) {
        const uint32_t word = m4ft_word(a, w);
        if constexpr (FAST) {
            float f[8];
            unpack8_16th(word, f);                                          // q / 16
#pragma unroll
            for (int e = 0; e < 8; e++) acc[8 * w + e] = __builtin_fmaf(xv, f[e] * c16, acc[8 * w + e]);      // rounded product first
        } else {
#pragma unroll
            for (int e = 0; e < 8; e++) acc[8 * w + e] = __builtin_fmaf(xv, (float)unpack1(word, e) * c, acc[8 * w + e]);
        }
    }
}

// group g of the walk from `cur` (loaded a group ago) while the next group's loads go to `nxt` -- issued UNCONDITIONALLY (beyond the last
// block: the last block again), so that the wait for `cur` lets them stay in flight.  xl = xs + the lane's chain, cl = cs + the lane's tile
template <int U, bool NT, bool FAST>
__device__ __forceinline__ void m4ft_group(const m4ft_piece (&cur)[U], m4ft_piece (&nxt)[U], const m4ft_piece *__restrict__ Ap, uint64_t stride, uint32_t g,
                                           uint32_t nblk, const float *xl, const float *cl, float (&acc)[8 * M4FT_WORDS])
{
    constexpr uint32_t CB = M4FT_CHUNK / 32;             // blocks per chunk
    m4ft_load<U, NT>(Ap, stride, g + 1, nblk, nxt);
    const uint32_t b0 = g * U, lb = b0 % CB;             // a group never straddles a chunk
#pragma unroll
    for (int u = 0; u < U; u++)
        if (b0 + u < nblk) m4ft_block<FAST>(cur[u], xl[32 * (lb + u)], cl[M4FT_TILES * ((lb + u) >> 1)], acc);
}

// FUSE... = nothing or one M4F32Fuse, as k_m4_mvm_f32 (mvm_f32.hip).  r (t of the fused ABI) may be NULL under FUSE; fuse.r2 may be fuse.u
template <int U, bool NT, typename... FUSE>
__global__ __launch_bounds__(M4FT_THREADS) void k_m4_mvm_f32_t(const uint8_t *__restrict__ A, const float *__restrict__ sA, uint64_t rows, uint64_t cols,
                                                               const float *__restrict__ x, float *__restrict__ r, FUSE... fuse)
{
    __shared__ __attribute__((aligned(16))) float stage[M4FT_CHUNK + M4FT_CHUNK / 64 * M4FT_TILES];
    float *xs = stage;                                   // M4FT_CHUNK values of x
    float *cs = stage + M4FT_CHUNK;                      // [M4FT_CHUNK / 64][M4FT_TILES] factors
    float *part = stage;                                 // epilogue: [32 chains][M4FT_PART_STRIDE]
    constexpr bool FUSED = sizeof...(FUSE) != 0;
    constexpr bool PARTIAL = M4FT_COLS > 128;            // cols % 128 == 0 makes narrower strips whole
    constexpr int NACC = 8 * M4FT_WORDS;

    const int tid = threadIdx.x, p = tid % M4FT_PIECES, k = tid / M4FT_PIECES;
    const uint64_t strip0 = (uint64_t)blockIdx.x * M4FT_COLS, G = cols / 64;
    // the epilogue's lane of column strip0 + tid: its element of u, fetched now so that the epilogue does not wait for it (and r2 may be u)
    const uint64_t col = strip0 + tid;
    const bool owner = tid < M4FT_COLS && (!PARTIAL || col < cols);
    float fuse_u = 0.0f;
    if (FUSED && owner) fuse_u = m4f32_fuse_load_u(col, fuse...);

    const uint64_t stride = cols / NACC;                 // pieces per row
    uint64_t c0 = strip0 + NACC * (uint64_t)p;
    if (PARTIAL && c0 >= cols) c0 = strip0;              // loads stay inside the matrix; nothing of it is stored
    const m4ft_piece *Ap = reinterpret_cast<const m4ft_piece *>(A) + c0 / NACC + (uint64_t)k * stride;
    const float *xl = xs + k, *cl = cs + (NACC * p) / 64;

    float acc[NACC];
#pragma unroll
    for (int e = 0; e < NACC; e++) acc[e] = 0.0f;

    // the walk over all rows in groups of U blocks; a chunk is a whole, even number of groups, so x is re-staged in front of an even group.
    // Two register sets take turns: no copies, and the loads of the group ahead stay in flight across the staging
    constexpr uint32_t CG = M4FT_CHUNK / 32 / U;
    const uint32_t nblk = (uint32_t)(rows / 32), ngroups = (nblk + U - 1) / U;
    m4ft_piece a[U], b[U];
    m4ft_load<U, NT>(Ap, stride, 0, nblk, a);
    bool fast = false;
    uint32_t g = 0;
    for (; g + 1 < ngroups; g += 2) {
        if (g % CG == 0) fast = m4ft_stage(xs, cs, x, sA, rows, G, strip0 / 64, (uint64_t)g * U * 32, tid);
        if (fast) {                                      // the same for every lane of the workgroup: a real branch
            m4ft_group<U, NT, true>(a, b, Ap, stride, g, nblk, xl, cl, acc);
            m4ft_group<U, NT, true>(b, a, Ap, stride, g + 1, nblk, xl, cl, acc);
        } else {
            m4ft_group<U, NT, false>(a, b, Ap, stride, g, nblk, xl, cl, acc);
            m4ft_group<U, NT, false>(b, a, Ap, stride, g + 1, nblk, xl, cl, acc);
        }
    }
    if (g < ngroups) {
        if (g % CG == 0) fast = m4ft_stage(xs, cs, x, sA, rows, G, strip0 / 64, (uint64_t)g * U * 32, tid);
        if (fast) m4ft_group<U, NT, true>(a, b, Ap, stride, g, nblk, xl, cl, acc);
        else m4ft_group<U, NT, false>(a, b, Ap, stride, g, nblk, xl, cl, acc);
    }

    // the 32 chain ends of every column meet in the column's lane
    __syncthreads();                                     // x and the factors have been consumed: the area is reused
#pragma unroll
    for (int e = 0; e < NACC; e++) part[k * M4FT_PART_STRIDE + NACC * p + e] = acc[e];
    __syncthreads();
    if (owner) {
        const float *q = part + tid;
        float s[8];
#pragma unroll
        for (int l = 0; l < 8; l++)
            s[l] = (q[l * M4FT_PART_STRIDE] + q[(8 + l) * M4FT_PART_STRIDE]) + (q[(16 + l) * M4FT_PART_STRIDE] + q[(24 + l) * M4FT_PART_STRIDE]);
        const float t0 = s[4] + s[0], t1 = s[5] + s[1], t2 = s[6] + s[2], t3 = s[7] + s[3];
        m4f32_store(r, col, (t0 + t2) + (t1 + t3), fuse_u, fuse...);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
#define M4F32_ALIGNED16(p) (((uintptr_t)(p) & 15u) == 0)
#define M4F32_ALIGNED4(p) (((uintptr_t)(p) & 3u) == 0)

// every check of the three products, before any device work.  The plain transposed call has u == t == NULL and r2 = r; the row-major
// fused call has transposed == false.  Returns CLV_OK, CLV_ERR_INVALID, or 1: valid and nothing to do
static int m4f32_check_args(const char *fn, const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, bool transposed, bool fused,
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
    CLV_REQUIRE(M4F32_ALIGNED16(A), "%s: A must be 16-byte aligned", fn);
    CLV_REQUIRE(M4F32_ALIGNED16(x), "%s: x must be 16-byte aligned", fn);
    CLV_REQUIRE(M4F32_ALIGNED4(sA) && M4F32_ALIGNED4(u) && M4F32_ALIGNED4(t) && M4F32_ALIGNED4(r2), "%s: sA%s and %s must be 4-byte aligned", fn,
                fused ? ", u, t" : "", out);
    CLV_REQUIRE(!cols || rows <= 0xFFFFFFFFFFFFull / cols, "%s: rows=%llu cols=%llu: matrix too large", fn, (unsigned long long)rows,
                (unsigned long long)cols);
    CLV_REQUIRE(rows / 32 <= 0x7FFFFFFFull && cols / 64 <= 0x7FFFFFFFull, "%s: rows=%llu cols=%llu: matrix too large", fn, (unsigned long long)rows,
                (unsigned long long)cols);
    const uint64_t nin = transposed ? rows : cols, nout = transposed ? cols : rows;
    std::vector<ClvRange> rg;
    rg.reserve(6);
    rg.push_back(clv_range(A, rows * (cols / 2), false, ~0ull, "A"));
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
static int m4f32_t_launch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, float *r, hipStream_t st, FUSE... fuse)
{
    const dim3 grid((unsigned)((cols + M4FT_COLS - 1) / M4FT_COLS)), block(M4FT_THREADS);
    if (m4f32_streaming(rows, cols))
        hipLaunchKernelGGL((k_m4_mvm_f32_t<M4FT_U, true, FUSE...>), grid, block, 0, st, (const uint8_t *)A, sA, rows, cols, x, r, fuse...);
    else
        hipLaunchKernelGGL((k_m4_mvm_f32_t<M4FT_U, false, FUSE...>), grid, block, 0, st, (const uint8_t *)A, sA, rows, cols, x, r, fuse...);
    CLV_LAUNCH_CHECK();
    return CLV_OK;
}

extern "C" int clm4_mvm_f32_scale_and_add(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, const float *u, float a,
                                          float *t, float *r2, void *stream)
{
    const int rc = m4f32_check_args("clm4_mvm_f32_scale_and_add", A, sA, rows, cols, x, false, true, u, t, r2);
    if (rc) return rc > 0 ? CLV_OK : rc;
    return clv_internal_m4_mvm_f32_fused(A, sA, rows, cols, x, t, M4F32Fuse{u, a, r2}, as_stream(stream));
}

extern "C" int clm4_mvm_f32_transposed(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, float *r, void *stream)
{
    const int rc = m4f32_check_args("clm4_mvm_f32_transposed", A, sA, rows, cols, x, true, false, nullptr, nullptr, r);
    if (rc) return rc > 0 ? CLV_OK : rc;
    return m4f32_t_launch(A, sA, rows, cols, x, r, as_stream(stream));
}

extern "C" int clm4_mvm_f32_transposed_scale_and_add(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, const float *u,
                                                     float a, float *t, float *r2, void *stream)
{
    const int rc = m4f32_check_args("clm4_mvm_f32_transposed_scale_and_add", A, sA, rows, cols, x, true, true, u, t, r2);
    if (rc) return rc > 0 ? CLV_OK : rc;
    return m4f32_t_launch(A, sA, rows, cols, x, t, as_stream(stream), M4F32Fuse{u, a, r2});
}

// Q_IHT / Q_GD (test/performance/01_measure.h:923-946, 999-1021) over CloverMatrix4 with CloverVector32 vectors, the driver of clm_f32_iht
// (fp32.hip) with 4-bit matrices: one call enqueues all iterations, one fused launch per product plus the threshold, nothing copied back.
// PhiT == NULL: the one-matrix form, whose gradient step takes Phi' t2 straight from Phi.
static int m4f32_iht(const char *fn, const int8_t *Phi, const float *sPhi, const int8_t *PhiT, const float *sPhiT, bool one_matrix, uint64_t m,
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
    CLV_REQUIRE(M4F32_ALIGNED16(Phi) && M4F32_ALIGNED16(PhiT), "%s: the matrices must be 16-byte aligned", fn);
    CLV_REQUIRE(M4F32_ALIGNED16(x), "%s: x must be 16-byte aligned", fn);
    CLV_REQUIRE(M4F32_ALIGNED16(t2), "%s: t2 must be 16-byte aligned", fn);
    CLV_REQUIRE(M4F32_ALIGNED4(sPhi) && M4F32_ALIGNED4(sPhiT) && M4F32_ALIGNED4(y) && M4F32_ALIGNED4(t1) && M4F32_ALIGNED4(t3),
                "%s: the scales, y, t1 and t3 must be 4-byte aligned", fn);
    CLV_REQUIRE(!n || m <= 0xFFFFFFFFFFFFull / n, "%s: m=%llu n=%llu: matrix too large", fn, (unsigned long long)m, (unsigned long long)n);
    {
        const uint64_t grid = (m / 64) * (n / 64) * 4;
        std::vector<ClvRange> rg;
        rg.reserve(9);
        rg.push_back(clv_range(Phi, m * (n / 2), false, ~0ull, "Phi"));
        rg.push_back(clv_range(sPhi, grid, false, ~0ull, "sPhi"));
        if (!one_matrix) {
            rg.push_back(clv_range(PhiT, m * (n / 2), false, ~0ull, "PhiT"));
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
        rc = clm4_mvm_f32_scale_and_add(Phi, sPhi, m, n, x, y, -1.0f, t1, t2, stream);                     // t1 = Phi x; t2 = y - t1
        if (!rc)                                                                                           // t3 = Phi' t2; x += mu t3
            rc = one_matrix ? clm4_mvm_f32_transposed_scale_and_add(Phi, sPhi, m, n, t2, x, mu, t3, x, stream)
                            : clm4_mvm_f32_scale_and_add(PhiT, sPhiT, n, m, t2, x, mu, t3, x, stream);
        if (!rc && threshold)                                                          // keep the K largest (2: the reference's survivor order)
            rc = clv_f32_threshold_mode(x, x_len, n, K, threshold == 2 ? CLV_THRESHOLD_REFERENCE : CLV_THRESHOLD_FAST, nullptr, stream);
    }
    return rc;
}

extern "C" int clm4_iht_f32(const int8_t *Phi, const float *sPhi, const int8_t *PhiT, const float *sPhiT, uint64_t m, uint64_t n, float *x,
                            uint64_t x_len, const float *y, float *t1, float *t2, float *t3, uint64_t iterations, uint64_t K, float mu, int threshold,
                            void *stream)
{
    return m4f32_iht("clm4_iht_f32", Phi, sPhi, PhiT, sPhiT, false, m, n, x, x_len, y, t1, t2, t3, iterations, K, mu, threshold, stream);
}

extern "C" int clm4_iht_f32_one_matrix(const int8_t *Phi, const float *sPhi, uint64_t m, uint64_t n, float *x, uint64_t x_len, const float *y, float *t1,
                                       float *t2, float *t3, uint64_t iterations, uint64_t K, float mu, int threshold, void *stream)
{
    return m4f32_iht("clm4_iht_f32_one_matrix", Phi, sPhi, nullptr, nullptr, true, m, n, x, x_len, y, t1, t2, t3, iterations, K, mu, threshold, stream);
}
