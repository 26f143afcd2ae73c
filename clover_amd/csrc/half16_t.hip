// half16_t.hip -- the transposed half-precision mvm: r = f16(A' x) for a CloverMatrix16 A and a CloverVector16 (or fp32) x straight from
// A's own bytes, no stored transpose (include/clover_hip_f16_t.h).
//
// Contract: bit for bit what clm_f16_transpose(A -> At) followed by clm_f16_mvm / clm_f16_mvm_f32 / clm_f16_mvm_scale_and_add on At gives.
// Output column j is row j of A' under the definition of k_f16_mvm (half16.hip): 32 sequential fp32 fma chains, row i of A on chain
// i mod 32 in increasing i, each from +0.0f, one step acc = fmaf(f32(x[i]), f32(A[i][j]), acc); then the tree of f16_chain_tree --
// s[l] = (acc[l] + acc[8 + l]) + (acc[16 + l] + acc[24 + l]), t[k] = s[k + 4] + s[k], (t0 + t2) + (t1 + t3) -- and the epilogues of
// half16_device.h.  tests/half16_t_restate.c states the same walk on the CPU.
//
// Mapping: a chain is ordered over ALL rows, so rows are never split between workgroups; the 32 chains of a column are independent until
// the tree, so they are spread over lanes, and each (column, chain) stays in ONE register of ONE lane for the whole walk.
//   workgroup = a strip of F16T_COLS columns, 256 threads; it walks all rows.  ceil(cols / F16T_COLS) workgroups; a strip wider than 128
//               columns leaves the last workgroup partial: its lanes beyond `cols` load the strip's first column group and store nothing;
//   thread    = (cg = tid % CG, L = tid / CG) with CG = F16T_COLS / 8 column groups of 8 halves (one 16-byte load) and 256 / CG chain
//               groups of CPL = 32 / (256 / CG) chains: rows 32 b + CPL L + i of block b, i < CPL.  8 CPL fp32 accumulators;
//   pipeline  = F16T_U 32-row blocks of loads per register set, two sets that take turns: the set ahead is loaded -- unconditionally,
//               clamped to the last block (f16t_group) -- before the arithmetic of the current one;
//   x         = staged per F16T_CHUNK rows in LDS, WIDENED to fp32 (exact; the fp32-vector form copies): all loads first, then the LDS
//               writes; a lane reads its CPL values of a block as one broadcast read;
//   epilogue  = the 32 chain ends of every column through LDS to one lane: the tree, the conversion and the fused epilogue
//               (f16_fuse_store).  u[j] is fetched before the walk, so r may be u.
#include "half16_device.h"
#include "clover_hip_f16_t.h"

#ifndef F16T_COLS
#define F16T_COLS 128       // columns per workgroup (the widths measured: DESIGN.md 3)
#endif
#ifndef F16T_U
#define F16T_U 4            // 32-row blocks of matrix loads per register set = blocks issued ahead of the arithmetic
#endif
#define F16T_CHUNK 4096u    // rows of x staged in LDS per pass
#define F16T_CG (F16T_COLS / 8)              // column groups = lanes per row
#define F16T_CPL (32 / (256 / F16T_CG))      // chains (rows of a 32-row block) per lane

static_assert(F16T_COLS == 64 || F16T_COLS == 128 || F16T_COLS == 256, "the lane map is (F16T_COLS / 8 column groups) x (256 / that many chain groups); one lane per column in the epilogue");
static_assert((F16T_CHUNK / 32) % (2 * F16T_U) == 0 && F16T_CHUNK % (8 * 256) == 0, "a chunk is whole pairs of load groups and whole rounds of 256 staging threads");

// stage x of the chunk that starts at row r0 as fp32: all loads first (one round trip), then the LDS writes
template <bool XF32>
__device__ __forceinline__ void f16t_stage(float *xs, const void *__restrict__ x, uint64_t rows, uint64_t r0, int tid)
{
    const uint32_t ch = (uint32_t)((rows - r0) < F16T_CHUNK ? (rows - r0) : F16T_CHUNK);
    if (r0) __syncthreads();                             // the previous chunk's x has been consumed
    if (XF32) {
        constexpr int NX = F16T_CHUNK / 4 / 256;         // 16-byte pieces of x per thread
        const f32x4 *xg = reinterpret_cast<const f32x4 *>(x) + r0 / 4;
        const uint32_t nx = ch / 4;
        f32x4 xr[NX];
#pragma unroll
        for (int j = 0; j < NX; j++) { const uint32_t i = tid + 256 * j; xr[j] = xg[i < nx ? i : 0]; }
#pragma unroll
        for (int j = 0; j < NX; j++) { const uint32_t i = tid + 256 * j; if (i < nx) reinterpret_cast<f32x4 *>(xs)[i] = xr[j]; }
    } else {
        constexpr int NX = F16T_CHUNK / 8 / 256;
        const h16x8 *xg = reinterpret_cast<const h16x8 *>(x) + r0 / 8;
        const uint32_t nx = ch / 8;
        h16x8 xr[NX];
#pragma unroll
        for (int j = 0; j < NX; j++) { const uint32_t i = tid + 256 * j; xr[j] = xg[i < nx ? i : 0]; }
#pragma unroll
        for (int j = 0; j < NX; j++) {
            const uint32_t i = tid + 256 * j;
            if (i < nx) {
                reinterpret_cast<f32x4 *>(xs)[2 * i] = f32x4{(float)xr[j][0], (float)xr[j][1], (float)xr[j][2], (float)xr[j][3]};
                reinterpret_cast<f32x4 *>(xs)[2 * i + 1] = f32x4{(float)xr[j][4], (float)xr[j][5], (float)xr[j][6], (float)xr[j][7]};
            }
        }
    }
    __syncthreads();
}

// the loads of group g (U blocks, CPL rows each) of the lane whose first row of block 0 and column group Ap points at; blocks beyond the
// last one read the last one again
template <int U, bool NT>
__device__ __forceinline__ void f16t_load(const h16x8 *__restrict__ Ap, uint64_t stride, uint32_t g, uint32_t nblk, h16x8 (&a)[U][F16T_CPL])
{
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint32_t b = g * U + u, bc = b < nblk ? b : nblk - 1;
#pragma unroll
        for (int i = 0; i < F16T_CPL; i++) a[u][i] = ld_stream<NT>(Ap + ((uint64_t)bc * 32 + i) * stride);
    }
}

// the chain steps of one block: xb = the lane's CPL values of x in LDS
__device__ __forceinline__ void f16t_block(const h16x8 (&a)[F16T_CPL], const float *xb, float (&acc)[F16T_CPL][8])
{
    float xv[F16T_CPL];
#pragma unroll
    for (int i = 0; i < F16T_CPL; i++) xv[i] = xb[i];
#pragma unroll
    for (int i = 0; i < F16T_CPL; i++)
#pragma unroll
        for (int e = 0; e < 8; e++) acc[i][e] = __builtin_fmaf(xv[i], (float)a[i][e], acc[i][e]);
}

// group g of the walk from `cur` (loaded a group ago) while the next group's loads go to `nxt` -- issued UNCONDITIONALLY (beyond the last
// block: the last block again), so that the wait for `cur` lets them stay in flight (m8t_group, matrix8_t.hip)
template <int U, bool NT>
__device__ __forceinline__ void f16t_group(const h16x8 (&cur)[U][F16T_CPL], h16x8 (&nxt)[U][F16T_CPL], const h16x8 *__restrict__ Ap, uint64_t stride,
                                           uint32_t g, uint32_t nblk, const float *xl, float (&acc)[F16T_CPL][8])
{
    constexpr uint32_t CB = F16T_CHUNK / 32;             // blocks per chunk
    f16t_load<U, NT>(Ap, stride, g + 1, nblk, nxt);
    const uint32_t b0 = g * U, lb = b0 % CB;             // a group never straddles a chunk
    if (nblk - b0 >= (uint32_t)U) {
#pragma unroll
        for (int u = 0; u < U; u++) f16t_block(cur[u], xl + 32 * (lb + u), acc);
    } else {
#pragma unroll
        for (int u = 0; u < U; u++)
            if (b0 + u < nblk) f16t_block(cur[u], xl + 32 * (lb + u), acc);
    }
}

// FUSE... = nothing or one F16Fuse, as k_f16_mvm (half16.hip).  r (t of the fused ABI) may be NULL under FUSE; fuse.r2 may be fuse.u
template <int U, bool NT, bool XF32, typename... FUSE>
__global__ __launch_bounds__(256) void k_f16_mvm_t(const uint16_t *__restrict__ A, uint64_t rows, uint64_t cols, const void *__restrict__ x,
                                                   void *__restrict__ r, FUSE... fuse)
{
    __shared__ __attribute__((aligned(16))) float xs[F16T_CHUNK];
    __shared__ __attribute__((aligned(16))) float part[32 * F16T_COLS];            // epilogue: part[chain][column]
    constexpr bool FUSED = sizeof...(FUSE) != 0;
    constexpr bool PARTIAL = F16T_COLS > 128;                                      // cols % 128 == 0 makes narrower strips whole

    const int tid = threadIdx.x, cg = tid % F16T_CG, L = tid / F16T_CG;
    const uint64_t strip0 = (uint64_t)blockIdx.x * F16T_COLS;
    // the epilogue's lane of column strip0 + tid: its element of u, fetched now so that the epilogue does not wait for it (and r may be u)
    const uint64_t col = strip0 + tid;
    const bool owner = tid < F16T_COLS && (!PARTIAL || col < cols);
    uint16_t fuse_u = 0;
    if (FUSED && owner) fuse_u = f16_fuse_load_u(col, fuse...);

    const uint64_t stride = cols / 8;                                              // 16-byte groups per row
    uint64_t c0 = strip0 + 8 * (uint64_t)cg;
    if (PARTIAL && c0 >= cols) c0 = strip0;                                        // loads stay inside the matrix; nothing of it is stored
    const h16x8 *Ap = reinterpret_cast<const h16x8 *>(A) + c0 / 8 + (uint64_t)(F16T_CPL * L) * stride;
    const float *xl = xs + F16T_CPL * L;

    float acc[F16T_CPL][8];
#pragma unroll
    for (int i = 0; i < F16T_CPL; i++)
#pragma unroll
        for (int e = 0; e < 8; e++) acc[i][e] = 0.0f;

    // the walk over all rows in groups of U blocks; a chunk is a whole, even number of groups, so x is re-staged in front of an even
    // group.  Two register sets take turns: no copies, and the loads of the group ahead stay in flight across the staging
    constexpr uint32_t CG = F16T_CHUNK / 32 / U;
    const uint32_t nblk = (uint32_t)(rows / 32), ngroups = (nblk + U - 1) / U;
    h16x8 a[U][F16T_CPL], b[U][F16T_CPL];
    f16t_load<U, NT>(Ap, stride, 0, nblk, a);
    uint32_t g = 0;
    for (; g + 1 < ngroups; g += 2) {
        if (g % CG == 0) f16t_stage<XF32>(xs, x, rows, (uint64_t)g * U * 32, tid);
        f16t_group<U, NT>(a, b, Ap, stride, g, nblk, xl, acc);
        f16t_group<U, NT>(b, a, Ap, stride, g + 1, nblk, xl, acc);
    }
    if (g < ngroups) {
        if (g % CG == 0) f16t_stage<XF32>(xs, x, rows, (uint64_t)g * U * 32, tid);
        f16t_group<U, NT>(a, b, Ap, stride, g, nblk, xl, acc);
    }

    // the 32 chain ends of every column meet in the column's lane
#pragma unroll
    for (int i = 0; i < F16T_CPL; i++) {
        f32x4 *p = reinterpret_cast<f32x4 *>(part + (F16T_CPL * L + i) * F16T_COLS + 8 * cg);
        p[0] = f32x4{acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
        p[1] = f32x4{acc[i][4], acc[i][5], acc[i][6], acc[i][7]};
    }
    __syncthreads();
    if (owner) {
        float s[8];
#pragma unroll
        for (int l = 0; l < 8; l++)
            s[l] = (part[l * F16T_COLS + tid] + part[(8 + l) * F16T_COLS + tid]) + (part[(16 + l) * F16T_COLS + tid] + part[(24 + l) * F16T_COLS + tid]);
        const float t0 = s[4] + s[0], t1 = s[5] + s[1], t2 = s[6] + s[2], t3 = s[7] + s[3];
        const float d = (t0 + t2) + (t1 + t3);
        if (FUSED) f16_fuse_store(r, col, d, fuse_u, fuse...);
        else if (XF32) reinterpret_cast<float *>(r)[col] = d;
        else reinterpret_cast<uint16_t *>(r)[col] = f16_bits(d);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
// every check of the three products, before any device work.  rb = bytes of an element of r; u == t == NULL in the plain calls.
// Returns CLV_OK, CLV_ERR_INVALID, or 1: valid and nothing to do
static int f16t_check_args(const char *fn, const uint16_t *A, uint64_t rows, uint64_t cols, const void *x, bool xf32, bool fused, const uint16_t *u,
                           const uint16_t *t, const void *r)
{
    const uint64_t eb = xf32 ? 4 : 2;
    CLV_REQUIRE(A && x && r && (!fused || u), "%s: null pointer", fn);
    CLV_REQUIRE(rows % 128 == 0 && cols % 128 == 0, "%s: rows=%llu cols=%llu must be multiples of 128", fn, (unsigned long long)rows,
                (unsigned long long)cols);
    CLV_REQUIRE(F16_ALIGNED(A) && F16_ALIGNED(x), "%s: the matrix and x must be 16-byte aligned", fn);
    CLV_REQUIRE(((uintptr_t)r & (eb - 1)) == 0 && ((uintptr_t)u & 1u) == 0 && ((uintptr_t)t & 1u) == 0, "%s: %s must be %llu-byte aligned", fn,
                fused ? "u, t and r" : "r", (unsigned long long)eb);
    CLV_REQUIRE(!cols || rows <= 0xFFFFFFFFFFFFull / cols, "%s: matrix too large", fn);
    CLV_REQUIRE(rows / 32 <= 0x7FFFFFFFull && (cols + F16T_COLS - 1) / F16T_COLS <= 0x7FFFFFFFull, "%s: matrix too large", fn);
    std::vector<ClvRange> rg;
    rg.reserve(5);
    rg.push_back(clv_range(A, rows * cols * 2, false, ~0ull, "A"));
    rg.push_back(clv_range(x, rows * eb, false, 0, "x"));
    rg.push_back(clv_range(r, cols * eb, true, 0, "r"));
    // the in-place form r == u: the result IS the input, only the lane that owns a column touches it in either
    if (fused && (const void *)u != r) rg.push_back(clv_range(u, cols * 2, false, 0, "u"));
    if (t) rg.push_back(clv_range(t, cols * 2, true, 0, "t"));
    int rc = clv_internal_check_ranges(fn, rg);
    if (rc) return rc;
    return rows && cols ? CLV_OK : 1;
}

template <bool XF32, typename... FUSE>
static int f16t_launch(const uint16_t *A, uint64_t rows, uint64_t cols, const void *x, void *r, hipStream_t st, FUSE... fuse)
{
    const dim3 grid((unsigned)((cols + F16T_COLS - 1) / F16T_COLS)), block(256);
    // streaming (nt) loads once the matrix cannot live in the 256 MiB Infinity Cache: the rule of f16_mvm() (half16.hip)
    if (F16_STREAMING(rows * cols * 2)) hipLaunchKernelGGL((k_f16_mvm_t<F16T_U, true, XF32, FUSE...>), grid, block, 0, st, A, rows, cols, x, r, fuse...);
    else hipLaunchKernelGGL((k_f16_mvm_t<F16T_U, false, XF32, FUSE...>), grid, block, 0, st, A, rows, cols, x, r, fuse...);
    CLV_LAUNCH_CHECK();
    return CLV_OK;
}

extern "C" int clm_f16_mvm_transposed(const uint16_t *A, uint64_t rows, uint64_t cols, const uint16_t *x, uint16_t *r, void *stream)
{
    const int rc = f16t_check_args("clm_f16_mvm_transposed", A, rows, cols, x, false, false, nullptr, nullptr, r);
    if (rc) return rc > 0 ? CLV_OK : rc;
    return f16t_launch<false>(A, rows, cols, x, r, as_stream(stream));
}

extern "C" int clm_f16_mvm_f32_transposed(const uint16_t *A, uint64_t rows, uint64_t cols, const float *x, float *r, void *stream)
{
    const int rc = f16t_check_args("clm_f16_mvm_f32_transposed", A, rows, cols, x, true, false, nullptr, nullptr, r);
    if (rc) return rc > 0 ? CLV_OK : rc;
    return f16t_launch<true>(A, rows, cols, x, r, as_stream(stream));
}

extern "C" int clm_f16_mvm_transposed_scale_and_add(const uint16_t *A, uint64_t rows, uint64_t cols, const uint16_t *x, const uint16_t *u, float a,
                                                    uint16_t *t, uint16_t *r, void *stream)
{
    const int rc = f16t_check_args("clm_f16_mvm_transposed_scale_and_add", A, rows, cols, x, false, true, u, t, r);
    if (rc) return rc > 0 ? CLV_OK : rc;
    const F16Fuse fuse = {u, a, r};
    return f16t_launch<false>(A, rows, cols, (const void *)x, (void *)t, as_stream(stream), fuse);
}

// clm_f16_iht (half16.hip) with ONE matrix: Phi' t2 comes straight from Phi, so no PhiT exists.  The same number of launches per
// iteration, and bit-identical to clm_f16_iht called with PhiT = transpose(Phi): x and t1 .. t3.
#define F16_IHT1 "clm_f16_iht_one_matrix"
extern "C" int clm_f16_iht_one_matrix(const uint16_t *Phi, uint64_t m, uint64_t n, uint16_t *x, uint64_t x_len, const uint16_t *y, uint16_t *t1,
                                      uint16_t *t2, uint16_t *t3, uint64_t iterations, uint64_t K, float mu, int threshold, void *stream)
{
    CLV_REQUIRE(Phi && x && y && t1 && t2 && t3, F16_IHT1 ": null pointer");
    CLV_REQUIRE(m % 128 == 0 && n % 128 == 0 && x_len <= n, F16_IHT1 ": m=%llu n=%llu x_len=%llu", (unsigned long long)m, (unsigned long long)n,
                (unsigned long long)x_len);
    CLV_REQUIRE(threshold >= 0 && threshold <= 2, F16_IHT1 ": unknown threshold %d", threshold);
    CLV_REQUIRE(F16_ALIGNED(Phi) && F16_ALIGNED(x) && F16_ALIGNED(t2), F16_IHT1 ": the matrix, x and t2 must be 16-byte aligned");
    CLV_REQUIRE((((uintptr_t)y | (uintptr_t)t1 | (uintptr_t)t3) & 1u) == 0, F16_IHT1 ": y, t1 and t3 must be 2-byte aligned");
    CLV_REQUIRE(!n || m <= 0xFFFFFFFFFFFFull / n, F16_IHT1 ": matrix too large");
    {
        std::vector<ClvRange> rg;
        rg.reserve(6);
        rg.push_back(clv_range(Phi, m * n * 2, false, ~0ull, "Phi"));
        rg.push_back(clv_range(y, m * 2, false, 0, "y"));
        rg.push_back(clv_range(x, n * 2, true, 0, "x"));
        rg.push_back(clv_range(t1, m * 2, true, 0, "t1"));
        rg.push_back(clv_range(t2, m * 2, true, 0, "t2"));
        rg.push_back(clv_range(t3, n * 2, true, 0, "t3"));
        int rc = clv_internal_check_ranges(F16_IHT1, rg);
        if (rc) return rc;
    }
    int rc = clv_internal_f16_clear(x, n, as_stream(stream));                                            // x.clear()
    for (uint64_t it = 0; !rc && it < iterations; it++) {
        rc = clm_f16_mvm_scale_and_add(Phi, m, n, x, y, -1.0f, t1, t2, stream);                          // t1 = Phi x; t2 = y - t1
        if (!rc) rc = clm_f16_mvm_transposed_scale_and_add(Phi, m, n, t2, x, mu, t3, x, stream);         // t3 = Phi' t2; x += mu t3
        if (!rc && threshold)                                                          // keep the K largest (2: the reference's survivor order)
            rc = clv_f16_threshold_mode(x, x_len, n, K, threshold == 2 ? CLV_THRESHOLD_REFERENCE : CLV_THRESHOLD_FAST, nullptr, stream);
    }
    return rc;
}
#undef F16_IHT1
