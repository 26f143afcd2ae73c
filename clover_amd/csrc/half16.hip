// half16.hip -- CloverVector16 / CloverMatrix16 on gfx950: the half-precision containers (raw IEEE binary16 bit patterns, no scales).
//
// quantize = fp32 -> f16 round-to-nearest-even with subnormal results kept (vcvtps2ph imm 0), restore = the exact widening,
// scaleAndAdd = f16(fma(f32(v), s, f32(u))), dot / mvm = 32 sequential fp32 fma chains (element j -> chain j mod 32) and the
// reference's fixed tree.  tests/half16_restate.c states the same orders on the CPU.
//
// The conversions are v_cvt_f16_f32 / v_cvt_f32_f16 under the default mode (RNE, f16 denormals on).  A chain step is "widen both
// operands exactly, one fp32 fma"; hipcc keeps the widening apart from the fma (it folds it into v_fma_mix_f32 only with fp32
// denormals flushed) and pairs the fmas into v_pk_fma_f32, each half still one fused, singly rounded fma.  The packed f16 dot
// instructions round differently and are not used.
#include "half16_device.h"      // the conversions, the 32 chains and their tree, the fused epilogue: shared with half16_batch.hip

// ================================================================================================
// streaming vector kernels: lane = 8 consecutive elements (16 bytes of f16), F16_VU groups in flight per lane
// ================================================================================================
#define F16_VU 4
#define F16_VEC_GROUPS_PER_WG (256 * F16_VU)

// CloverVector16::quantize (CloverVector16.h:212-243), CloverMatrix16::quantize (CloverMatrix16.h:383-410)
template <bool NT>
__global__ __launch_bounds__(256) void k_f16_quantize(const f32x4 *__restrict__ x, h16x8 *__restrict__ h, uint64_t ngroups)
{
    const uint64_t g0 = (uint64_t)blockIdx.x * F16_VEC_GROUPS_PER_WG + threadIdx.x;
    f32x4 lo[F16_VU], hi[F16_VU];
#pragma unroll
    for (int u = 0; u < F16_VU; u++) {
        const uint64_t g = g0 + 256 * u, gc = g < ngroups ? g : 0;
        lo[u] = ld_stream<NT>(&x[2 * gc]);
        hi[u] = ld_stream<NT>(&x[2 * gc + 1]);
    }
#pragma unroll
    for (int u = 0; u < F16_VU; u++) {
        const uint64_t g = g0 + 256 * u;
        const h16x8 o = {(_Float16)lo[u].x, (_Float16)lo[u].y, (_Float16)lo[u].z, (_Float16)lo[u].w,
                         (_Float16)hi[u].x, (_Float16)hi[u].y, (_Float16)hi[u].z, (_Float16)hi[u].w};
        if (g < ngroups) st_stream<NT>(o, &h[g]);
    }
}

// CloverVector16::restore (CloverVector16.h:279-307)
template <bool NT>
__global__ __launch_bounds__(256) void k_f16_restore(const h16x8 *__restrict__ h, f32x4 *__restrict__ x, uint64_t ngroups)
{
    const uint64_t g0 = (uint64_t)blockIdx.x * F16_VEC_GROUPS_PER_WG + threadIdx.x;
    h16x8 v[F16_VU];
#pragma unroll
    for (int u = 0; u < F16_VU; u++) {
        const uint64_t g = g0 + 256 * u;
        v[u] = ld_stream<NT>(&h[g < ngroups ? g : 0]);
    }
#pragma unroll
    for (int u = 0; u < F16_VU; u++) {
        const uint64_t g = g0 + 256 * u;
        if (g < ngroups) {
            st_stream<NT>(f32x4{(float)v[u][0], (float)v[u][1], (float)v[u][2], (float)v[u][3]}, &x[2 * g]);
            st_stream<NT>(f32x4{(float)v[u][4], (float)v[u][5], (float)v[u][6], (float)v[u][7]}, &x[2 * g + 1]);
        }
    }
}

// CloverVector16::scaleAndAdd (CloverVector16.h:309-386): r = f16(fma(f32(v), s, f32(u))); r may be u (a lane reads its own 16 bytes
// before it writes them)
template <bool NT>
__global__ __launch_bounds__(256) void k_f16_scale_and_add(const h16x8 *u, const h16x8 *__restrict__ v, float s, h16x8 *r, uint64_t ngroups)
{
    const uint64_t g0 = (uint64_t)blockIdx.x * F16_VEC_GROUPS_PER_WG + threadIdx.x;
    h16x8 a[F16_VU], b[F16_VU];
#pragma unroll
    for (int k = 0; k < F16_VU; k++) {
        const uint64_t g = g0 + 256 * k, gc = g < ngroups ? g : 0;
        a[k] = ld_stream<NT>(&u[gc]);
        b[k] = ld_stream<NT>(&v[gc]);
    }
#pragma unroll
    for (int k = 0; k < F16_VU; k++) {
        const uint64_t g = g0 + 256 * k;
        h16x8 o;
#pragma unroll
        for (int e = 0; e < 8; e++) o[e] = (_Float16)__builtin_fmaf((float)b[k][e], s, (float)a[k][e]);
        if (g < ngroups) st_stream<NT>(o, &r[g]);
    }
}

// CloverVector16::clear() on the stream (the first step of clm_f16_iht): a kernel, not a memset, so that a captured call replays it as one
// more kernel node in stream order
__global__ __launch_bounds__(256) void k_f16_clear(u32x4 *__restrict__ h, uint64_t ngroups)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += stride) h[g] = u32x4{0u, 0u, 0u, 0u};
}

// ================================================================================================
// mvm  (CloverMatrix16.h:230-308 f16 vectors, :321-381 fp32 vectors; mvm_parallel :133-228 has the same order per row)
// ================================================================================================
// Workgroup = 16 * WAVES rows, four lanes per row.  x is staged in LDS once per workgroup, 16 KiB at a time (8192 f16 or 4096 fp32
// elements); the matrix is read 16 bytes per lane, F16_MVM_U requests in flight (512 contiguous bytes of every row).  Rows beyond
// `rows` (a workgroup's tail) re-read the last row and store nothing.
#define F16_MVM_U 8
#define F16_X_BYTES 16384

template <int U, bool NT, bool XF32>
__device__ __forceinline__ void f16_mvm_steps(const h16x8 *__restrict__ Ap, const char *xs, int p, uint32_t t0, float acc[8])
{
    h16x8 a[U];
#pragma unroll
    for (int u = 0; u < U; u++) a[u] = ld_stream<NT>(&Ap[4 * (t0 + u) + p]);
#pragma unroll
    for (int u = 0; u < U; u++) {
        if (XF32) {
            const f32x4 *x4 = reinterpret_cast<const f32x4 *>(xs) + 8 * (t0 + u) + 2 * p;
            f16_chain_step(a[u], x4[0], x4[1], acc);
        } else {
            f16_chain_step(a[u], reinterpret_cast<const h16x8 *>(xs)[4 * (t0 + u) + p], acc);
        }
    }
}

// F16Fuse, the fused epilogue of clm_f16_mvm_scale_and_add (k_f16_mvm_saa below): half16_device.h
// fuse.r2 may be fuse.u: the lane that writes r2[row] has read u[row] before the loop.  r (t of the ABI) is apart from x, u and r2.
template <int WAVES, bool NT, bool XF32, typename... FUSE>
__global__ __launch_bounds__(64 * WAVES) void k_f16_mvm(const uint16_t *__restrict__ A, uint64_t rows, uint64_t cols, const void *__restrict__ x,
                                                        void *__restrict__ r, FUSE... fuse)
{
    __shared__ __attribute__((aligned(16))) char xs[F16_X_BYTES];
    constexpr bool FUSED = sizeof...(FUSE) != 0;
    constexpr int THREADS = 64 * WAVES;
    constexpr int XB = XF32 ? 4 : 2;
    constexpr uint32_t CH = F16_X_BYTES / XB;                 // elements of x per chunk
    constexpr int NX = F16_X_BYTES / 16 / THREADS;            // 16-byte pieces per thread and chunk
    const int tid = threadIdx.x, p = tid & 3, rho = tid >> 2;
    const uint64_t row = (uint64_t)blockIdx.x * (16 * WAVES) + rho;
    const h16x8 *Arow = reinterpret_cast<const h16x8 *>(A + (row < rows ? row : rows - 1) * cols);
    float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    uint16_t fuse_u = 0;
    if (FUSED && p == 0 && row < rows) fuse_u = f16_fuse_load_u(row, fuse...);      // ahead of the streaming loop: the epilogue waits on nothing

    for (uint64_t c0 = 0; c0 < cols; c0 += CH) {
        const uint32_t cw = (uint32_t)((cols - c0) < CH ? (cols - c0) : CH);
        if (c0) __syncthreads();
        {   // all loads first (one round trip), then the LDS writes
            const u32x4 *xg = reinterpret_cast<const u32x4 *>(reinterpret_cast<const char *>(x) + c0 * XB);
            const uint32_t n16 = cw * XB / 16;
            u32x4 xr[NX];
#pragma unroll
            for (int k = 0; k < NX; k++) { const uint32_t i = tid + THREADS * k; xr[k] = xg[i < n16 ? i : 0]; }
#pragma unroll
            for (int k = 0; k < NX; k++) { const uint32_t i = tid + THREADS * k; if (i < n16) reinterpret_cast<u32x4 *>(xs)[i] = xr[k]; }
        }
        __syncthreads();
        const h16x8 *Ap = Arow + c0 / 8;
        const uint32_t nsteps = cw / 32;
        uint32_t t = 0;
        for (; t + F16_MVM_U <= nsteps; t += F16_MVM_U) f16_mvm_steps<F16_MVM_U, NT, XF32>(Ap, xs, p, t, acc);
        for (; t < nsteps; t++) f16_mvm_steps<1, NT, XF32>(Ap, xs, p, t, acc);
    }
    const float d = f16_chain_tree(acc);
    if (p == 0 && row < rows) {
        if (FUSED) f16_fuse_store(r, row, d, fuse_u, fuse...);
        else if (XF32) reinterpret_cast<float *>(r)[row] = d;
        else reinterpret_cast<uint16_t *>(r)[row] = f16_bits(d);         // _mm256_cvtps_ph(.., 0) of the row block (:302-306)
    }
}
#define k_f16_mvm_saa(WAVES, NT) k_f16_mvm<WAVES, NT, false, F16Fuse>

// ================================================================================================
// dot  (CloverVector16.h:473-530)
// ================================================================================================
// EXACT: the 32 chains are sequential by definition (n / 32 dependent fmas each).  One workgroup: all 256 threads move u and v through
// LDS (8192 elements of each per round, requested while the previous round is being consumed), and one quad of lanes -- lane p =
// accumulator p, as in mvm -- walks the chains from LDS.
#define F16_DOT_CH 8192u
__global__ __launch_bounds__(256) void k_f16_dot_exact(const u32x4 *__restrict__ u, const u32x4 *__restrict__ v, uint64_t n, float *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) u32x4 us[F16_DOT_CH / 8], vs[F16_DOT_CH / 8];
    constexpr int NX = F16_DOT_CH / 8 / 256;                  // 16-byte pieces per thread, operand and round
    const int tid = threadIdx.x;
    float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    u32x4 ur[NX], vr[NX];
    const uint64_t n16 = n / 8;
#pragma unroll
    for (int k = 0; k < NX; k++) {
        const uint64_t i = (uint64_t)tid + 256 * k, ic = i < n16 ? i : 0;
        ur[k] = u[ic];
        vr[k] = v[ic];
    }
    for (uint64_t c0 = 0; c0 < n; c0 += F16_DOT_CH) {
        const uint32_t cw = (uint32_t)((n - c0) < F16_DOT_CH ? (n - c0) : F16_DOT_CH);
        if (c0) __syncthreads();                              // the quad has finished with the previous round
#pragma unroll
        for (int k = 0; k < NX; k++) {
            us[tid + 256 * k] = ur[k];
            vs[tid + 256 * k] = vr[k];
        }
        // the next round's loads are in flight while the quad works
        const uint64_t nb = (c0 + F16_DOT_CH) / 8;
#pragma unroll
        for (int k = 0; k < NX; k++) {
            const uint64_t i = nb + tid + 256 * k, ic = i < n16 ? i : 0;
            ur[k] = u[ic];
            vr[k] = v[ic];
        }
        __syncthreads();
        if (tid < 4) {
            const h16x8 *uh = reinterpret_cast<const h16x8 *>(us), *vh = reinterpret_cast<const h16x8 *>(vs);
            const uint32_t nsteps = cw / 32;
#pragma unroll 4
            for (uint32_t t = 0; t < nsteps; t++) f16_chain_step(uh[4 * t + tid], vh[4 * t + tid], acc);
        }
    }
    const float d = f16_chain_tree(acc);                      // wave 0 only matters; the shuffles stay inside the quad
    if (tid == 0) *out = d;
}

// FAST: one launch; a lane keeps 8 fp32 partial sums over its 16-byte groups (the same exact products, another summation order), fixed
// trees inside the lane, the workgroup and across workgroups (dot_common.h)
template <int U>
__global__ __launch_bounds__(DOT_FAST_THREADS) void k_f16_dot_fast1(const h16x8 *__restrict__ u, const h16x8 *__restrict__ v, uint64_t ngroups,
                                                                    unsigned long long *slots, float *__restrict__ out)
{
    __shared__ float sh[4];
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ngroups; i += U * stride) {
        h16x8 a[U], b[U];
#pragma unroll
        for (int k = 0; k < U; k++) {
            const uint64_t j = i + k * stride, jc = j < ngroups ? j : i;
            a[k] = __builtin_nontemporal_load(&u[jc]);
            b[k] = __builtin_nontemporal_load(&v[jc]);
        }
#pragma unroll
        for (int k = 0; k < U; k++)
            if (i + k * stride < ngroups) f16_chain_step(a[k], b[k], acc);
    }
    const float t = ((acc[0] + acc[4]) + (acc[2] + acc[6])) + ((acc[1] + acc[5]) + (acc[3] + acc[7]));
    dot_hand_over_and_collect(block_sum_256(t, sh), slots, out, sh);
}

// ================================================================================================
// transpose  (CloverMatrix16.h:424-474): a pure 16-bit element transpose
// ================================================================================================
// Workgroup = one 64 x 64-element tile through LDS (row stride 66 elements = 33 dwords: the column gathers of a wave-instruction spread
// over the banks).  Thread t reads 16 bytes (8 elements) of input rows (t >> 3) + 32 j and writes 16 bytes of output rows
// (t >> 3) + 32 j.  rows and cols are multiples of 8; 8-element groups beyond the edges are masked.
#define TR16_T 64
#define TR16_STRIDE (TR16_T + 2)
template <bool NT>
__global__ __launch_bounds__(256) void k_f16_transpose(const uint16_t *__restrict__ h, uint64_t rows, uint64_t cols, uint16_t *__restrict__ ht,
                                                       uint32_t tiles_x)
{
    __shared__ __attribute__((aligned(16))) uint16_t tl[TR16_T * TR16_STRIDE];
    const uint32_t bj = blockIdx.x % tiles_x;
    const uint64_t bi = blockIdx.x / tiles_x;
    const int tid = threadIdx.x, cq = tid & 7, rr = tid >> 3;
    const uint64_t r0 = bi * TR16_T, c0 = (uint64_t)bj * TR16_T;
    u32x4 in[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const uint64_t row = r0 + rr + 32 * j, col = c0 + 8 * cq;
        const bool ok = row < rows && col < cols;
        const u32x4 *src = reinterpret_cast<const u32x4 *>(h + (ok ? row * cols + col : 0));
        in[j] = ld_stream<NT>(src);
    }
#pragma unroll
    for (int j = 0; j < 2; j++) {
        uint32_t *d = reinterpret_cast<uint32_t *>(tl + (rr + 32 * j) * TR16_STRIDE + 8 * cq);
        d[0] = in[j].x;
        d[1] = in[j].y;
        d[2] = in[j].z;
        d[3] = in[j].w;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int oc = rr + 32 * j;              // output row within the tile = input column
        uint32_t w[4];
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const uint16_t *src = tl + (8 * cq + 2 * d) * TR16_STRIDE + oc;
            w[d] = (uint32_t)src[0] | ((uint32_t)src[TR16_STRIDE] << 16);
        }
        const u32x4 o = {w[0], w[1], w[2], w[3]};
        const uint64_t orow = c0 + oc, ocol = r0 + 8 * cq;
        if (orow < cols && ocol < rows) st_stream<NT>(o, reinterpret_cast<u32x4 *>(ht + orow * rows + ocol));
    }
}

// ================================================================================================
// C ABI
// ================================================================================================
static int f16_check_vec(const char *fn, uint64_t n_pad)
{
    CLV_REQUIRE(n_pad % 128 == 0, "%s: n_pad=%llu is not a multiple of 128", fn, (unsigned long long)n_pad);
    CLV_REQUIRE(n_pad / 8 / F16_VEC_GROUPS_PER_WG < 0x7FFFFFFFull, "%s: n_pad=%llu is too large", fn, (unsigned long long)n_pad);
    return CLV_OK;
}

static inline unsigned f16_vec_grid(uint64_t ngroups) { return (unsigned)((ngroups + F16_VEC_GROUPS_PER_WG - 1) / F16_VEC_GROUPS_PER_WG); }

static int f16_quantize(const char *fn, const float *x, uint64_t n, uint16_t *h, void *stream)
{
    CLV_REQUIRE(x && h, "%s: null pointer", fn);
    CLV_REQUIRE(F16_ALIGNED(x) && F16_ALIGNED(h), "%s: pointers must be 16-byte aligned", fn);
    int rc = f16_check_vec(fn, n);
    if (rc) return rc;
    if (!n) return CLV_OK;
    const uint64_t ng = n / 8;
    if (F16_STREAMING(n * 6))
        hipLaunchKernelGGL(k_f16_quantize<true>, dim3(f16_vec_grid(ng)), dim3(256), 0, as_stream(stream), (const f32x4 *)x, (h16x8 *)h, ng);
    else
        hipLaunchKernelGGL(k_f16_quantize<false>, dim3(f16_vec_grid(ng)), dim3(256), 0, as_stream(stream), (const f32x4 *)x, (h16x8 *)h, ng);
    CLV_LAUNCH_CHECK();
    return CLV_OK;
}

extern "C" int clv_f16_quantize(const float *x, uint64_t n_pad, uint16_t *h, void *stream)
{
    return f16_quantize("clv_f16_quantize", x, n_pad, h, stream);
}

extern "C" int clv_f16_restore(const uint16_t *h, uint64_t n_pad, float *x, void *stream)
{
    CLV_REQUIRE(x && h, "clv_f16_restore: null pointer");
    CLV_REQUIRE(F16_ALIGNED(x) && F16_ALIGNED(h), "clv_f16_restore: pointers must be 16-byte aligned");
    int rc = f16_check_vec("clv_f16_restore", n_pad);
    if (rc) return rc;
    if (!n_pad) return CLV_OK;
    const uint64_t ng = n_pad / 8;
    if (F16_STREAMING(n_pad * 6))
        hipLaunchKernelGGL(k_f16_restore<true>, dim3(f16_vec_grid(ng)), dim3(256), 0, as_stream(stream), (const h16x8 *)h, (f32x4 *)x, ng);
    else
        hipLaunchKernelGGL(k_f16_restore<false>, dim3(f16_vec_grid(ng)), dim3(256), 0, as_stream(stream), (const h16x8 *)h, (f32x4 *)x, ng);
    CLV_LAUNCH_CHECK();
    return CLV_OK;
}

extern "C" int clv_f16_scale_and_add(const uint16_t *u, const uint16_t *v, float a, uint64_t n_pad, uint16_t *r, void *stream)
{
    CLV_REQUIRE(u && v && r, "clv_f16_scale_and_add: null pointer");
    CLV_REQUIRE(F16_ALIGNED(u) && F16_ALIGNED(v) && F16_ALIGNED(r), "clv_f16_scale_and_add: pointers must be 16-byte aligned");
    int rc = f16_check_vec("clv_f16_scale_and_add", n_pad);
    if (rc) return rc;
    if (!n_pad) return CLV_OK;
    const uint64_t ng = n_pad / 8;
    if (F16_STREAMING(n_pad * 6))
        hipLaunchKernelGGL(k_f16_scale_and_add<true>, dim3(f16_vec_grid(ng)), dim3(256), 0, as_stream(stream), (const h16x8 *)u, (const h16x8 *)v, a,
                           (h16x8 *)r, ng);
    else
        hipLaunchKernelGGL(k_f16_scale_and_add<false>, dim3(f16_vec_grid(ng)), dim3(256), 0, as_stream(stream), (const h16x8 *)u, (const h16x8 *)v, a,
                           (h16x8 *)r, ng);
    CLV_LAUNCH_CHECK();
    return CLV_OK;
}

// neither mode needs caller memory: EXACT walks the chains out of LDS, FAST hands over through the stream's slots
extern "C" uint64_t clv_f16_dot_workspace_bytes(uint64_t n_pad)
{
    (void)n_pad;
    return 0;
}

extern "C" int clv_f16_dot(const uint16_t *u, const uint16_t *v, uint64_t n_pad, int mode, float *out_dev, void *workspace, void *stream)
{
    CLV_REQUIRE(u && v && out_dev, "clv_f16_dot: null pointer");
    CLV_REQUIRE(F16_ALIGNED(u) && F16_ALIGNED(v), "clv_f16_dot: pointers must be 16-byte aligned");
    CLV_REQUIRE(n_pad % 128 == 0, "clv_f16_dot: n_pad=%llu is not a multiple of 128", (unsigned long long)n_pad);
    CLV_REQUIRE(mode == CLV_DOT_EXACT || mode == CLV_DOT_FAST, "clv_f16_dot: unknown mode %d", mode);
    CLV_REQUIRE_WORKSPACE("clv_f16_dot", workspace);      // unused, but one rule for every workspace argument
    hipStream_t st = as_stream(stream);
    if (!n_pad) { CLV_HIP(hipMemsetAsync(out_dev, 0, sizeof(float), st)); return CLV_OK; }
    if (mode == CLV_DOT_EXACT) {
        hipLaunchKernelGGL(k_f16_dot_exact, dim3(1), dim3(256), 0, st, (const u32x4 *)u, (const u32x4 *)v, n_pad, out_dev);
        CLV_LAUNCH_CHECK();
        return CLV_OK;
    }
    const uint64_t ng = n_pad / 8;
    const uint64_t want = (ng + DOT_FAST_THREADS - 1) / DOT_FAST_THREADS, cap_cu = (uint64_t)clv_cu_count() * 4,
                   cap = cap_cu < (uint64_t)DOT_FAST_THREADS * DOT_MAX_SLOTS_PER_THREAD ? cap_cu : (uint64_t)DOT_FAST_THREADS * DOT_MAX_SLOTS_PER_THREAD;
    const int grid = (int)(want < cap ? want : cap);
    void *slots = nullptr;
    int rc = clv_internal_sync_slots(&slots, (uint64_t)grid * 8, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_f16_dot_fast1<4>, dim3(grid), dim3(DOT_FAST_THREADS), 0, st, (const h16x8 *)u, (const h16x8 *)v, ng,
                       (unsigned long long *)slots, out_dev);
    CLV_LAUNCH_CHECK();
    return CLV_OK;
}

extern "C" int clm_f16_quantize(const float *A, uint64_t rows, uint64_t cols, uint16_t *h, void *stream)
{
    CLV_REQUIRE(rows % 128 == 0 && cols % 128 == 0, "clm_f16_quantize: rows=%llu cols=%llu must be multiples of 128", (unsigned long long)rows,
                (unsigned long long)cols);
    CLV_REQUIRE(!cols || rows <= 0xFFFFFFFFFFFFull / cols, "clm_f16_quantize: matrix too large");
    return f16_quantize("clm_f16_quantize", A, rows * cols, h, stream);
}

template <bool XF32>
static int f16_mvm(const char *fn, const uint16_t *A, uint64_t rows, uint64_t cols, const void *x, void *r, void *stream)
{
    CLV_REQUIRE(A && x && r, "%s: null pointer", fn);
    CLV_REQUIRE(F16_ALIGNED(A) && F16_ALIGNED(x), "%s: the matrix and x must be 16-byte aligned", fn);
    // a whole CloverMatrix16 has rows % 128 == 0; any row count is a row shard of one
    CLV_REQUIRE(cols % 128 == 0, "%s: cols=%llu must be a multiple of 128", fn, (unsigned long long)cols);
    CLV_REQUIRE(x != r, "%s: the result must not alias the vector being multiplied", fn);
    CLV_REQUIRE(rows / 16 < 0x7FFFFFFFull, "%s: matrix too large", fn);
    if (!rows) return CLV_OK;
    hipStream_t st = as_stream(stream);
    const bool streaming = F16_STREAMING(rows * cols * 2);
    // four waves (64 rows) per workgroup; one wave (16 rows) while that leaves fewer than two workgroups per CU
    if (rows / 64 >= 2 * (uint64_t)clv_cu_count()) {
        const dim3 grid((unsigned)((rows + 63) / 64)), block(256);
        if (streaming) hipLaunchKernelGGL((k_f16_mvm<4, true, XF32>), grid, block, 0, st, A, rows, cols, x, r);
        else hipLaunchKernelGGL((k_f16_mvm<4, false, XF32>), grid, block, 0, st, A, rows, cols, x, r);
    } else {
        const dim3 grid((unsigned)((rows + 15) / 16)), block(64);
        if (streaming) hipLaunchKernelGGL((k_f16_mvm<1, true, XF32>), grid, block, 0, st, A, rows, cols, x, r);
        else hipLaunchKernelGGL((k_f16_mvm<1, false, XF32>), grid, block, 0, st, A, rows, cols, x, r);
    }
    CLV_LAUNCH_CHECK();
    return CLV_OK;
}

extern "C" int clm_f16_mvm(const uint16_t *A, uint64_t rows, uint64_t cols, const uint16_t *x, uint16_t *r, void *stream)
{
    return f16_mvm<false>("clm_f16_mvm", A, rows, cols, x, r, stream);
}

extern "C" int clm_f16_mvm_f32(const uint16_t *A, uint64_t rows, uint64_t cols, const float *x, float *r, void *stream)
{
    return f16_mvm<true>("clm_f16_mvm_f32", A, rows, cols, x, r, stream);
}

#define F16_SAA "clm_f16_mvm_scale_and_add"
extern "C" int clm_f16_mvm_scale_and_add(const uint16_t *A, uint64_t rows, uint64_t cols, const uint16_t *x, const uint16_t *u, float a, uint16_t *t,
                                         uint16_t *r, void *stream)
{
    CLV_REQUIRE(A && x && u && r, F16_SAA ": null pointer");
    CLV_REQUIRE(F16_ALIGNED(A) && F16_ALIGNED(x), F16_SAA ": the matrix and x must be 16-byte aligned");
    CLV_REQUIRE(((uintptr_t)u & 1u) == 0 && ((uintptr_t)t & 1u) == 0 && ((uintptr_t)r & 1u) == 0, F16_SAA ": u, t and r must be 2-byte aligned");
    CLV_REQUIRE(cols % 128 == 0, F16_SAA ": cols=%llu must be a multiple of 128", (unsigned long long)cols);
    CLV_REQUIRE(r != x && t != x, F16_SAA ": the results must not alias the vector being multiplied");
    CLV_REQUIRE(t != r && (!t || t != u), F16_SAA ": t must not alias r or u");
    CLV_REQUIRE(rows / 16 < 0x7FFFFFFFull, F16_SAA ": matrix too large");
    if (!rows) return CLV_OK;
    hipStream_t st = as_stream(stream);
    const bool streaming = F16_STREAMING(rows * cols * 2);                // the workgroup and nontemporal rules of f16_mvm()
    const F16Fuse fuse = {u, a, r};
    if (rows / 64 >= 2 * (uint64_t)clv_cu_count()) {
        const dim3 grid((unsigned)((rows + 63) / 64)), block(256);
        if (streaming) hipLaunchKernelGGL((k_f16_mvm_saa(4, true)), grid, block, 0, st, A, rows, cols, (const void *)x, (void *)t, fuse);
        else hipLaunchKernelGGL((k_f16_mvm_saa(4, false)), grid, block, 0, st, A, rows, cols, (const void *)x, (void *)t, fuse);
    } else {
        const dim3 grid((unsigned)((rows + 15) / 16)), block(64);
        if (streaming) hipLaunchKernelGGL((k_f16_mvm_saa(1, true)), grid, block, 0, st, A, rows, cols, (const void *)x, (void *)t, fuse);
        else hipLaunchKernelGGL((k_f16_mvm_saa(1, false)), grid, block, 0, st, A, rows, cols, (const void *)x, (void *)t, fuse);
    }
    CLV_LAUNCH_CHECK();
    return CLV_OK;
}
#undef F16_SAA

int clv_internal_f16_clear(uint16_t *x, uint64_t n_pad, hipStream_t st)
{
    if (!n_pad) return CLV_OK;
    const uint64_t ng = n_pad / 8, want = (ng + 255) / 256;
    hipLaunchKernelGGL(k_f16_clear, dim3((unsigned)(want < 1024 ? want : 1024)), dim3(256), 0, st, (u32x4 *)x, ng);
    CLV_LAUNCH_CHECK();
    return CLV_OK;
}

// Q_IHT / Q_GD (test/performance/01_measure.h:923-946, 999-1021) over a CloverMatrix16 with CloverVector16 vectors
// (test/performance/02_bit16.cpp:112-117).  One call enqueues all iterations: 3 launches per iteration (2 for GD), nothing copied back.
extern "C" int clm_f16_iht(const uint16_t *Phi, const uint16_t *PhiT, uint64_t m, uint64_t n, uint16_t *x, uint64_t x_len, const uint16_t *y,
                           uint16_t *t1, uint16_t *t2, uint16_t *t3, uint64_t iterations, uint64_t K, float mu, int threshold, void *stream)
{
    CLV_REQUIRE(Phi && PhiT && x && y && t1 && t2 && t3, "clm_f16_iht: null pointer");
    CLV_REQUIRE(m % 128 == 0 && n % 128 == 0 && x_len <= n, "clm_f16_iht: m=%llu n=%llu x_len=%llu", (unsigned long long)m, (unsigned long long)n,
                (unsigned long long)x_len);
    CLV_REQUIRE(threshold >= 0 && threshold <= 2, "clm_f16_iht: unknown threshold %d", threshold);
    CLV_REQUIRE(F16_ALIGNED(Phi) && F16_ALIGNED(PhiT) && F16_ALIGNED(x) && F16_ALIGNED(t2), "clm_f16_iht: the matrices, x and t2 must be 16-byte aligned");
    int rc = clv_internal_f16_clear(x, n, as_stream(stream));                                            // x.clear()
    for (uint64_t it = 0; !rc && it < iterations; it++) {
        rc = clm_f16_mvm_scale_and_add(Phi, m, n, x, y, -1.0f, t1, t2, stream);                          // t1 = Phi x; t2 = y - t1
        if (!rc) rc = clm_f16_mvm_scale_and_add(PhiT, n, m, t2, x, mu, t3, x, stream);                   // t3 = Phi' t2; x += mu t3
        if (!rc && threshold)                                                          // keep the K largest (2: the reference's survivor order)
            rc = clv_f16_threshold_mode(x, x_len, n, K, threshold == 2 ? CLV_THRESHOLD_REFERENCE : CLV_THRESHOLD_FAST, nullptr, stream);
    }
    return rc;
}

extern "C" int clm_f16_transpose(const uint16_t *h, uint64_t rows, uint64_t cols, uint16_t *ht, void *stream)
{
    CLV_REQUIRE(h && ht, "clm_f16_transpose: null pointer");
    CLV_REQUIRE(F16_ALIGNED(h) && F16_ALIGNED(ht), "clm_f16_transpose: pointers must be 16-byte aligned");
    CLV_REQUIRE(rows % 8 == 0 && cols % 8 == 0, "clm_f16_transpose: rows=%llu cols=%llu must be multiples of 8", (unsigned long long)rows,
                (unsigned long long)cols);
    CLV_REQUIRE(h != ht, "clm_f16_transpose: in-place transposition is not supported");
    if (!rows || !cols) return CLV_OK;
    const uint64_t tiles_x = (cols + TR16_T - 1) / TR16_T, tiles = ((rows + TR16_T - 1) / TR16_T) * tiles_x;
    CLV_REQUIRE(tiles <= 0x7FFFFFFFull && tiles_x <= 0xFFFFFFFFull, "clm_f16_transpose: too many tiles");
    // streaming loads and stores once input + output cannot live in the Infinity Cache (the clm4_transpose rule)
    if (F16_STREAMING(rows * cols * 4))
        hipLaunchKernelGGL(k_f16_transpose<true>, dim3((unsigned)tiles), dim3(256), 0, as_stream(stream), h, rows, cols, ht, (uint32_t)tiles_x);
    else
        hipLaunchKernelGGL(k_f16_transpose<false>, dim3((unsigned)tiles), dim3(256), 0, as_stream(stream), h, rows, cols, ht, (uint32_t)tiles_x);
    CLV_LAUNCH_CHECK();
    return CLV_OK;
}
