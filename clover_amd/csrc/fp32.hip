// fp32.hip -- CloverVector32 / CloverMatrix32 on gfx950: the reference's 32-bit classes, its comparison baseline and the containers every
// caller's data starts in.  Plain fp32 values, no scales.  include/clover_fp32.h states every order on the host; what runs here equals it
// bit for bit (dot FAST excepted: another, fixed summation order).
//
// scaleAndAdd = fma(v, s, u) per element, dot / mvm = 32 sequential fma chains (element j -> chain j mod 32) and the reference's tree, as
// half16.hip has them for f16 -- with twice the bytes per chain step: a 32-element step is 128 contiguous bytes of the row.
//
// The chain layout: EIGHT lanes per row, ONE 16-byte load per lane and step (not four lanes with two loads each).  A wave instruction then
// reads the whole 128-byte line of each of its 8 rows, where four lanes x two loads would touch every line twice, half of it each time;
// a lane carries 4 accumulators instead of 8; and a matrix of 8192 rows gives 1024 waves, four per CU, where four lanes per row would
// leave two -- with F32_MVM_U requests of 16 bytes in flight per lane that is the 32 KiB per CU the HBM latency asks for.  Lane
// p = tid & 7 keeps chains 4 p .. 4 p + 3; f32_chain_step / f32_chain_tree below are the only code that knows this mapping.
//
// fp32 subnormals are kept (hipcc's default kernel mode; no flushing instruction is used), every sum is a separately rounded v_add_f32
// (-ffp-contract=off) and every fma one fused v_fma_f32 / half of a v_pk_fma_f32.
#include "dot_common.h"
#include "mvm_f32_host.h"           // f32_iht_loop: the loop body the quantized matrices share with clm_f32_iht
#include "clover_hip_fp32.h"

template <bool NT, typename T> __device__ __forceinline__ T ld_stream(const T *p) { return NT ? __builtin_nontemporal_load(p) : *p; }
template <bool NT, typename T> __device__ __forceinline__ void st_stream(T v, T *p)
{
    if (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// ================================================================================================
// streaming vector kernels: lane = 4 consecutive elements (16 bytes), F32_VU groups in flight per lane and operand
// ================================================================================================
#define F32_VU 4
#define F32_VEC_GROUPS_PER_WG (256 * F32_VU)

// CloverVector32::scaleAndAdd (CloverVector32.h:291-323, the FMA branch): r = fma(v, s, u); r may be u (a lane reads its own 16 bytes before
// it writes them)
template <bool NT>
__global__ __launch_bounds__(256) void k_f32_scale_and_add(const f32x4 *u, const f32x4 *__restrict__ v, float s, f32x4 *r, uint64_t ngroups)
{
    const uint64_t g0 = (uint64_t)blockIdx.x * F32_VEC_GROUPS_PER_WG + threadIdx.x;
    f32x4 a[F32_VU], b[F32_VU];
#pragma unroll
    for (int k = 0; k < F32_VU; k++) {
        const uint64_t g = g0 + 256 * k, gc = g < ngroups ? g : 0;
        a[k] = ld_stream<NT>(&u[gc]);
        b[k] = ld_stream<NT>(&v[gc]);
    }
#pragma unroll
    for (int k = 0; k < F32_VU; k++) {
        const uint64_t g = g0 + 256 * k;
        const f32x4 o = {__builtin_fmaf(b[k].x, s, a[k].x), __builtin_fmaf(b[k].y, s, a[k].y), __builtin_fmaf(b[k].z, s, a[k].z),
                         __builtin_fmaf(b[k].w, s, a[k].w)};
        if (g < ngroups) st_stream<NT>(o, &r[g]);
    }
}

// CloverVector32::clear() on the stream (the first step of clm_f32_iht): a kernel, not a memset, so that a captured call replays it as one
// more kernel node in stream order
__global__ __launch_bounds__(256) void k_f32_clear(u32x4 *__restrict__ x, uint64_t ngroups)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += stride) x[g] = u32x4{0u, 0u, 0u, 0u};
}

// ================================================================================================
// the 32 chains and their tree
// ================================================================================================
// Eight lanes own one row (or the one dot): lane p = tid & 7 keeps chains 4 p .. 4 p + 3 in acc[0..3], i.e. half q = p & 1 of the
// reference's __m256 accumulator p >> 1.  A 16-byte load is 4 consecutive elements, one step of those 4 chains; the eight lanes read the
// 128 contiguous bytes of a 32-element step.
__device__ __forceinline__ void f32_chain_step(const f32x4 a, const f32x4 x, float acc[4])
{
    acc[0] = __builtin_fmaf(x.x, a.x, acc[0]);
    acc[1] = __builtin_fmaf(x.y, a.y, acc[1]);
    acc[2] = __builtin_fmaf(x.z, a.z, acc[2]);
    acc[3] = __builtin_fmaf(x.w, a.w, acc[3]);
}

// (acc0 + acc1) + (acc2 + acc3) lane-wise, then _mm256_haddf32_ps (CloverBase.h:149-157): t[i] = s[i + 4] + s[i], (t0 + t2) + (t1 + t3).
// Accumulators 0 and 1 sit in lanes p, p ^ 2, the sum of the two pairs in lanes p, p ^ 4; s[i] and s[i + 4] in lanes p, p ^ 1.  fp32
// addition commutes, so both partners of an exchange compute the same bits: every lane of the eight ends with the value.
__device__ __forceinline__ float f32_chain_tree(const float acc[4])
{
    float t[4];
#pragma unroll
    for (int l = 0; l < 4; l++) {
        const float pair = acc[l] + __shfl_xor(acc[l], 2);
        const float s = pair + __shfl_xor(pair, 4);
        t[l] = s + __shfl_xor(s, 1);
    }
    return (t[0] + t[2]) + (t[1] + t[3]);
}

// ================================================================================================
// mvm  (CloverMatrix32.h:90-128; every row in the order of CloverVector32::dot, clover_fp32::mvm_rows)
// ================================================================================================
// Workgroup = 8 * WAVES rows, eight lanes per row.  x is staged in LDS once per workgroup, F32_X_BYTES (4096 elements) at a time; the matrix
// is read 16 bytes per lane, F32_MVM_U requests in flight (1 KiB of every row).  Every lane of a row reads the same eight 16-byte
// pieces of x as the lanes of the other rows (a broadcast, no bank conflict).  Rows beyond `rows` (a workgroup's tail; none while rows is
// a multiple of 8 * WAVES) re-read the last row and store nothing.
#define F32_MVM_U 8
#define F32_X_BYTES 16384

template <int U, bool NT>
__device__ __forceinline__ void f32_mvm_steps(const f32x4 *__restrict__ Ap, const f32x4 *xs, int p, uint32_t t0, float acc[4])
{
    f32x4 a[U];
#pragma unroll
    for (int u = 0; u < U; u++) a[u] = ld_stream<NT>(&Ap[8 * (uint64_t)(t0 + u) + p]);
#pragma unroll
    for (int u = 0; u < U; u++) f32_chain_step(a[u], xs[8 * (t0 + u) + p], acc);
}

// FUSED (clm_f32_mvm_scale_and_add): the CloverVector32::scaleAndAdd that follows this mvm in the IHT / GD loops, done by the lane that stores
// the row: d = the row value; t[row] = d when t is given; r2[row] = fma(d, a, u[row]) -- what the two separate calls compute.  A row
// depends on no other row: no workgroup-wide step.  u[row] is requested before the streaming loop.
struct F32Fuse {
    const float *u;
    float a;
    float *r2;               // may alias u (the in-place form): a lane reads its element of u before it writes it
};

// r is the result (plain) or t (FUSED, may be NULL); apart from x, u and r2
template <int WAVES, bool NT, bool FUSED>
__global__ __launch_bounds__(64 * WAVES) void k_f32_mvm(const float *__restrict__ A, uint64_t rows, uint64_t cols, const float *__restrict__ x,
                                                        float *__restrict__ r, F32Fuse fuse)
{
    __shared__ __attribute__((aligned(16))) f32x4 xs[F32_X_BYTES / 16];
    constexpr int THREADS = 64 * WAVES;
    constexpr uint32_t CH = F32_X_BYTES / 4;                  // elements of x per chunk
    constexpr int NX = F32_X_BYTES / 16 / THREADS;            // 16-byte pieces per thread and chunk
    const int tid = threadIdx.x, p = tid & 7, rho = tid >> 3;
    const uint64_t row = (uint64_t)blockIdx.x * (8 * WAVES) + rho;
    const f32x4 *Arow = reinterpret_cast<const f32x4 *>(A + (row < rows ? row : rows - 1) * cols);
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float fuse_u = 0.0f;
    if (FUSED && p == 0 && row < rows) fuse_u = fuse.u[row];      // ahead of the streaming loop: the epilogue waits on nothing

    for (uint64_t c0 = 0; c0 < cols; c0 += CH) {
        const uint32_t cw = (uint32_t)((cols - c0) < CH ? (cols - c0) : CH);
        if (c0) __syncthreads();
        {   // all loads first (one round trip), then the LDS writes
            const f32x4 *xg = reinterpret_cast<const f32x4 *>(x + c0);
            const uint32_t n16 = cw / 4;
            f32x4 xr[NX];
#pragma unroll
            for (int k = 0; k < NX; k++) { const uint32_t i = tid + THREADS * k; xr[k] = xg[i < n16 ? i : 0]; }
#pragma unroll
            for (int k = 0; k < NX; k++) { const uint32_t i = tid + THREADS * k; if (i < n16) xs[i] = xr[k]; }
        }
        __syncthreads();
        const f32x4 *Ap = Arow + c0 / 4;
        const uint32_t nsteps = cw / 32;
        uint32_t t = 0;
        for (; t + F32_MVM_U <= nsteps; t += F32_MVM_U) f32_mvm_steps<F32_MVM_U, NT>(Ap, xs, p, t, acc);
        for (; t < nsteps; t++) f32_mvm_steps<1, NT>(Ap, xs, p, t, acc);
    }
    const float d = f32_chain_tree(acc);
    if (p == 0 && row < rows) {
        if (FUSED) {
            if (r) r[row] = d;
            fuse.r2[row] = __builtin_fmaf(d, fuse.a, fuse_u);
        } else {
            r[row] = d;
        }
    }
}

// ================================================================================================
// dot  (CloverVector32.h:406-451)
// ================================================================================================
// EXACT: the 32 chains are sequential by definition (n / 32 dependent fmas each).  One workgroup: all 256 threads move u and v through
// LDS (F32_DOT_CH elements of each per round, requested while the previous round is being consumed), and one group of eight lanes --
// lane p = chains 4 p .. 4 p + 3, as in mvm -- walks the chains from LDS.
#define F32_DOT_CH 4096u
__global__ __launch_bounds__(256) void k_f32_dot_exact(const f32x4 *__restrict__ u, const f32x4 *__restrict__ v, uint64_t n, float *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) f32x4 us[F32_DOT_CH / 4], vs[F32_DOT_CH / 4];
    constexpr int NX = F32_DOT_CH / 4 / 256;                  // 16-byte pieces per thread, operand and round
    const int tid = threadIdx.x;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 ur[NX], vr[NX];
    const uint64_t n16 = n / 4;
#pragma unroll
    for (int k = 0; k < NX; k++) {
        const uint64_t i = (uint64_t)tid + 256 * k, ic = i < n16 ? i : 0;
        ur[k] = u[ic];
        vr[k] = v[ic];
    }
    for (uint64_t c0 = 0; c0 < n; c0 += F32_DOT_CH) {
        const uint32_t cw = (uint32_t)((n - c0) < F32_DOT_CH ? (n - c0) : F32_DOT_CH);
        if (c0) __syncthreads();                              // the eight lanes have finished with the previous round
#pragma unroll
        for (int k = 0; k < NX; k++) {
            us[tid + 256 * k] = ur[k];
            vs[tid + 256 * k] = vr[k];
        }
        // the next round's loads are in flight while the eight lanes work
        const uint64_t nb = (c0 + F32_DOT_CH) / 4;
#pragma unroll
        for (int k = 0; k < NX; k++) {
            const uint64_t i = nb + tid + 256 * k, ic = i < n16 ? i : 0;
            ur[k] = u[ic];
            vr[k] = v[ic];
        }
        __syncthreads();
        if (tid < 8) {
            const uint32_t nsteps = cw / 32;
#pragma unroll 4
            for (uint32_t t = 0; t < nsteps; t++) f32_chain_step(us[8 * t + tid], vs[8 * t + tid], acc);
        }
    }
    const float d = f32_chain_tree(acc);                      // wave 0 only matters; the shuffles stay inside the eight lanes
    if (tid == 0) *out = d;
}

// FAST: one launch; a lane keeps 4 fp32 partial sums over its 16-byte groups (one fma per element, another summation order), then fixed
// trees inside the lane, the workgroup and across workgroups (dot_common.h).  The same bits on every call: the grid and every tree are
// functions of n and the device's CU count alone.  Roundings on the longest path (what tests/fp32_helpers.py's fast_dot_bound counts):
//   L = ceil(n / 4 / (grid * 256)) fmas of a lane's chain, 2 additions inside the lane, 6 + 2 in block_sum_256, up to
//   DOT_MAX_SLOTS_PER_THREAD = 8 in the collector's thread, 6 + 2 in its block_sum_256: D = L + 26.
template <int U>
__global__ __launch_bounds__(DOT_FAST_THREADS) void k_f32_dot_fast1(const f32x4 *__restrict__ u, const f32x4 *__restrict__ v, uint64_t ngroups,
                                                                    unsigned long long *slots, float *__restrict__ out)
{
    __shared__ float sh[4];
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ngroups; i += U * stride) {
        f32x4 a[U], b[U];
#pragma unroll
        for (int k = 0; k < U; k++) {
            const uint64_t j = i + k * stride, jc = j < ngroups ? j : i;
            a[k] = __builtin_nontemporal_load(&u[jc]);
            b[k] = __builtin_nontemporal_load(&v[jc]);
        }
#pragma unroll
        for (int k = 0; k < U; k++)
            if (i + k * stride < ngroups) f32_chain_step(a[k], b[k], acc);
    }
    const float t = (acc[0] + acc[2]) + (acc[1] + acc[3]);
    dot_hand_over_and_collect(block_sum_256(t, sh), slots, out, sh);
}

// ================================================================================================
// transpose  (CloverMatrix32.h:169-179): a 32-bit element transpose
// ================================================================================================
// Workgroup = one 64 x 64-element tile through LDS, row stride 65 dwords: thread t (cq = t & 7, rr = t >> 3) moves 16 bytes (4 elements) at
// tile row rr + 32 (j & 1), tile column 4 cq + 32 (j >> 1), j = 0 .. 3 -- eight lanes read 128 contiguous bytes of an input row and write
// 128 contiguous bytes of an output row.  With the odd stride both the row-wise LDS writes and the column gathers of a 32-lane group
// land on bank (4 cq + rr + const) mod 32: 32 different banks.  rows and cols are multiples of 4; 4-element groups beyond the edges are masked.
#define TR32_T 64
#define TR32_STRIDE (TR32_T + 1)
template <bool NT>
__global__ __launch_bounds__(256) void k_f32_transpose(const uint32_t *__restrict__ A, uint64_t rows, uint64_t cols, uint32_t *__restrict__ At,
                                                       uint32_t tiles_x)
{
    __shared__ uint32_t tl[TR32_T * TR32_STRIDE];
    const uint32_t bj = blockIdx.x % tiles_x;
    const uint64_t bi = blockIdx.x / tiles_x;
    const int tid = threadIdx.x, cq = tid & 7, rr = tid >> 3;
    const uint64_t r0 = bi * TR32_T, c0 = (uint64_t)bj * TR32_T;
    u32x4 in[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint64_t row = r0 + rr + 32 * (j & 1), col = c0 + 4 * cq + 32 * (j >> 1);
        const bool ok = row < rows && col < cols;
        in[j] = ld_stream<NT>(reinterpret_cast<const u32x4 *>(A + (ok ? row * cols + col : 0)));
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        uint32_t *d = tl + (rr + 32 * (j & 1)) * TR32_STRIDE + 4 * cq + 32 * (j >> 1);
        d[0] = in[j].x;
        d[1] = in[j].y;
        d[2] = in[j].z;
        d[3] = in[j].w;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int oc = rr + 32 * (j & 1), ir = 4 * cq + 32 * (j >> 1);      // output row within the tile = input column; 4 input rows from ir
        const uint32_t *src = tl + ir * TR32_STRIDE + oc;
        const u32x4 o = {src[0], src[TR32_STRIDE], src[2 * TR32_STRIDE], src[3 * TR32_STRIDE]};
        const uint64_t orow = c0 + oc, ocol = r0 + ir;
        if (orow < cols && ocol < rows) st_stream<NT>(o, reinterpret_cast<u32x4 *>(At + orow * rows + ocol));
    }
}

// ================================================================================================
// C ABI (include/clover_hip_fp32.h)
// ================================================================================================
#define F32_ALIGNED(p) (((uintptr_t)(p) & 15u) == 0)
#define F32_ALIGNED4(p) (((uintptr_t)(p) & 3u) == 0)

// streaming loads / stores once the operands cannot stay in the 256 MiB Infinity Cache (the clm4_mvm rule)
#define F32_STREAMING(bytes) ((bytes) > (256ull << 20))

static inline unsigned f32_vec_grid(uint64_t ngroups) { return (unsigned)((ngroups + F32_VEC_GROUPS_PER_WG - 1) / F32_VEC_GROUPS_PER_WG); }

extern "C" int clv_f32_scale_and_add(const float *u, const float *v, float a, uint64_t n_pad, float *r, void *stream)
{
    CLV_REQUIRE(u && v && r, "clv_f32_scale_and_add: null pointer");
    CLV_REQUIRE(F32_ALIGNED(u) && F32_ALIGNED(v) && F32_ALIGNED(r), "clv_f32_scale_and_add: pointers must be 16-byte aligned");
    CLV_REQUIRE(n_pad % 128 == 0, "clv_f32_scale_and_add: n_pad=%llu is not a multiple of 128", (unsigned long long)n_pad);
    CLV_REQUIRE(n_pad / 4 / F32_VEC_GROUPS_PER_WG < 0x7FFFFFFFull, "clv_f32_scale_and_add: n_pad=%llu is too large", (unsigned long long)n_pad);
    CLV_REQUIRE(v != r, "clv_f32_scale_and_add: the result may alias u, not v");
    if (!n_pad) return CLV_OK;
    const uint64_t ng = n_pad / 4;
    if (F32_STREAMING(n_pad * 12))
        hipLaunchKernelGGL(k_f32_scale_and_add<true>, dim3(f32_vec_grid(ng)), dim3(256), 0, as_stream(stream), (const f32x4 *)u, (const f32x4 *)v, a,
                           (f32x4 *)r, ng);
    else
        hipLaunchKernelGGL(k_f32_scale_and_add<false>, dim3(f32_vec_grid(ng)), dim3(256), 0, as_stream(stream), (const f32x4 *)u, (const f32x4 *)v, a,
                           (f32x4 *)r, ng);
    CLV_LAUNCH_CHECK();
    return CLV_OK;
}

// neither mode needs caller memory: EXACT walks the chains out of LDS, FAST hands over through the stream's slots
extern "C" uint64_t clv_f32_dot_workspace_bytes(uint64_t n_pad)
{
    (void)n_pad;
    return 0;
}

extern "C" int clv_f32_dot(const float *u, const float *v, uint64_t n_pad, int mode, float *out_dev, void *workspace, void *stream)
{
    CLV_REQUIRE(u && v && out_dev, "clv_f32_dot: null pointer");
    CLV_REQUIRE(F32_ALIGNED(u) && F32_ALIGNED(v) && F32_ALIGNED4(out_dev), "clv_f32_dot: u and v must be 16-byte aligned, out_dev 4-byte");
    CLV_REQUIRE(n_pad % 128 == 0, "clv_f32_dot: n_pad=%llu is not a multiple of 128", (unsigned long long)n_pad);
    CLV_REQUIRE(mode == CLV_DOT_EXACT || mode == CLV_DOT_FAST, "clv_f32_dot: unknown mode %d", mode);
    CLV_REQUIRE_WORKSPACE("clv_f32_dot", workspace);      // unused, but one rule for every workspace argument
    hipStream_t st = as_stream(stream);
    if (!n_pad) { CLV_HIP(hipMemsetAsync(out_dev, 0, sizeof(float), st)); return CLV_OK; }
    if (mode == CLV_DOT_EXACT) {
        hipLaunchKernelGGL(k_f32_dot_exact, dim3(1), dim3(256), 0, st, (const f32x4 *)u, (const f32x4 *)v, n_pad, out_dev);
        CLV_LAUNCH_CHECK();
        return CLV_OK;
    }
    const uint64_t ng = n_pad / 4;
    const uint64_t want = (ng + DOT_FAST_THREADS - 1) / DOT_FAST_THREADS, cap_cu = (uint64_t)clv_cu_count() * 4,
                   cap = cap_cu < (uint64_t)DOT_FAST_THREADS * DOT_MAX_SLOTS_PER_THREAD ? cap_cu : (uint64_t)DOT_FAST_THREADS * DOT_MAX_SLOTS_PER_THREAD;
    const int grid = (int)(want < cap ? want : cap);
    void *slots = nullptr;
    int rc = clv_internal_sync_slots(&slots, (uint64_t)grid * 8, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_f32_dot_fast1<4>, dim3(grid), dim3(DOT_FAST_THREADS), 0, st, (const f32x4 *)u, (const f32x4 *)v, ng,
                       (unsigned long long *)slots, out_dev);
    CLV_LAUNCH_CHECK();
    return CLV_OK;
}

int clv_internal_f32_clear(float *x, uint64_t n, hipStream_t st)
{
    if (!n) return CLV_OK;
    const uint64_t ng = n / 4, want = (ng + 255) / 256;
    hipLaunchKernelGGL(k_f32_clear, dim3((unsigned)(want < 1024 ? want : 1024)), dim3(256), 0, st, (u32x4 *)x, ng);
    CLV_LAUNCH_CHECK();
    return CLV_OK;
}

// the checks and the launch of both mvm forms; t is the plain result (fuse == nullptr) or the optional copy of the row values
static int f32_mvm(const char *fn, const float *A, uint64_t rows, uint64_t cols, const float *x, float *t, const F32Fuse *fuse, void *stream)
{
    CLV_REQUIRE(A && x && (fuse ? fuse->u && fuse->r2 : t != nullptr), "%s: null pointer", fn);
    CLV_REQUIRE(F32_ALIGNED(A) && F32_ALIGNED(x), "%s: the matrix and x must be 16-byte aligned", fn);
    CLV_REQUIRE(F32_ALIGNED4(t) && (!fuse || (F32_ALIGNED4(fuse->u) && F32_ALIGNED4(fuse->r2))), "%s: the row vectors must be 4-byte aligned", fn);
    CLV_REQUIRE(rows % 128 == 0 && cols % 128 == 0, "%s: rows=%llu cols=%llu must be multiples of 128", fn, (unsigned long long)rows,
                (unsigned long long)cols);
    CLV_REQUIRE(t != x && (!fuse || fuse->r2 != x), "%s: the results must not alias the vector being multiplied", fn);
    CLV_REQUIRE(!fuse || (t != fuse->r2 && (!t || t != fuse->u)), "%s: t must not alias r2 or u", fn);
    CLV_REQUIRE(rows / 8 < 0x7FFFFFFFull && (!cols || rows <= 0x3FFFFFFFFFFFull / cols), "%s: matrix too large", fn);
    if (!rows) return CLV_OK;
    hipStream_t st = as_stream(stream);
    const bool streaming = F32_STREAMING(rows * cols * 4);
    const F32Fuse f = fuse ? *fuse : F32Fuse{nullptr, 0.0f, nullptr};
    // four waves (32 rows) per workgroup; one wave (8 rows) while that leaves fewer than two workgroups per CU
    const bool wide = rows / 32 >= 2 * (uint64_t)clv_cu_count();
    const dim3 grid((unsigned)(wide ? (rows + 31) / 32 : (rows + 7) / 8)), block(wide ? 256 : 64);
#define F32_MVM_LAUNCH(W, NT, FU) hipLaunchKernelGGL((k_f32_mvm<W, NT, FU>), grid, block, 0, st, A, rows, cols, x, t, f)
    if (fuse) {
        if (wide) { if (streaming) F32_MVM_LAUNCH(4, true, true); else F32_MVM_LAUNCH(4, false, true); }
        else { if (streaming) F32_MVM_LAUNCH(1, true, true); else F32_MVM_LAUNCH(1, false, true); }
    } else {
        if (wide) { if (streaming) F32_MVM_LAUNCH(4, true, false); else F32_MVM_LAUNCH(4, false, false); }
        else { if (streaming) F32_MVM_LAUNCH(1, true, false); else F32_MVM_LAUNCH(1, false, false); }
    }
#undef F32_MVM_LAUNCH
    CLV_LAUNCH_CHECK();
    return CLV_OK;
}

extern "C" int clm_f32_mvm(const float *A, uint64_t rows, uint64_t cols, const float *x, float *r, void *stream)
{
    return f32_mvm("clm_f32_mvm", A, rows, cols, x, r, nullptr, stream);
}

extern "C" int clm_f32_mvm_scale_and_add(const float *A, uint64_t rows, uint64_t cols, const float *x, const float *u, float a, float *t, float *r2,
                                         void *stream)
{
    const F32Fuse fuse = {u, a, r2};
    return f32_mvm("clm_f32_mvm_scale_and_add", A, rows, cols, x, t, &fuse, stream);
}

// Q_IHT / Q_GD (test/performance/01_measure.h:923-946, 999-1021) over a CloverMatrix32 with CloverVector32 vectors, the baseline of every
// table of the reference.  One call enqueues all iterations: 3 launches per iteration (2 for GD), nothing copied back.
extern "C" int clm_f32_iht(const float *Phi, const float *PhiT, uint64_t m, uint64_t n, float *x, uint64_t x_len, const float *y, float *t1, float *t2,
                           float *t3, uint64_t iterations, uint64_t K, float mu, int threshold, void *stream)
{
    CLV_REQUIRE(Phi && PhiT && x && y && t1 && t2 && t3, "clm_f32_iht: null pointer");
    CLV_REQUIRE(m % 128 == 0 && n % 128 == 0 && x_len <= n, "clm_f32_iht: m=%llu n=%llu x_len=%llu", (unsigned long long)m, (unsigned long long)n,
                (unsigned long long)x_len);
    CLV_REQUIRE(threshold >= 0 && threshold <= 2, "clm_f32_iht: unknown threshold %d", threshold);
    CLV_REQUIRE(F32_ALIGNED(Phi) && F32_ALIGNED(PhiT) && F32_ALIGNED(x) && F32_ALIGNED(t2), "clm_f32_iht: the matrices, x and t2 must be 16-byte aligned");
    return f32_iht_loop(
        x, x_len, n, iterations, K, threshold, stream, [&] { return clm_f32_mvm_scale_and_add(Phi, m, n, x, y, -1.0f, t1, t2, stream); },
        [&] { return clm_f32_mvm_scale_and_add(PhiT, n, m, t2, x, mu, t3, x, stream); });
}

extern "C" int clm_f32_transpose(const float *A, uint64_t rows, uint64_t cols, float *At, void *stream)
{
    CLV_REQUIRE(A && At, "clm_f32_transpose: null pointer");
    CLV_REQUIRE(F32_ALIGNED(A) && F32_ALIGNED(At), "clm_f32_transpose: pointers must be 16-byte aligned");
    CLV_REQUIRE(rows % 4 == 0 && cols % 4 == 0, "clm_f32_transpose: rows=%llu cols=%llu must be multiples of 4", (unsigned long long)rows,
                (unsigned long long)cols);
    CLV_REQUIRE(A != At, "clm_f32_transpose: in-place transposition is not supported");
    if (!rows || !cols) return CLV_OK;
    const uint64_t tiles_x = (cols + TR32_T - 1) / TR32_T, tiles = ((rows + TR32_T - 1) / TR32_T) * tiles_x;
    CLV_REQUIRE(tiles <= 0x7FFFFFFFull && tiles_x <= 0xFFFFFFFFull, "clm_f32_transpose: too many tiles");
    // streaming loads and stores once input + output cannot live in the Infinity Cache (the clm4_transpose rule)
    if (F32_STREAMING(rows * cols * 8))
        hipLaunchKernelGGL(k_f32_transpose<true>, dim3((unsigned)tiles), dim3(256), 0, as_stream(stream), (const uint32_t *)A, rows, cols, (uint32_t *)At,
                           (uint32_t)tiles_x);
    else
        hipLaunchKernelGGL(k_f32_transpose<false>, dim3((unsigned)tiles), dim3(256), 0, as_stream(stream), (const uint32_t *)A, rows, cols, (uint32_t *)At,
                           (uint32_t)tiles_x);
    CLV_LAUNCH_CHECK();
    return CLV_OK;
}
