// half16_batch.hip -- CloverMatrix16 x CloverVector16 for several right-hand sides: ONE pass over the half-precision matrix for up to
// CLM4_MVM_BATCH_MAX vectors, as matrix8_batch.hip does for the 8-bit matrix.  include/clover_hip_batch_f16.h is the contract.
//
// The half-precision pair has no scales, no re-quantisation across a block and no generator: a row is 32 sequential fp32 fma chains and one
// fixed tree (f16_chain_step, f16_chain_tree, half16_device.h), and no row depends on another.  The batched kernel loads each 16 matrix
// bytes of a lane once, widens them once and runs, per vector, one 16-byte LDS read of x and the 8 fmas of f16_chain_step on the lane's 8
// chains: per vector the instruction sequence of k_f16_mvm (half16.hip), so the results equal the single calls bit for bit.
//
// The host side is a small driver of its own (the driver of the other families, mvm_batch_host.h, carries scale pointers and draw positions
// throughout); it shares with them mvm_batch_forced(), the overlap check, the launch counter and CLM4_MVM_BATCH_MAX.
#include "half16_batch.h"
#include "mvm_batch_host.h"

#include "clover_hip_batch_f16.h"

// Columns of x staged in LDS per pass: 512 per wave of the workgroup, i.e. every thread stages ONE 16-byte piece per vector and chunk in
// either workgroup form.  The 64-row form holds 4 KiB of binary16 per vector, 32 KiB at NV = 8 -- by LDS alone five workgroups per CU, one
// more than the four the registers of the NV = 8 instantiation allow; the 16-row form 1 KiB per vector, 8 KiB at NV = 8, so that LDS
// never limits its one-wave workgroups either (figures: DESIGN.md 3).  The 16 KiB per vector of k_f16_mvm would be 128 KiB at NV = 8, one
// workgroup per CU.  A row's chains run over the columns in order whatever the chunk is: the bits do not depend on it.  The values were
// chosen by that budget and have not been swept.
#define F16B_CHUNK(WAVES) (512u * (WAVES))
// 16-byte matrix requests in flight per lane: 8 as in k_f16_mvm while the accumulators leave room, 4 at NV = 8 (64 accumulators)
#define F16B_U(NV) ((NV) == 8 ? 4 : 8)

// the vectors of one launch, by value in the kernel arguments.  r: the f16 A x[v] (under FUSE: t of the ABI, NULL = not stored)
template <int NV>
struct F16BatchArgs {
    const uint16_t *x[NV];
    uint16_t *r[NV];
};
// FUSE: r2[v][row] = f16(fma(f32(f16(A x[v])), a, f32(u[v][row]))); r2[v] may be u[v]
template <int NV>
struct F16BatchFuse {
    const uint16_t *u[NV];
    uint16_t *r2[NV];
    float a;
};

// U steps (32 columns each) of this lane's row for every vector of the group: each matrix load and its widening ONCE, then per vector the
// fmas of f16_chain_step with x read from LDS as binary16 and widened in the lane.  x stays binary16 in LDS: staged already widened it
// would double the LDS reads, which at NV = 8 are the other resource this loop runs close to; the widening is exact either
// way and neither form has been timed against the other.  The mixed-precision fma (v_fma_mix_f32) is not used: hipcc selects it only with
// fp32 denormals flushed (half16.hip), and its bits on subnormal operands have not been checked on this chip.
template <int NV, int U, bool NT, uint32_t XS>
__device__ __forceinline__ void f16b_steps(const h16x8 *__restrict__ Ap, const h16x8 *xs, int p, uint32_t t0, int nv, float (&acc)[NV][8])
{
    h16x8 a[U];                                               // XS: h16x8 of x per vector in LDS
#pragma unroll
    for (int u = 0; u < U; u++) a[u] = ld_stream<NT>(&Ap[4 * (t0 + u) + p]);
#pragma unroll
    for (int u = 0; u < U; u++) {
        float af[8];
#pragma unroll
        for (int l = 0; l < 8; l++) af[l] = (float)a[u][l];
#pragma unroll
        for (int v = 0; v < NV; v++)
            if (v < nv) {
                const h16x8 x = xs[v * XS + 4 * (t0 + u) + p];
#pragma unroll
                for (int l = 0; l < 8; l++) acc[v][l] = __builtin_fmaf((float)x[l], af[l], acc[v][l]);
            }
    }
}

// The row mapping of k_f16_mvm: workgroup = 16 * WAVES rows, a quad of lanes per row, lane p keeps chains 8p .. 8p + 7 -- here of every
// vector, NV x 8 accumulators.  Rows beyond `rows` (a workgroup's tail; any row count is a row shard) re-read the last row and store
// nothing.  Slots v >= nv are absent: never staged, never accumulated, never stored.  cols is a multiple of 128, so a chunk is a multiple
// of 4 steps.  amdgpu_waves_per_eu(4) holds the NV = 8 instantiations to 128 registers (four waves per SIMD; left alone hipcc took 140 to
// 180 and two or three waves); NV = 2 and 4 stay below that by themselves.
template <int NV, int WAVES, bool NT, bool FUSE>
__global__ __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(4))) void k_f16_mvm_batch(
    const uint16_t *__restrict__ A, uint64_t rows, uint64_t cols, int nv, F16BatchArgs<NV> arg, F16BatchFuse<NV> fuse)
{
    constexpr int THREADS = 64 * WAVES, U = F16B_U(NV);
    constexpr uint32_t CH = F16B_CHUNK(WAVES), XS = CH / 8;   // columns per chunk; h16x8 (16-byte pieces) of x per vector and chunk
    static_assert(XS == THREADS && U % 4 == 0, "one piece per thread, vector and chunk; the tail loop takes 4 steps");
    __shared__ __attribute__((aligned(16))) h16x8 xs[NV * XS];
    const int tid = threadIdx.x, p = tid & 3, rho = tid >> 2;
    const uint64_t row = (uint64_t)blockIdx.x * (16 * WAVES) + rho;
    const h16x8 *Arow = reinterpret_cast<const h16x8 *>(A + (row < rows ? row : rows - 1) * cols);
    float acc[NV][8];
    uint16_t fuse_u[NV];
#pragma unroll
    for (int v = 0; v < NV; v++) {
#pragma unroll
        for (int l = 0; l < 8; l++) acc[v][l] = 0.0f;
        fuse_u[v] = 0;
        // ahead of the streaming loop, as k_f16_mvm: the epilogue waits on nothing, and the lane that writes r2[v][row] has read u[v][row]
        if (FUSE && v < nv && p == 0 && row < rows) fuse_u[v] = fuse.u[v][row];
    }

    for (uint64_t c0 = 0; c0 < cols; c0 += CH) {
        const uint32_t cw = (uint32_t)((cols - c0) < CH ? (cols - c0) : CH);
        if (c0) __syncthreads();
        {   // four vectors at a time (16 registers beside the accumulators): their loads first (one round trip), then their LDS writes
            const uint32_t n16 = cw / 8, ix = (uint32_t)tid < n16 ? tid : 0;
#pragma unroll
            for (int v0 = 0; v0 < NV; v0 += 4) {
                constexpr int NG = NV < 4 ? NV : 4;
                u32x4 xr[NG];
#pragma unroll
                for (int k = 0; k < NG; k++)
                    if (v0 + k < nv) xr[k] = reinterpret_cast<const u32x4 *>(arg.x[v0 + k] + c0)[ix];
#pragma unroll
                for (int k = 0; k < NG; k++)
                    if (v0 + k < nv && (uint32_t)tid < n16) reinterpret_cast<u32x4 *>(xs)[(v0 + k) * XS + tid] = xr[k];
            }
        }
        __syncthreads();
        const h16x8 *Ap = Arow + c0 / 8;
        const uint32_t nsteps = cw / 32;
        uint32_t t = 0;
        if (U > 4)
            for (; t + U <= nsteps; t += U) f16b_steps<NV, U, NT, XS>(Ap, xs, p, t, nv, acc);
        for (; t < nsteps; t += 4) f16b_steps<NV, 4, NT, XS>(Ap, xs, p, t, nv, acc);
    }

#pragma unroll
    for (int v = 0; v < NV; v++)
        if (v < nv) {
            const float d = f16_chain_tree(acc[v]);
            if (p == 0 && row < rows) {
                if (FUSE) f16_fuse_store(arg.r[v], row, d, fuse_u[v], F16Fuse{fuse.u[v], fuse.a, fuse.r2[v]});
                else arg.r[v][row] = f16_bits(d);                        // _mm256_cvtps_ph(.., 0) of the row block, as k_f16_mvm
            }
        }
}

// ---- host driver (F16BatchVectors, the vectors of a call: half16_batch.h) ------------------------------------------------------
template <int NV, int WAVES>
static void f16_batch_launch_form(const uint16_t *A, uint64_t rows, uint64_t cols, int nv, const F16BatchArgs<NV> &arg, const F16BatchFuse<NV> &fuse,
                                  bool fused, hipStream_t st)
{
    const dim3 grid((unsigned)((rows + 16 * WAVES - 1) / (16 * WAVES))), block(64 * WAVES);
    // nontemporal loads by the rule of the single calls: once the matrix cannot live in the 256 MiB Infinity Cache
    const bool nt = F16_STREAMING(rows * cols * 2);
    switch (2 * nt + fused) {
    case 3: hipLaunchKernelGGL((k_f16_mvm_batch<NV, WAVES, true, true>), grid, block, 0, st, A, rows, cols, nv, arg, fuse); break;
    case 2: hipLaunchKernelGGL((k_f16_mvm_batch<NV, WAVES, true, false>), grid, block, 0, st, A, rows, cols, nv, arg, fuse); break;
    case 1: hipLaunchKernelGGL((k_f16_mvm_batch<NV, WAVES, false, true>), grid, block, 0, st, A, rows, cols, nv, arg, fuse); break;
    default: hipLaunchKernelGGL((k_f16_mvm_batch<NV, WAVES, false, false>), grid, block, 0, st, A, rows, cols, nv, arg, fuse); break;
    }
}

// one launch for the first g <= NV vectors of v; the workgroup form by the rule of the single calls (f16_mvm_wide)
template <int NV>
static int f16_batch_launch(const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t g, const F16BatchVectors &v, hipStream_t st)
{
    F16BatchArgs<NV> arg;
    F16BatchFuse<NV> fuse;
    const bool fused = v.u != nullptr;
    for (uint64_t i = 0; i < NV; i++) {
        const bool in = i < g;
        arg.x[i] = in ? v.x[i] : nullptr;
        arg.r[i] = !in ? nullptr : fused ? (v.t ? v.t[i] : nullptr) : v.r[i];
        fuse.u[i] = in && fused ? v.u[i] : nullptr;
        fuse.r2[i] = in && fused ? v.r[i] : nullptr;
    }
    fuse.a = v.a;
    if (f16_mvm_wide(rows)) f16_batch_launch_form<NV, 4>(A, rows, cols, (int)g, arg, fuse, fused, st);
    else f16_batch_launch_form<NV, 1>(A, rows, cols, (int)g, arg, fuse, fused, st);
    CLV_LAUNCH_CHECK();
    clv_internal_mvm_batch_count();
    return CLV_OK;
}

// a group of g <= CLM4_MVM_BATCH_MAX vectors on the smallest instantiation that holds it (half16_t_batch.hip runs step 1 of its loop on it)
int f16_batch_launch_group(const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t g, const F16BatchVectors &v, hipStream_t st)
{
    return g <= 2 ? f16_batch_launch<2>(A, rows, cols, g, v, st) : g <= 4 ? f16_batch_launch<4>(A, rows, cols, g, v, st) : f16_batch_launch<8>(A, rows, cols, g, v, st);
}

// Whether a group of g vectors of a call of two or more runs as one batched launch or as g single launches.  CLV_MVM_BATCH = 1 / 0 forces
// one or the other for every group -- forced to 1 a remainder group of ONE vector (nvec = 9, 17, ...) runs batched too, so that a forced
// call is ceil(nvec / 8) batched launches and nothing else.  Unset = the rule measured on the MI355X ("Several vectors, one
// CloverMatrix16 pass"; profiles/f16_mvm_batch_kernel_bench.json, profiles/f16_mvm_batch_groups_kernel_bench.json): batched exactly where
// the batched launch beat the single calls by more than their spread --
//   a streaming matrix (above the 256 MiB rule; 65536^2 and 32768^2): every group of two or more (2: 1.95 x ... 8: 4.1 - 5.1 x);
//   a cache-resident one (the fused step at 8192 x 4096, 64 MiB): groups of three or more (3: 1.03 x, 4: 1.17, 8: 1.28); TWO vectors lost
//   to the two single calls (0.95 x) and are forwarded.
// Not measured: matrices between 64 MiB and 1 GiB, below 64 MiB, and streaming matrices of fewer than 32768 rows (the 16-row form).
static bool f16_batch_selected(uint64_t g, uint64_t rows, uint64_t cols)
{
    const int force = mvm_batch_forced();
    if (force >= 0) return force != 0;
    return g >= (F16_STREAMING(rows * cols * 2) ? 2u : 3u);
}

// the checked arguments of clm_f16_mvm_batch (v.u == NULL) / clm_f16_mvm_scale_and_add_batch on the stream, group by group
static int f16_batch_run(const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t nvec, const F16BatchVectors &v, void *stream)
{
    for (uint64_t j0 = 0; j0 < nvec; j0 += CLM4_MVM_BATCH_MAX) {
        const uint64_t g = nvec - j0 < CLM4_MVM_BATCH_MAX ? nvec - j0 : CLM4_MVM_BATCH_MAX;
        int rc = CLV_OK;
        if (!f16_batch_selected(g, rows, cols)) {
            for (uint64_t j = j0; j < j0 + g && !rc; j++)
                rc = v.u ? clm_f16_mvm_scale_and_add(A, rows, cols, v.x[j], v.u[j], v.a, v.t ? v.t[j] : nullptr, v.r[j], stream)
                         : clm_f16_mvm(A, rows, cols, v.x[j], v.r[j], stream);
        } else {
            rc = f16_batch_launch_group(A, rows, cols, g, v.from(j0), as_stream(stream));
        }
        if (rc) return rc;
    }
    return CLV_OK;
}

// every check of the two mvm batch calls, before any device work: the single calls' size and alignment rules, then the arrays, the
// entries, the aliases the single calls refuse by name and the overlap check.  u == NULL and t == NULL in the plain call.
static int f16_batch_check_args(const char *fn, const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t nvec, const uint16_t *const *x,
                                const uint16_t *const *u, uint16_t *const *t, uint16_t *const *r, bool fused)
{
    CLV_REQUIRE(A, "%s: null pointer", fn);
    CLV_REQUIRE(F16_ALIGNED(A), "%s: the matrix and x must be 16-byte aligned", fn);
    CLV_REQUIRE(cols % 128 == 0, "%s: cols=%llu must be a multiple of 128", fn, (unsigned long long)cols);
    CLV_REQUIRE(rows / 16 < 0x7FFFFFFFull, "%s: matrix too large", fn);
    if (!nvec) return CLV_OK;
    CLV_REQUIRE(x && r && (!fused || u), "%s: null pointer array", fn);
    for (uint64_t j = 0; j < nvec; j++)
        CLV_REQUIRE(x[j] && r[j] && (!fused || u[j]) && (!t || t[j]), "%s: null pointer in vector %llu", fn, (unsigned long long)j);
    for (uint64_t j = 0; j < nvec; j++) {
        CLV_REQUIRE(F16_ALIGNED(x[j]), "%s: the matrix and x must be 16-byte aligned (x of vector %llu)", fn, (unsigned long long)j);
        CLV_REQUIRE(((uintptr_t)r[j] & 1u) == 0 && (!fused || ((uintptr_t)u[j] & 1u) == 0) && (!t || ((uintptr_t)t[j] & 1u) == 0),
                    "%s: u, t and r must be 2-byte aligned (vector %llu)", fn, (unsigned long long)j);
        CLV_REQUIRE(r[j] != x[j] && (!t || t[j] != x[j]), "%s: the results of vector %llu must not alias the vector being multiplied", fn,
                    (unsigned long long)j);
        CLV_REQUIRE(!t || (t[j] != r[j] && t[j] != u[j]), "%s: t of vector %llu must not alias r or u", fn, (unsigned long long)j);
    }
    std::vector<ClvRange> rg;
    rg.reserve(4 * nvec + 1);
    const uint64_t xb = cols * 2, rb = rows * 2;
    rg.push_back(clv_range(A, rows * cols * 2, false, ~0ull, "A"));
    for (uint64_t j = 0; j < nvec; j++) {
        rg.push_back(clv_range(x[j], xb, false, j, "x"));
        rg.push_back(clv_range(r[j], rb, true, j, "r"));
        // the in-place form r[j] == u[j]: the result IS the input, only the lane that owns a row touches it in either
        if (fused && r[j] != u[j]) rg.push_back(clv_range(u[j], rb, false, j, "u"));
        if (t) rg.push_back(clv_range(t[j], rb, true, j, "t"));
    }
    return clv_internal_check_ranges(fn, rg);
}

// ---- C ABI -------------------------------------------------------------------------------------------------------------------
extern "C" int clm_f16_mvm_batch(const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t nvec, const uint16_t *const *x, uint16_t *const *r,
                                 void *stream)
{
    int rc = f16_batch_check_args("clm_f16_mvm_batch", A, rows, cols, nvec, x, nullptr, nullptr, r, false);
    if (rc) return rc;
    if (!nvec || !rows) return CLV_OK;
    if (nvec == 1) return clm_f16_mvm(A, rows, cols, x[0], r[0], stream);
    return f16_batch_run(A, rows, cols, nvec, {x, nullptr, 0.0f, nullptr, r}, stream);
}

extern "C" int clm_f16_mvm_scale_and_add_batch(const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t nvec, const uint16_t *const *x,
                                               const uint16_t *const *u, float a, uint16_t *const *t, uint16_t *const *r, void *stream)
{
    int rc = f16_batch_check_args("clm_f16_mvm_scale_and_add_batch", A, rows, cols, nvec, x, u, t, r, true);
    if (rc) return rc;
    if (!nvec || !rows) return CLV_OK;
    if (nvec == 1) return clm_f16_mvm_scale_and_add(A, rows, cols, x[0], u[0], a, t ? t[0] : nullptr, r[0], stream);
    return f16_batch_run(A, rows, cols, nvec, {x, u, a, t, r}, stream);
}

// Q_IHT / Q_GD for nvec signals with one Phi: the loop of clm_f16_iht (half16.hip) with every step batched.  Per iteration and group two
// fused launches and, with a threshold, one clv_f16_threshold_batch.  Bit-identical to clm_f16_iht per signal.
#define F16_IHTB "clm_f16_iht_batch"
extern "C" int clm_f16_iht_batch(const uint16_t *Phi, const uint16_t *PhiT, uint64_t m, uint64_t n, uint64_t nvec, uint16_t *const *x, uint64_t x_len,
                                 const uint16_t *const *y, uint16_t *const *t1, uint16_t *const *t2, uint16_t *const *t3, uint64_t iterations,
                                 uint64_t K, float mu, int threshold, void *stream)
{
    CLV_REQUIRE(Phi && PhiT, F16_IHTB ": null pointer");
    CLV_REQUIRE(m % 128 == 0 && n % 128 == 0 && x_len <= n, F16_IHTB ": m=%llu n=%llu x_len=%llu", (unsigned long long)m, (unsigned long long)n,
                (unsigned long long)x_len);
    CLV_REQUIRE(threshold >= 0 && threshold <= 2, F16_IHTB ": unknown threshold %d", threshold);
    CLV_REQUIRE(F16_ALIGNED(Phi) && F16_ALIGNED(PhiT), F16_IHTB ": the matrices, x and t2 must be 16-byte aligned");
    CLV_REQUIRE(m / 16 < 0x7FFFFFFFull && n / 16 < 0x7FFFFFFFull, F16_IHTB ": matrix too large");
    if (!nvec) return CLV_OK;
    CLV_REQUIRE(x && y && t1 && t2 && t3, F16_IHTB ": null pointer array");
    for (uint64_t j = 0; j < nvec; j++)
        CLV_REQUIRE(x[j] && y[j] && t1[j] && t2[j] && t3[j], F16_IHTB ": null pointer in vector %llu", (unsigned long long)j);
    for (uint64_t j = 0; j < nvec; j++) {
        CLV_REQUIRE(F16_ALIGNED(x[j]) && F16_ALIGNED(t2[j]), F16_IHTB ": the matrices, x and t2 must be 16-byte aligned (vector %llu)",
                    (unsigned long long)j);
        CLV_REQUIRE((((uintptr_t)y[j] | (uintptr_t)t1[j] | (uintptr_t)t3[j]) & 1u) == 0, F16_IHTB ": y, t1 and t3 must be 2-byte aligned (vector %llu)",
                    (unsigned long long)j);
    }
    {   // the range check of mvm_batch_iht without its scale arrays
        std::vector<ClvRange> rg;
        rg.reserve(5 * nvec + 2);
        const uint64_t mb = m * 2, nb = n * 2;
        rg.push_back(clv_range(Phi, m * n * 2, false, ~0ull, "Phi"));
        rg.push_back(clv_range(PhiT, m * n * 2, false, ~0ull, "PhiT"));
        for (uint64_t j = 0; j < nvec; j++) {
            rg.push_back(clv_range(y[j], mb, false, j, "y"));
            rg.push_back(clv_range(x[j], nb, true, j, "x"));
            rg.push_back(clv_range(t1[j], mb, true, j, "t1"));
            rg.push_back(clv_range(t2[j], mb, true, j, "t2"));
            rg.push_back(clv_range(t3[j], nb, true, j, "t3"));
        }
        int rc = clv_internal_check_ranges(F16_IHTB, rg);
        if (rc) return rc;
    }
    const int mode = threshold == 2 ? CLV_THRESHOLD_REFERENCE : CLV_THRESHOLD_FAST;
    hipStream_t st = as_stream(stream);
    for (uint64_t j0 = 0; j0 < nvec; j0 += CLM4_MVM_BATCH_MAX) {
        const uint64_t g = nvec - j0 < CLM4_MVM_BATCH_MAX ? nvec - j0 : CLM4_MVM_BATCH_MAX;
        if (nvec == 1 || !(m && n && f16_batch_selected(g, m, n))) {      // one signal, an empty matrix, or forwarded: the single call, signal after signal
            for (uint64_t j = j0; j < j0 + g; j++) {
                int rc = clm_f16_iht(Phi, PhiT, m, n, x[j], x_len, y[j], t1[j], t2[j], t3[j], iterations, K, mu, threshold, stream);
                if (rc) return rc;
            }
            continue;
        }
        for (uint64_t j = j0; j < j0 + g; j++) {
            int rc = clv_internal_f16_clear(x[j], n, st);                                   // x.clear()
            if (rc) return rc;
        }
        const F16BatchVectors step1 = {x + j0, y + j0, -1.0f, t1 + j0, t2 + j0};            // t1 = Phi x; t2 = y - t1
        const F16BatchVectors step2 = {t2 + j0, x + j0, mu, t3 + j0, x + j0};               // t3 = Phi' t2; x += mu t3
        for (uint64_t it = 0; it < iterations; it++) {
            int rc = f16_batch_launch_group(Phi, m, n, g, step1, st);
            if (!rc) rc = f16_batch_launch_group(PhiT, n, m, g, step2, st);
            if (!rc && threshold) rc = clv_f16_threshold_batch(x + j0, g, x_len, n, K, mode, stream);      // keep the K largest
            if (rc) return rc;
        }
    }
    return CLV_OK;
}
#undef F16_IHTB
