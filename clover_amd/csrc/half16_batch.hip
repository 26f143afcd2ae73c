// half16_batch.hip -- CloverMatrix16 x CloverVector16 for several right-hand sides: ONE pass over the half-precision matrix for up to
// CLM4_MVM_BATCH_MAX vectors, as matrix8_batch.hip does for the 8-bit matrix.  include/clover_hip_batch_f16.h is the contract.
//
// The half-precision pair has no scales, no re-quantisation across a block and no generator: a row is 32 sequential fp32 fma chains and one
// fixed tree (f16_chain_step, f16_chain_tree, half16_device.h), and no row depends on another.  The batched kernel loads each 16 matrix
// bytes of a lane once, widens them once and runs, per vector, one 16-byte LDS read of x and the 8 fmas of f16_chain_step on the lane's 8
// chains: per vector the instruction sequence of k_f16_mvm (half16.hip), so the results equal the single calls bit for bit.
//
// The host side is half16_batch_host.h, shared with the transposed family (half16_t_batch.hip) and a driver of its own beside that of the
// other families (mvm_batch_host.h carries scale pointers and draw positions throughout); it shares with them mvm_batch_forced(), the
// overlap check, the launch counter and CLM4_MVM_BATCH_MAX.  The traits of this family, F16Batch, are declared there.
#include "half16_batch_host.h"

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

// ---- launches: declared in half16_batch_host.h, instantiated here for the driver's NV = 2, 4, 8 ----------------------------------------
template <int NV, int WAVES>
static void f16_batch_launch_form(hipStream_t st, const uint16_t *A, uint64_t rows, uint64_t cols, int nv, const F16BatchArgs<NV> &arg,
                                  const F16BatchFuse<NV> &fuse, bool fused)
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

// the kernel's two argument structs from the slots; the workgroup form by the rule of the single calls (f16_mvm_wide)
template <int NV>
void F16Batch::launch(hipStream_t st, const uint16_t *A, uint64_t rows, uint64_t cols, int nv, const F16BatchSlots<NV> &s)
{
    F16BatchArgs<NV> arg;
    F16BatchFuse<NV> fuse;
    for (int i = 0; i < NV; i++) {
        arg.x[i] = s.x[i];
        arg.r[i] = s.r[i];
        fuse.u[i] = s.u[i];
        fuse.r2[i] = s.r2[i];
    }
    fuse.a = s.a;
    if (f16_mvm_wide(rows)) f16_batch_launch_form<NV, 4>(st, A, rows, cols, nv, arg, fuse, s.fused);
    else f16_batch_launch_form<NV, 1>(st, A, rows, cols, nv, arg, fuse, s.fused);
}
template void F16Batch::launch<2>(hipStream_t, const uint16_t *, uint64_t, uint64_t, int, const F16BatchSlots<2> &);
template void F16Batch::launch<4>(hipStream_t, const uint16_t *, uint64_t, uint64_t, int, const F16BatchSlots<4> &);
template void F16Batch::launch<8>(hipStream_t, const uint16_t *, uint64_t, uint64_t, int, const F16BatchSlots<8> &);

// ---- C ABI (include/clover_hip_batch_f16.h) ------------------------------------------------------------------------------------------
extern "C" int clm_f16_mvm_batch(const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t nvec, const uint16_t *const *x, uint16_t *const *r,
                                 void *stream)
{
    return f16_batch_entry<F16Batch>("clm_f16_mvm_batch", A, rows, cols, nvec, x, r, stream);
}

extern "C" int clm_f16_mvm_scale_and_add_batch(const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t nvec, const uint16_t *const *x,
                                               const uint16_t *const *u, float a, uint16_t *const *t, uint16_t *const *r, void *stream)
{
    return f16_batch_fused_entry<F16Batch>("clm_f16_mvm_scale_and_add_batch", A, rows, cols, nvec, x, u, a, t, r, stream);
}

// Q_IHT / Q_GD for nvec signals with Phi and a held PhiT (f16_batch_iht, half16_batch_host.h)
extern "C" int clm_f16_iht_batch(const uint16_t *Phi, const uint16_t *PhiT, uint64_t m, uint64_t n, uint64_t nvec, uint16_t *const *x, uint64_t x_len,
                                 const uint16_t *const *y, uint16_t *const *t1, uint16_t *const *t2, uint16_t *const *t3, uint64_t iterations,
                                 uint64_t K, float mu, int threshold, void *stream)
{
    return f16_batch_iht<F16Batch>("clm_f16_iht_batch", Phi, PhiT, m, n, nvec, x, x_len, y, t1, t2, t3, iterations, K, mu, threshold, stream);
}
