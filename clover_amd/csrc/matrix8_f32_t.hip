// matrix8_f32_t.hip -- CloverMatrix8 on fp32 vectors beyond the single product of matrix8.hip (include/clover_hip_m8_f32.h): the transposed
// product r = A' x straight from A's own bytes, and the entry points of the three product calls and of the IHT / GD loop of
// <CloverMatrix8, CloverVector32> in one call, with two matrices or with one.  The column walk is that of mvm_f32_t_device.h, the host side
// that of mvm_f32_host.h; this file holds what the 8-bit width puts into either: its lane map, its chain step and its launch.
//
// Contract of the transposed product: bit for bit what clm8_transpose(A -> At) followed by clm8_mvm_f32(At, cols, rows, x -> r) gives.
// Output column c is row c of A' under the definition of k_m8_mvm_f32 (matrix8.hip): 32 sequential fp32 fma chains, row i of A on chain
// i mod 32 in increasing i, each from +0.0f, one step acc = fma(f32(x[i] * f32(s / 127.0f)), (float)q(i, c), acc) with s read from A's OWN
// scale grid at (row tile i / 64, column tile c / 64) -- the scale multiplies x, not q; then (acc1 + acc2) + (acc3 + acc4) per AVX lane and
// the _mm256_haddf32_ps tree, as the last lines of k_m8_mvm_f32.  tests/m8_f32_t_restate.c states the same walk on the CPU.
//
// What the width sets (M8FTWidth); unlike k_m8_mvm_t (matrix8_t.hip), no byte is transposed and no sdot4 is used:
//   strip     = M8FT_COLS columns = M8FT_COLS contiguous bytes of every row (128: one whole 128-byte line): cols / M8FT_COLS workgroups, all
//               whole, so nothing is masked and no tile index clamped;
//   piece     = ONE 16-byte load = 16 columns of a row; a wave's load instruction reads 8 rows x 128 B;
//   factor    = f32(s / 127.0f), the expression of k_m8_mvm_f32;
//   step      = one multiply t = x * f, then 16 converts and 16 fmas; no fast path, a plain barrier behind the staging;
//   bytes     = (float)(int8_t) of the stored byte: -128 is a legal byte and converts exactly.
#include "mvm_f32_t_device.h"
#include "mvm_f32_host.h"
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

static_assert(M8FT_COLS == 64 || M8FT_COLS == 128, "a strip is whole 64-column tiles and divides cols (a multiple of 128)");

// byte e (0..3) of a dword as a float, exactly, -128 included
__device__ __forceinline__ float m8ft_byte(uint32_t w, int e)
{
#if M8FT_CVT == 1
    return (float)(((w ^ 0x80808080u) >> (8 * e)) & 0xFFu) - 128.0f;
#else
    return (float)((int)(w << (24 - 8 * e)) >> 24);
#endif
}

struct M8FTWidth {
    typedef u32x4 piece;
    static constexpr int NACC = 16, COLS = M8FT_COLS;
    static constexpr uint32_t CHUNK = CLM8_F32_T_CHUNK;
    static constexpr bool PARTIAL = false, CLAMP_TILE = false, HAS_FAST = false;
    static __device__ __forceinline__ float factor(float s) { return s / 127.0f; }
    template <bool> static __device__ __forceinline__ void step(const piece &a, float xv, float c, float (&acc)[NACC])
    {
        const float t = xv * c;
#pragma unroll
        for (int w = 0; w < 4; w++)
#pragma unroll
            for (int e = 0; e < 4; e++) acc[4 * w + e] = __builtin_fmaf(t, m8ft_byte(a[w], e), acc[4 * w + e]);
    }
};

// FUSE... = nothing or one M4F32Fuse, as k_m8_mvm_f32 (matrix8.hip).  r (t of the fused ABI) may be NULL under FUSE; fuse.r2 may be fuse.u
template <int U, bool NT, typename... FUSE>
__global__ __launch_bounds__(MvmF32T<M8FTWidth>::THREADS) void k_m8_mvm_f32_t(const uint8_t *__restrict__ A, const float *__restrict__ sA, uint64_t rows,
                                                                              uint64_t cols, const float *__restrict__ x, float *__restrict__ r,
                                                                              FUSE... fuse)
{
    mvm_f32_t_walk<M8FTWidth, U, NT>(A, sA, rows, cols, x, r, fuse...);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
struct M8F32 {
    static uint64_t matrix_bytes(uint64_t rows, uint64_t cols) { return rows * cols; }
    static constexpr uint64_t max_elements = 0x1000000000000ull;
    static bool streaming(uint64_t rows, uint64_t cols) { return m8f32_streaming(rows, cols); }
    static constexpr auto row_major_fused = clv_internal_m8_mvm_f32_fused;
    static constexpr auto scale_and_add = clm8_mvm_f32_scale_and_add, transposed_scale_and_add = clm8_mvm_f32_transposed_scale_and_add;
    template <typename... FUSE>
    static int transposed_launch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, float *r, hipStream_t st, FUSE... fuse)
    {
        const dim3 grid((unsigned)(cols / M8FT_COLS)), block(MvmF32T<M8FTWidth>::THREADS);
        if (streaming(rows, cols))
            hipLaunchKernelGGL((k_m8_mvm_f32_t<M8FT_U, true, FUSE...>), grid, block, 0, st, (const uint8_t *)A, sA, rows, cols, x, r, fuse...);
        else
            hipLaunchKernelGGL((k_m8_mvm_f32_t<M8FT_U, false, FUSE...>), grid, block, 0, st, (const uint8_t *)A, sA, rows, cols, x, r, fuse...);
        CLV_LAUNCH_CHECK();
        return CLV_OK;
    }
};

extern "C" int clm8_mvm_f32_scale_and_add(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, const float *u, float a,
                                          float *t, float *r2, void *stream)
{
    return mvm_f32_fused_entry<M8F32>("clm8_mvm_f32_scale_and_add", A, sA, rows, cols, x, u, a, t, r2, stream);
}

extern "C" int clm8_mvm_f32_transposed(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, float *r, void *stream)
{
    return mvm_f32_t_entry<M8F32>("clm8_mvm_f32_transposed", A, sA, rows, cols, x, r, stream);
}

extern "C" int clm8_mvm_f32_transposed_scale_and_add(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, const float *u,
                                                     float a, float *t, float *r2, void *stream)
{
    return mvm_f32_t_fused_entry<M8F32>("clm8_mvm_f32_transposed_scale_and_add", A, sA, rows, cols, x, u, a, t, r2, stream);
}

extern "C" int clm8_iht_f32(const int8_t *Phi, const float *sPhi, const int8_t *PhiT, const float *sPhiT, uint64_t m, uint64_t n, float *x,
                            uint64_t x_len, const float *y, float *t1, float *t2, float *t3, uint64_t iterations, uint64_t K, float mu, int threshold,
                            void *stream)
{
    return mvm_f32_iht<M8F32>("clm8_iht_f32", Phi, sPhi, PhiT, sPhiT, false, m, n, x, x_len, y, t1, t2, t3, iterations, K, mu, threshold, stream);
}

extern "C" int clm8_iht_f32_one_matrix(const int8_t *Phi, const float *sPhi, uint64_t m, uint64_t n, float *x, uint64_t x_len, const float *y, float *t1,
                                       float *t2, float *t3, uint64_t iterations, uint64_t K, float mu, int threshold, void *stream)
{
    return mvm_f32_iht<M8F32>("clm8_iht_f32_one_matrix", Phi, sPhi, nullptr, nullptr, true, m, n, x, x_len, y, t1, t2, t3, iterations, K, mu, threshold,
                              stream);
}
