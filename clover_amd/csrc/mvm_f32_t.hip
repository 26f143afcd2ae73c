// mvm_f32_t.hip -- CloverMatrix4 on fp32 vectors beyond the single product of mvm_f32.hip (include/clover_hip_m4_f32.h): the transposed
// product r = A' x straight from A's own bytes, and the entry points of the three product calls and of the IHT / GD loop of
// <CloverMatrix4, CloverVector32> in one call, with two matrices or with one.  The column walk is that of mvm_f32_t_device.h, the host side
// that of mvm_f32_host.h; this file holds what the 4-bit width puts into either: its lane map, its chain step and its launch.
//
// Contract of the transposed product: bit for bit what clm4_transpose(A -> At) followed by clm4_mvm_f32(At, cols, rows, x -> r) gives.
// Output column c is row c of A' under the definition of k_m4_mvm_f32 (mvm_f32.hip): 32 sequential fp32 fma chains, row i of A on chain
// i mod 32 in increasing i, each from +0.0f, one step acc = fma(x[i], f32((float)q(i, c) * f32(s / 7)), acc) with s read from A's OWN
// scale grid at (row tile i / 64, column tile c / 64); then (acc1 + acc2) + (acc3 + acc4) per AVX lane and the _mm256_haddf32_ps tree, as
// the last lines of k_m4_mvm_f32.  tests/m4_f32_t_restate.c states the same walk on the CPU.
//
// What the width sets (M4FTWidth); unlike k_m4_mvm_t (mvm_t4.hip), NO nibble is transposed:
//   strip     = M4FT_COLS columns = M4FT_COLS / 2 contiguous bytes of every row: ceil(cols / M4FT_COLS) workgroups.  A strip of 256 columns
//               leaves the last workgroup half outside when cols / 128 is odd (PARTIAL);
//   piece     = M4FT_WORDS dwords = 8 M4FT_WORDS columns of a row;
//   factor    = f32(s / 7) (div7);
//   (q / 16) (16 c): where every factor c of the strip's chunk survives 16 c (times16_is_finite), the nibbles are taken as q / 16 by
//               v_cvt_off_f32_i4 (unpack8_16th, common.h) and the product rounds like q * c; otherwise the chunk takes the plain conversion.
#include "mvm_f32_t_device.h"
#include "mvm_f32_host.h"
#include "clover_hip_m4_f32.h"

#ifndef M4FT_COLS
#define M4FT_COLS 128       // columns per workgroup (the maps measured: DESIGN.md 3)
#endif
#ifndef M4FT_WORDS
#define M4FT_WORDS 1        // dwords (8 columns each) per lane and row: 1, 2 or 4
#endif
#ifndef M4FT_U
#define M4FT_U 8            // 32-row blocks of matrix loads per register set = blocks issued ahead of the arithmetic
#endif

static_assert(M4FT_COLS == 64 || M4FT_COLS == 128 || M4FT_COLS == 256, "a strip is whole 64-column tiles; 256 columns are 128 B of every row");
static_assert(M4FT_WORDS == 1 || M4FT_WORDS == 2 || M4FT_WORDS == 4, "a lane loads 4, 8 or 16 bytes");

template <int W> struct m4ft_words;
template <> struct m4ft_words<1> { typedef uint32_t type; };
template <> struct m4ft_words<2> { typedef u32x2 type; };
template <> struct m4ft_words<4> { typedef u32x4 type; };

__device__ __forceinline__ uint32_t m4ft_word(uint32_t v, int) { return v; }
__device__ __forceinline__ uint32_t m4ft_word(const u32x2 &v, int i) { return v[i]; }
__device__ __forceinline__ uint32_t m4ft_word(const u32x4 &v, int i) { return v[i]; }

struct M4FTWidth {
    typedef m4ft_words<M4FT_WORDS>::type piece;
    static constexpr int NACC = 8 * M4FT_WORDS, COLS = M4FT_COLS;
    static constexpr uint32_t CHUNK = CLM4_F32_T_CHUNK;
    static constexpr bool PARTIAL = M4FT_COLS > 128;     // cols % 128 == 0 makes narrower strips whole
    static constexpr bool CLAMP_TILE = true;             // at every strip width, as the kernel has been measured
    static constexpr bool HAS_FAST = true;
    static __device__ __forceinline__ float factor(float s) { return div7(s); }
    static __device__ __forceinline__ bool fast_ok(float c) { return times16_is_finite(c); }
    template <bool FAST> static __device__ __forceinline__ void step(const piece &a, float xv, float c, float (&acc)[NACC])
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
};

// FUSE... = nothing or one M4F32Fuse, as k_m4_mvm_f32 (mvm_f32.hip).  r (t of the fused ABI) may be NULL under FUSE; fuse.r2 may be fuse.u
template <int U, bool NT, typename... FUSE>
__global__ __launch_bounds__(MvmF32T<M4FTWidth>::THREADS) void k_m4_mvm_f32_t(const uint8_t *__restrict__ A, const float *__restrict__ sA, uint64_t rows,
                                                                              uint64_t cols, const float *__restrict__ x, float *__restrict__ r,
                                                                              FUSE... fuse)
{
    mvm_f32_t_walk<M4FTWidth, U, NT>(A, sA, rows, cols, x, r, fuse...);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
struct M4F32 {
    static uint64_t matrix_bytes(uint64_t rows, uint64_t cols) { return rows * (cols / 2); }
    static constexpr uint64_t max_elements = 0xFFFFFFFFFFFFull;
    static bool streaming(uint64_t rows, uint64_t cols) { return m4f32_streaming(rows, cols); }
    static constexpr auto row_major_fused = clv_internal_m4_mvm_f32_fused;
    static constexpr auto scale_and_add = clm4_mvm_f32_scale_and_add, transposed_scale_and_add = clm4_mvm_f32_transposed_scale_and_add;
    template <typename... FUSE>
    static int transposed_launch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, float *r, hipStream_t st, FUSE... fuse)
    {
        const dim3 grid((unsigned)((cols + M4FT_COLS - 1) / M4FT_COLS)), block(MvmF32T<M4FTWidth>::THREADS);
        if (streaming(rows, cols))
            hipLaunchKernelGGL((k_m4_mvm_f32_t<M4FT_U, true, FUSE...>), grid, block, 0, st, (const uint8_t *)A, sA, rows, cols, x, r, fuse...);
        else
            hipLaunchKernelGGL((k_m4_mvm_f32_t<M4FT_U, false, FUSE...>), grid, block, 0, st, (const uint8_t *)A, sA, rows, cols, x, r, fuse...);
        CLV_LAUNCH_CHECK();
        return CLV_OK;
    }
};

extern "C" int clm4_mvm_f32_scale_and_add(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, const float *u, float a,
                                          float *t, float *r2, void *stream)
{
    return mvm_f32_fused_entry<M4F32>("clm4_mvm_f32_scale_and_add", A, sA, rows, cols, x, u, a, t, r2, stream);
}

extern "C" int clm4_mvm_f32_transposed(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, float *r, void *stream)
{
    return mvm_f32_t_entry<M4F32>("clm4_mvm_f32_transposed", A, sA, rows, cols, x, r, stream);
}

extern "C" int clm4_mvm_f32_transposed_scale_and_add(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const float *x, const float *u,
                                                     float a, float *t, float *r2, void *stream)
{
    return mvm_f32_t_fused_entry<M4F32>("clm4_mvm_f32_transposed_scale_and_add", A, sA, rows, cols, x, u, a, t, r2, stream);
}

extern "C" int clm4_iht_f32(const int8_t *Phi, const float *sPhi, const int8_t *PhiT, const float *sPhiT, uint64_t m, uint64_t n, float *x,
                            uint64_t x_len, const float *y, float *t1, float *t2, float *t3, uint64_t iterations, uint64_t K, float mu, int threshold,
                            void *stream)
{
    return mvm_f32_iht<M4F32>("clm4_iht_f32", Phi, sPhi, PhiT, sPhiT, false, m, n, x, x_len, y, t1, t2, t3, iterations, K, mu, threshold, stream);
}

extern "C" int clm4_iht_f32_one_matrix(const int8_t *Phi, const float *sPhi, uint64_t m, uint64_t n, float *x, uint64_t x_len, const float *y, float *t1,
                                       float *t2, float *t3, uint64_t iterations, uint64_t K, float mu, int threshold, void *stream)
{
    return mvm_f32_iht<M4F32>("clm4_iht_f32_one_matrix", Phi, sPhi, nullptr, nullptr, true, m, n, x, x_len, y, t1, t2, t3, iterations, K, mu, threshold,
                              stream);
}
