// gemm8.hip -- CloverMatrix8 x CloverMatrix8^T and CloverMatrix4 x CloverMatrix8^T -> fp32 (and the exact int32 sums of the 8 x 8 form)
// on the gfx950 int8 matrix cores.
//
// The reference has no GEMM; semantics are build-defined ("8-bit operands"), stated as for the 4-bit GEMM:
//   C[i][j] = fold_b fmaf(c_b, (float)S_b, C),  S_b = exact int32 sum of the 64 products of K-block b,
//   8 x 8:  c_b = f32(f32(sA[i>>6][b] * 1/127) * f32(sB[j>>6][b] * 1/127))      (the factor of clm8_mvm)
//   4 x 8:  c_b = f32(f32(sA[i>>6][b] * 1/7)   * f32(sB[j>>6][b] * 1/127))      (the factor of clm4_mvm_v8)
// clm8_gemm_i32 returns the sum of S_b over a range of K-blocks.  One K-block (64 elements, one Clover scale block) is exactly one
// v_mfma_i32_16x16x64_i8, and the 8-bit format IS that instruction's operand: no re-code pass, no scratch, no workspace.
//
// One kernel template, k_gemm8<A4, I32>; tile, LDS image, fold and tile order are those of gemm4.hip (copied, that file is unchanged):
//   workgroup 512 threads = 2x4 waves, tile 128x128; wave tile 64x32 = 4x2 MFMA tiles inside ONE scale tile of A and of B, so c_b is
//   wave-uniform.  One LDS stage = 2 K-blocks, double-buffered, one barrier per stage.
//   LDS: [kblock][row][64 B] int8, 16-byte slots XOR-swizzled with swz(row, kblock) on the write AND on the fragment read, so that each
//   ds_read_b128 lane group touches 16 distinct slots.
//   byte operands: global -> registers -> LDS with 16-byte loads and stores and no VALU in between; per stage a thread moves one slot of
//   each of the two K-blocks (the four threads of a row read 64 contiguous bytes per load instruction).
//   nibble operand (A4): gemm4.hip's image, every nibble as the int8 16*q (unpack32), which permutes the 8 elements of a packed dword to
//   [e0 e2 e4 e6 | e1 e3 e5 e7]; the bytes of B get the same permutation on their way to LDS (two v_perm_b32 per 8 bytes: the integer
//   sum is order-free, the PAIRING is not).  The MFMA then returns 16*S_b (|16 S_b| <= 2^20); the 2^-4 is folded into c_b, or, for a
//   c_b so small that c_b/16 could lose bits, into the integer (wave-uniform selects, see fold_half).
//   fold (fp32 forms): the MFMA accumulates onto 0x4B400000 = 12582912.0f, where one ulp is 1: read as fp32 the result IS
//   12582912 + S_b exactly (|S_b| <= 64 * 128 * 128 = 2^20 keeps it inside [2^23, 2^24)); one exact subtract, one fma, as packed pairs.
//   int32 form (I32): the accumulators stay in the MFMA across the K-block range [kb0, kb0 + kbc); a range of odd length ends with a
//   stage whose second K-block is staged as zeros.
#include "common.h"

typedef int i32x4 __attribute__((ext_vector_type(4)));

#define G8_RCP127 (1.0f / 127.0f)        // clover_mm256_rcp_127_ps (CloverBase.h:87), CLV_RCP127 of mixed8.hip
#define G8_RCP7 (1.0f / 7.0f)            // CloverMatrix4.h:1147-1149
#define G8_BIAS_BITS 0x4B400000          // 12582912.0f
#define G8_BIAS_F 12582912.0f
#define G8_BIAS4 (i32x4{G8_BIAS_BITS, G8_BIAS_BITS, G8_BIAS_BITS, G8_BIAS_BITS})
#define G8_TILE 128
#define G8_KBS 2
#define G8_STAGE_BYTES (2 * G8_KBS * G8_TILE * 64)          // A + B, 64 int8 bytes per row and K-block
// the scheduler may not move instructions across this point: it would otherwise issue all eight MFMAs of a K-block first, and the
// whole of S beside the accumulators and the staged operands does not fit 128 registers
#define G8_KEEP_ORDER() __builtin_amdgcn_sched_barrier(0)
#define G8_MAX_KB_I32 2047ull                               // 2047 * 64 * 2^14 < 2^31

// acc[t] = fma(c, raw[t] - bias, acc[t]) for the 4 results one lane holds of a 16x16 MFMA tile, as two packed-fp32 pairs
__device__ __forceinline__ void g8_fold4(float (&acc)[4], const i32x4 raw, float c)
{
    const f32x2 bias = {G8_BIAS_F, G8_BIAS_F}, cc = {c, c};
    const f32x2 lo = {__int_as_float(raw.x), __int_as_float(raw.y)}, hi = {__int_as_float(raw.z), __int_as_float(raw.w)};
    f32x2 a0 = {acc[0], acc[1]}, a1 = {acc[2], acc[3]};
    a0 = __builtin_elementwise_fma(cc, lo - bias, a0);
    a1 = __builtin_elementwise_fma(cc, hi - bias, a1);
    acc[0] = a0.x; acc[1] = a0.y; acc[2] = a1.x; acc[3] = a1.y;
}
// the mixed form, whose raw[t] is the float 12582912 + 16 S: acc[t] = fma(c, fma(raw[t], m, -bias * m), acc[t]) with m = 1 (the inner fma is
// the exact subtraction, 16 S) or m = 1/16 (it is S: every term and the result are exact) -- the same two instructions for either
__device__ __forceinline__ void g8_fold4_scaled(float (&acc)[4], const i32x4 raw, float c, float m, float nbias)
{
    const f32x2 nb = {nbias, nbias}, cc = {c, c}, mm = {m, m};
    const f32x2 lo = {__int_as_float(raw.x), __int_as_float(raw.y)}, hi = {__int_as_float(raw.z), __int_as_float(raw.w)};
    f32x2 a0 = {acc[0], acc[1]}, a1 = {acc[2], acc[3]};
    a0 = __builtin_elementwise_fma(cc, __builtin_elementwise_fma(lo, mm, nb), a0);
    a1 = __builtin_elementwise_fma(cc, __builtin_elementwise_fma(hi, mm, nb), a1);
    acc[0] = a0.x; acc[1] = a0.y; acc[2] = a1.x; acc[3] = a1.y;
}

// f(row>>2) = {0,2,3,1} makes every ds_read_b128 lane group conflict-free; the XOR with the K-block index is constant per access
__device__ __forceinline__ int g8_swz(int row, int kb) { return ((0x1320 >> (4 * ((row >> 2) & 3))) ^ kb) & 3; }

// 16 packed bytes (32 nibbles) -> two 16-byte int8 slots (each nibble as 16*q); per dword the order becomes [e0 e2 e4 e6 | e1 e3 e5 e7]
__device__ __forceinline__ void g8_unpack32(const u32x4 p, u32x4 &s0, u32x4 &s1)
{
    const uint32_t M = 0xF0F0F0F0u;
    s0 = u32x4{p.x & M, (p.x << 4) & M, p.y & M, (p.y << 4) & M};
    s1 = u32x4{p.z & M, (p.z << 4) & M, p.w & M, (p.w << 4) & M};
}
// the same order for 16 int8 bytes that meet such a slot in the MFMA
__device__ __forceinline__ u32x4 g8_pair_order(const u32x4 b)
{
    return u32x4{__builtin_amdgcn_perm(b.y, b.x, 0x06040200u), __builtin_amdgcn_perm(b.y, b.x, 0x07050301u),
                 __builtin_amdgcn_perm(b.w, b.z, 0x06040200u), __builtin_amdgcn_perm(b.w, b.z, 0x07050301u)};
}

// c / 16 is exact unless it leaves the normal range (2^-126 * 16 = 2^-122); the margin costs nothing
__device__ __forceinline__ bool g8_sixteenth_is_exact(float c) { return __builtin_fabsf(c) >= 0x1p-100f || c == 0.0f; }

// A4: A holds packed nibbles (CloverMatrix4), else int8 (CloverMatrix8); B is int8.  I32: out = int32 sums over K-blocks [kb0, kb0 + kbc),
// else out = fp32 fold over them (the hosts pass the whole K: kb0 = 0, kbc = K / 64, even).
template <bool A4, bool I32>
__global__ __launch_bounds__(512, 4) void k_gemm8(const uint8_t *__restrict__ A, const float *__restrict__ sA, const uint8_t *__restrict__ B,
                                                  const float *__restrict__ sB, uint64_t N, uint64_t K, uint32_t kb0, uint32_t kbc,
                                                  void *__restrict__ out, uint32_t tiles_m, uint32_t tiles_n)
{
    static_assert(!(A4 && I32), "the mixed form has no int32 entry point");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    // ---- tile assignment: XCD-aware (block b runs on XCD b % 8): give each XCD a contiguous range of tiles,
    // walked in 8-wide column groups so neighbours share A rows / B columns in that XCD's L2
    const uint32_t nwg = tiles_m * tiles_n;
    uint32_t id = blockIdx.x;
    {
        const uint32_t q = nwg / 8, r = nwg % 8, xcd = id % 8, s = id / 8;
        id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + s;       // bijective for any nwg
    }
    const uint32_t GROUP = 8;
    const uint32_t per_group = GROUP * tiles_n;
    const uint32_t group = id / per_group;
    const uint32_t first_m = group * GROUP;
    const uint32_t gsize = (tiles_m - first_m) < GROUP ? (tiles_m - first_m) : GROUP;
    const uint32_t tm = first_m + (id % per_group) % gsize;
    const uint32_t tn = (id % per_group) / gsize;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;                   // 2 x 4 waves, each 64 rows x 32 columns
    const uint64_t m0 = (uint64_t)tm * G8_TILE, n0 = (uint64_t)tn * G8_TILE;
    const uint64_t kbn = K / 64;                               // K-blocks of the operands
    const uint32_t nstages = (kbc + 1) / G8_KBS;

    // staging role: row tid / 4, piece tid % 4.  Bytes: slot `piece` of both K-blocks of the stage; nibbles: 16 packed bytes = half
    // (piece & 1) of K-block (piece >> 1), as in gemm4.hip
    const int srow = tid >> 2, spiece = tid & 3;
    const uint8_t *gA = A + (m0 + srow) * (A4 ? K / 2 : K);
    const uint8_t *gB = B + (n0 + srow) * K;
    u32x4 pa[A4 ? 1 : 2], pb[2];
    auto fetch = [&](uint32_t st) {
        const uint64_t blk = (uint64_t)kb0 + (uint64_t)st * G8_KBS;
        const bool two = !I32 || 2 * st + 1 < kbc;             // the last stage of an odd range has one K-block
        const u32x4 zero = {0u, 0u, 0u, 0u};
        if (A4) pa[0] = *reinterpret_cast<const u32x4 *>(gA + blk * 32 + 16 * spiece);
        else {
            pa[0] = *reinterpret_cast<const u32x4 *>(gA + blk * 64 + 16 * spiece);
            pa[A4 ? 0 : 1] = two ? *reinterpret_cast<const u32x4 *>(gA + (blk + 1) * 64 + 16 * spiece) : zero;
        }
        pb[0] = *reinterpret_cast<const u32x4 *>(gB + blk * 64 + 16 * spiece);
        pb[1] = two ? *reinterpret_cast<const u32x4 *>(gB + (blk + 1) * 64 + 16 * spiece) : zero;
    };
    auto stash = [&](int buf) {
        char *tA = smem + buf * G8_STAGE_BYTES;
        char *tB = tA + G8_KBS * G8_TILE * 64;
        if (A4) {
            const int kb = spiece >> 1, half = spiece & 1;
            u32x4 s0, s1;
            g8_unpack32(pa[0], s0, s1);
            char *r = tA + (kb * G8_TILE + srow) * 64;
            const int f = g8_swz(srow, kb);
            *reinterpret_cast<u32x4 *>(r + (((2 * half) ^ f) << 4)) = s0;
            *reinterpret_cast<u32x4 *>(r + (((2 * half + 1) ^ f) << 4)) = s1;
        } else {
#pragma unroll
            for (int kb = 0; kb < G8_KBS; kb++)
                *reinterpret_cast<u32x4 *>(tA + (kb * G8_TILE + srow) * 64 + ((spiece ^ g8_swz(srow, kb)) << 4)) = pa[A4 ? 0 : kb];
        }
#pragma unroll
        for (int kb = 0; kb < G8_KBS; kb++)
            *reinterpret_cast<u32x4 *>(tB + (kb * G8_TILE + srow) * 64 + ((spiece ^ g8_swz(srow, kb)) << 4)) = A4 ? g8_pair_order(pb[kb]) : pb[kb];
    };

    float acc[4][2][4];                                        // fp32 forms
    i32x4 S[4][2], fa[4], fb[2];                               // S: one K-block's sums (fp32 forms) / the running sums (I32)
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) {
            S[a][b] = i32x4{0, 0, 0, 0};
#pragma unroll
            for (int t = 0; t < 4; t++) acc[a][b][t] = 0.0f;
        }

    const float *sArow = I32 ? nullptr : sA + ((m0 >> 6) + wr) * kbn;
    const float *sBrow = I32 ? nullptr : sB + ((n0 >> 6) + (wc >> 1)) * kbn;
    const int frow = lane & 15, fkg = lane >> 4;

    auto frag = [&](const char *tile, int kb, int row) -> i32x4 {
        return *reinterpret_cast<const i32x4 *>(tile + (kb * G8_TILE + row) * 64 + ((fkg ^ g8_swz(row, kb)) << 4));
    };
    auto load_frags = [&](const char *tA, const char *tB, int kb) {
#pragma unroll
        for (int a = 0; a < 4; a++) fa[a] = frag(tA, kb, wr * 64 + a * 16 + frow);
#pragma unroll
        for (int b = 0; b < 2; b++) fb[b] = frag(tB, kb, wc * 32 + b * 16 + frow);
    };
    // h: rows 32 h .. 32 h + 31 of the wave tile (two of the four MFMA row tiles).  The fp32 forms fold each half before the next one's
    // MFMAs are issued, so only half of S is live beside the accumulators (the whole of it spills at 4 waves per SIMD); the
    // MFMA -> VALU dependency is covered by the other resident waves
    auto mfma_half = [&](int h) {
#pragma unroll
        for (int a = 2 * h; a < 2 * h + 2; a++)
#pragma unroll
            for (int b = 0; b < 2; b++) S[a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[a], fb[b], I32 ? S[a][b] : G8_BIAS4, 0, 0, 0);
    };
    // The mixed form's MFMA returns 16 S_b.  Where c_b / 16 is exact the 2^-4 goes into the factor (fma(c_b / 16, 16 S_b, C) rounds the
    // same real number as fma(c_b, S_b, C)); for a c_b so small that c_b / 16 would lose bits it goes into the integer instead, which is
    // exact too.  gemm4.hip takes a uniform branch there; here the choice is two wave-uniform selects per K-block and the fold is the
    // same two packed instructions either way (a branch per fold left all of S live across it and spilled)
    auto fold_half = [&](int h, float c) {
        const bool in_factor = g8_sixteenth_is_exact(c);
        const float cs = A4 && in_factor ? c * 0.0625f : c, m = in_factor ? 1.0f : 0.0625f;
#pragma unroll
        for (int a = 2 * h; a < 2 * h + 2; a++)
#pragma unroll
            for (int b = 0; b < 2; b++) {
                if (A4) g8_fold4_scaled(acc[a][b], S[a][b], cs, m, -G8_BIAS_F * m);
                else g8_fold4(acc[a][b], S[a][b], cs);
            }
    };
    auto scale = [&](uint64_t blk) -> float {
        return (sArow[blk] * (A4 ? G8_RCP7 : G8_RCP127)) * (sBrow[blk] * G8_RCP127);
    };

    fetch(0);
    stash(0);
    __syncthreads();

    // one stage out of LDS buffer st & 1
    auto compute = [&](uint32_t st) {
        const char *tA = smem + (st & 1) * G8_STAGE_BYTES;
        const char *tB = tA + G8_KBS * G8_TILE * 64;
        if (I32) {
            load_frags(tA, tB, 0);
            mfma_half(0);
            mfma_half(1);
            load_frags(tA, tB, 1);
            mfma_half(0);
            mfma_half(1);
        } else {
            // the fragments of K-block 1 are requested once the last MFMAs of K-block 0 were issued: their latency hides behind a fold
            const uint64_t blk = (uint64_t)st * G8_KBS;
            const float c0 = scale(blk), c1 = scale(blk + 1);
            load_frags(tA, tB, 0);
            mfma_half(0);
            G8_KEEP_ORDER();
            fold_half(0, c0);
            mfma_half(1);
            G8_KEEP_ORDER();
            load_frags(tA, tB, 1);
            fold_half(1, c0);
            G8_KEEP_ORDER();
            mfma_half(0);
            G8_KEEP_ORDER();
            fold_half(0, c1);
            mfma_half(1);
            G8_KEEP_ORDER();
            fold_half(1, c1);
        }
    };
    // the last stage is peeled: a conditional stash behind the folds lets the compiler sink every fold of the stage below the branch,
    // with all of S live above it
    for (uint32_t st = 0; st + 1 < nstages; st++) {
        fetch(st + 1);
        compute(st);
        stash((int)((st & 1) ^ 1));
        __syncthreads();
    }
    compute(nstages - 1);

    // C/D layout of the 16x16 MFMA: column = lane & 15, row = 4 * (lane >> 4) + t
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const uint64_t i = m0 + wr * 64 + a * 16 + 4 * (lane >> 4) + t;
                const uint64_t j = n0 + wc * 32 + b * 16 + (lane & 15);
                if (I32) __builtin_nontemporal_store(S[a][b][t], &static_cast<int32_t *>(out)[i * N + j]);
                else __builtin_nontemporal_store(acc[a][b][t], &static_cast<float *>(out)[i * N + j]);
            }
}

// ================================================================================================
// C ABI
// ================================================================================================
static int check_gemm8_shape(const char *fn, uint64_t M, uint64_t N, uint64_t K)
{
    CLV_REQUIRE(M && N && K && M % 128 == 0 && N % 128 == 0 && K % 128 == 0, "%s: M=%llu N=%llu K=%llu must be non-zero multiples of 128", fn,
                (unsigned long long)M, (unsigned long long)N, (unsigned long long)K);
    CLV_REQUIRE(M / G8_TILE <= 0x7FFFFFFFull && N / G8_TILE <= 0x7FFFFFFFull && (M / G8_TILE) * (N / G8_TILE) <= 0x7FFFFFFFull &&
                    K / 64 <= 0xFFFFFFFFull, "%s: too many tiles", fn);
    return CLV_OK;
}

#define G8_ALIGNED(p) (((uintptr_t)(p) & 15) == 0)          // the kernel moves the operands as 16-byte vectors
#define G8_SCALES_ALIGNED(a, b) ((((uintptr_t)(a) | (uintptr_t)(b)) & 3) == 0)

template <bool A4, bool I32>
static int launch_gemm8(const int8_t *A, const float *sA, uint64_t M, uint64_t K, const int8_t *B, const float *sB, uint64_t N, uint64_t kb0,
                        uint64_t kbc, void *out, hipStream_t st)
{
    const uint32_t tiles_m = (uint32_t)(M / G8_TILE), tiles_n = (uint32_t)(N / G8_TILE);
    const size_t lds = 2 * (size_t)G8_STAGE_BYTES;
    CLV_HIP(hipFuncSetAttribute((const void *)k_gemm8<A4, I32>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_gemm8<A4, I32>), dim3(tiles_m * tiles_n), dim3(512), lds, st, (const uint8_t *)A, sA, (const uint8_t *)B, sB, N, K,
                       (uint32_t)kb0, (uint32_t)kbc, out, tiles_m, tiles_n);
    CLV_LAUNCH_CHECK();
    return CLV_OK;
}

extern "C" int clm8_gemm(const int8_t *A, const float *sA, uint64_t M, uint64_t K, const int8_t *B, const float *sB, uint64_t N, float *C,
                         void *stream)
{
    CLV_REQUIRE(A && sA && B && sB && C, "clm8_gemm: null pointer");
    int rc = check_gemm8_shape("clm8_gemm", M, N, K);
    if (rc) return rc;
    CLV_REQUIRE(G8_ALIGNED(A) && G8_ALIGNED(B) && G8_ALIGNED(C) && G8_SCALES_ALIGNED(sA, sB), "clm8_gemm: A, B and C must be 16-byte aligned (scales: 4)");
    return launch_gemm8<false, false>(A, sA, M, K, B, sB, N, 0, K / 64, C, as_stream(stream));
}

extern "C" int clm8_gemm_i32(const int8_t *A, uint64_t M, uint64_t K, const int8_t *B, uint64_t N, uint64_t kb_begin, uint64_t kb_count,
                             int32_t *S, void *stream)
{
    CLV_REQUIRE(A && B && S, "clm8_gemm_i32: null pointer");
    int rc = check_gemm8_shape("clm8_gemm_i32", M, N, K);
    if (rc) return rc;
    CLV_REQUIRE(G8_ALIGNED(A) && G8_ALIGNED(B) && G8_ALIGNED(S), "clm8_gemm_i32: A, B and S must be 16-byte aligned");
    CLV_REQUIRE(kb_count && kb_begin <= K / 64 && kb_count <= K / 64 - kb_begin, "clm8_gemm_i32: K-blocks [%llu, +%llu) of %llu",
                (unsigned long long)kb_begin, (unsigned long long)kb_count, (unsigned long long)(K / 64));
    // |S_b| <= 64 * 128 * 128 = 2^20 per K-block: 2047 of them stay below 2^31 for every byte pattern
    CLV_REQUIRE(kb_count <= G8_MAX_KB_I32, "clm8_gemm_i32: %llu K-blocks could overflow int32 (at most %llu per call)", (unsigned long long)kb_count,
                G8_MAX_KB_I32);
    return launch_gemm8<false, true>(A, nullptr, M, K, B, nullptr, N, kb_begin, kb_count, S, as_stream(stream));
}

extern "C" int clm4_gemm_m8(const int8_t *A4, const float *sA, uint64_t M, uint64_t K, const int8_t *B8, const float *sB, uint64_t N, float *C,
                            void *stream)
{
    CLV_REQUIRE(A4 && sA && B8 && sB && C, "clm4_gemm_m8: null pointer");
    int rc = check_gemm8_shape("clm4_gemm_m8", M, N, K);
    if (rc) return rc;
    CLV_REQUIRE(G8_ALIGNED(A4) && G8_ALIGNED(B8) && G8_ALIGNED(C) && G8_SCALES_ALIGNED(sA, sB),
                "clm4_gemm_m8: A4, B8 and C must be 16-byte aligned (scales: 4)");
    return launch_gemm8<true, false>(A4, sA, M, K, B8, sB, N, 0, K / 64, C, as_stream(stream));
}
