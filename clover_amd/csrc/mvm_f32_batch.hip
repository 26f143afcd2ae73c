// mvm_f32_batch.hip -- several fp32 vectors, one pass over a quantized matrix (include/clover_hip_batch_f32.h): r[j] = A x[j] for up to 8
// CloverVector32 with one CloverMatrix4 or one CloverMatrix8, the fused mvm + scaleAndAdd of the IHT / GD loops for several vectors, and
// the two-matrix loop for several signals.  One kernel family for both widths, one host driver over a traits struct per width.
//
// Every result equals the single call's (k_m4_mvm_f32, mvm_f32.hip; k_m8_mvm_f32, matrix8.hip) bit for bit: 32 sequential fma chains per
// row, chain e mod 32 takes elements e, e + 32, ... in ascending order, the link of each width as there --
//   4 bit: acc = fma(x[e], f32((float)q * f32(s / 7)), acc)          8 bit: acc = fma(f32(x[e] * f32(s / 127)), (float)q, acc)
// -- and the closing tree (acc1 + acc2) + (acc3 + acc4) per AVX lane, then CloverBase.h:149-157.  Nothing is flushed.
//
// Mapping.  A workgroup owns ONE 64-row tile row of the matrix (one row of the scale grid), whatever the width.  Four lanes (a quad) own a
// matrix row: they load 64 contiguous bytes, one dwordx4 each, and transpose the 4 x 4 dwords inside the quad (quad_transpose4), which
// leaves lane a with dwords a, 4 + a, 8 + a, 12 + a.  For the 4-bit matrix those are the words of accumulator a (8 chains, as in
// k_m4_mvm_f32); for the 8-bit matrix dword d holds elements 4 d .. 4 d + 3 of the 64-byte block, so lane a owns chains 4 a .. 4 a + 3 and
// 16 + 4 a .. 16 + 4 a + 3: 8 chains per lane, row and vector in either width.  A quad walks R rows of the tile (q and q + 64 / R, ...):
// what a lane reads of x for one matrix dword is applied to R rows, which divides the LDS reads per matrix byte by R; the workgroup has
// 256 / R lanes.
//
// x in LDS.  MVFB_CHUNK columns of each of the NV vectors, restaged every MVFB_CHUNK columns; the matrix loads of the next steps are
// requested before the barrier of a restaging and stay in flight across it.  4 bit: raw x plus the chunk's factors f32(s / 7), and the
// barrier tells whether every factor survives 16 c (the (q / 16) (16 c) shortcut of k_m4_mvm_f32, same guard).  8 bit: the tile row has ONE
// factor per 64 columns, so the staging stores f32(x * f32(s / 127)) -- the rounded first operand of the link -- and the inner loop is the
// fma alone.  What does not depend on the vector (transpose, unpack, convert, the 4-bit dequantised value) is computed once per matrix
// dword and row; per vector remain the LDS read and 8 (4) fmas per row.
#include "mvm_f32_device.h"
#include "mvm_batch_host.h"

#include "clover_hip_batch_f32.h"
#include "clover_hip_fp32.h"
#include "clover_hip_m4_f32.h"
#include "clover_hip_m8_f32.h"

#ifndef MVFB_CHUNK
#define MVFB_CHUNK CLMQ_F32_BATCH_CHUNK      // -DMVFB_CHUNK: an A/B build with a shorter chunk (tools/mq_f32_batch_variants.py)
#endif
// rows per quad and matrix loads (dwordx4 per lane and row) requested ahead, per instantiation: from the resource listing and the variants
// timed with tools/mq_f32_batch_variants.py (profiles/mq_f32_batch_variants.json; DESIGN.md 3, "Several fp32 vectors, one pass") -- the
// 4- and 8-vector forms of the 4-bit matrix and the 8-vector form of the 8-bit one run fastest at R = 1, U = 2 (fewer registers, more
// waves); the others keep R = 2, U = 4, which was not compared.  -DMVFB_R / -DMVFB_U / -DMVFB_WAVES force one value for every
// instantiation: the builds of that tool
#ifdef MVFB_R
constexpr int mvfb_rows(int, int) { return MVFB_R; }
#else
constexpr int mvfb_rows(int bits, int nv) { return nv == 2 || (bits == 8 && nv == 4) ? 2 : 1; }
#endif
#ifdef MVFB_U
constexpr int mvfb_depth(int, int) { return MVFB_U; }
#else
constexpr int mvfb_depth(int bits, int nv) { return mvfb_rows(bits, nv) == 1 ? 2 : 4; }
#endif
#ifndef MVFB_WAVES
#define MVFB_WAVES 2                // minimum waves per SIMD the register allocation must leave room for
#endif

// the vectors of one pass, by value in the kernel arguments: no pointer table in device memory.  Slots v >= nv are NULL and never
// dereferenced.  r: the product (fused: t of the ABI, NULL = not stored); fused: r2[v] = fma(product, a, u[v]), r2[v] may be u[v]
template <int NV>
struct MqF32BatchArgs {
    const float *x[NV];
    float *r[NV];
    const float *u[NV];
    float *r2[NV];
    float a;
};

// stage columns c0 .. c0 + cw of every vector (and the factors of the tile row `su`); returns whether the chunk takes the 16 c shortcut
template <int BITS, int NV, int T>
__device__ __forceinline__ int mqb_stage(uint64_t c0, uint32_t cw, int tid, int nv, const MqF32BatchArgs<NV> &args, const float *__restrict__ su,
                                         float *xs, float *s7)
{
    constexpr int NX = MVFB_CHUNK / 4 / T;                               // f32x4 per lane and vector
    const uint32_t nx = cw / 4, nb = cw / 64;
    float f[NX];
    if (BITS == 8) {
#pragma unroll
        for (int k = 0; k < NX; k++) {
            const uint32_t i = tid + T * k;
            f[k] = su[c0 / 64 + (i < nx ? i : 0) / 16] / 127.0f;         // the factor of the 64-column block of this lane's four columns
        }
    }
#pragma unroll
    for (int v = 0; v < NV; v++)
        if (v < nv) {
            const f32x4 *xg = reinterpret_cast<const f32x4 *>(args.x[v] + c0);
#pragma unroll
            for (int k = 0; k < NX; k++) {
                const uint32_t i = tid + T * k;
                if (i < nx) {
                    f32x4 xv = xg[i];
                    if (BITS == 8) { xv.x = xv.x * f[k]; xv.y = xv.y * f[k]; xv.z = xv.z * f[k]; xv.w = xv.w * f[k]; }
                    reinterpret_cast<f32x4 *>(xs + v * MVFB_CHUNK)[i] = xv;
                }
            }
        }
    if (BITS == 4) {
        int fast = 1;
        if ((uint32_t)tid < nb) {
            const float c = div7(su[c0 / 64 + tid]);
            s7[tid] = c;
            fast = times16_is_finite(c);
        }
        return __builtin_amdgcn_readfirstlane(__syncthreads_and(fast));      // scalar: a real branch, not two predicated bodies
    }
    __syncthreads();
    return 1;
}

// one step of a quad on the 4-bit matrix: 16 words = 128 columns of R rows; gl = the step inside the chunk
template <int NV, int R, bool FAST>
__device__ __forceinline__ void mqb_step4(const u32x4 (&av)[R], uint32_t gl, int a, int nv, const float *xs, const float *s7, float (&acc)[NV][R][8])
{
    uint32_t w[R][4];
#pragma unroll
    for (int k = 0; k < R; k++) {
        w[k][0] = av[k].x; w[k][1] = av[k].y; w[k][2] = av[k].z; w[k][3] = av[k].w;
        quad_transpose4(w[k][0], w[k][1], w[k][2], w[k][3], a);              // words a, 4 + a, 8 + a, 12 + a of the step
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t wi = 16 * gl + 4 * i + a;                             // word index inside the chunk
        const float sc = s7[wi >> 3];
        float d[R][8];                                                       // f32(q c): the same for every vector
#pragma unroll
        for (int k = 0; k < R; k++) {
            if constexpr (FAST) {
                const float sc16 = sc * 16.0f;
                float f16[8];
                unpack8_16th(w[k][i], f16);                                  // q / 16
#pragma unroll
                for (int j = 0; j < 8; j++) d[k][j] = f16[j] * sc16;
            } else {
#pragma unroll
                for (int j = 0; j < 8; j++) d[k][j] = (float)unpack1(w[k][i], j) * sc;
            }
        }
#pragma unroll
        for (int v = 0; v < NV; v++)
            if (v < nv) {
                const f32x4 xl = reinterpret_cast<const f32x4 *>(xs + v * MVFB_CHUNK)[2 * wi];
                const f32x4 xh = reinterpret_cast<const f32x4 *>(xs + v * MVFB_CHUNK)[2 * wi + 1];
                const float xv[8] = {xl.x, xl.y, xl.z, xl.w, xh.x, xh.y, xh.z, xh.w};
#pragma unroll
                for (int k = 0; k < R; k++)
#pragma unroll
                    for (int j = 0; j < 8; j++) acc[v][k][j] = __builtin_fmaf(xv[j], d[k][j], acc[v][k][j]);
            }
    }
}

// one step of a quad on the 8-bit matrix: one 64-byte block of R rows.  Dword i of the lane = elements 16 i + 4 a + l of the block, chain
// (16 i + 4 a + l) mod 32: accumulator 4 (i & 1) + l of the lane, i = 0 before i = 2 and 1 before 3 as the elements ascend
template <int NV, int R>
__device__ __forceinline__ void mqb_step8(const u32x4 (&av)[R], uint32_t gl, int a, int nv, const float *xs, float (&acc)[NV][R][8])
{
    uint32_t w[R][4];
#pragma unroll
    for (int k = 0; k < R; k++) {
        w[k][0] = av[k].x; w[k][1] = av[k].y; w[k][2] = av[k].z; w[k][3] = av[k].w;
        quad_transpose4(w[k][0], w[k][1], w[k][2], w[k][3], a);              // dwords a, 4 + a, 8 + a, 12 + a of the block
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        float qf[R][4];                                                      // (float)q: the same for every vector
#pragma unroll
        for (int k = 0; k < R; k++)
#pragma unroll
            for (int l = 0; l < 4; l++) qf[k][l] = (float)((int)(w[k][i] << (24 - 8 * l)) >> 24);
        const uint32_t col = 64 * gl + 16 * i + 4 * a;
#pragma unroll
        for (int v = 0; v < NV; v++)
            if (v < nv) {
                const f32x4 xf = *reinterpret_cast<const f32x4 *>(xs + v * MVFB_CHUNK + col);      // f32(x f), rounded at the staging
                const float xv[4] = {xf.x, xf.y, xf.z, xf.w};
#pragma unroll
                for (int k = 0; k < R; k++)
#pragma unroll
                    for (int l = 0; l < 4; l++) acc[v][k][4 * (i & 1) + l] = __builtin_fmaf(xv[l], qf[k][l], acc[v][k][4 * (i & 1) + l]);
            }
    }
}

// the row value from a lane's 8 chains; every lane of the quad ends with it
template <int BITS>
__device__ __forceinline__ float mqb_close(const float (&c)[8])
{
    if (BITS == 4) {
        // lane a = accumulator a + 1: (acc1 + acc2) + (acc3 + acc4) per AVX lane j, then the CloverBase.h:149-157 tree
        float s3[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float s12 = c[j] + __shfl_xor(c[j], 1);
            s3[j] = s12 + __shfl_xor(s12, 2);
        }
        const float t0 = s3[4] + s3[0], t1 = s3[5] + s3[1], t2 = s3[6] + s3[2], t3 = s3[7] + s3[3];
        return (t0 + t2) + (t1 + t3);
    }
    // lane a: c[l] = AVX lane 4 (a & 1) + l of accumulator 1 + (a >> 1), c[4 + l] = the same lane of accumulator 3 + (a >> 1).
    // acc1 + acc2 and acc3 + acc4: lanes a, a ^ 2; their sum; sum[i + 4] + sum[i]: lanes a, a ^ 1
    float x[4];
#pragma unroll
    for (int l = 0; l < 4; l++) {
        const float s12 = c[l] + __shfl_xor(c[l], 2), s34 = c[4 + l] + __shfl_xor(c[4 + l], 2);
        const float s = s12 + s34;
        x[l] = s + __shfl_xor(s, 1);
    }
    return (x[0] + x[2]) + (x[1] + x[3]);
}

template <int BITS, int NV, int R, int U, bool NT, bool FUSED>
__global__ __launch_bounds__(256 / R, MVFB_WAVES) void k_mq_mvm_f32_batch(const u32x4 *__restrict__ A, const float *__restrict__ sA, uint64_t cols, int nv,
                                                                 const MqF32BatchArgs<NV> args)
{
    constexpr int T = 256 / R, NQ = 64 / R;                              // lanes and quads of the workgroup
    constexpr uint32_t GC = BITS == 4 ? 128 : 64, GPC = MVFB_CHUNK / GC;  // columns per step (64 bytes of a row), steps per chunk
    static_assert(GPC % U == 0 && MVFB_CHUNK % (4 * T) == 0, "a restaging falls on the first step of a round");
    __shared__ __attribute__((aligned(16))) float xs[NV * MVFB_CHUNK + (BITS == 4 ? MVFB_CHUNK / 64 : 0)];
    float *s7 = xs + NV * MVFB_CHUNK;
    const int tid = threadIdx.x, a = tid & 3, q = tid >> 2;
    uint64_t row[R];
    const u32x4 *Arow[R];
#pragma unroll
    for (int k = 0; k < R; k++) {
        row[k] = (uint64_t)blockIdx.x * 64 + q + k * NQ;
        Arow[k] = A + row[k] * (cols * BITS / 128);
    }
    const float *su = sA + (uint64_t)blockIdx.x * (cols / 64);
    float acc[NV][R][8];
#pragma unroll
    for (int v = 0; v < NV; v++)
#pragma unroll
        for (int k = 0; k < R; k++)
#pragma unroll
            for (int j = 0; j < 8; j++) acc[v][k][j] = 0.0f;
    // the epilogue of vector v belongs to lane v mod 4 of the quad (every lane ends with the row value): u is requested ahead of the
    // column loop by the lane that will store r2, so r2[v] may be u[v]
    float fu[(NV + 3) / 4][R];
#pragma unroll
    for (int v = 0; v < NV; v++)
#pragma unroll
        for (int k = 0; k < R; k++)
            if ((v & 3) == 0) fu[v >> 2][k] = 0.0f;
    if (FUSED) {
#pragma unroll
        for (int v = 0; v < NV; v++)
            if (v < nv && (v & 3) == a) {
#pragma unroll
                for (int k = 0; k < R; k++) fu[v >> 2][k] = args.u[v][row[k]];
            }
    }
    const uint32_t nsteps = (uint32_t)(cols / GC), last = nsteps - 1;
    auto ld = [&](uint32_t g, int k) {                                   // clamped: a step past the end re-reads the last one
        const u32x4 *p = &Arow[k][4 * (g < last ? g : last) + a];
        return NT ? __builtin_nontemporal_load(p) : *p;
    };
    u32x4 cur[U][R];
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
        for (int k = 0; k < R; k++) cur[u][k] = ld(u, k);
    int fast = 1;
    for (uint32_t g = 0; g < nsteps; g += U) {
        u32x4 nxt[U][R];
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int k = 0; k < R; k++) nxt[u][k] = ld(g + U + u, k);
        asm volatile("" ::: "memory");                                   // the next round's loads are issued HERE, before a restaging and this round's arithmetic
        if (g % GPC == 0) {
            const uint64_t c0 = (uint64_t)g * GC;
            if (g) __syncthreads();                                      // every lane is done with the chunk before
            fast = mqb_stage<BITS, NV, T>(c0, (uint32_t)((cols - c0) < MVFB_CHUNK ? (cols - c0) : MVFB_CHUNK), tid, nv, args, su, xs, s7);
        }
#pragma unroll
        for (int u = 0; u < U; u++)
            if (g + u < nsteps) {
                const uint32_t gl = (g + u) % GPC;
                if constexpr (BITS == 8) mqb_step8<NV, R>(cur[u], gl, a, nv, xs, acc);
                else if (fast) mqb_step4<NV, R, true>(cur[u], gl, a, nv, xs, s7, acc);
                else mqb_step4<NV, R, false>(cur[u], gl, a, nv, xs, s7, acc);
            }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int k = 0; k < R; k++) cur[u][k] = nxt[u][k];
    }
#pragma unroll
    for (int v = 0; v < NV; v++)
        if (v < nv) {
#pragma unroll
            for (int k = 0; k < R; k++) {
                const float d = mqb_close<BITS>(acc[v][k]);
                if ((v & 3) == a) {
                    if (!FUSED) {
                        args.r[v][row[k]] = d;
                    } else {
                        if (args.r[v]) args.r[v][row[k]] = d;
                        args.r2[v][row[k]] = __builtin_fmaf(d, args.a, fu[v >> 2][k]);
                    }
                }
            }
        }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
// the vectors of a call (host arrays of device pointers).  u == NULL: the plain product, r[j] = A x[j].  Else the fused form: t[j] =
// A x[j] (t == NULL or t[j] == NULL: not stored), r[j] = fma(A x[j], a, u[j])
struct MqF32BatchVectors {
    const float *const *x;
    const float *const *u;
    float a;
    float *const *t;
    float *const *r;
    MqF32BatchVectors from(uint64_t j0) const { return {x + j0, u ? u + j0 : nullptr, a, t ? t + j0 : nullptr, r + j0}; }
};

// what differs between the widths: the bytes of a matrix, the streaming rule and the single calls a group is forwarded to
struct M4F32Batch {
    static constexpr int BITS = 4;
    static constexpr uint64_t max_elements = 0xFFFFFFFFFFFFull;      // the bound of clm4_mvm_f32_scale_and_add (mvm_f32_t.hip)
    static uint64_t matrix_bytes(uint64_t rows, uint64_t cols) { return rows * (cols / 2); }
    static bool streaming(uint64_t rows, uint64_t cols) { return m4f32_streaming(rows, cols); }
    // Measured on the MI355X ("Several fp32 vectors, one pass"; profiles/m4_mvm_f32_batch_kernel_bench.json): batched exactly
    // in the classes where the pass beat the single calls by more than their spread -- 8 vectors from the cache-resident step
    // (8192 x 4096, 16 MiB) up; 2 and 4 vectors from 2 GiB (65536^2) up: they lost at 32768^2 and at 8192 x 4096.  Everything not measured
    // is forwarded: groups of 3 and 5-7, smaller matrices
    static bool batched_by_rule(uint64_t g, uint64_t rows, uint64_t cols)
    {
        const uint64_t b = matrix_bytes(rows, cols);
        return (g == 8 && b >= (16ull << 20)) || ((g == 2 || g == 4) && b >= (2ull << 30));
    }
    static constexpr auto mvm = clm4_mvm_f32;
    static constexpr auto scale_and_add = clm4_mvm_f32_scale_and_add;
    static constexpr auto iht = clm4_iht_f32;
};
struct M8F32Batch {
    static constexpr int BITS = 8;
    static constexpr uint64_t max_elements = 0x1000000000000ull;     // the bound of clm8_mvm_f32_scale_and_add (matrix8_f32_t.hip)
    static uint64_t matrix_bytes(uint64_t rows, uint64_t cols) { return rows * cols; }
    static bool streaming(uint64_t rows, uint64_t cols) { return m8f32_streaming(rows, cols); }
    // Measured (profiles/m8_mvm_f32_batch_kernel_bench.json): 2, 4 and 8 vectors over 1 GiB (32768^2) and 4 GiB (65536^2) won by 1.9 to
    // 5.5 x; the cache-resident step and the loop at N = 8192 lost.  Batched from 1 GiB up, groups of 3 and 5-7 riding between measured
    // neighbours that won by a factor; everything smaller is forwarded (between 32 MiB and 1 GiB nothing was measured)
    static bool batched_by_rule(uint64_t g, uint64_t rows, uint64_t cols) { return g >= 2 && matrix_bytes(rows, cols) >= (1ull << 30); }
    static constexpr auto mvm = clm8_mvm_f32;
    static constexpr auto scale_and_add = clm8_mvm_f32_scale_and_add;
    static constexpr auto iht = clm8_iht_f32;
};

// one launch (counted) for the first g <= NV vectors of v: one workgroup per 64-row tile row, 256 / R lanes
template <class F, int NV>
static int mqf32_batch_launch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t g, const MqF32BatchVectors &v, hipStream_t st)
{
    constexpr int R = mvfb_rows(F::BITS, NV), U = mvfb_depth(F::BITS, NV);
    MqF32BatchArgs<NV> s;
    const bool fused = v.u != nullptr;
    for (uint64_t i = 0; i < NV; i++) {
        const bool in = i < g;
        s.x[i] = in ? v.x[i] : nullptr;
        s.r[i] = !in ? nullptr : fused ? (v.t ? v.t[i] : nullptr) : v.r[i];
        s.u[i] = in && fused ? v.u[i] : nullptr;
        s.r2[i] = in && fused ? v.r[i] : nullptr;
    }
    s.a = v.a;
    const dim3 grid((unsigned)(rows / 64)), block(256 / R);
    const u32x4 *Av = (const u32x4 *)A;
    const int nv = (int)g;
    switch (2 * F::streaming(rows, cols) + fused) {
    case 3: hipLaunchKernelGGL((k_mq_mvm_f32_batch<F::BITS, NV, R, U, true, true>), grid, block, 0, st, Av, sA, cols, nv, s); break;
    case 2: hipLaunchKernelGGL((k_mq_mvm_f32_batch<F::BITS, NV, R, U, true, false>), grid, block, 0, st, Av, sA, cols, nv, s); break;
    case 1: hipLaunchKernelGGL((k_mq_mvm_f32_batch<F::BITS, NV, R, U, false, true>), grid, block, 0, st, Av, sA, cols, nv, s); break;
    default: hipLaunchKernelGGL((k_mq_mvm_f32_batch<F::BITS, NV, R, U, false, false>), grid, block, 0, st, Av, sA, cols, nv, s); break;
    }
    CLV_LAUNCH_CHECK();
    clv_internal_mvm_batch_count();
    return CLV_OK;
}

// a group of 2 <= g <= CLM4_MVM_BATCH_MAX vectors on the smallest instantiation that holds it
template <class F>
static int mqf32_batch_launch_group(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t g, const MqF32BatchVectors &v, hipStream_t st)
{
    return g <= 2   ? mqf32_batch_launch<F, 2>(A, sA, rows, cols, g, v, st)
           : g <= 4 ? mqf32_batch_launch<F, 4>(A, sA, rows, cols, g, v, st)
                    : mqf32_batch_launch<F, 8>(A, sA, rows, cols, g, v, st);
}

// whether a group of g vectors runs as one batched launch or as g single launches: a group of one is the single call; then
// CLV_MVM_BATCH, then the width's rule
template <class F>
static bool mqf32_batch_selected(uint64_t g, uint64_t rows, uint64_t cols)
{
    if (g < 2) return false;
    const int force = mvm_batch_forced();
    return force >= 0 ? force != 0 : F::batched_by_rule(g, rows, cols);
}

// the checked arguments of the width's product batch call (v.u == NULL) / fused batch call on the stream, group by group
template <class F>
static int mqf32_batch_run(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const MqF32BatchVectors &v, void *stream)
{
    for (uint64_t j0 = 0; j0 < nvec; j0 += CLM4_MVM_BATCH_MAX) {
        const uint64_t g = nvec - j0 < CLM4_MVM_BATCH_MAX ? nvec - j0 : CLM4_MVM_BATCH_MAX;
        int rc = CLV_OK;
        if (!mqf32_batch_selected<F>(g, rows, cols)) {
            for (uint64_t j = j0; j < j0 + g && !rc; j++)
                rc = v.u ? F::scale_and_add(A, sA, rows, cols, v.x[j], v.u[j], v.a, v.t ? v.t[j] : nullptr, v.r[j], stream)
                         : F::mvm(A, sA, rows, cols, v.x[j], v.r[j], stream);
        } else {
            rc = mqf32_batch_launch_group<F>(A, sA, rows, cols, g, v.from(j0), as_stream(stream));
        }
        if (rc) return rc;
    }
    return CLV_OK;
}

#define MQF32_ALIGNED(p, n) (((uintptr_t)(p) & ((n) - 1u)) == 0)

// the size and alignment rules of the single calls for a matrix of the loop or of a product
template <class F>
static int mqf32_batch_check_matrix(const char *fn, const char *name, const int8_t *A, const float *sA, uint64_t rows, uint64_t cols)
{
    CLV_REQUIRE(A && sA, "%s: %s or its scales are NULL", fn, name);
    CLV_REQUIRE(MQF32_ALIGNED(A, 16) && MQF32_ALIGNED(sA, 4), "%s: %s must be 16-byte aligned, its scales 4-byte", fn, name);
    CLV_REQUIRE(rows / 64 <= 0x7FFFFFFFull && cols / 64 <= 0x7FFFFFFFull && (!cols || rows <= F::max_elements / cols),
                "%s: rows=%llu cols=%llu: matrix too large", fn, (unsigned long long)rows, (unsigned long long)cols);
    return CLV_OK;
}

// every check of the width's two product batch calls, before any device work.  u == NULL and t == NULL in the plain call
template <class F>
static int mqf32_batch_check_args(const char *fn, const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const float *const *x,
                                  const float *const *u, float *const *t, float *const *r, bool fused)
{
    const char *out = fused ? "r2" : "r";
    CLV_REQUIRE(rows % 64 == 0 && cols % 128 == 0, "%s: rows=%llu must be a multiple of 64 (a row shard) and cols=%llu of 128", fn,
                (unsigned long long)rows, (unsigned long long)cols);
    int rc = mqf32_batch_check_matrix<F>(fn, "A", A, sA, rows, cols);
    if (rc) return rc;
    if (!nvec) return CLV_OK;
    CLV_REQUIRE(x && r && (!fused || u), "%s: null pointer array", fn);
    for (uint64_t j = 0; j < nvec; j++)
        CLV_REQUIRE(x[j] && r[j] && (!fused || u[j]), "%s: null pointer in vector %llu", fn, (unsigned long long)j);
    for (uint64_t j = 0; j < nvec; j++) {
        CLV_REQUIRE(MQF32_ALIGNED(x[j], 16), "%s: x of vector %llu must be 16-byte aligned", fn, (unsigned long long)j);
        CLV_REQUIRE(MQF32_ALIGNED(r[j], 4) && (!fused || MQF32_ALIGNED(u[j], 4)) && (!t || MQF32_ALIGNED(t[j], 4)),
                    "%s: %s%s of vector %llu must be 4-byte aligned", fn, fused ? "u, t and " : "", out, (unsigned long long)j);
    }
    std::vector<ClvRange> rg;
    rg.reserve(4 * nvec + 2);
    rg.push_back(clv_range(A, F::matrix_bytes(rows, cols), false, ~0ull, "A"));
    rg.push_back(clv_range(sA, (rows / 64) * (cols / 64) * 4, false, ~0ull, "sA"));
    for (uint64_t j = 0; j < nvec; j++) {
        rg.push_back(clv_range(x[j], cols * 4, false, j, "x"));
        rg.push_back(clv_range(r[j], rows * 4, true, j, out));
        // the in-place form r2[j] == u[j]: the result IS the input, only the lane that owns an element touches it in either
        if (fused && r[j] != u[j]) rg.push_back(clv_range(u[j], rows * 4, false, j, "u"));
        if (t && t[j]) rg.push_back(clv_range(t[j], rows * 4, true, j, "t"));
    }
    return clv_internal_check_ranges(fn, rg);
}

// ---- the bodies of a width's extern "C" entry points; fn = the name of the entry point that was called ----------------------------------
template <class F>
static int mqf32_batch_entry(const char *fn, const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const float *const *x,
                             float *const *r, void *stream)
{
    int rc = mqf32_batch_check_args<F>(fn, A, sA, rows, cols, nvec, x, nullptr, nullptr, r, false);
    if (rc) return rc;
    if (!nvec || !rows || !cols) return CLV_OK;
    return mqf32_batch_run<F>(A, sA, rows, cols, nvec, {x, nullptr, 0.0f, nullptr, r}, stream);
}

template <class F>
static int mqf32_batch_fused_entry(const char *fn, const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const float *const *x,
                                   const float *const *u, float a, float *const *t, float *const *r2, void *stream)
{
    int rc = mqf32_batch_check_args<F>(fn, A, sA, rows, cols, nvec, x, u, t, r2, true);
    if (rc) return rc;
    if (!nvec || !rows || !cols) return CLV_OK;
    return mqf32_batch_run<F>(A, sA, rows, cols, nvec, {x, u, a, t, r2}, stream);
}

// Q_IHT / Q_GD for nvec signals with one Phi and its stored transpose: the loop of mvm_f32_iht (mvm_f32_host.h) with both products batched.
// The checks run once; per group there is one decision, and a selected group costs per iteration two fused launches and, with a
// threshold, one clv_f32_threshold_mode per signal.  Bit-identical to F::iht per signal.
template <class F>
static int mqf32_batch_iht(const char *fn, const int8_t *Phi, const float *sPhi, const int8_t *PhiT, const float *sPhiT, uint64_t m, uint64_t n,
                           uint64_t nvec, float *const *x, uint64_t x_len, const float *const *y, float *const *t1, float *const *t2, float *const *t3,
                           uint64_t iterations, uint64_t K, float mu, int threshold, void *stream)
{
    CLV_REQUIRE(m % 128 == 0 && n % 128 == 0, "%s: m=%llu n=%llu must be multiples of 128", fn, (unsigned long long)m, (unsigned long long)n);
    CLV_REQUIRE(x_len <= n, "%s: x_len=%llu exceeds n=%llu", fn, (unsigned long long)x_len, (unsigned long long)n);
    CLV_REQUIRE(threshold >= 0 && threshold <= 2, "%s: unknown threshold %d", fn, threshold);
    int rc = mqf32_batch_check_matrix<F>(fn, "Phi", Phi, sPhi, m, n);
    if (!rc) rc = mqf32_batch_check_matrix<F>(fn, "PhiT", PhiT, sPhiT, n, m);
    if (rc) return rc;
    if (!nvec) return CLV_OK;
    CLV_REQUIRE(x && y && t1 && t2 && t3, "%s: null pointer array", fn);
    for (uint64_t j = 0; j < nvec; j++)
        CLV_REQUIRE(x[j] && y[j] && t1[j] && t2[j] && t3[j], "%s: null pointer in vector %llu", fn, (unsigned long long)j);
    for (uint64_t j = 0; j < nvec; j++) {
        CLV_REQUIRE(MQF32_ALIGNED(x[j], 16) && MQF32_ALIGNED(t2[j], 16), "%s: x and t2 of vector %llu must be 16-byte aligned", fn, (unsigned long long)j);
        CLV_REQUIRE(MQF32_ALIGNED(y[j], 4) && MQF32_ALIGNED(t1[j], 4) && MQF32_ALIGNED(t3[j], 4), "%s: y, t1 and t3 of vector %llu must be 4-byte aligned", fn,
                    (unsigned long long)j);
    }
    {
        const uint64_t grid = (m / 64) * (n / 64) * 4;
        std::vector<ClvRange> rg;
        rg.reserve(5 * nvec + 4);
        rg.push_back(clv_range(Phi, F::matrix_bytes(m, n), false, ~0ull, "Phi"));
        rg.push_back(clv_range(sPhi, grid, false, ~0ull, "sPhi"));
        rg.push_back(clv_range(PhiT, F::matrix_bytes(m, n), false, ~0ull, "PhiT"));
        rg.push_back(clv_range(sPhiT, grid, false, ~0ull, "sPhiT"));
        for (uint64_t j = 0; j < nvec; j++) {
            rg.push_back(clv_range(y[j], m * 4, false, j, "y"));
            rg.push_back(clv_range(x[j], n * 4, true, j, "x"));
            rg.push_back(clv_range(t1[j], m * 4, true, j, "t1"));
            rg.push_back(clv_range(t2[j], m * 4, true, j, "t2"));
            rg.push_back(clv_range(t3[j], n * 4, true, j, "t3"));
        }
        rc = clv_internal_check_ranges(fn, rg);
        if (rc) return rc;
    }
    const int mode = threshold == 2 ? CLV_THRESHOLD_REFERENCE : CLV_THRESHOLD_FAST;
    hipStream_t st = as_stream(stream);
    for (uint64_t j0 = 0; j0 < nvec; j0 += CLM4_MVM_BATCH_MAX) {
        const uint64_t g = nvec - j0 < CLM4_MVM_BATCH_MAX ? nvec - j0 : CLM4_MVM_BATCH_MAX;
        if (!(m && n && mqf32_batch_selected<F>(g, m, n))) {      // one signal, an empty matrix, or forwarded: the single call, signal after signal
            for (uint64_t j = j0; j < j0 + g; j++) {
                rc = F::iht(Phi, sPhi, PhiT, sPhiT, m, n, x[j], x_len, y[j], t1[j], t2[j], t3[j], iterations, K, mu, threshold, stream);
                if (rc) return rc;
            }
            continue;
        }
        for (uint64_t j = j0; j < j0 + g; j++) {
            rc = clv_internal_f32_clear(x[j], n, st);                                         // x.clear()
            if (rc) return rc;
        }
        const MqF32BatchVectors step1 = {x + j0, y + j0, -1.0f, t1 + j0, t2 + j0};            // t1 = Phi x; t2 = y - t1
        const MqF32BatchVectors step2 = {t2 + j0, x + j0, mu, t3 + j0, x + j0};               // t3 = Phi' t2; x += mu t3, in place
        for (uint64_t it = 0; it < iterations; it++) {
            rc = mqf32_batch_launch_group<F>(Phi, sPhi, m, n, g, step1, st);
            if (!rc) rc = mqf32_batch_launch_group<F>(PhiT, sPhiT, n, m, g, step2, st);
            for (uint64_t j = j0; !rc && threshold && j < j0 + g; j++)                        // keep the K largest, signal after signal
                rc = clv_f32_threshold_mode(x[j], x_len, n, K, mode, nullptr, stream);
            if (rc) return rc;
        }
    }
    return CLV_OK;
}

#define MQF32_BATCH_ENTRIES(W, F)                                                                                                                    \
    extern "C" int clm##W##_mvm_f32_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const float *const *x,    \
                                          float *const *r, void *stream)                                                                            \
    {                                                                                                                                                \
        return mqf32_batch_entry<F>("clm" #W "_mvm_f32_batch", A, sA, rows, cols, nvec, x, r, stream);                                               \
    }                                                                                                                                                \
    extern "C" int clm##W##_mvm_f32_scale_and_add_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec,             \
                                                        const float *const *x, const float *const *u, float a, float *const *t, float *const *r2,   \
                                                        void *stream)                                                                                \
    {                                                                                                                                                \
        return mqf32_batch_fused_entry<F>("clm" #W "_mvm_f32_scale_and_add_batch", A, sA, rows, cols, nvec, x, u, a, t, r2, stream);                 \
    }                                                                                                                                                \
    extern "C" int clm##W##_iht_f32_batch(const int8_t *Phi, const float *sPhi, const int8_t *PhiT, const float *sPhiT, uint64_t m, uint64_t n,    \
                                          uint64_t nvec, float *const *x, uint64_t x_len, const float *const *y, float *const *t1,                  \
                                          float *const *t2, float *const *t3, uint64_t iterations, uint64_t K, float mu, int threshold,             \
                                          void *stream)                                                                                             \
    {                                                                                                                                                \
        return mqf32_batch_iht<F>("clm" #W "_iht_f32_batch", Phi, sPhi, PhiT, sPhiT, m, n, nvec, x, x_len, y, t1, t2, t3, iterations, K, mu,        \
                                  threshold, stream);                                                                                               \
    }
MQF32_BATCH_ENTRIES(4, M4F32Batch)
MQF32_BATCH_ENTRIES(8, M8F32Batch)
