// mvm_t4.hip -- the transposed 4-bit mvm: r = quantize(A' x) straight from A's own bytes, no stored transpose.
//
// Contract: byte for byte what clm4_transpose(A -> At) followed by clm4_mvm(At, cols, rows, x -> r) gives, the generator state included.
// Output element j is row j of A' under the definition of k_m4_mvm64 (matrix4.hip): 16 sequential fp32 fma chains, chain wi mod 16 takes
// word wi = the eight elements A[8 wi .. 8 wi + 7][j], factor c = f32(f32(sA[b][j / 64] * 1/49) * sx[b]) with b = wi / 8 read from A's OWN
// scale grid at (row tile b, column tile j / 64), then the fixed tree and the 64-wide re-quantisation.  The link, the tree and the
// re-quantisation are the functions of mvm_device.h; the words come out of transpose8x8_nibbles (nibble_transpose.h), which produces the
// very words clm4_transpose stores.
//
// Mapping:
//   workgroup = MVT_W = 4 adjacent output blocks = 256 columns = 128 contiguous bytes of every row, 256 threads; it walks ALL rows (the
//               chains are sequential over the rows, so rows are not split across workgroups: cols / 256 workgroups);
//   lane      = (chain k = tid >> 4, column pair cg = tid & 15): per 128-row step it loads 8 B (columns 16 cg .. 16 cg + 15) of the rows
//               8 k .. 8 k + 7 of the step -- a wave's load instruction reads 4 rows x 128 B --, transposes the two 8 x 8 pieces in
//               registers and feeds the 16 column words to 16 accumulators against the ONE x word (word 16 step + k) the piece shares;
//   x, c      = staged per MVT_CHUNK rows in LDS: the x words (MVT_CHUNK / 2 bytes) and the factors c[b][tile] of the workgroup's 4 column
//               tiles (MVT_CHUNK / 64 x 4 floats);
//   epilogue  = the 16 chain ends of every column go through LDS (stride 257: no bank conflicts) to four lanes per column in the layout
//               mvm_tree expects, the 256 dots to one wave per output block: requantize_wave and the MvmFuse epilogue as in k_m4_mvm64.
// The last workgroup of a cols / 64 that is no multiple of 4 is masked: its missing columns read column 0 (addresses stay inside the
// matrix) and their blocks are not stored.
// Stochastic rounding: output block cb takes draws 2 cb, 2 cb + 1 and, fused, 2 G + 2 cb, 2 G + 2 cb + 1 (G = cols / 64); the state is
// left advanced by 2 G (4 G): what clm4_mvm (clm4_mvm_scale_and_add) on a stored A' does.
#include "rng_device.h"
#include "mvm_device.h"
#include "nibble_transpose.h"

#define MVT_CHUNK 32768u   // rows staged in LDS per pass
#define MVT_U 2            // unroll depth in 128-row steps: 16 x 8 B loads of a lane in flight (2 / 4 / 8 and two double-buffered forms measured: DESIGN.md 3)
#define MVT_W 4            // output blocks (64 columns each) per workgroup
#define MVT_PART_STRIDE (64 * MVT_W + 1)

static_assert(MVT_W == 4, "the lane map (16 column pairs of 16 columns, one wave per output block) assumes 256 columns per workgroup");
static_assert(MVT_CHUNK % (128 * 256) == 0, "the staging loops assume whole rounds of 256 threads");
static_assert(16 * MVT_PART_STRIDE * sizeof(float) <= MVT_CHUNK / 2 + MVT_CHUNK / 64 * MVT_W * sizeof(float), "the chain ends reuse the staging area");

// U steps of 128 rows.  Ap: this lane's column pair in row 8 k of the chunk; stride: u32x2 per matrix row
template <int U, bool NT>
__device__ __forceinline__ void mvt_steps(const u32x2 *__restrict__ Ap, uint64_t stride, const uint32_t *xs, const float *cs, int k, int tile,
                                          uint32_t s0, float (&acc)[16])
{
    u32x2 a[U][8];
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const u32x2 *p = Ap + ((uint64_t)(s0 + u) * 128 + i) * stride;
            a[u][i] = NT ? __builtin_nontemporal_load(p) : *p;
        }
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint32_t xw = xs[16 * (s0 + u) + k];
        const float c = cs[MVT_W * (2 * (s0 + u) + (k >> 3)) + tile];
        uint32_t W[8], O[8];
#pragma unroll
        for (int i = 0; i < 8; i++) W[i] = a[u][i].x;
        transpose8x8_nibbles(W, O);
#pragma unroll
        for (int e = 0; e < 8; e++) acc[e] = mvm_chain_word(c, O[e], xw, acc[e]);
#pragma unroll
        for (int i = 0; i < 8; i++) W[i] = a[u][i].y;
        transpose8x8_nibbles(W, O);
#pragma unroll
        for (int e = 0; e < 8; e++) acc[8 + e] = mvm_chain_word(c, O[e], xw, acc[8 + e]);
    }
}

template <int U, bool NT, bool ST, bool FUSE>
__global__ __launch_bounds__(256) void k_m4_mvm_t(const uint8_t *__restrict__ A, const float *__restrict__ sA, uint64_t rows, uint64_t cols,
                                                  const uint8_t *__restrict__ x, const float *__restrict__ sx, uint32_t *r, float *sr,
                                                  uint64_t *rng_state, uint64_t seq, const uint64_t *__restrict__ pow_rows, MvmFuse fuse)
{
    __shared__ __attribute__((aligned(16))) char stage[MVT_CHUNK / 2 + MVT_CHUNK / 64 * MVT_W * sizeof(float)];
    __shared__ float dsh[64 * MVT_W];
    __shared__ uint64_t rbase[4], raw[8 * MVT_W], rbase2[4], raw2[8 * MVT_W];     // ST: 4 lane bases, the raw draws of MVT_W blocks (twice with FUSE)
    uint32_t *xs = reinterpret_cast<uint32_t *>(stage);                            // MVT_CHUNK / 8 words
    float *cs = reinterpret_cast<float *>(stage + MVT_CHUNK / 2);                  // [MVT_CHUNK / 64][MVT_W]
    float *part = reinterpret_cast<float *>(stage);                                // epilogue: [16 chains][MVT_PART_STRIDE]

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint64_t G = cols / 64;                                   // output blocks = column tiles of A
    const uint64_t cb0 = (uint64_t)blockIdx.x * MVT_W, cb = cb0 + wave;
    if (ST) {
        const uint64_t a0 = rng_workgroup_begin(rng_state, seq, pow_rows, cb0, 1, (FUSE ? 4ull : 2ull) * G, rbase);
        if (FUSE) {
            const uint64_t b2 = wave_pow_apply(pow_rows, a0, G + cb0, 1);
            if (lane == 0) rbase2[wave] = b2;                                      // read in the epilogue, barriers in between
        }
    }
    // FUSE: this wave's block of u, fetched now so that the epilogue does not wait for it
    uint32_t fuse_w = 0;
    float fuse_s = 0.0f;
    if (FUSE && cb < G) {
        fuse_w = fuse.qu[cb * 8 + (lane >> 3)];
        fuse_s = fuse.su[cb];
    }

    const int k = tid >> 4, cg = tid & 15, tile = cg >> 2;
    const uint64_t stride = cols / 16;                              // u32x2 per row
    const uint64_t colg = cb0 * 4 + cg;                             // this lane's column pair; beyond the matrix: column pair 0
    const u32x2 *Acol = reinterpret_cast<const u32x2 *>(A) + (colg < stride ? colg : 0);

    float acc[16];
#pragma unroll
    for (int e = 0; e < 16; e++) acc[e] = 0.0f;

    for (uint64_t r0 = 0; r0 < rows; r0 += MVT_CHUNK) {
        const uint32_t ch = (uint32_t)((rows - r0) < MVT_CHUNK ? (rows - r0) : MVT_CHUNK);
        if (r0) __syncthreads();
        // stage x and c[b][tile]: all loads first (one round trip), then the LDS writes, as k_m4_mvm64 does
        {
            constexpr int NX = MVT_CHUNK / 32 / 256;             // 16-byte pieces of x per thread
            constexpr int NC = MVT_CHUNK / 64 * MVT_W / 256;     // factors per thread
            const u32x4 *xg = reinterpret_cast<const u32x4 *>(x + r0 / 2);
            u32x4 xr[NX];
            float sa[NC], sv[NC];
            const uint32_t nx = ch / 32, nc = ch / 64 * MVT_W;
#pragma unroll
            for (int j = 0; j < NX; j++) { const uint32_t i = tid + 256 * j; xr[j] = xg[i < nx ? i : 0]; }
#pragma unroll
            for (int j = 0; j < NC; j++) {
                const uint32_t i = tid + 256 * j, ii = i < nc ? i : 0;
                const uint64_t b = r0 / 64 + ii / MVT_W, t = cb0 + ii % MVT_W;
                sa[j] = sA[b * G + (t < G ? t : 0)];
                sv[j] = sx[b];
            }
#pragma unroll
            for (int j = 0; j < NX; j++) { const uint32_t i = tid + 256 * j; if (i < nx) reinterpret_cast<u32x4 *>(xs)[i] = xr[j]; }
#pragma unroll
            for (int j = 0; j < NC; j++) { const uint32_t i = tid + 256 * j; if (i < nc) cs[i] = (sa[j] * CLV_RCP49) * sv[j]; }
        }
        __syncthreads();

        const u32x2 *Ap = Acol + (r0 + 8 * k) * stride;
        const uint32_t nsteps = ch / 128;
        uint32_t s = 0;
        for (; s + U <= nsteps; s += U) mvt_steps<U, NT>(Ap, stride, xs, cs, k, tile, s, acc);
        for (; s < nsteps; s++) mvt_steps<1, NT>(Ap, stride, xs, cs, k, tile, s, acc);
    }

    // the 16 chain ends of column c (local) = part[chain][c]; four lanes per column hold them as mvm_tree wants: quarter q = chains 4q .. 4q + 3
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 16; e++) part[k * MVT_PART_STRIDE + 16 * cg + e] = acc[e];
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < MVT_W; rr++) {
        const int col = 64 * rr + (tid >> 2), q = tid & 3;
        const float *p = part + 4 * q * MVT_PART_STRIDE + col;
        const float dot = mvm_tree(p[0], p[MVT_PART_STRIDE], p[2 * MVT_PART_STRIDE], p[3 * MVT_PART_STRIDE]);
        if (q == 0) dsh[col] = dot;
    }
    if (ST && tid < 4) {
        gen_blocks(rbase[tid], MVT_W, raw, tid);
        if (FUSE) gen_blocks(rbase2[tid], MVT_W, raw2, tid);
    }
    __syncthreads();
    if (cb < G) {                                                   // wave-uniform: one wave per output block
        float noise = 0.0f;
        if (ST) {
            const int grp = lane & 7, j = lane >> 3;
            noise = noise_of(reinterpret_cast<const uint32_t *>(raw + 8 * wave + (size_t)(grp >> 2) * 4)[j], grp & 3);
        }
        float m;
        const int qv = requantize_wave(dsh[tid], noise, r ? r + cb * 8 : nullptr, r ? sr + cb : nullptr, &m);
        if (FUSE) {
            const float su7 = div7(fuse_s), sv7 = div7(m * fuse.a);
            const float val = __builtin_fmaf((float)qv, sv7, (float)unpack1(fuse_w, lane & 7) * su7);
            float noise2 = 0.0f;
            if (ST) {
                const int g = (lane & 7) ^ 1, j = lane >> 3;
                noise2 = noise_of(reinterpret_cast<const uint32_t *>(raw2 + 8 * wave + (size_t)(g >> 2) * 4)[j], g & 3);
            }
            float m2;
            requantize_wave(val, noise2, fuse.r2 + cb * 8, fuse.sr2 + cb, &m2);
        }
    }
}

static int launch_mvm_t(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const int8_t *x, const float *sx, int8_t *r, float *sr,
                        uint64_t *rng, hipStream_t st, const MvmFuse *fuse)
{
    const uint64_t G = cols / 64;
    const dim3 grid((unsigned)((G + MVT_W - 1) / MVT_W)), block(256);
    RngTables T = {nullptr, nullptr, nullptr};
    uint64_t seq = 0;
    if (rng) {
        int rc = clv_rng_tables(&T);
        if (rc) return rc;
        seq = clv_rng_seq_for(rng, st);
    }
    const MvmFuse no_fuse = {nullptr, nullptr, 0.0f, nullptr, nullptr};
#define MVT_LAUNCH_F(NT, ST, FUSE)                                                                                                        \
    hipLaunchKernelGGL((k_m4_mvm_t<MVT_U, NT, ST, FUSE>), grid, block, 0, st, (const uint8_t *)A, sA, rows, cols, (const uint8_t *)x, sx, \
                       (uint32_t *)r, sr, rng, seq, T.pow_rows, FUSE ? *fuse : no_fuse)
#define MVT_LAUNCH(NT, ST)                                  \
    do {                                                    \
        if (fuse) MVT_LAUNCH_F(NT, ST, true);               \
        else MVT_LAUNCH_F(NT, ST, false);                   \
    } while (0)
    // streaming (nt) loads once the matrix cannot live in the 256 MiB Infinity Cache: the rule of launch_mvm (matrix4.hip)
    const bool streaming = rows * (cols / 2) > (256ull << 20);
    if (streaming) {
        if (rng) MVT_LAUNCH(true, true); else MVT_LAUNCH(true, false);
    } else {
        if (rng) MVT_LAUNCH(false, true); else MVT_LAUNCH(false, false);
    }
#undef MVT_LAUNCH
#undef MVT_LAUNCH_F
    CLV_LAUNCH_CHECK();
    return CLV_OK;
}

// the argument checks of both calls, before any device work.  qu == NULL: the plain call.  > 0: nothing to do (an empty matrix)
static int check_mvm_t_args(const char *fn, const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const int8_t *x, const float *sx,
                            bool fused, const int8_t *qu, const float *su, const int8_t *t, const float *st_, const int8_t *r, const float *sr)
{
    CLV_REQUIRE(A && sA && x && sx && r && sr && (!fused || (qu && su)), "%s: null pointer", fn);
    CLV_REQUIRE((t == nullptr) == (st_ == nullptr), "%s: t and st must both be given or both be NULL", fn);
    CLV_REQUIRE(rows % 128 == 0 && cols % 128 == 0, "%s: rows=%llu cols=%llu must be multiples of 128", fn, (unsigned long long)rows,
                (unsigned long long)cols);
    CLV_REQUIRE(cols / 64 <= 0x7FFFFFFFull, "%s: too many columns", fn);
    if (!rows || !cols) return 1;
    std::vector<ClvRange> rg;
    rg.reserve(10);
    const uint64_t sc = sizeof(float);
    rg.push_back(clv_range(A, rows * (cols / 2), false, ~0ull, "A"));
    rg.push_back(clv_range(sA, (rows / 64) * (cols / 64) * sc, false, ~0ull, "sA"));
    rg.push_back(clv_range(x, rows / 2, false, 0, "x"));
    rg.push_back(clv_range(sx, rows / 64 * sc, false, 0, "sx"));
    rg.push_back(clv_range(r, cols / 2, true, 0, "r"));
    rg.push_back(clv_range(sr, cols / 64 * sc, true, 0, "sr"));
    if (fused) {
        // the in-place result IS its input: a workgroup reads its own blocks of u before it writes them
        if ((const void *)qu != (const void *)r) rg.push_back(clv_range(qu, cols / 2, false, 0, "qu"));
        if ((const void *)su != (const void *)sr) rg.push_back(clv_range(su, cols / 64 * sc, false, 0, "su"));
        if (t) {
            rg.push_back(clv_range(t, cols / 2, true, 0, "t"));
            rg.push_back(clv_range(st_, cols / 64 * sc, true, 0, "st"));
        }
    }
    return clv_internal_check_ranges(fn, rg);
}

extern "C" int clm4_mvm_transposed(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const int8_t *x, const float *sx, int8_t *r,
                                   float *sr, uint64_t *rng_state_dev, void *stream)
{
    const int rc = check_mvm_t_args("clm4_mvm_transposed", A, sA, rows, cols, x, sx, false, nullptr, nullptr, nullptr, nullptr, r, sr);
    if (rc) return rc > 0 ? CLV_OK : rc;
    return launch_mvm_t(A, sA, rows, cols, x, sx, r, sr, rng_state_dev, as_stream(stream), nullptr);
}

extern "C" int clm4_mvm_transposed_scale_and_add(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, const int8_t *x, const float *sx,
                                                 const int8_t *qu, const float *su, float a, int8_t *t, float *st_, int8_t *r, float *sr,
                                                 uint64_t *rng_state_dev, void *stream)
{
    const int rc = check_mvm_t_args("clm4_mvm_transposed_scale_and_add", A, sA, rows, cols, x, sx, true, qu, su, t, st_, r, sr);
    if (rc) return rc > 0 ? CLV_OK : rc;
    const MvmFuse fuse = {(const uint32_t *)qu, su, a, (uint32_t *)r, sr};
    return launch_mvm_t(A, sA, rows, cols, x, sx, t, st_, rng_state_dev, as_stream(stream), &fuse);
}
