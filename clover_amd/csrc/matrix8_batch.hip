// matrix8_batch.hip -- CloverMatrix8 x CloverVector8 (the reference's pure 8-bit configuration, 02_bit08.cpp) for several right-hand
// sides: ONE pass over the matrix for up to CLM4_MVM_BATCH_MAX vectors, as mvm_batch8.hip does for the 4-bit matrix.
//
// The 8-bit matrix has twice the bytes of the 4-bit one and needs no nibble transpose or widening: a workgroup loads each 16 matrix bytes
// of a lane once and runs, per vector and block, one 16-byte LDS read of x, one of the factor, four v_dot4_i32_i8, two converts and two
// fmas.  Each vector's instruction sequence is the one of m8_mvm_body (matrix8.hip), so the results equal the single calls bit for bit;
// the re-quantisation and the scaleAndAdd behind it are mvm8_requantize_wave (mvm8_device.h), the same arithmetic as k_m8_mvm_saa's.
#include "mvm_batch_device.h"
#include "mvm8_device.h"

#include <stdlib.h>

// Columns of x staged in LDS per pass: 4 KiB of int8 + 256 B of block factors + 256 B of row dots per vector, 36 KiB at NV = 8 (36.5 KiB
// with the generator starts of the fused stochastic form): four workgroups per CU, the budget of mvm_batch8.hip.
#define M8B_CHUNK 4096u
#define M8B_THREADS 256
#define M8B_U 8          // blocks in flight per lane: 4 U registers of matrix words + 2 accumulators per vector

// the size rules of clm8_mvm (matrix8.hip)
int clv_internal_m8_check_mvm(const char *fn, const void *A, const void *sA, uint64_t rows, uint64_t cols, const void *x, const void *r);

// the vectors of one pass, BY VALUE in the kernel arguments (see MvmBatchArgs, mvm_batch4.hip).  Slots >= nv are absent: NULL, never dereferenced.
template <int NV>
struct M8BatchArgs {
    const int8_t *x[NV];
    const float *sx[NV];
    int8_t *r[NV];           // all NULL: the mvm result is not stored (FUSE only)
    float *sr[NV];
};
template <int NV>
struct M8BatchFuse {         // see M8Fuse
    const int8_t *qu[NV];
    const float *su[NV];
    int8_t *r2[NV];          // may be qu (in place)
    float *sr2[NV];
    float a;
};

#define M8B_X_BYTES(NV) ((NV) * (M8B_CHUNK + (M8B_CHUNK / 64) * sizeof(float) + 64 * sizeof(float)))
// ST: behind the row dots, per vector and window the start of each of the 4 generator lanes (32 B): 512 B at NV = 8 fused
#define M8B_LDS_BYTES(NV, ST, FUSE) (M8B_X_BYTES(NV) + ((ST) ? (NV) * ((FUSE) ? 2 : 1) * 4 * sizeof(uint64_t) : 0))

// one block (64 columns) of this lane's row: lo = bytes 8p..8p+7, hi = bytes 32+8p..32+8p+7, for every vector of the group.  x lies in
// LDS in the LANE's order: u32x4 number 4 b + p of a vector holds {x[8p..8p+7], x[32+8p..32+8p+7]} of block b, one 16-byte read.
template <int NV>
__device__ __forceinline__ void m8b_block(const u32x2 lo, const u32x2 hi, uint32_t b, int p, int nv, const u32x4 *xs, const float *cs,
                                          float (&a0)[NV], float (&a1)[NV])
{
    constexpr uint32_t XS = M8B_CHUNK / 16, CS = M8B_CHUNK / 64;
#pragma unroll
    for (int v = 0; v < NV; v++)
        if (v < nv) {
            const u32x4 xv = xs[v * XS + 4 * b + p];
            const float c = cs[v * CS + b];
            a0[v] = __builtin_fmaf(c, (float)sdot4(hi.x, xv.z, sdot4(lo.x, xv.x, 0)), a0[v]);      // chain 2p
            a1[v] = __builtin_fmaf(c, (float)sdot4(hi.y, xv.w, sdot4(lo.y, xv.y, 0)), a1[v]);      // chain 2p + 1
        }
}

// Mapping of k_m8_mvm: workgroup = one 64-row group, lane = (row rho = tid >> 2, quarter p = tid & 3) owning chains 2p and 2p + 1 of its
// row, two 8-byte matrix loads per block; per vector 2 accumulators.  amdgpu_waves_per_eu(4, 4) holds every instantiation to 128
// registers (four waves per SIMD, what the LDS allows; figures: DESIGN.md 3).  Vector v's epilogue (tree -> re-quantise [-> scaleAndAdd])
// runs on wave v & 3.  ST: the jump-ahead of mvm_batch_device.h; the draw layout is k_m8_mvm's.
template <int NV, int U, bool NT, bool FUSE, bool ST>
__global__ __launch_bounds__(M8B_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_m8_mvm_batch(
    const uint8_t *__restrict__ A, const float *__restrict__ sA, uint64_t cols, int nv, M8BatchArgs<NV> arg, M8BatchFuse<NV> fuse, MvmBatchRng rs)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr uint32_t XS = M8B_CHUNK / 16, CS = M8B_CHUNK / 64;            // per vector: u32x4 of x, factors
    u32x4 *xs = reinterpret_cast<u32x4 *>(smem);                            // NV x M8B_CHUNK bytes of int8
    float *cs = reinterpret_cast<float *>(smem + NV * M8B_CHUNK);           // NV x M8B_CHUNK / 64 factors
    float *dsh = cs + NV * CS;                                              // NV x 64 row dots
    static_assert(XS == M8B_THREADS && CS == 64, "one u32x4 of x per thread and vector, one factor per lane of the first wave");
    constexpr int NW = FUSE ? 2 : 1;                                        // windows per vector: the mvm's draws, the scaleAndAdd's
    uint64_t *sbase = reinterpret_cast<uint64_t *>(dsh + NV * 64);          // ST: [NV][NW][4] lane starts

    const uint64_t rb = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t st_seq = 0;
    uint64_t *st_next = nullptr;
    if constexpr (ST) st_next = mvmb_rng_prologue<NV, NW>(rs, nv, rb, sbase, st_seq);

    const int p = tid & 3, rho = tid >> 2;
    const uint64_t row = rb * 64 + rho;
    const u32x2 *Arow = reinterpret_cast<const u32x2 *>(A + row * cols);
    const float *sArow = sA + rb * (cols / 64);

    float a0[NV], a1[NV];
#pragma unroll
    for (int v = 0; v < NV; v++) a0[v] = a1[v] = 0.0f;

    for (uint64_t c0 = 0; c0 < cols; c0 += M8B_CHUNK) {
        const uint32_t cw = (uint32_t)((cols - c0) < M8B_CHUNK ? (cols - c0) : M8B_CHUNK);
        if (c0) __syncthreads();
        {   // stage x and the factors of every present vector: the loads first, then the LDS writes.  Thread tid holds bytes 16 q .. 16 q + 15
            // of block tid >> 2 (q = tid & 3): the 8-byte units 2 q and 2 q + 1; unit j goes to lane j & 3's u32x4, half j >> 2
            const uint32_t nx = cw / 16, nc = cw / 64;
            const uint32_t ix = (uint32_t)tid < nx ? tid : 0, ic = (uint32_t)tid < nc ? tid : 0;
            u32x4 xr[NV];
            float sv[NV];
            const float sa = sArow[c0 / 64 + ic];
#pragma unroll
            for (int v = 0; v < NV; v++)
                if (v < nv) {
                    xr[v] = reinterpret_cast<const u32x4 *>(arg.x[v] + c0)[ix];
                    sv[v] = arg.sx[v][c0 / 64 + ic];
                }
            const uint32_t j = 2 * (tid & 3), slot = 8 * (tid >> 2) + 2 * (j & 3) + (j >> 2);      // unit j + 1: slot + 2
#pragma unroll
            for (int v = 0; v < NV; v++)
                if (v < nv) {
                    u32x2 *xw = reinterpret_cast<u32x2 *>(xs + v * XS);
                    if ((uint32_t)tid < nx) {
                        xw[slot] = u32x2{xr[v].x, xr[v].y};
                        xw[slot + 2] = u32x2{xr[v].z, xr[v].w};
                    }
                    if ((uint32_t)tid < nc) cs[v * CS + tid] = (sa * (1.0f / 127.0f)) * (sv[v] * (1.0f / 127.0f));
                }
        }
        __syncthreads();

        const u32x2 *Ap = Arow + c0 / 8;
        const uint32_t nb = cw / 64;
        uint32_t b = 0;
        for (; b + U <= nb; b += U) {
            u32x2 lo[U], hi[U];                                             // each matrix byte ONCE for all vectors
#pragma unroll
            for (int u = 0; u < U; u++) {
                lo[u] = NT ? __builtin_nontemporal_load(&Ap[8 * (b + u) + p]) : Ap[8 * (b + u) + p];
                hi[u] = NT ? __builtin_nontemporal_load(&Ap[8 * (b + u) + 4 + p]) : Ap[8 * (b + u) + 4 + p];
            }
#pragma unroll
            for (int u = 0; u < U; u++) m8b_block<NV>(lo[u], hi[u], b + u, p, nv, xs, cs, a0, a1);
        }
        for (; b < nb; b++) {
            const u32x2 lo = NT ? __builtin_nontemporal_load(&Ap[8 * b + p]) : Ap[8 * b + p];
            const u32x2 hi = NT ? __builtin_nontemporal_load(&Ap[8 * b + 4 + p]) : Ap[8 * b + 4 + p];
            m8b_block<NV>(lo, hi, b, p, nv, xs, cs, a0, a1);
        }
    }

    // FUSE: this row group's block of u of the vectors whose epilogue this wave runs, requested here, behind the
    // column loop (they would cost registers across it), so that the tree and the barrier cover the latency
    int fuse_q[(NV + 3) / 4] = {};
    float fuse_s[(NV + 3) / 4] = {};
    if (FUSE) {
#pragma unroll
        for (int v = 0; v < NV; v++)
            if (v < nv && wave == (v & 3)) {
                fuse_q[v >> 2] = fuse.qu[v][rb * 64 + lane];
                fuse_s[v >> 2] = fuse.su[v][rb];
            }
    }

    // lane p holds acc[2p], acc[2p+1]: ((a0+a4)+(a2+a6))+((a1+a5)+(a3+a7)) is mvm8_tree's order (lanes p ^ 2, then p ^ 1)
#pragma unroll
    for (int v = 0; v < NV; v++)
        if (v < nv) {
            const float dot = mvm8_tree(a0[v], a1[v]);
            if (p == 0) dsh[v * 64 + rho] = dot;
        }
    __syncthreads();
    if constexpr (ST) mvmb_rng_stamp(st_next, st_seq);        // every wave's part of the new state was written before the barrier
#pragma unroll
    for (int v = 0; v < NV; v++)
        if (v < nv && wave == (v & 3)) {
            int8_t *r = arg.r[v];
            float noise = 0.0f, noise2 = 0.0f;
            if constexpr (ST) {
                // k_m8_mvm's lanes.  mvm: lane l takes draw l >> 5, word l & 7, byte (l >> 3) & 3;
                // scaleAndAdd: draw l >> 5, word (l & 31) >> 2, byte l & 3
                noise = mvmb_noise(sbase + (v * NW) * 4, lane >> 3, lane & 7);
                if (FUSE) noise2 = mvmb_noise(sbase + (v * NW + 1) * 4, ((lane >> 5) << 2) | (lane & 3), (lane & 31) >> 2);
            }
            mvm8_requantize_wave<FUSE>(dsh[v * 64 + lane], noise, noise2, lane, r ? r + rb * 64 : nullptr, r ? arg.sr[v] + rb : nullptr,
                                       fuse_q[v >> 2], fuse_s[v >> 2], fuse.a, FUSE ? fuse.r2[v] + rb * 64 : nullptr,
                                       FUSE ? fuse.sr2[v] + rb : nullptr);
        }
}

// ---- dispatch ----------------------------------------------------------------------------------------------------------------
// Whether a group of g vectors runs as one batched launch or as g single launches: CLV_MVM_BATCH as in mvm_batch4.hip (1 = always batched,
// with an rng a remainder group of ONE vector too; 0 = never); unset = the rule measured on the MI355X (DESIGN.md 3,
// profiles/m8_mvm_batch_kernel_bench.json; stochastic: profiles/m8_mvm_batch_st_kernel_bench.json): at 2, 4 and 8 vectors the batched
// launch beat the single calls by more than their spread in every row -- 65536^2 and 32768^2 (streaming), fused at 8192 x 4096
// (cache-resident) and at 65536^2, the IHT loop at N = 8192, either rounding -- so every group of two or more runs batched, whatever
// the shape.  Not measured: groups of 3 and 5-7, matrices between 32 MiB and 1 GiB or below 32 MiB.
static bool m8_batch_selected(uint64_t rows, uint64_t cols, uint64_t g, bool stochastic)
{
    if (g < 2 && !stochastic) return false;
    const char *e = clv_env("CLV_MVM_BATCH");
    if (e && *e) return atoi(e) != 0;
    if (g < 2) return false;
    (void)rows;
    (void)cols;
    return true;
}

// the draws of a batched launch on the host side: rng == NULL = rounding disabled
struct M8BatchDraws {
    uint64_t *rng;
    uint64_t base, stride, commit;
};

template <int NV>
static int launch_m8_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t g, const int8_t *const *x,
                           const float *const *sx, int8_t *const *r, float *const *sr, const int8_t *const *qu, const float *const *su, float a,
                           int8_t *const *r2, float *const *sr2, const M8BatchDraws &dr, hipStream_t st)
{
    M8BatchArgs<NV> arg;
    M8BatchFuse<NV> fuse;
    for (uint64_t v = 0; v < NV; v++) {
        const bool in = v < g;
        arg.x[v] = in ? x[v] : nullptr;
        arg.sx[v] = in ? sx[v] : nullptr;
        arg.r[v] = in && r ? r[v] : nullptr;
        arg.sr[v] = in && r ? sr[v] : nullptr;
        fuse.qu[v] = in && qu ? qu[v] : nullptr;
        fuse.su[v] = in && qu ? su[v] : nullptr;
        fuse.r2[v] = in && qu ? r2[v] : nullptr;
        fuse.sr2[v] = in && qu ? sr2[v] : nullptr;
    }
    fuse.a = a;
    MvmBatchRng rs = {nullptr, 0, nullptr, 0, 0, 0};
    if (dr.rng) {
        RngTables T = {nullptr, nullptr, nullptr};
        int rc = clv_rng_tables(&T);
        if (rc) return rc;
        // every launch takes a number of its own, committing or not: it is what picks the slot to read
        rs = MvmBatchRng{dr.rng, clv_rng_seq_for(dr.rng, st), T.pow_rows, dr.base, dr.stride, dr.commit};
    }
    const dim3 grid((unsigned)(rows / 64)), block(M8B_THREADS);
    // nontemporal loads by the rule of clm8_mvm: once the matrix cannot live in the 256 MiB Infinity Cache
    const bool streaming = rows * cols > (256ull << 20);
#define M8B_LAUNCH(NT, FUSE, ST)                                                                                                       \
    hipLaunchKernelGGL((k_m8_mvm_batch<NV, M8B_U, NT, FUSE, ST>), grid, block, M8B_LDS_BYTES(NV, ST, FUSE), st, (const uint8_t *)A, sA, cols, \
                       (int)g, arg, fuse, rs)
#define M8B_LAUNCH_R(NT, FUSE) do { if (dr.rng) M8B_LAUNCH(NT, FUSE, true); else M8B_LAUNCH(NT, FUSE, false); } while (0)
    if (streaming) { if (qu) M8B_LAUNCH_R(true, true); else M8B_LAUNCH_R(true, false); }
    else { if (qu) M8B_LAUNCH_R(false, true); else M8B_LAUNCH_R(false, false); }
#undef M8B_LAUNCH_R
#undef M8B_LAUNCH
    CLV_LAUNCH_CHECK();
    clv_internal_mvm_batch_count();
    return CLV_OK;
}

static int m8_launch_group(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t j0, uint64_t g, const int8_t *const *x,
                           const float *const *sx, int8_t *const *r, float *const *sr, const int8_t *const *qu, const float *const *su, float a,
                           int8_t *const *r2, float *const *sr2, const M8BatchDraws &dr, hipStream_t st)
{
#define M8B_GROUP(NV) \
    launch_m8_batch<NV>(A, sA, rows, cols, g, x + j0, sx + j0, r ? r + j0 : nullptr, r ? sr + j0 : nullptr, qu ? qu + j0 : nullptr, \
                        qu ? su + j0 : nullptr, a, qu ? r2 + j0 : nullptr, qu ? sr2 + j0 : nullptr, dr, st)
    return g <= 2 ? M8B_GROUP(2) : g <= 4 ? M8B_GROUP(4) : M8B_GROUP(8);
#undef M8B_GROUP
}

// the checked arguments of clm8_mvm_batch (qu == NULL) / clm8_mvm_scale_and_add_batch on the stream, group by group; r / sr NULL: the mvm
// result is not stored (fused form only).  With an rng every group starts at the state the group before it left, so batched and
// forwarded groups mix freely.
static int m8_batch_run(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                        const float *const *sx, int8_t *const *r, float *const *sr, const int8_t *const *qu, const float *const *su, float a,
                        int8_t *const *r2, float *const *sr2, uint64_t *rng, void *stream)
{
    hipStream_t st = as_stream(stream);
    const uint64_t per_vector = (qu ? 4ull : 2ull) * (rows / 64);
    for (uint64_t j0 = 0; j0 < nvec; j0 += CLM4_MVM_BATCH_MAX) {
        const uint64_t g = nvec - j0 < CLM4_MVM_BATCH_MAX ? nvec - j0 : CLM4_MVM_BATCH_MAX;
        int rc = CLV_OK;
        if (!m8_batch_selected(rows, cols, g, rng != nullptr)) {
            for (uint64_t j = j0; j < j0 + g && !rc; j++)
                rc = qu ? clm8_mvm_scale_and_add(A, sA, rows, cols, x[j], sx[j], qu[j], su[j], a, r ? r[j] : nullptr, r ? sr[j] : nullptr, r2[j],
                                                 sr2[j], rng, stream)
                        : clm8_mvm(A, sA, rows, cols, x[j], sx[j], r[j], sr[j], rng, stream);
        } else {
            rc = m8_launch_group(A, sA, rows, cols, j0, g, x, sx, r, sr, qu, su, a, r2, sr2, M8BatchDraws{rng, 0, per_vector, g * per_vector}, st);
        }
        if (rc) return rc;
    }
    return CLV_OK;
}

// The positioned form: vector j's window begins draw_base + j * draw_stride draws behind the state the call finds, across groups too;
// only the last group's launch commits.  Always the batched kernel.  rng == NULL: the deterministic kernel, the positions unused.
static int m8_batch_at(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                       const float *const *sx, int8_t *const *r, float *const *sr, const int8_t *const *qu, const float *const *su, float a,
                       int8_t *const *r2, float *const *sr2, uint64_t *rng, uint64_t draw_base, uint64_t draw_stride, uint64_t commit_draws,
                       void *stream)
{
    hipStream_t st = as_stream(stream);
    for (uint64_t j0 = 0; j0 < nvec; j0 += CLM4_MVM_BATCH_MAX) {
        const uint64_t g = nvec - j0 < CLM4_MVM_BATCH_MAX ? nvec - j0 : CLM4_MVM_BATCH_MAX;
        const bool last = j0 + g == nvec;
        int rc = m8_launch_group(A, sA, rows, cols, j0, g, x, sx, r, sr, qu, su, a, r2, sr2,
                                 M8BatchDraws{rng, draw_base + j0 * draw_stride, draw_stride, last ? commit_draws : 0}, st);
        if (rc) return rc;
    }
    return CLV_OK;
}

// ---- C ABI -------------------------------------------------------------------------------------------------------------------
// every check of the three mvm calls, before any device work
static int m8_check_batch_args(const char *fn, const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                               const float *const *sx, const int8_t *const *qu, const float *const *su, int8_t *const *t, float *const *st_,
                               int8_t *const *r, float *const *sr, bool fused)
{
    // a NULL vector array is reported as such, not as one of the single call's pointers
    int rc = clv_internal_m8_check_mvm(fn, A, sA, rows, cols, A, A);
    if (rc) return rc;
    if (!nvec) return CLV_OK;
    CLV_REQUIRE(x && sx && r && sr && (!fused || (qu && su)), "%s: null pointer array", fn);
    CLV_REQUIRE((t == nullptr) == (st_ == nullptr), "%s: t and st must both be given or both be NULL", fn);
    for (uint64_t j = 0; j < nvec; j++)
        CLV_REQUIRE(x[j] && sx[j] && r[j] && sr[j] && (!fused || (qu[j] && su[j])) && (!t || (t[j] && st_[j])), "%s: null pointer in vector %llu", fn,
                    (unsigned long long)j);
    for (uint64_t j = 0; j < nvec; j++)
        CLV_REQUIRE((const void *)r[j] != (const void *)x[j] && (const void *)sr[j] != (const void *)sx[j],
                    "%s: the result of vector %llu must not alias the vector being multiplied", fn, (unsigned long long)j);
    std::vector<ClvRange> rg;
    rg.reserve(8 * nvec + 2);
    const uint64_t sc = sizeof(float);
    rg.push_back(clv_range(A, rows * cols, false, ~0ull, "A"));
    rg.push_back(clv_range(sA, (rows / 64) * (cols / 64) * sc, false, ~0ull, "sA"));
    for (uint64_t j = 0; j < nvec; j++) {
        rg.push_back(clv_range(x[j], cols, false, j, "x"));
        rg.push_back(clv_range(sx[j], cols / 64 * sc, false, j, "sx"));
        rg.push_back(clv_range(r[j], rows, true, j, "r"));
        rg.push_back(clv_range(sr[j], rows / 64 * sc, true, j, "sr"));
        if (fused) {
            // the in-place form r[j] == qu[j], sr[j] == su[j]: the result IS the input, only workgroup rb touches block rb of either
            const bool in_place = (const void *)r[j] == (const void *)qu[j] && (const void *)sr[j] == (const void *)su[j];
            if (!in_place) {
                rg.push_back(clv_range(qu[j], rows, false, j, "qu"));
                rg.push_back(clv_range(su[j], rows / 64 * sc, false, j, "su"));
            }
        }
        if (t) {
            rg.push_back(clv_range(t[j], rows, true, j, "t"));
            rg.push_back(clv_range(st_[j], rows / 64 * sc, true, j, "st"));
        }
    }
    return clv_internal_check_ranges(fn, rg);
}

extern "C" int clm8_mvm_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                              const float *const *sx, int8_t *const *r, float *const *sr, uint64_t *rng_state_dev, void *stream)
{
    int rc = m8_check_batch_args("clm8_mvm_batch", A, sA, rows, cols, nvec, x, sx, nullptr, nullptr, nullptr, nullptr, r, sr, false);
    if (rc) return rc;
    if (!nvec || !rows) return CLV_OK;
    if (nvec == 1) return clm8_mvm(A, sA, rows, cols, x[0], sx[0], r[0], sr[0], rng_state_dev, stream);
    return m8_batch_run(A, sA, rows, cols, nvec, x, sx, r, sr, nullptr, nullptr, 0.0f, nullptr, nullptr, rng_state_dev, stream);
}

extern "C" int clm8_mvm_batch_at(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                                 const float *const *sx, int8_t *const *r, float *const *sr, uint64_t *rng_state_dev, uint64_t draw_base,
                                 uint64_t draw_stride, uint64_t commit_draws, void *stream)
{
    const char *fn = "clm8_mvm_batch_at";
    int rc = m8_check_batch_args(fn, A, sA, rows, cols, nvec, x, sx, nullptr, nullptr, nullptr, nullptr, r, sr, false);
    if (rc) return rc;
    if (!rng_state_dev) return clm8_mvm_batch(A, sA, rows, cols, nvec, x, sx, r, sr, nullptr, stream);
    CLV_REQUIRE(commit_draws < (1ull << (RNG_POW_LEVELS - 1)), "%s: commit_draws=%llu must stay below 2^55", fn, (unsigned long long)commit_draws);
    const uint64_t bad = clv_internal_first_bad_window(nvec, draw_base, draw_stride, 2 * (rows / 64));
    CLV_REQUIRE(bad == nvec, "%s: the draws of vector %llu (draw_base=%llu, draw_stride=%llu) do not stay below 2^55", fn, (unsigned long long)bad,
                (unsigned long long)draw_base, (unsigned long long)draw_stride);
    if (!nvec || !rows) return CLV_OK;
    return m8_batch_at(A, sA, rows, cols, nvec, x, sx, r, sr, nullptr, nullptr, 0.0f, nullptr, nullptr, rng_state_dev, draw_base, draw_stride,
                       commit_draws, stream);
}

extern "C" int clm8_mvm_scale_and_add_batch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                                            const float *const *sx, const int8_t *const *qu, const float *const *su, float a, int8_t *const *t,
                                            float *const *st_, int8_t *const *r, float *const *sr, uint64_t *rng_state_dev, void *stream)
{
    int rc = m8_check_batch_args("clm8_mvm_scale_and_add_batch", A, sA, rows, cols, nvec, x, sx, qu, su, t, st_, r, sr, true);
    if (rc) return rc;
    if (!nvec || !rows) return CLV_OK;
    if (nvec == 1)
        return clm8_mvm_scale_and_add(A, sA, rows, cols, x[0], sx[0], qu[0], su[0], a, t ? t[0] : nullptr, t ? st_[0] : nullptr, r[0], sr[0],
                                      rng_state_dev, stream);
    return m8_batch_run(A, sA, rows, cols, nvec, x, sx, t, st_, qu, su, a, r, sr, rng_state_dev, stream);
}

// Q_IHT / Q_GD over a CloverMatrix8 for nvec signals with one Phi: the loop of clm8_iht with every step batched.  Arrays are HOST arrays of
// nvec device pointers.  Bit-identical to clm8_iht per vector; no single clm8_iht takes a persistent kernel.
extern "C" int clm8_iht_batch(const int8_t *Phi, const float *sPhi, const int8_t *PhiT, const float *sPhiT, uint64_t m, uint64_t n, uint64_t nvec,
                              int8_t *const *x, float *const *sx, uint64_t x_len, const int8_t *const *y, const float *const *sy,
                              int8_t *const *t1, float *const *st1, int8_t *const *t2, float *const *st2, int8_t *const *t3, float *const *st3,
                              uint64_t iterations, uint64_t K, float mu, int threshold, uint64_t *rng_state_dev, void *stream)
{
    const char *fn = "clm8_iht_batch";
    CLV_REQUIRE(Phi && sPhi && PhiT && sPhiT, "%s: null pointer", fn);
    CLV_REQUIRE(m % 128 == 0 && n % 128 == 0 && x_len <= n, "%s: m=%llu n=%llu x_len=%llu", fn, (unsigned long long)m, (unsigned long long)n,
                (unsigned long long)x_len);
    CLV_REQUIRE(m / 64 <= 0x7FFFFFFFull && n / 64 <= 0x7FFFFFFFull, "%s: too many rows", fn);
    if (!nvec) return CLV_OK;
    CLV_REQUIRE(x && sx && y && sy && t1 && st1 && t2 && st2 && t3 && st3, "%s: null pointer array", fn);
    for (uint64_t j = 0; j < nvec; j++)
        CLV_REQUIRE(x[j] && sx[j] && y[j] && sy[j] && t1[j] && st1[j] && t2[j] && st2[j] && t3[j] && st3[j], "%s: null pointer in vector %llu", fn,
                    (unsigned long long)j);
    {
        std::vector<ClvRange> rg;
        rg.reserve(10 * nvec + 4);
        const uint64_t sc = sizeof(float), tiles = (m / 64) * (n / 64);
        rg.push_back(clv_range(Phi, m * n, false, ~0ull, "Phi"));
        rg.push_back(clv_range(sPhi, tiles * sc, false, ~0ull, "sPhi"));
        rg.push_back(clv_range(PhiT, m * n, false, ~0ull, "PhiT"));
        rg.push_back(clv_range(sPhiT, tiles * sc, false, ~0ull, "sPhiT"));
        for (uint64_t j = 0; j < nvec; j++) {
            rg.push_back(clv_range(y[j], m, false, j, "y"));
            rg.push_back(clv_range(sy[j], m / 64 * sc, false, j, "sy"));
            rg.push_back(clv_range(x[j], n, true, j, "x"));
            rg.push_back(clv_range(sx[j], n / 64 * sc, true, j, "sx"));
            rg.push_back(clv_range(t1[j], m, true, j, "t1"));
            rg.push_back(clv_range(st1[j], m / 64 * sc, true, j, "st1"));
            rg.push_back(clv_range(t2[j], m, true, j, "t2"));
            rg.push_back(clv_range(st2[j], m / 64 * sc, true, j, "st2"));
            rg.push_back(clv_range(t3[j], n, true, j, "t3"));
            rg.push_back(clv_range(st3[j], n / 64 * sc, true, j, "st3"));
        }
        int rc = clv_internal_check_ranges(fn, rg);
        if (rc) return rc;
    }
    // Which groups run the batched loop: the rule of the fused mvm (m8_batch_selected; a single clm8_iht is the launch-per-step loop with
    // the same three launches per iteration per SIGNAL).  CLV_MVM_BATCH = 1 / 0 forces one or the other.
    // The draws keep the order of the single calls, all iterations of vector 0 first: one iteration draws P = 4 (m / 64) + 4 (n / 64), so
    // vector j of a group has its Phi window of iteration `it` at (j * iterations + it) * P and its PhiT window 4 (m / 64) further on; only
    // the group's last launch commits, all g * iterations * P.
    const uint64_t P = 4 * (m / 64) + 4 * (n / 64);
    hipStream_t st = as_stream(stream);
    for (uint64_t j0 = 0; j0 < nvec; j0 += CLM4_MVM_BATCH_MAX) {
        const uint64_t g = nvec - j0 < CLM4_MVM_BATCH_MAX ? nvec - j0 : CLM4_MVM_BATCH_MAX;
        bool batched = g >= 2 && m && n && m8_batch_selected(m, n, g, rng_state_dev != nullptr);
        if (rng_state_dev && P && iterations > ((1ull << 55) - 1) / (g * P)) batched = false;      // positions beyond the jump-ahead tables
        if (!batched) {
            for (uint64_t j = j0; j < j0 + g; j++) {
                int rc = clm8_iht(Phi, sPhi, PhiT, sPhiT, m, n, x[j], sx[j], x_len, y[j], sy[j], t1[j], st1[j], t2[j], st2[j], t3[j], st3[j],
                                  iterations, K, mu, threshold, rng_state_dev, stream);
                if (rc) return rc;
            }
            continue;
        }
        for (uint64_t j = j0; j < j0 + g; j++) {
            int rc = clv_internal_v8_clear(x[j], sx[j], n, st);      // x.clear()
            if (rc) return rc;
        }
        const uint64_t stride = iterations * P;
        for (uint64_t it = 0; it < iterations; it++) {
            // t1 = Phi * x, t2 = y - t1;  t3 = Phi' * t2, x += mu * t3;  keep the K largest: three launches for the group
            const uint64_t commit = it + 1 == iterations ? g * stride : 0;
            int rc = m8_batch_at(Phi, sPhi, m, n, g, x + j0, sx + j0, t1 + j0, st1 + j0, y + j0, sy + j0, -1.0f, t2 + j0, st2 + j0, rng_state_dev,
                                 it * P, stride, 0, stream);
            if (!rc)
                rc = m8_batch_at(PhiT, sPhiT, n, m, g, t2 + j0, st2 + j0, t3 + j0, st3 + j0, x + j0, sx + j0, mu, x + j0, sx + j0, rng_state_dev,
                                 it * P + 4 * (m / 64), stride, commit, stream);
            if (!rc && threshold)
                rc = clv8_threshold_batch(x + j0, sx + j0, g, x_len, n, K, threshold == 2 ? CLV_THRESHOLD_REFERENCE : CLV_THRESHOLD_FAST, stream);
            if (rc) return rc;
        }
    }
    return CLV_OK;
}
