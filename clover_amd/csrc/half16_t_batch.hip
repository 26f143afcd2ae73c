// half16_t_batch.hip -- the batched transposed half-precision mvm: r[j] = f16(A' x[j]) for up to CLM4_MVM_BATCH_MAX CloverVector16 in ONE
// pass over a CloverMatrix16's own bytes, no stored transpose, and the half-precision IHT / GD loop for several signals that holds ONE
// matrix.  include/clover_hip_batch_f16_t.h is the contract: bit for bit the single calls of half16_t.hip, vector after vector.
//
// The kernel keeps the mapping of k_f16_mvm_t (half16_t.hip): a workgroup owns a strip of F16TB_COLS(NV) columns and walks ALL rows (a chain is
// ordered over all rows); a lane owns (cg = a column group of 8 halves, one 16-byte load) x (L = a chain group of CPL rows of every 32-row
// block).  Each matrix load and its widening to fp32 happens ONCE; per present vector the lane then runs the single kernel's fma steps
// into 8 CPL accumulators of that vector's own.  Vectors are independent chains, which is what makes the bits equal.
//   pipeline  = F16TB_U(NV) 32-row blocks of loads per register set, two sets that take turns: the set ahead is requested
//               unconditionally, clamped to the last block, before the arithmetic of the current one; every address stays inside the matrix;
//   x         = staged per F16TB_CHUNK rows in LDS as BINARY16 (2 KiB per vector; widened in the lane, exact either way): every thread
//               issues all its loads first, then the LDS writes; a lane reads its CPL values of a block and vector as one broadcast read;
//   epilogue  = one vector at a time: the 32 chain ends of every column through LDS -- the staging area again -- to one lane: the tree,
//               the conversion and the fused epilogue written as in k_f16_mvm_t.  u[v][col] is fetched before the walk, so r[v] may be u[v].
// Slots v >= nv are absent: never staged, never accumulated, never stored, their pointers never dereferenced.
//
// The host side is a small driver of its own in the style of half16_batch.hip.
#include "half16_batch.h"
#include "mvm_batch_host.h"

#include "clover_hip_batch_f16.h"
#include "clover_hip_batch_f16_t.h"
#include "clover_hip_f16_t.h"

// Chosen by budget from the single kernel, then timed against their neighbours ("A'x for several CloverVector16";
// profiles/f16_mvm_transposed_batch_variants.json):
//   the strip is the single kernel's 128 columns at NV = 2 and 4 (CPL = 2: 16 accumulators per vector and lane) and 64 at NV = 8 (CPL = 1:
//   8 per vector, 64 in all -- at 128 columns the 128 accumulators left hipcc at 340 registers, one wave per SIMD, or in scratch; not
//   timed).  Swept: 64 columns at NV = 2 and 4 are 21 % faster on the cache-resident step and 3 - 15 % slower once the matrix streams;
//   256 columns at NV = 2 (with U = 2; U = 4 spills) win 8 % at 65536^2 and lose 22 % at 32768^2 and 60 % in the cache;
//   two sets of U = 4 blocks are 32 CPL load registers.  Swept: U = 2 is 2 - 7 % faster at NV = 2 while streaming, 4 % slower in the
//   cache, and 9 - 12 % slower at NV = 8; U = 8 at NV = 2 is level (beyond NV = 2 it spills);
//   the chunk makes 8 vectors of binary16 x exactly the 16 KiB the chain ends of a 128-column strip need: LDS is 16 KiB for every NV.
//   Not swept (2048 rows spill at NV = 8 under two waves per SIMD).
// (the #ifndef lets tools/f16_tb_variants.py build the other values it times)
#ifndef F16TB_COLS
#define F16TB_COLS(NV) ((NV) == 8 ? 64 : 128)      // columns per workgroup
#endif
#ifndef F16TB_CHUNK
#define F16TB_CHUNK 1024u                          // rows of x staged in LDS per pass and vector
#endif
#ifndef F16TB_U
#define F16TB_U(NV) 4                              // 32-row blocks of matrix loads per register set
#endif
#define F16TB_XS (F16TB_CHUNK / 8)                 // 16-byte pieces of x per vector and chunk

static_assert(256 % F16TB_XS == 0 && F16TB_CHUNK % 32 == 0, "a round of the 256 staging threads is whole vectors of a chunk");

// the vectors of one launch, by value in the kernel arguments.  r: the f16 A' x[v] (under FUSE: t of the ABI, NULL = not stored); under
// FUSE r2[v][col] = f16(fma(f32(f16(A' x[v])), a, f32(u[v][col]))), r2[v] may be u[v]
template <int NV>
struct F16TBatchArgs {
    const uint16_t *x[NV];
    uint16_t *r[NV];
    const uint16_t *u[NV];
    uint16_t *r2[NV];
    float a;
};

// a lane's CPL values of x of one block and vector: one LDS read
template <int CPL>
struct alignas(2 * CPL) F16TBX {
    _Float16 h[CPL];
};

// stage x of every present vector for the chunk that starts at row r0, as binary16: thread (v0 = tid / XS, i = tid % XS) takes piece i
// of vectors v0, v0 + PER, ...: all loads first (one round trip), then the LDS writes
template <int NV>
__device__ __forceinline__ void f16tb_stage(u32x4 *xs, const F16TBatchArgs<NV> &arg, int nv, uint64_t rows, uint64_t r0, int tid)
{
    constexpr int PER = 256 / F16TB_XS, NR = NV / PER;                       // vectors per round of the workgroup, rounds
    static_assert(NV % PER == 0, "whole rounds");
    const uint32_t ch = (uint32_t)((rows - r0) < F16TB_CHUNK ? (rows - r0) : F16TB_CHUNK), nx = ch / 8;
    const uint32_t i = tid % F16TB_XS;
    const int v0 = tid / F16TB_XS;
    if (r0) __syncthreads();                             // the previous chunk's x has been consumed
    u32x4 xr[NR];
#pragma unroll
    for (int k = 0; k < NR; k++) {
        // the slot by selects over constant indices: the argument array is never indexed by a run-time value
        const uint16_t *p = arg.x[PER * k];
#pragma unroll
        for (int q = 1; q < PER; q++)
            if (v0 == q) p = arg.x[PER * k + q];
        if (PER * k + v0 < nv) xr[k] = reinterpret_cast<const u32x4 *>(p + r0)[i < nx ? i : 0];
    }
#pragma unroll
    for (int k = 0; k < NR; k++)
        if (PER * k + v0 < nv && i < nx) xs[(PER * k + v0) * F16TB_XS + i] = xr[k];
    __syncthreads();
}

// the loads of group g (U blocks, CPL rows each) of the lane whose first row of block 0 and column group Ap points at; blocks beyond the
// last one read the last one again
template <int U, int CPL, bool NT>
__device__ __forceinline__ void f16tb_load(const h16x8 *__restrict__ Ap, uint64_t stride, uint32_t g, uint32_t nblk, h16x8 (&a)[U][CPL])
{
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint32_t b = g * U + u, bc = b < nblk ? b : nblk - 1;
#pragma unroll
        for (int i = 0; i < CPL; i++) a[u][i] = ld_stream<NT>(Ap + ((uint64_t)bc * 32 + i) * stride);
    }
}

// the chain steps of one block for every present vector: the widening of the block's matrix values once, then per vector the steps of
// f16t_block (half16_t.hip).  xb = the lane's CPL values of vector 0 in LDS; vector v lies F16TB_CHUNK halves further on
template <int NV, int CPL>
__device__ __forceinline__ void f16tb_block(const h16x8 (&a)[CPL], const _Float16 *xb, int nv, float (&acc)[NV][CPL][8])
{
    float af[CPL][8];
#pragma unroll
    for (int i = 0; i < CPL; i++)
#pragma unroll
        for (int e = 0; e < 8; e++) af[i][e] = (float)a[i][e];
#pragma unroll
    for (int v = 0; v < NV; v++)
        if (v < nv) {
            const F16TBX<CPL> xv = *reinterpret_cast<const F16TBX<CPL> *>(xb + v * F16TB_CHUNK);
#pragma unroll
            for (int i = 0; i < CPL; i++) {
                const float xf = (float)xv.h[i];
#pragma unroll
                for (int e = 0; e < 8; e++) acc[v][i][e] = __builtin_fmaf(xf, af[i][e], acc[v][i][e]);
            }
        }
}

// group g of the walk from `cur` (loaded a group ago) while the next group's loads go to `nxt` -- issued UNCONDITIONALLY (beyond the last
// block: the last block again), so that the wait for `cur` lets them stay in flight (f16t_group, half16_t.hip)
template <int NV, int U, int CPL, bool NT>
__device__ __forceinline__ void f16tb_group(const h16x8 (&cur)[U][CPL], h16x8 (&nxt)[U][CPL], const h16x8 *__restrict__ Ap, uint64_t stride,
                                            uint32_t g, uint32_t nblk, const _Float16 *xl, int nv, float (&acc)[NV][CPL][8])
{
    constexpr uint32_t CB = F16TB_CHUNK / 32;            // blocks per chunk
    f16tb_load<U, CPL, NT>(Ap, stride, g + 1, nblk, nxt);
    const uint32_t b0 = g * U, lb = b0 % CB;             // a group never straddles a chunk
    if (nblk - b0 >= (uint32_t)U) {
#pragma unroll
        for (int u = 0; u < U; u++) f16tb_block<NV, CPL>(cur[u], xl + 32 * (lb + u), nv, acc);
    } else {
#pragma unroll
        for (int u = 0; u < U; u++)
            if (b0 + u < nblk) f16tb_block<NV, CPL>(cur[u], xl + 32 * (lb + u), nv, acc);
    }
}

// amdgpu_waves_per_eu(2): 256 registers, two of these four-wave workgroups per CU; no instantiation needs scratch for it
template <int NV, bool NT, bool FUSE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_f16_mvm_t_batch(const uint16_t *__restrict__ A, uint64_t rows, uint64_t cols,
                                                                                                 int nv, F16TBatchArgs<NV> arg)
{
    constexpr int U = F16TB_U(NV), COLS = F16TB_COLS(NV);
    constexpr int CG = COLS / 8, CPL = 32 / (256 / CG);  // column groups = lanes per row; chains (rows of a 32-row block) per lane
    constexpr uint32_t XBYTES = NV * F16TB_CHUNK * 2, PBYTES = 32 * COLS * 4;
    static_assert(COLS == 64 || COLS == 128 || COLS == 256, "the lane map is (COLS / 8 column groups) x (256 / that many chain groups); one lane per column in the epilogue");
    static_assert((F16TB_CHUNK / 32) % (2 * U) == 0, "a chunk is whole pairs of load groups");
    // x of the chunk during the walk, then part[chain][column] of one vector at a time
    __shared__ __attribute__((aligned(16))) unsigned char lds[XBYTES > PBYTES ? XBYTES : PBYTES];
    float *part = reinterpret_cast<float *>(lds);
    constexpr bool PARTIAL = COLS > 128;                                           // cols % 128 == 0 makes narrower strips whole

    const int tid = threadIdx.x, cg = tid % CG, L = tid / CG;
    const uint64_t strip0 = (uint64_t)blockIdx.x * COLS;
    // the epilogue's lane of column strip0 + tid: its element of every u, fetched now so that the epilogue does not wait for it (and r may be u)
    const uint64_t col = strip0 + tid;
    const bool owner = tid < COLS && (!PARTIAL || col < cols);
    uint16_t fuse_u[NV];
#pragma unroll
    for (int v = 0; v < NV; v++) {
        fuse_u[v] = 0;
        if (FUSE && v < nv && owner) fuse_u[v] = arg.u[v][col];
    }

    const uint64_t stride = cols / 8;                                              // 16-byte groups per row
    uint64_t c0 = strip0 + 8 * (uint64_t)cg;
    if (PARTIAL && c0 >= cols) c0 = strip0;                                        // loads stay inside the matrix; nothing of it is stored
    const h16x8 *Ap = reinterpret_cast<const h16x8 *>(A) + c0 / 8 + (uint64_t)(CPL * L) * stride;
    const _Float16 *xl = reinterpret_cast<const _Float16 *>(lds) + CPL * L;

    float acc[NV][CPL][8];
#pragma unroll
    for (int v = 0; v < NV; v++)
#pragma unroll
        for (int i = 0; i < CPL; i++)
#pragma unroll
            for (int e = 0; e < 8; e++) acc[v][i][e] = 0.0f;

    // the walk over all rows in groups of U blocks; a chunk is a whole, even number of groups, so x is re-staged in front of an even
    // group.  Two register sets take turns: no copies, and the loads of the group ahead stay in flight across the staging
    constexpr uint32_t CGR = F16TB_CHUNK / 32 / U;
    const uint32_t nblk = (uint32_t)(rows / 32), ngroups = (nblk + U - 1) / U;
    h16x8 a[U][CPL], b[U][CPL];
    f16tb_load<U, CPL, NT>(Ap, stride, 0, nblk, a);
    uint32_t g = 0;
    for (; g + 1 < ngroups; g += 2) {
        if (g % CGR == 0) f16tb_stage<NV>(reinterpret_cast<u32x4 *>(lds), arg, nv, rows, (uint64_t)g * U * 32, tid);
        f16tb_group<NV, U, CPL, NT>(a, b, Ap, stride, g, nblk, xl, nv, acc);
        f16tb_group<NV, U, CPL, NT>(b, a, Ap, stride, g + 1, nblk, xl, nv, acc);
    }
    if (g < ngroups) {
        if (g % CGR == 0) f16tb_stage<NV>(reinterpret_cast<u32x4 *>(lds), arg, nv, rows, (uint64_t)g * U * 32, tid);
        f16tb_group<NV, U, CPL, NT>(a, b, Ap, stride, g, nblk, xl, nv, acc);
    }

    // vector after vector, the 32 chain ends of every column meet in the column's lane
#pragma unroll
    for (int v = 0; v < NV; v++)
        if (v < nv) {
            __syncthreads();                             // the last chunk's x, or the chain ends of the vector before, have been consumed
#pragma unroll
            for (int i = 0; i < CPL; i++) {
                f32x4 *p = reinterpret_cast<f32x4 *>(part + (CPL * L + i) * COLS + 8 * cg);
                p[0] = f32x4{acc[v][i][0], acc[v][i][1], acc[v][i][2], acc[v][i][3]};
                p[1] = f32x4{acc[v][i][4], acc[v][i][5], acc[v][i][6], acc[v][i][7]};
            }
            __syncthreads();
            if (owner) {
                float s[8];
#pragma unroll
                for (int l = 0; l < 8; l++)
                    s[l] = (part[l * COLS + tid] + part[(8 + l) * COLS + tid]) + (part[(16 + l) * COLS + tid] + part[(24 + l) * COLS + tid]);
                const float t0 = s[4] + s[0], t1 = s[5] + s[1], t2 = s[6] + s[2], t3 = s[7] + s[3];
                const float d = (t0 + t2) + (t1 + t3);
                if (FUSE) f16_fuse_store(arg.r[v], col, d, fuse_u[v], F16Fuse{arg.u[v], arg.a, arg.r2[v]});
                else arg.r[v][col] = f16_bits(d);
            }
        }
}

// ---- host driver -------------------------------------------------------------------------------------------------------------
// one launch for the first g <= NV vectors of v (F16BatchVectors, half16_batch.h: here x[j] has `rows` elements, the others `cols`)
template <int NV>
static int f16tb_launch(const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t g, const F16BatchVectors &v, hipStream_t st)
{
    F16TBatchArgs<NV> arg;
    const bool fused = v.u != nullptr;
    for (uint64_t i = 0; i < NV; i++) {
        const bool in = i < g;
        arg.x[i] = in ? v.x[i] : nullptr;
        arg.r[i] = !in ? nullptr : fused ? (v.t ? v.t[i] : nullptr) : v.r[i];
        arg.u[i] = in && fused ? v.u[i] : nullptr;
        arg.r2[i] = in && fused ? v.r[i] : nullptr;
    }
    arg.a = v.a;
    const dim3 grid((unsigned)((cols + F16TB_COLS(NV) - 1) / F16TB_COLS(NV))), block(256);
    const int nv = (int)g;
    // nontemporal loads by the rule of the single calls: once the matrix cannot live in the 256 MiB Infinity Cache
    const bool nt = F16_STREAMING(rows * cols * 2);
    switch (2 * nt + fused) {
    case 3: hipLaunchKernelGGL((k_f16_mvm_t_batch<NV, true, true>), grid, block, 0, st, A, rows, cols, nv, arg); break;
    case 2: hipLaunchKernelGGL((k_f16_mvm_t_batch<NV, true, false>), grid, block, 0, st, A, rows, cols, nv, arg); break;
    case 1: hipLaunchKernelGGL((k_f16_mvm_t_batch<NV, false, true>), grid, block, 0, st, A, rows, cols, nv, arg); break;
    default: hipLaunchKernelGGL((k_f16_mvm_t_batch<NV, false, false>), grid, block, 0, st, A, rows, cols, nv, arg); break;
    }
    CLV_LAUNCH_CHECK();
    clv_internal_mvm_batch_count();
    return CLV_OK;
}

// a group of g <= CLM4_MVM_BATCH_MAX vectors on the smallest instantiation that holds it
static int f16tb_launch_group(const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t g, const F16BatchVectors &v, hipStream_t st)
{
    return g <= 2 ? f16tb_launch<2>(A, rows, cols, g, v, st) : g <= 4 ? f16tb_launch<4>(A, rows, cols, g, v, st) : f16tb_launch<8>(A, rows, cols, g, v, st);
}

// Whether a group of g vectors of a call of two or more runs as one batched launch or as g single transposed launches.  CLV_MVM_BATCH =
// 1 / 0 forces one or the other for every group -- forced to 1 a remainder group of ONE vector (nvec = 9, 17, ...) runs batched too, so
// that a forced call is ceil(nvec / 8) batched launches and nothing else.  Unset = the rule measured on the MI355X ("A'x for
// several CloverVector16, one CloverMatrix16"; profiles/f16_mvm_transposed_batch_kernel_bench.json for 2, 4 and 8 vectors,
// profiles/f16_mvm_transposed_batch_groups_kernel_bench.json for 3, 5, 6 and 7): batched exactly where the batched launch beat the g single
// transposed calls by more than the spread of their rounds -- which is every group of two or more in both size classes:
//   a streaming matrix (above the 256 MiB rule; 32768^2 and 65536^2, plain, and fused at 65536^2): 2: 2.0 x ... 8: 5.2 - 5.3 x;
//   a cache-resident one (the fused step on Phi 4096 x 8192, 64 MiB): 2: 1.11 x (0.0281 against 0.0310 ms, spread 0.0004), 3: 1.12,
//   4: 1.31, 5: 1.55, 8: 1.93; the loop at N = 8192 for 8 signals 1.49 x.
// Not measured: the plain call in the cache-resident class (it takes the fused step's numbers), matrices between 64 MiB and 1 GiB and
// below 64 MiB, the loop for groups other than 8.
static bool f16tb_selected(uint64_t g, uint64_t, uint64_t)
{
    const int force = mvm_batch_forced();
    if (force >= 0) return force != 0;
    return g >= 2;
}

// the checked arguments of clm_f16_mvm_transposed_batch (v.u == NULL) / clm_f16_mvm_transposed_scale_and_add_batch on the stream, group by group
static int f16tb_run(const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t nvec, const F16BatchVectors &v, void *stream)
{
    for (uint64_t j0 = 0; j0 < nvec; j0 += CLM4_MVM_BATCH_MAX) {
        const uint64_t g = nvec - j0 < CLM4_MVM_BATCH_MAX ? nvec - j0 : CLM4_MVM_BATCH_MAX;
        int rc = CLV_OK;
        if (!f16tb_selected(g, rows, cols)) {
            for (uint64_t j = j0; j < j0 + g && !rc; j++)
                rc = v.u ? clm_f16_mvm_transposed_scale_and_add(A, rows, cols, v.x[j], v.u[j], v.a, v.t ? v.t[j] : nullptr, v.r[j], stream)
                         : clm_f16_mvm_transposed(A, rows, cols, v.x[j], v.r[j], stream);
        } else {
            rc = f16tb_launch_group(A, rows, cols, g, v.from(j0), as_stream(stream));
        }
        if (rc) return rc;
    }
    return CLV_OK;
}

// every check of the two product calls, before any device work: the single transposed call's size and alignment rules, then the arrays,
// the entries, the aliases the single calls refuse by name and the overlap check -- x sized by the ROWS, r / u / t by the COLUMNS.
// u == NULL and t == NULL in the plain call.
static int f16tb_check_args(const char *fn, const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t nvec, const uint16_t *const *x,
                            const uint16_t *const *u, uint16_t *const *t, uint16_t *const *r, bool fused)
{
    CLV_REQUIRE(A, "%s: null pointer", fn);
    CLV_REQUIRE(rows % 128 == 0 && cols % 128 == 0, "%s: rows=%llu cols=%llu must be multiples of 128", fn, (unsigned long long)rows,
                (unsigned long long)cols);
    CLV_REQUIRE(F16_ALIGNED(A), "%s: the matrix and x must be 16-byte aligned", fn);
    CLV_REQUIRE(!cols || rows <= 0xFFFFFFFFFFFFull / cols, "%s: matrix too large", fn);
    CLV_REQUIRE(rows / 32 <= 0x7FFFFFFFull && cols / 64 <= 0x7FFFFFFFull, "%s: matrix too large", fn);
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
    const uint64_t xb = rows * 2, rb = cols * 2;
    rg.push_back(clv_range(A, rows * cols * 2, false, ~0ull, "A"));
    for (uint64_t j = 0; j < nvec; j++) {
        rg.push_back(clv_range(x[j], xb, false, j, "x"));
        rg.push_back(clv_range(r[j], rb, true, j, "r"));
        // the in-place form r[j] == u[j]: the result IS the input, only the lane that owns a column touches it in either
        if (fused && r[j] != u[j]) rg.push_back(clv_range(u[j], rb, false, j, "u"));
        if (t) rg.push_back(clv_range(t[j], rb, true, j, "t"));
    }
    return clv_internal_check_ranges(fn, rg);
}

// ---- C ABI -------------------------------------------------------------------------------------------------------------------
extern "C" int clm_f16_mvm_transposed_batch(const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t nvec, const uint16_t *const *x,
                                            uint16_t *const *r, void *stream)
{
    int rc = f16tb_check_args("clm_f16_mvm_transposed_batch", A, rows, cols, nvec, x, nullptr, nullptr, r, false);
    if (rc) return rc;
    if (!nvec || !rows || !cols) return CLV_OK;
    if (nvec == 1) return clm_f16_mvm_transposed(A, rows, cols, x[0], r[0], stream);
    return f16tb_run(A, rows, cols, nvec, {x, nullptr, 0.0f, nullptr, r}, stream);
}

extern "C" int clm_f16_mvm_transposed_scale_and_add_batch(const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t nvec, const uint16_t *const *x,
                                                          const uint16_t *const *u, float a, uint16_t *const *t, uint16_t *const *r, void *stream)
{
    int rc = f16tb_check_args("clm_f16_mvm_transposed_scale_and_add_batch", A, rows, cols, nvec, x, u, t, r, true);
    if (rc) return rc;
    if (!nvec || !rows || !cols) return CLV_OK;
    if (nvec == 1) return clm_f16_mvm_transposed_scale_and_add(A, rows, cols, x[0], u[0], a, t ? t[0] : nullptr, r[0], stream);
    return f16tb_run(A, rows, cols, nvec, {x, u, a, t, r}, stream);
}

// Q_IHT / Q_GD for nvec signals with ONE matrix: the loop of clm_f16_iht_batch (half16_batch.hip) with Phi' t2 straight from Phi's own
// bytes.  The checks run once; per group there is one decision, and a selected group costs per iteration two fused launches and, with a
// threshold, one clv_f16_threshold_batch.  Bit-identical to clm_f16_iht_one_matrix per signal.
#define F16_IHTB1 "clm_f16_iht_batch_one_matrix"
extern "C" int clm_f16_iht_batch_one_matrix(const uint16_t *Phi, uint64_t m, uint64_t n, uint64_t nvec, uint16_t *const *x, uint64_t x_len,
                                            const uint16_t *const *y, uint16_t *const *t1, uint16_t *const *t2, uint16_t *const *t3,
                                            uint64_t iterations, uint64_t K, float mu, int threshold, void *stream)
{
    CLV_REQUIRE(Phi, F16_IHTB1 ": null pointer");
    CLV_REQUIRE(m % 128 == 0 && n % 128 == 0 && x_len <= n, F16_IHTB1 ": m=%llu n=%llu x_len=%llu", (unsigned long long)m, (unsigned long long)n,
                (unsigned long long)x_len);
    CLV_REQUIRE(threshold >= 0 && threshold <= 2, F16_IHTB1 ": unknown threshold %d", threshold);
    CLV_REQUIRE(F16_ALIGNED(Phi), F16_IHTB1 ": the matrix, x and t2 must be 16-byte aligned");
    CLV_REQUIRE(m / 16 < 0x7FFFFFFFull && n / 16 < 0x7FFFFFFFull && (!n || m <= 0xFFFFFFFFFFFFull / n), F16_IHTB1 ": matrix too large");
    if (!nvec) return CLV_OK;
    CLV_REQUIRE(x && y && t1 && t2 && t3, F16_IHTB1 ": null pointer array");
    for (uint64_t j = 0; j < nvec; j++)
        CLV_REQUIRE(x[j] && y[j] && t1[j] && t2[j] && t3[j], F16_IHTB1 ": null pointer in vector %llu", (unsigned long long)j);
    for (uint64_t j = 0; j < nvec; j++) {
        CLV_REQUIRE(F16_ALIGNED(x[j]) && F16_ALIGNED(t2[j]), F16_IHTB1 ": the matrix, x and t2 must be 16-byte aligned (vector %llu)",
                    (unsigned long long)j);
        CLV_REQUIRE((((uintptr_t)y[j] | (uintptr_t)t1[j] | (uintptr_t)t3[j]) & 1u) == 0, F16_IHTB1 ": y, t1 and t3 must be 2-byte aligned (vector %llu)",
                    (unsigned long long)j);
    }
    {   // the range check of clm_f16_iht_batch without PhiT
        std::vector<ClvRange> rg;
        rg.reserve(5 * nvec + 1);
        const uint64_t mb = m * 2, nb = n * 2;
        rg.push_back(clv_range(Phi, m * n * 2, false, ~0ull, "Phi"));
        for (uint64_t j = 0; j < nvec; j++) {
            rg.push_back(clv_range(y[j], mb, false, j, "y"));
            rg.push_back(clv_range(x[j], nb, true, j, "x"));
            rg.push_back(clv_range(t1[j], mb, true, j, "t1"));
            rg.push_back(clv_range(t2[j], mb, true, j, "t2"));
            rg.push_back(clv_range(t3[j], nb, true, j, "t3"));
        }
        int rc = clv_internal_check_ranges(F16_IHTB1, rg);
        if (rc) return rc;
    }
    const int mode = threshold == 2 ? CLV_THRESHOLD_REFERENCE : CLV_THRESHOLD_FAST;
    hipStream_t st = as_stream(stream);
    for (uint64_t j0 = 0; j0 < nvec; j0 += CLM4_MVM_BATCH_MAX) {
        const uint64_t g = nvec - j0 < CLM4_MVM_BATCH_MAX ? nvec - j0 : CLM4_MVM_BATCH_MAX;
        if (nvec == 1 || !(m && n && f16tb_selected(g, m, n))) {      // one signal, an empty matrix, or forwarded: the single call, signal after signal
            for (uint64_t j = j0; j < j0 + g; j++) {
                int rc = clm_f16_iht_one_matrix(Phi, m, n, x[j], x_len, y[j], t1[j], t2[j], t3[j], iterations, K, mu, threshold, stream);
                if (rc) return rc;
            }
            continue;
        }
        for (uint64_t j = j0; j < j0 + g; j++) {
            int rc = clv_internal_f16_clear(x[j], n, st);                                   // x.clear()
            if (rc) return rc;
        }
        const F16BatchVectors step1 = {x + j0, y + j0, -1.0f, t1 + j0, t2 + j0};            // t1 = Phi x; t2 = y - t1
        const F16BatchVectors step2 = {t2 + j0, x + j0, mu, t3 + j0, x + j0};               // t3 = Phi' t2; x += mu t3, in place
        for (uint64_t it = 0; it < iterations; it++) {
            int rc = f16_batch_launch_group(Phi, m, n, g, step1, st);
            if (!rc) rc = f16tb_launch_group(Phi, m, n, g, step2, st);
            if (!rc && threshold) rc = clv_f16_threshold_batch(x + j0, g, x_len, n, K, mode, stream);      // keep the K largest
            if (rc) return rc;
        }
    }
    return CLV_OK;
}
#undef F16_IHTB1
