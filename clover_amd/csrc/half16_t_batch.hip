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
// The host side is half16_batch_host.h, shared with the row-major family (half16_batch.hip).
#include "half16_batch_host.h"

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

// ---- what differs from the row-major family (half16_batch_host.h) --------------------------------------------------------------------
struct F16TBatch {
    // the size and alignment rules of clm_f16_mvm_transposed (half16_t.hip)
    static int check_matrix(const char *fn, const uint16_t *A, uint64_t rows, uint64_t cols)
    {
        CLV_REQUIRE(A, "%s: null pointer", fn);
        CLV_REQUIRE(rows % 128 == 0 && cols % 128 == 0, "%s: rows=%llu cols=%llu must be multiples of 128", fn, (unsigned long long)rows,
                    (unsigned long long)cols);
        CLV_REQUIRE(F16_ALIGNED(A), "%s: the matrix and x must be 16-byte aligned", fn);
        CLV_REQUIRE(!cols || rows <= 0xFFFFFFFFFFFFull / cols, "%s: matrix too large", fn);
        CLV_REQUIRE(rows / 32 <= 0x7FFFFFFFull && cols / 64 <= 0x7FFFFFFFull, "%s: matrix too large", fn);
        return CLV_OK;
    }
    // A is rows x cols: x has `rows` elements, r = A' x (and u, t) `cols`
    static uint64_t x_len(uint64_t rows, uint64_t) { return rows; }
    static uint64_t r_len(uint64_t, uint64_t cols) { return cols; }
    // a matrix without rows has nothing to multiply, one without columns nothing to write
    static bool nothing_to_do(uint64_t nvec, uint64_t rows, uint64_t cols) { return !nvec || !rows || !cols; }
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
    static bool batched_by_rule(uint64_t g, uint64_t, uint64_t) { return g >= 2; }
    static constexpr auto mvm = clm_f16_mvm_transposed;
    static constexpr auto scale_and_add = clm_f16_mvm_transposed_scale_and_add;
    static constexpr auto iht_one_matrix = clm_f16_iht_one_matrix;
    template <int NV>
    static void launch(hipStream_t st, const uint16_t *A, uint64_t rows, uint64_t cols, int nv, const F16BatchSlots<NV> &s);
};

// the kernel's argument struct from the slots; instantiated for the driver's NV = 2, 4, 8
template <int NV>
void F16TBatch::launch(hipStream_t st, const uint16_t *A, uint64_t rows, uint64_t cols, int nv, const F16BatchSlots<NV> &s)
{
    F16TBatchArgs<NV> arg;
    for (int i = 0; i < NV; i++) {
        arg.x[i] = s.x[i];
        arg.r[i] = s.r[i];
        arg.u[i] = s.u[i];
        arg.r2[i] = s.r2[i];
    }
    arg.a = s.a;
    const dim3 grid((unsigned)((cols + F16TB_COLS(NV) - 1) / F16TB_COLS(NV))), block(256);
    // nontemporal loads by the rule of the single calls: once the matrix cannot live in the 256 MiB Infinity Cache
    const bool nt = F16_STREAMING(rows * cols * 2);
    switch (2 * nt + s.fused) {
    case 3: hipLaunchKernelGGL((k_f16_mvm_t_batch<NV, true, true>), grid, block, 0, st, A, rows, cols, nv, arg); break;
    case 2: hipLaunchKernelGGL((k_f16_mvm_t_batch<NV, true, false>), grid, block, 0, st, A, rows, cols, nv, arg); break;
    case 1: hipLaunchKernelGGL((k_f16_mvm_t_batch<NV, false, true>), grid, block, 0, st, A, rows, cols, nv, arg); break;
    default: hipLaunchKernelGGL((k_f16_mvm_t_batch<NV, false, false>), grid, block, 0, st, A, rows, cols, nv, arg); break;
    }
}
template void F16TBatch::launch<2>(hipStream_t, const uint16_t *, uint64_t, uint64_t, int, const F16BatchSlots<2> &);
template void F16TBatch::launch<4>(hipStream_t, const uint16_t *, uint64_t, uint64_t, int, const F16BatchSlots<4> &);
template void F16TBatch::launch<8>(hipStream_t, const uint16_t *, uint64_t, uint64_t, int, const F16BatchSlots<8> &);

// ---- C ABI (include/clover_hip_batch_f16_t.h) ----------------------------------------------------------------------------------------
extern "C" int clm_f16_mvm_transposed_batch(const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t nvec, const uint16_t *const *x,
                                            uint16_t *const *r, void *stream)
{
    return f16_batch_entry<F16TBatch>("clm_f16_mvm_transposed_batch", A, rows, cols, nvec, x, r, stream);
}

extern "C" int clm_f16_mvm_transposed_scale_and_add_batch(const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t nvec, const uint16_t *const *x,
                                                          const uint16_t *const *u, float a, uint16_t *const *t, uint16_t *const *r, void *stream)
{
    return f16_batch_fused_entry<F16TBatch>("clm_f16_mvm_transposed_scale_and_add_batch", A, rows, cols, nvec, x, u, a, t, r, stream);
}

// Q_IHT / Q_GD for nvec signals with ONE matrix: step 1 on the row-major family, Phi' t2 straight from Phi's own bytes on this one
// (f16_batch_iht, half16_batch_host.h)
extern "C" int clm_f16_iht_batch_one_matrix(const uint16_t *Phi, uint64_t m, uint64_t n, uint64_t nvec, uint16_t *const *x, uint64_t x_len,
                                            const uint16_t *const *y, uint16_t *const *t1, uint16_t *const *t2, uint16_t *const *t3,
                                            uint64_t iterations, uint64_t K, float mu, int threshold, void *stream)
{
    return f16_batch_iht<F16Batch, F16TBatch>("clm_f16_iht_batch_one_matrix", Phi, nullptr, m, n, nvec, x, x_len, y, t1, t2, t3, iterations, K, mu,
                                              threshold, stream);
}
