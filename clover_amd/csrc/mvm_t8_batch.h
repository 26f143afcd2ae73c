// mvm_t8_batch.h -- what the host driver (mvm_batch_host.h) needs to know of the batched TRANSPOSED mixed family: r[j] = quantize8(A' x[j])
// for up to CLM4_MVM_BATCH_MAX CloverVector8 in one pass over a CloverMatrix4's own bytes.  The kernel and the launches are in
// mvm_t8_batch.hip; the traits are declared here because the one-matrix IHT loop (clm4_iht_v8_batch_one_matrix, mvm_batch8.hip) runs
// step 1 on Mvm8Batch and step 2 on this family.
#pragma once

#include "mvm_batch_host.h"
#include "mvm8_device.h"

#define MVT8B_W 2          // output blocks (64 columns each) per workgroup: MVT8_W of the single kernel (mvm_t8.hip)

struct MvmT8Batch : MvmBatchByCols {
    template <int NV> using Args = Mvm8BatchArgs<NV>;
    template <int NV> using Fuse = Mvm8BatchFuse<NV>;
    static uint64_t matrix_bytes(uint64_t rows, uint64_t cols) { return rows * (cols / 2); }
    static uint64_t vector_bytes(uint64_t n) { return n; }
    // A is rows x cols: x has `rows` elements, r = A' x has `cols`; a workgroup owns MVT8B_W output blocks (64 bytes of every row) and
    // walks all rows
    static dim3 grid(uint64_t, uint64_t cols) { return dim3((unsigned)(cols / (64 * MVT8B_W))); }
    // the size rules of clm4_mvm_v8_transposed (mvm_t8.hip)
    static int check_matrix(const char *fn, const int8_t *A, const float *sA, uint64_t rows, uint64_t cols)
    {
        CLV_REQUIRE(A && sA, "%s: null pointer", fn);
        CLV_REQUIRE(rows % 128 == 0 && cols % 128 == 0, "%s: rows=%llu cols=%llu must be multiples of 128", fn, (unsigned long long)rows,
                    (unsigned long long)cols);
        CLV_REQUIRE(cols / 64 <= 0x7FFFFFFFull, "%s: too many columns", fn);
        CLV_REQUIRE(rows / 64 <= 0x7FFFFFFFull, "%s: too many rows", fn);
        return CLV_OK;
    }
    static constexpr auto mvm = clm4_mvm_v8_transposed;
    static constexpr auto scale_and_add = clm4_mvm_v8_transposed_scale_and_add;
    static constexpr auto iht_one_matrix = clm4_iht_v8_one_matrix;
    // The dispatch rule with CLV_MVM_BATCH unset, measured on the MI355X (DESIGN.md 3 "A′x for several CloverVector8, one CloverMatrix4",
    // profiles/mvm_v8_transposed_batch_kernel_bench.json, stochastic profiles/mvm_v8_transposed_batch_st_kernel_bench.json): at 2, 4 and 8
    // vectors the batched launch beat the g single calls by more than the spread of the rounds of both in every row -- 32768^2 and
    // 65536^2 (streaming) plain, fused at 8192 x 4096 (cache-resident) and at 65536^2, the loop at N = 8192 for 8 signals, either
    // rounding; the smallest margin is 2 vectors fused at 8192 x 4096, 1.18 x -- so every group of two or more runs batched.  Not
    // measured: groups of 3 and 5-7, the plain call in the cache-resident class, matrices between 16 MiB and 512 MiB.
    static bool batched_by_rule(uint64_t g, uint64_t, uint64_t, bool, bool) { return g >= 2; }
    // no single clm4_iht_v8_one_matrix takes a persistent kernel: a group of the loop runs batched wherever the fused launch does
    static bool iht_prefers_single(uint64_t m, uint64_t n, uint64_t, int, bool stochastic, uint64_t g) { return !batched_by_rule(g, m, n, true, stochastic); }
    template <int NV, bool NT, bool FUSE, bool ST>
    static void launch(dim3 grid, hipStream_t st, const uint8_t *A, const float *sA, uint64_t rows, uint64_t cols, int nv, const Args<NV> &arg,
                       const Fuse<NV> &fuse, const MvmBatchRng &rs);      // mvm_t8_batch.hip, instantiated there for NV = 2, 4, 8
};
