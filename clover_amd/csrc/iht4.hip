// iht4.hip -- the quantized IHT / GD loop on the device: the five steps of an iteration, nothing copied back between them.
// One of the callers either side of the hot path.  With mvm these are the five steps of the reference's quantized IHT / GD
// iterations (test/performance/01_measure.h:923-946, 999-1021), so x, t1..t3 can stay in HBM across iterations.
#include "common.h"

#include <stdlib.h>

// =================================================================================================
// f4  The application loops that call the hot path: quantized Iterative Hard Thresholding / Gradient Descent
//     (test/performance/01_measure.h:923-946, 999-1021).  One call enqueues all iterations on the stream; nothing
//     returns to the host in between.
// =================================================================================================
__global__ void k_v4_clear(uint32_t *q, float *s, uint64_t nwords, uint64_t nblocks)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += stride) q[i] = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nblocks; i += stride) s[i] = 1.0f;
}

// iht_persist.hip: the whole loop as one persistent launch with Phi and PhiT in LDS (N <= 8192, rounding disabled, threshold FAST or none);
// 1 = launched, 0 = does not qualify, < 0 = error
int clm4_iht_persistent(const int8_t *Phi, const float *sPhi, const int8_t *PhiT, const float *sPhiT, uint64_t m, uint64_t n, int8_t *x,
                        float *sx, uint64_t x_len, const int8_t *y, const float *sy, int8_t *t1, float *st1, int8_t *t2, float *st2, int8_t *t3,
                        float *st3, uint64_t iterations, uint64_t K, float mu, int threshold, uint64_t *rng, hipStream_t st);

static int iht_iteration(const int8_t *Phi, const float *sPhi, const int8_t *PhiT, const float *sPhiT, uint64_t m, uint64_t n,
                         int8_t *x, float *sx, uint64_t x_len, const int8_t *y, const float *sy, int8_t *t1, float *st1, int8_t *t2,
                         float *st2, int8_t *t3, float *st3, uint64_t K, float mu, int threshold, uint64_t *rng, void *stream)
{
    // each scaleAndAdd rides in the epilogue of the mvm before it (same bits, same XORShift positions): 3 launches, not 5
    int rc = clm4_mvm_scale_and_add(Phi, sPhi, m, n, x, sx, y, sy, -1.0f, t1, st1, t2, st2, rng, stream);     // t1 = Phi * x; t2 = y - t1
    if (!rc) rc = clm4_mvm_scale_and_add(PhiT, sPhiT, n, m, t2, st2, x, sx, mu, t3, st3, x, sx, rng, stream); // t3 = Phi' * t2; x += mu * t3
    if (!rc && threshold)                                                                    // keep the K largest (2: in the reference's survivor order)
        rc = clv4_threshold_mode(x, sx, x_len, n, K, threshold == 2 ? CLV_THRESHOLD_REFERENCE : CLV_THRESHOLD_FAST, nullptr, stream);
    return rc;
}

extern "C" int clm4_iht(const int8_t *Phi, const float *sPhi, const int8_t *PhiT, const float *sPhiT, uint64_t m, uint64_t n,
                        int8_t *x, float *sx, uint64_t x_len, const int8_t *y, const float *sy, int8_t *t1, float *st1, int8_t *t2,
                        float *st2, int8_t *t3, float *st3, uint64_t iterations, uint64_t K, float mu, int threshold,
                        uint64_t *rng_state_dev, void *stream)
{
    CLV_REQUIRE(Phi && sPhi && PhiT && sPhiT && x && sx && y && sy && t1 && st1 && t2 && st2 && t3 && st3, "clm4_iht: null pointer");
    CLV_REQUIRE(m % 128 == 0 && n % 128 == 0 && x_len <= n, "clm4_iht: m=%llu n=%llu x_len=%llu", (unsigned long long)m,
                (unsigned long long)n, (unsigned long long)x_len);
    hipStream_t st = as_stream(stream);
    {
        const int p = clm4_iht_persistent(Phi, sPhi, PhiT, sPhiT, m, n, x, sx, x_len, y, sy, t1, st1, t2, st2, t3, st3, iterations, K, mu, threshold,
                                          rng_state_dev, st);
        if (p < 0) return CLV_ERR_HIP;
        if (p > 0) return CLV_OK;
    }
    hipLaunchKernelGGL(k_v4_clear, dim3(64), dim3(256), 0, st, (uint32_t *)x, sx, n / 8, n / 64);   // x.clear()
    CLV_LAUNCH_CHECK();
    if (!iterations) return CLV_OK;
    // plain launches: a captured-graph replay of the five kernels was measured SLOWER on MI355X (39 vs 33 us per
    // iteration at N = 8192: the per-replay cost exceeds the five launch gaps it removes), so none is used
    for (uint64_t it = 0; it < iterations; it++) {
        int rc = iht_iteration(Phi, sPhi, PhiT, sPhiT, m, n, x, sx, x_len, y, sy, t1, st1, t2, st2, t3, st3, K, mu, threshold,
                               rng_state_dev, stream);
        if (rc) return rc;
    }
    return CLV_OK;
}

// The same loop with ONE matrix: Phi' t2 comes straight from Phi (clm4_mvm_transposed_scale_and_add, mvm_t4.hip), so no PhiT exists.
// Always the launch-per-step loop -- the persistent kernel keeps both matrices in LDS -- and bit-identical to clm4_iht called with
// PhiT = transpose(Phi): x, t1 .. t3 and the generator state.
extern "C" int clm4_iht_one_matrix(const int8_t *Phi, const float *sPhi, uint64_t m, uint64_t n, int8_t *x, float *sx, uint64_t x_len,
                                   const int8_t *y, const float *sy, int8_t *t1, float *st1, int8_t *t2, float *st2, int8_t *t3, float *st3,
                                   uint64_t iterations, uint64_t K, float mu, int threshold, uint64_t *rng_state_dev, void *stream)
{
    CLV_REQUIRE(Phi && sPhi && x && sx && y && sy && t1 && st1 && t2 && st2 && t3 && st3, "clm4_iht_one_matrix: null pointer");
    CLV_REQUIRE(m % 128 == 0 && n % 128 == 0 && x_len <= n, "clm4_iht_one_matrix: m=%llu n=%llu x_len=%llu", (unsigned long long)m,
                (unsigned long long)n, (unsigned long long)x_len);
    hipLaunchKernelGGL(k_v4_clear, dim3(64), dim3(256), 0, as_stream(stream), (uint32_t *)x, sx, n / 8, n / 64);   // x.clear()
    CLV_LAUNCH_CHECK();
    for (uint64_t it = 0; it < iterations; it++) {
        int rc = clm4_mvm_scale_and_add(Phi, sPhi, m, n, x, sx, y, sy, -1.0f, t1, st1, t2, st2, rng_state_dev, stream);     // t1 = Phi * x; t2 = y - t1
        if (!rc) rc = clm4_mvm_transposed_scale_and_add(Phi, sPhi, m, n, t2, st2, x, sx, mu, t3, st3, x, sx, rng_state_dev, stream);   // t3 = Phi' * t2; x += mu * t3
        if (!rc && threshold)
            rc = clv4_threshold_mode(x, sx, x_len, n, K, threshold == 2 ? CLV_THRESHOLD_REFERENCE : CLV_THRESHOLD_FAST, nullptr, stream);
        if (rc) return rc;
    }
    return CLV_OK;
}

// Q_IHT / Q_GD for nvec signals with one Phi: the loop above with every step batched.  Arrays are HOST arrays of nvec device pointers.
// Bit-identical to clm4_iht per vector (which may take the persistent kernel: that one equals the launch-per-step loop bit for bit).
extern "C" int clm4_iht_batch(const int8_t *Phi, const float *sPhi, const int8_t *PhiT, const float *sPhiT, uint64_t m, uint64_t n, uint64_t nvec,
                              int8_t *const *x, float *const *sx, uint64_t x_len, const int8_t *const *y, const float *const *sy,
                              int8_t *const *t1, float *const *st1, int8_t *const *t2, float *const *st2, int8_t *const *t3, float *const *st3,
                              uint64_t iterations, uint64_t K, float mu, int threshold, uint64_t *rng_state_dev, void *stream)
{
    const char *fn = "clm4_iht_batch";
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
        rg.push_back(clv_range(Phi, m * (n / 2), false, ~0ull, "Phi"));
        rg.push_back(clv_range(sPhi, tiles * sc, false, ~0ull, "sPhi"));
        rg.push_back(clv_range(PhiT, m * (n / 2), false, ~0ull, "PhiT"));
        rg.push_back(clv_range(sPhiT, tiles * sc, false, ~0ull, "sPhiT"));
        for (uint64_t j = 0; j < nvec; j++) {
            rg.push_back(clv_range(y[j], m / 2, false, j, "y"));
            rg.push_back(clv_range(sy[j], m / 64 * sc, false, j, "sy"));
            rg.push_back(clv_range(x[j], n / 2, true, j, "x"));
            rg.push_back(clv_range(sx[j], n / 64 * sc, true, j, "sx"));
            rg.push_back(clv_range(t1[j], m / 2, true, j, "t1"));
            rg.push_back(clv_range(st1[j], m / 64 * sc, true, j, "st1"));
            rg.push_back(clv_range(t2[j], m / 2, true, j, "t2"));
            rg.push_back(clv_range(st2[j], m / 64 * sc, true, j, "st2"));
            rg.push_back(clv_range(t3[j], n / 2, true, j, "t3"));
            rg.push_back(clv_range(st3[j], n / 64 * sc, true, j, "st3"));
        }
        int rc = clv_internal_check_ranges(fn, rg);
        if (rc) return rc;
    }
    // Which groups run the batched loop.  A single clm4_iht at m, n <= 8192 (threshold FAST or none) takes the persistent kernel, 9.4 us per
    // iteration and signal at N = 8192: against it the batched loop was measured for a full group of 8 only (64.2 us per iteration for 8 signals
    // against 75.5), so smaller groups of that class run as single calls (not measured: by the mvm rows a group of 2 would lose).
    // Elsewhere the single call is the launch-per-step loop with the same three launches per iteration per SIGNAL, and the batched mvm was
    // faster at every group size.  CLV_MVM_BATCH (mvm_batch4.hip) = 1 / 0 forces one or the other.
    // With an rng the same rule: the full group of 8 beat the stochastic persistent kernel too (80.2 us per iteration for 8 signals against
    // 94.7, profiles/mvm_batch_st_kernel_bench.json), and the stochastic fused mvm was faster than the single launches at 2, 4 and 8 vectors
    // (DESIGN.md 3).  The draws keep the order of the single calls, all iterations of vector 0 first: one iteration draws
    // P = 4 (m / 64) + 4 (n / 64), so vector j of a group has its Phi window of iteration `it` at (j * iterations + it) * P and its PhiT
    // window 4 (m / 64) further on; only the group's last launch commits, all g * iterations * P.
    const char *e = clv_env("CLV_MVM_BATCH");
    const int force = e && *e ? (atoi(e) != 0) : -1;
    const bool persistent_class = threshold <= 1 && iterations && m <= 8192 && n <= 8192 && clv_env_int("CLV_IHT_PERSISTENT", 1) != 0;
    const uint64_t P = 4 * (m / 64) + 4 * (n / 64);
    hipStream_t st = as_stream(stream);
    for (uint64_t j0 = 0; j0 < nvec; j0 += CLM4_MVM_BATCH_MAX) {
        const uint64_t g = nvec - j0 < CLM4_MVM_BATCH_MAX ? nvec - j0 : CLM4_MVM_BATCH_MAX;
        bool batched = g >= 2 && force != 0 && (force == 1 || !persistent_class || g == CLM4_MVM_BATCH_MAX);
        if (rng_state_dev && iterations > ((1ull << 55) - 1) / (g * P)) batched = false;      // positions beyond the jump-ahead tables
        if (!batched) {
            for (uint64_t j = j0; j < j0 + g; j++) {
                int rc = clm4_iht(Phi, sPhi, PhiT, sPhiT, m, n, x[j], sx[j], x_len, y[j], sy[j], t1[j], st1[j], t2[j], st2[j], t3[j], st3[j], iterations, K,
                                  mu, threshold, rng_state_dev, stream);
                if (rc) return rc;
            }
            continue;
        }
        for (uint64_t j = j0; j < j0 + g; j++)
            hipLaunchKernelGGL(k_v4_clear, dim3(64), dim3(256), 0, st, (uint32_t *)x[j], sx[j], n / 8, n / 64);   // x.clear()
        CLV_LAUNCH_CHECK();
        const uint64_t stride = iterations * P;
        for (uint64_t it = 0; it < iterations; it++) {
            // t1 = Phi * x, t2 = y - t1;  t3 = Phi' * t2, x += mu * t3;  keep the K largest: three launches for the group
            const uint64_t commit = it + 1 == iterations ? g * stride : 0;
            int rc = clv_internal_mvm_batch_at(Phi, sPhi, m, n, g, x + j0, sx + j0, t1 + j0, st1 + j0, y + j0, sy + j0, -1.0f, t2 + j0, st2 + j0,
                                               rng_state_dev, it * P, stride, 0, stream);
            if (!rc)
                rc = clv_internal_mvm_batch_at(PhiT, sPhiT, n, m, g, t2 + j0, st2 + j0, t3 + j0, st3 + j0, x + j0, sx + j0, mu, x + j0, sx + j0,
                                               rng_state_dev, it * P + 4 * (m / 64), stride, commit, stream);
            if (!rc && threshold)
                rc = clv4_threshold_batch(x + j0, sx + j0, g, x_len, n, K, threshold == 2 ? CLV_THRESHOLD_REFERENCE : CLV_THRESHOLD_FAST, stream);
            if (rc) return rc;
        }
    }
    return CLV_OK;
}
