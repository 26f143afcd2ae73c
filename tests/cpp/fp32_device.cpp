// fp32_device.cpp -- CloverVector32.h / CloverMatrix32.h / CloverIHT.h through a C++ client with the reference's method names, built with
// -DCLOVER_FP32_ON_DEVICE (tests/test_fp32_dropin.py; page-tracked and -DCLOVER_HIP_EXPLICIT_SYNC, default and -DCLOVER_FAST).  Every routed
// method runs against the clover_fp32:: function on the same data, bit for bit; under -DCLOVER_FAST dot is held to the bound of the FAST
// order and threshold to its rule (the same multiset of magnitudes, lowest indices among equal ones).  Prints one `name=0|1` per check.
// Built WITHOUT the switch (tests/test_fp32_device_cpu.py, compile only) the same calls are the host loops and no clv_f32_* / clm_f32_*
// symbol is referenced.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "CloverIHT.h"
#include "CloverMatrix32.h"
#include "CloverVector32.h"

static int failures = 0;
static void report(const char *name, bool ok)
{
    printf("%s=%d\n", name, ok ? 1 : 0);
    if (!ok) failures++;
}
static bool same_bits(const float *a, const float *b, uint64_t n) { return memcmp(a, b, n * sizeof(float)) == 0; }
static std::vector<float> copy_of(const CloverVector32 &v) { return std::vector<float>(v.host_ro(), v.host_ro() + v.size_pad()); }

// threshold FAST on the host: everything above the k-th largest magnitude, then the lowest-index elements equal to it
static void keep_top_k_lowest_index(float *v, uint64_t n, uint64_t k)
{
    if (k >= n) return;
    std::vector<float> mag(n);
    for (uint64_t i = 0; i < n; i++) mag[i] = std::fabs(v[i]);
    std::vector<float> sorted(mag);
    std::sort(sorted.begin(), sorted.end());
    const float tau = k ? sorted[n - k] : INFINITY;
    uint64_t above = 0;
    for (uint64_t i = 0; i < n; i++) above += mag[i] > tau;
    uint64_t ties_left = k - (k ? above : 0);
    for (uint64_t i = 0; i < n; i++) {
        if (mag[i] > tau) continue;
        if (k && mag[i] == tau && ties_left) { ties_left--; continue; }
        v[i] = 0.0f;
    }
}

int main(int argc, char **argv)
{
    const uint64_t N = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1024;
    const uint64_t m = N / 2, n = N, K = 32, iters = 8;
#ifdef CLOVER_FAST
    const bool fast = true;
#else
    const bool fast = false;
#endif
    CloverMatrix32 Phi(m, n), PhiT(n, m);
    Phi.setRandomFloats(-1.0f, 1.0f, 11);
    std::vector<float> A(Phi.host_ro(), Phi.host_ro() + m * n);

    // ---- transpose / transpose_parallel, through a pointer taken BEFORE the device wrote
    const float *pt = PhiT.getData();
    std::vector<float> At(m * n);
    clover_fp32::transpose(A.data(), m, n, At.data(), false);
    Phi.transpose(PhiT);
    report("transpose", same_bits(PhiT.host_ro(), At.data(), m * n) && same_bits(pt, At.data(), m * n));
    PhiT.clear();
    Phi.transpose_parallel(PhiT);
    report("transpose_parallel", same_bits(PhiT.host_ro(), At.data(), m * n));

    // ---- mvm / mvm_parallel
    CloverVector32 x(n), r(m), r2(m), want_m(m);
    x.setRandomFloats(-2.0f, 2.0f, 5);
    const float *pr = r.getData();
    clover_fp32::mvm_rows(A.data(), m, n, x.host_ro(), want_m.host_rw(), false);
    Phi.mvm(x, r);
    report("mvm", same_bits(r.host_ro(), want_m.host_ro(), m));
    report("getData_stays_current", same_bits(pr, want_m.host_ro(), m) && pr == r.getData());
    Phi.mvm_parallel(x, r2);
    report("mvm_parallel", same_bits(r2.host_ro(), want_m.host_ro(), m));

    // ---- scaleAndAdd, both forms and _parallel; a view writes through to the caller's memory
    CloverVector32 u(m), v(m), w(m);
    u.setRandomFloats(-1.0f, 1.0f, 6);
    v.setRandomFloats(-1.0f, 1.0f, 7);
    std::vector<float> u0 = copy_of(u), v0 = copy_of(v), want(m);
    clover_fp32::axpy_fma(u0.data(), v0.data(), 0.37f, want.data(), m, false);
    u.scaleAndAdd(v, 0.37f, w);
    report("scaleAndAdd_out_of_place", same_bits(w.host_ro(), want.data(), m) && same_bits(u.host_ro(), u0.data(), m));
    w.clear();
    u.scaleAndAdd_parallel(v, 0.37f, w);
    report("scaleAndAdd_parallel_out_of_place", same_bits(w.host_ro(), want.data(), m));
    u.scaleAndAdd(v, 0.37f);
    report("scaleAndAdd_in_place", same_bits(u.host_ro(), want.data(), m));
    clover_fp32::axpy_fma(want.data(), v0.data(), -1.5f, want.data(), m, false);
    u.scaleAndAdd_parallel(v, -1.5f);
    report("scaleAndAdd_parallel_in_place", same_bits(u.host_ro(), want.data(), m));
    {
        float *mine = static_cast<float *>(aligned_alloc(4096, m * sizeof(float)));
        memset(mine, 0, m * sizeof(float));
        CloverVector32 view(m, mine);
        clover_fp32::axpy_fma(u0.data(), v0.data(), 2.0f, want.data(), m, false);
        CloverVector32 uu(m);
        memcpy(uu.host_rw(), u0.data(), m * sizeof(float));
        uu.scaleAndAdd(v, 2.0f, view);
        report("view_writes_through", same_bits(mine, want.data(), m));
        free(mine);
    }

    // ---- dot / dot_parallel
    {
        CloverVector32 a(n), b(n);
        a.setRandomFloats(-1.0f, 1.0f, 8);
        b.setRandomFloats(-1.0f, 1.0f, 9);
        const float exact_order = clover_fp32::dot_chains32(a.host_ro(), b.host_ro(), n);
        const float d = a.dot(b), dp = a.dot_parallel(b);
        if (!fast) {
            report("dot", memcmp(&d, &exact_order, 4) == 0);
            report("dot_parallel", memcmp(&dp, &exact_order, 4) == 0);
        } else {
            // the FAST order: D = ceil(n / 1024 / grid) + 26 roundings on the longest path (clover_hip_fp32.h), against float64
            int cus = 0;
            clover_hip::check(clv_device_info(nullptr, 0, &cus, nullptr), "clv_device_info");
            double e = 0, s = 0;
            for (uint64_t i = 0; i < n; i++) { const double p = (double)a.get(i) * (double)b.get(i); e += p; s += std::fabs(p); }
            uint64_t grid = (n / 4 + 255) / 256;
            if (grid > 4ull * cus) grid = 4ull * cus;
            if (grid > 2048) grid = 2048;
            const double D = (double)((n / 4 + grid * 256 - 1) / (grid * 256)) + 26, uu = std::ldexp(1.0, -24), lim = D * uu / (1 - D * uu) * s;
            report("dot", std::fabs((double)d - e) <= lim);
            report("dot_parallel", memcmp(&d, &dp, 4) == 0);
        }
        const float ds = a.dot_scalar(b), ds_want = clover_fp32::dot_sequential(a.host_ro(), b.host_ro(), n);
        report("dot_scalar_stays_host", memcmp(&ds, &ds_want, 4) == 0);
    }

    // ---- threshold / threshold_parallel: distinct magnitudes, and small integers (ties across the cut); ragged length
    for (int tied = 0; tied < 2; tied++) {
        CloverVector32 t(n - 37);
        if (tied) t.setRandomInteger(4.0f, 3);
        else t.setRandomFloats(-1.0f, 1.0f, 4);
        t.getData()[t.size() + 1] = 9.0f;                               // padding: must be left alone
        std::vector<float> before = copy_of(t), want_t(before);
        const uint64_t k = t.size() / 4;
        if (fast) keep_top_k_lowest_index(want_t.data(), t.size(), k);
        else clover_fp32::keep_top_k(want_t.data(), t.size(), k);
        CloverVector32 t2(t);
        t.threshold(k);
        t2.threshold_parallel(k);
        uint64_t kept = 0;
        for (uint64_t i = 0; i < t.size(); i++) kept += t.get(i) != 0.0f;
        report(tied ? "threshold_ties" : "threshold_distinct", same_bits(t.host_ro(), want_t.data(), t.size_pad()) && (tied || kept == k));
        report(tied ? "threshold_parallel_ties" : "threshold_parallel_distinct", same_bits(t2.host_ro(), want_t.data(), t.size_pad()));
    }

    // ---- the loops: y = Phi x_true for a K-sparse signal of ones
    CloverVector32 xs(n), y(m), t1(m), t2(m), t3(n);
    xs.clear();
    for (uint64_t j = 0; j < K; j++) xs.set((j * 2654435761ull) % n, 1.0f);
    uint64_t support = 0;
    for (uint64_t i = 0; i < n; i++) support += xs.get(i) != 0.0f;
    clover_fp32::mvm_rows(A.data(), m, n, xs.host_ro(), y.host_rw(), false);
    const float mu = 1.0f / (float)m;
#ifdef CLOVER_FP32_ON_DEVICE
    // ---- mvm_scaleAndAdd = mvm, then scaleAndAdd (both forms)
    {
        CloverVector32 ta(m), ra(m), tb(m), rb(m);
        Phi.mvm(x, ta);
        y.scaleAndAdd(ta, -1.0f, ra);
        Phi.mvm_scaleAndAdd(x, y, -1.0f, tb, rb);
        report("mvm_scaleAndAdd", same_bits(ta.host_ro(), tb.host_ro(), m) && same_bits(ra.host_ro(), rb.host_ro(), m));
        CloverVector32 yc(y);
        Phi.mvm_scaleAndAdd(x, yc, -1.0f, tb);
        report("mvm_scaleAndAdd_in_place", same_bits(yc.host_ro(), ra.host_ro(), m));
    }
#endif
    // ---- Q_IHT / Q_GD on <CloverMatrix32, CloverVector32> = the five method calls
    for (int gd = 0; gd < 2; gd++) {
        CloverVector32 xa(n), xb(n), a1(m), a2(m), a3(n);
        xa.setRandomFloats(-1.0f, 1.0f, 1);                            // the loop clears x itself
        if (gd) Q_GD<CloverMatrix32, CloverVector32>(Phi, PhiT, xa, y, t1, t2, t3, iters, mu);
        else Q_IHT<CloverMatrix32, CloverVector32>(Phi, PhiT, xa, y, t1, t2, t3, iters, K, mu);
        xb.clear();
        for (uint64_t it = 0; it < iters; it++) {
            Phi.mvm_parallel(xb, a1);
            y.scaleAndAdd_parallel(a1, -1.0f, a2);
            PhiT.mvm_parallel(a2, a3);
            xb.scaleAndAdd_parallel(a3, mu);
            if (!gd) xb.threshold_parallel(K);
        }
        const bool eq = same_bits(xa.host_ro(), xb.host_ro(), n) && same_bits(t1.host_ro(), a1.host_ro(), m) && same_bits(t2.host_ro(), a2.host_ro(), m) &&
                        same_bits(t3.host_ro(), a3.host_ro(), n);
        report(gd ? "q_gd_equals_method_calls" : "q_iht_equals_method_calls", eq);
    }
    // ---- recovery: 60 iterations of IHT bring the support back
    {
        CloverVector32 xr(n);
        Q_IHT<CloverMatrix32, CloverVector32>(Phi, PhiT, xr, y, t1, t2, t3, 60, support, mu);
        uint64_t hit = 0, nonzero = 0;
        double err = 0, norm = 0;
        for (uint64_t i = 0; i < n; i++) {
            nonzero += xr.get(i) != 0.0f;
            hit += xr.get(i) != 0.0f && xs.get(i) != 0.0f;
            err += ((double)xr.get(i) - xs.get(i)) * ((double)xr.get(i) - xs.get(i));
            norm += (double)xs.get(i) * xs.get(i);
        }
        printf("recovery: support %llu/%llu, relative error %.4f\n", (unsigned long long)hit, (unsigned long long)support, std::sqrt(err / norm));
        report("q_iht_recovers_the_support", hit == support && nonzero <= support && std::sqrt(err / norm) < 0.05);
    }
    if (failures) printf("FAILED %d\n", failures);
    else printf("done\n");
    return failures ? 1 : 0;
}
