// half16_batch_host.h -- the host side of the two batched half-precision mvm families, written once: the slots of a launch, group policy,
// the group loop, the argument and overlap check, the bodies of the product entry points and the batched IHT / GD loop.  Included by
// half16_batch.hip (CloverMatrix16 x CloverVector16, row-major) and half16_t_batch.hip (CloverMatrix16' x CloverVector16 straight from the
// matrix's own bytes).  It is mvm_batch_host.h without scale pointers and draw positions, which that driver carries through every layer,
// and in its vocabulary; mvm_batch_forced(), the overlap check, the launch counter and CLM4_MVM_BATCH_MAX are shared with it.  Each of the
// two families defines its kernel and a traits struct F with exactly what differs:
//   check_matrix(fn, A, rows, cols)           the single call's size and alignment rules, in the single call's order
//   x_len, r_len                              which dimension sizes x and which r / u / t
//   nothing_to_do(nvec, rows, cols)           the empty-call rule of the two product entry points: checked arguments, no device work
//   batched_by_rule(g, rows, cols)            the measured dispatch rule
//   mvm, scale_and_add                        the single calls a group is forwarded to
//   iht / iht_one_matrix                      the single loop a group of the batched loop is forwarded to
//   launch<NV>(st, A, rows, cols, nv, slots)  grid, workgroup form, the nontemporal switch and the hipLaunchKernelGGL of the family's
//                                             kernel; defined beside the kernel and instantiated there for NV = 2, 4, 8
// The extern "C" entry points forward to f16_batch_entry, f16_batch_fused_entry and f16_batch_iht (below) with their own names, which the
// messages quote.
#pragma once

#include "half16_device.h"
#include "mvm_batch_host.h"

#include "clover_hip_batch_f16.h"

// the vectors of a call (host arrays of device pointers).  u == NULL: the plain mvm, r[j] = f16(A x[j]).  Else the fused form: t[j] =
// f16(A x[j]) (t == NULL: not stored), r[j] = f16(fma(f32(t[j]), a, f32(u[j])))
struct F16BatchVectors {
    const uint16_t *const *x;
    const uint16_t *const *u;
    float a;
    uint16_t *const *t;
    uint16_t *const *r;
    F16BatchVectors from(uint64_t j0) const { return {x + j0, u ? u + j0 : nullptr, a, t ? t + j0 : nullptr, r + j0}; }
};

// the vectors of one launch in the kernels' terms, on the host side; a family's launch fills its kernel's by-value arguments from it.
// r: the f16 product (fused: t of the ABI, NULL = not stored); fused: r2[v] = f16(fma(f32(product), a, f32(u[v]))), r2[v] may be u[v].
// Slots v >= nv are NULL
template <int NV>
struct F16BatchSlots {
    const uint16_t *x[NV];
    uint16_t *r[NV];
    const uint16_t *u[NV];
    uint16_t *r2[NV];
    float a;
    bool fused;
};

// The row-major family (kernel and launches: half16_batch.hip).  Declared here because the one-matrix loop (clm_f16_iht_batch_one_matrix,
// half16_t_batch.hip) runs step 1 on this family and step 2 on the transposed one of its own file.
struct F16Batch {
    // the size and alignment rules of clm_f16_mvm (half16.hip)
    static int check_matrix(const char *fn, const uint16_t *A, uint64_t rows, uint64_t cols)
    {
        CLV_REQUIRE(A, "%s: null pointer", fn);
        CLV_REQUIRE(F16_ALIGNED(A), "%s: the matrix and x must be 16-byte aligned", fn);
        CLV_REQUIRE(cols % 128 == 0, "%s: cols=%llu must be a multiple of 128", fn, (unsigned long long)cols);
        CLV_REQUIRE(rows / 16 < 0x7FFFFFFFull, "%s: matrix too large", fn);
        return CLV_OK;
    }
    static uint64_t x_len(uint64_t, uint64_t cols) { return cols; }
    static uint64_t r_len(uint64_t rows, uint64_t) { return rows; }
    static bool nothing_to_do(uint64_t nvec, uint64_t rows, uint64_t) { return !nvec || !rows; }
    // Whether a group of g vectors of a call of two or more runs as one batched launch or as g single launches.  CLV_MVM_BATCH = 1 / 0 forces
    // one or the other for every group -- forced to 1 a remainder group of ONE vector (nvec = 9, 17, ...) runs batched too, so that a forced
    // call is ceil(nvec / 8) batched launches and nothing else.  Unset = the rule measured on the MI355X ("Several vectors, one
    // CloverMatrix16 pass"; profiles/f16_mvm_batch_kernel_bench.json, profiles/f16_mvm_batch_groups_kernel_bench.json): batched exactly where
    // the batched launch beat the single calls by more than their spread --
    //   a streaming matrix (above the 256 MiB rule; 65536^2 and 32768^2): every group of two or more (2: 1.95 x ... 8: 4.1 - 5.1 x);
    //   a cache-resident one (the fused step at 8192 x 4096, 64 MiB): groups of three or more (3: 1.03 x, 4: 1.17, 8: 1.28); TWO vectors lost
    //   to the two single calls (0.95 x) and are forwarded.
    // Not measured: matrices between 64 MiB and 1 GiB, below 64 MiB, and streaming matrices of fewer than 32768 rows (the 16-row form).
    static bool batched_by_rule(uint64_t g, uint64_t rows, uint64_t cols) { return g >= (F16_STREAMING(rows * cols * 2) ? 2u : 3u); }
    static constexpr auto mvm = clm_f16_mvm;
    static constexpr auto scale_and_add = clm_f16_mvm_scale_and_add;
    static constexpr auto iht = clm_f16_iht;
    template <int NV>
    static void launch(hipStream_t st, const uint16_t *A, uint64_t rows, uint64_t cols, int nv, const F16BatchSlots<NV> &s);
};

// one launch (counted) for the first g <= NV vectors of v
template <class F, int NV>
static int f16_batch_launch(const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t g, const F16BatchVectors &v, hipStream_t st)
{
    F16BatchSlots<NV> s;
    s.fused = v.u != nullptr;
    for (uint64_t i = 0; i < NV; i++) {
        const bool in = i < g;
        s.x[i] = in ? v.x[i] : nullptr;
        s.r[i] = !in ? nullptr : s.fused ? (v.t ? v.t[i] : nullptr) : v.r[i];
        s.u[i] = in && s.fused ? v.u[i] : nullptr;
        s.r2[i] = in && s.fused ? v.r[i] : nullptr;
    }
    s.a = v.a;
    F::template launch<NV>(st, A, rows, cols, (int)g, s);
    CLV_LAUNCH_CHECK();
    clv_internal_mvm_batch_count();
    return CLV_OK;
}

// a group of g <= CLM4_MVM_BATCH_MAX vectors on the smallest instantiation that holds it
template <class F>
static int f16_batch_launch_group(const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t g, const F16BatchVectors &v, hipStream_t st)
{
    return g <= 2   ? f16_batch_launch<F, 2>(A, rows, cols, g, v, st)
           : g <= 4 ? f16_batch_launch<F, 4>(A, rows, cols, g, v, st)
                    : f16_batch_launch<F, 8>(A, rows, cols, g, v, st);
}

// whether a group of g vectors runs as one batched launch or as g single launches: CLV_MVM_BATCH first, then the family's measured rule
template <class F>
static bool f16_batch_selected(uint64_t g, uint64_t rows, uint64_t cols)
{
    const int force = mvm_batch_forced();
    return force >= 0 ? force != 0 : F::batched_by_rule(g, rows, cols);
}

// the checked arguments of the family's mvm batch call (v.u == NULL) / fused batch call on the stream, group by group
template <class F>
static int f16_batch_run(const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t nvec, const F16BatchVectors &v, void *stream)
{
    for (uint64_t j0 = 0; j0 < nvec; j0 += CLM4_MVM_BATCH_MAX) {
        const uint64_t g = nvec - j0 < CLM4_MVM_BATCH_MAX ? nvec - j0 : CLM4_MVM_BATCH_MAX;
        int rc = CLV_OK;
        if (!f16_batch_selected<F>(g, rows, cols)) {
            for (uint64_t j = j0; j < j0 + g && !rc; j++)
                rc = v.u ? F::scale_and_add(A, rows, cols, v.x[j], v.u[j], v.a, v.t ? v.t[j] : nullptr, v.r[j], stream)
                         : F::mvm(A, rows, cols, v.x[j], v.r[j], stream);
        } else {
            rc = f16_batch_launch_group<F>(A, rows, cols, g, v.from(j0), as_stream(stream));
        }
        if (rc) return rc;
    }
    return CLV_OK;
}

// every check of the family's two mvm batch calls, before any device work: the single call's size and alignment rules, then the arrays,
// the entries, the aliases the single calls refuse by name and the overlap check.  u == NULL and t == NULL in the plain call.
template <class F>
static int f16_batch_check_args(const char *fn, const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t nvec, const uint16_t *const *x,
                                const uint16_t *const *u, uint16_t *const *t, uint16_t *const *r, bool fused)
{
    int rc = F::check_matrix(fn, A, rows, cols);
    if (rc) return rc;
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
    const uint64_t xb = F::x_len(rows, cols) * 2, rb = F::r_len(rows, cols) * 2;
    rg.push_back(clv_range(A, rows * cols * 2, false, ~0ull, "A"));
    for (uint64_t j = 0; j < nvec; j++) {
        rg.push_back(clv_range(x[j], xb, false, j, "x"));
        rg.push_back(clv_range(r[j], rb, true, j, "r"));
        // the in-place form r[j] == u[j]: the result IS the input, only the lane that owns an element touches it in either
        if (fused && r[j] != u[j]) rg.push_back(clv_range(u[j], rb, false, j, "u"));
        if (t) rg.push_back(clv_range(t[j], rb, true, j, "t"));
    }
    return clv_internal_check_ranges(fn, rg);
}

// ---- the bodies of a family's extern "C" entry points; fn = the name of the entry point that was called -------------------------------
// *_batch: r[j] = f16(A x[j]) (the transposed family: A' x[j]); one vector is the single call
template <class F>
static int f16_batch_entry(const char *fn, const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t nvec, const uint16_t *const *x,
                           uint16_t *const *r, void *stream)
{
    int rc = f16_batch_check_args<F>(fn, A, rows, cols, nvec, x, nullptr, nullptr, r, false);
    if (rc) return rc;
    if (F::nothing_to_do(nvec, rows, cols)) return CLV_OK;
    if (nvec == 1) return F::mvm(A, rows, cols, x[0], r[0], stream);
    return f16_batch_run<F>(A, rows, cols, nvec, {x, nullptr, 0.0f, nullptr, r}, stream);
}

// *_scale_and_add_batch: t[j] = the product (stored if t != NULL), r[j] = f16(fma(f32(t[j]), a, f32(u[j]))); one vector is the single call
template <class F>
static int f16_batch_fused_entry(const char *fn, const uint16_t *A, uint64_t rows, uint64_t cols, uint64_t nvec, const uint16_t *const *x,
                                 const uint16_t *const *u, float a, uint16_t *const *t, uint16_t *const *r, void *stream)
{
    int rc = f16_batch_check_args<F>(fn, A, rows, cols, nvec, x, u, t, r, true);
    if (rc) return rc;
    if (F::nothing_to_do(nvec, rows, cols)) return CLV_OK;
    if (nvec == 1) return F::scale_and_add(A, rows, cols, x[0], u[0], a, t ? t[0] : nullptr, r[0], stream);
    return f16_batch_run<F>(A, rows, cols, nvec, {x, u, a, t, r}, stream);
}

// Q_IHT / Q_GD for nvec signals with one Phi: the loop of clm_f16_iht (half16.hip) with every step batched.  Arrays are HOST arrays of nvec
// device pointers.  The checks run once; per group there is one decision, and a selected group costs per iteration two fused launches
// and, with a threshold, one clv_f16_threshold_batch.  FT = the family that takes step 2, t3 = Phi' t2: F itself on the held PhiT, or the
// transposed family on Phi's own bytes (PhiT is then NULL and unused).  The decision and the single call a group is forwarded to are
// FT's: F::iht, or FT::iht_one_matrix.  Bit-identical to that single call per signal.
template <class F, class FT = F>
static int f16_batch_iht(const char *fn, const uint16_t *Phi, const uint16_t *PhiT, uint64_t m, uint64_t n, uint64_t nvec, uint16_t *const *x,
                         uint64_t x_len, const uint16_t *const *y, uint16_t *const *t1, uint16_t *const *t2, uint16_t *const *t3,
                         uint64_t iterations, uint64_t K, float mu, int threshold, void *stream)
{
    constexpr bool one_matrix = !std::is_same<F, FT>::value;
    const char *const held = one_matrix ? "matrix" : "matrices";
    CLV_REQUIRE(Phi && (one_matrix || PhiT), "%s: null pointer", fn);
    CLV_REQUIRE(m % 128 == 0 && n % 128 == 0 && x_len <= n, "%s: m=%llu n=%llu x_len=%llu", fn, (unsigned long long)m, (unsigned long long)n,
                (unsigned long long)x_len);
    CLV_REQUIRE(threshold >= 0 && threshold <= 2, "%s: unknown threshold %d", fn, threshold);
    CLV_REQUIRE(F16_ALIGNED(Phi) && (one_matrix || F16_ALIGNED(PhiT)), "%s: the %s, x and t2 must be 16-byte aligned", fn, held);
    // m n below 2^48 is a rule of the single transposed call, which the two-matrix loop never reaches
    CLV_REQUIRE(m / 16 < 0x7FFFFFFFull && n / 16 < 0x7FFFFFFFull && (!one_matrix || !n || m <= 0xFFFFFFFFFFFFull / n), "%s: matrix too large", fn);
    if (!nvec) return CLV_OK;
    CLV_REQUIRE(x && y && t1 && t2 && t3, "%s: null pointer array", fn);
    for (uint64_t j = 0; j < nvec; j++)
        CLV_REQUIRE(x[j] && y[j] && t1[j] && t2[j] && t3[j], "%s: null pointer in vector %llu", fn, (unsigned long long)j);
    for (uint64_t j = 0; j < nvec; j++) {
        CLV_REQUIRE(F16_ALIGNED(x[j]) && F16_ALIGNED(t2[j]), "%s: the %s, x and t2 must be 16-byte aligned (vector %llu)", fn, held,
                    (unsigned long long)j);
        CLV_REQUIRE((((uintptr_t)y[j] | (uintptr_t)t1[j] | (uintptr_t)t3[j]) & 1u) == 0, "%s: y, t1 and t3 must be 2-byte aligned (vector %llu)", fn,
                    (unsigned long long)j);
    }
    {   // the range check of mvm_batch_iht without its scale arrays
        std::vector<ClvRange> rg;
        rg.reserve(5 * nvec + 2);
        const uint64_t mb = m * 2, nb = n * 2;
        rg.push_back(clv_range(Phi, m * n * 2, false, ~0ull, "Phi"));
        if (!one_matrix) rg.push_back(clv_range(PhiT, m * n * 2, false, ~0ull, "PhiT"));
        for (uint64_t j = 0; j < nvec; j++) {
            rg.push_back(clv_range(y[j], mb, false, j, "y"));
            rg.push_back(clv_range(x[j], nb, true, j, "x"));
            rg.push_back(clv_range(t1[j], mb, true, j, "t1"));
            rg.push_back(clv_range(t2[j], mb, true, j, "t2"));
            rg.push_back(clv_range(t3[j], nb, true, j, "t3"));
        }
        int rc = clv_internal_check_ranges(fn, rg);
        if (rc) return rc;
    }
    const int mode = threshold == 2 ? CLV_THRESHOLD_REFERENCE : CLV_THRESHOLD_FAST;
    hipStream_t st = as_stream(stream);
    for (uint64_t j0 = 0; j0 < nvec; j0 += CLM4_MVM_BATCH_MAX) {
        const uint64_t g = nvec - j0 < CLM4_MVM_BATCH_MAX ? nvec - j0 : CLM4_MVM_BATCH_MAX;
        if (nvec == 1 || !(m && n && f16_batch_selected<FT>(g, m, n))) {      // one signal, an empty matrix, or forwarded: the single call, signal after signal
            for (uint64_t j = j0; j < j0 + g; j++) {
                int rc;
                if constexpr (one_matrix) rc = FT::iht_one_matrix(Phi, m, n, x[j], x_len, y[j], t1[j], t2[j], t3[j], iterations, K, mu, threshold, stream);
                else rc = F::iht(Phi, PhiT, m, n, x[j], x_len, y[j], t1[j], t2[j], t3[j], iterations, K, mu, threshold, stream);
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
            int rc = f16_batch_launch_group<F>(Phi, m, n, g, step1, st);
            if (!rc) rc = one_matrix ? f16_batch_launch_group<FT>(Phi, m, n, g, step2, st) : f16_batch_launch_group<F>(PhiT, n, m, g, step2, st);
            if (!rc && threshold) rc = clv_f16_threshold_batch(x + j0, g, x_len, n, K, mode, stream);      // keep the K largest
            if (rc) return rc;
        }
    }
    return CLV_OK;
}
