// mvm_batch_host.h -- the host side of the batched mvm families, written once: group policy, launch, the two group loops, the argument
// and overlap check and the batched IHT / GD loop.  Included by mvm_batch4.hip (CloverMatrix4 x CloverVector4), mvm_batch8.hip
// (CloverMatrix4 x CloverVector8), matrix8_batch.hip (CloverMatrix8 x CloverVector8), mvm_t4_batch.hip (CloverMatrix4' x CloverVector4
// straight from the matrix's own bytes), mvm_t8_batch.hip (CloverMatrix4' x CloverVector8, likewise) and matrix8_t_batch.hip (CloverMatrix8' x
// CloverVector8, likewise); half16_batch_host.h (the driver of the two half-precision families, no scales and no draws) includes it for
// mvm_batch_forced() alone.  Each of the six defines its
// kernel and a traits struct F with exactly what differs between the families:
//   Args<NV>, Fuse<NV>                        the kernel's by-value argument structs (their pointer types decide the casts)
//   matrix_bytes(rows, cols), vector_bytes(n) sizes for the overlap check; the matrix streams (NT) above the 256 MiB Infinity Cache
//   check_matrix(fn, A, sA, rows, cols)       the single call's size rules
//   result_may_not_alias_x(fused)             whether r[j] == x[j] is refused by name (otherwise the range check reports it as an overlap)
//   mvm, scale_and_add, iht                   the single calls a group is forwarded to
//   clear, threshold_batch                    x.clear() of one vector, the threshold of a group
//   iht_prefers_single(...)                   whether a group of the IHT loop is better off as single calls (measured per family)
//   launch<NV, NT, FUSE, ST>(...)             the hipLaunchKernelGGL of the family's kernel, with its U and LDS bytes
//   x_len, r_len, grid, batched_by_rule       which dimension sizes x and which r, the grid of a launch and the measured dispatch rule:
//                                             MvmBatchByRows (below) for the three families that walk the matrix by rows; the transposed
//                                             three take x_len and r_len from MvmBatchByCols and keep a grid and a rule of their own
//   nothing_to_do(nvec, rows, cols)           the empty-call rule of the three mvm batch entry points: checked arguments, no device work
// The extern "C" mvm batch entry points of a family forward to mvm_batch_entry, mvm_batch_at_entry and mvm_batch_fused_entry (below) with
// their own names, which the messages quote.
#pragma once

#include "mvm_batch_device.h"

#include <stdlib.h>

#include <type_traits>

// CLV_MVM_BATCH, read on every call (as CLV_IHT_PERSISTENT: the tests and tools/kernel_bench.py flip it inside one process):
// 1 = always batched, 0 = never, -1 = unset
static inline int mvm_batch_forced()
{
    const char *e = clv_env("CLV_MVM_BATCH");
    return e && *e ? (atoi(e) != 0) : -1;
}

// what the three row-major families share: r = A x has `rows` elements, x `cols`; one workgroup per 64-row block; every group of two
// or more runs batched (measured, see mvm_batch_selected)
struct MvmBatchByRows {
    static uint64_t x_len(uint64_t, uint64_t cols) { return cols; }
    static uint64_t r_len(uint64_t rows, uint64_t) { return rows; }
    static dim3 grid(uint64_t rows, uint64_t) { return dim3((unsigned)(rows / 64)); }
    static bool batched_by_rule(uint64_t g, uint64_t, uint64_t, bool, bool) { return g >= 2; }
    static bool nothing_to_do(uint64_t nvec, uint64_t rows, uint64_t) { return !nvec || !rows; }
};

// what the three transposed families share: A is rows x cols, x has `rows` elements and r = A' x has `cols`; a matrix without rows has
// nothing to multiply, one without columns nothing to write; r[j] == x[j] is left to the range check
struct MvmBatchByCols {
    static uint64_t x_len(uint64_t rows, uint64_t) { return rows; }
    static uint64_t r_len(uint64_t, uint64_t cols) { return cols; }
    static bool nothing_to_do(uint64_t nvec, uint64_t rows, uint64_t cols) { return !nvec || !rows || !cols; }
    static bool result_may_not_alias_x(bool) { return false; }
};

// the explicit instantiations of F::launch behind a transposed family's definition of it, for the driver's NV = 2, 4, 8 (the traits are
// declared in a header of their own, the launches defined beside the kernel)
#define MVM_BATCH_INSTANTIATE_LAUNCH(F, NV, NT, FUSE, ST)                                                                     \
    template void F::launch<NV, NT, FUSE, ST>(dim3, hipStream_t, const uint8_t *, const float *, uint64_t, uint64_t, int, \
                                              const F::Args<NV> &, const F::Fuse<NV> &, const MvmBatchRng &);
#define MVM_BATCH_INSTANTIATE_LAUNCHES_NV(F, NV)                                                                                      \
    MVM_BATCH_INSTANTIATE_LAUNCH(F, NV, false, false, false) MVM_BATCH_INSTANTIATE_LAUNCH(F, NV, false, false, true)              \
    MVM_BATCH_INSTANTIATE_LAUNCH(F, NV, false, true, false) MVM_BATCH_INSTANTIATE_LAUNCH(F, NV, false, true, true)                \
    MVM_BATCH_INSTANTIATE_LAUNCH(F, NV, true, false, false) MVM_BATCH_INSTANTIATE_LAUNCH(F, NV, true, false, true)                \
    MVM_BATCH_INSTANTIATE_LAUNCH(F, NV, true, true, false) MVM_BATCH_INSTANTIATE_LAUNCH(F, NV, true, true, true)
#define MVM_BATCH_INSTANTIATE_LAUNCHES(F) \
    MVM_BATCH_INSTANTIATE_LAUNCHES_NV(F, 2) MVM_BATCH_INSTANTIATE_LAUNCHES_NV(F, 4) MVM_BATCH_INSTANTIATE_LAUNCHES_NV(F, 8)

// Whether a group of g vectors runs as one batched launch or as g single launches.  Forced to 1, with an rng a remainder group of ONE vector
// (nvec = 9, 17, ...) runs batched too: a forced call then hands the state from batched launch to batched launch throughout, which is what
// the tests of that hand-over need.  Unset = the rule measured on the MI355X, the same for the three families: every group of
// two or more, whatever the shape.
//   4-bit   profiles/mvm_batch_kernel_bench.json, stochastic profiles/mvm_batch_st_kernel_bench.json
//   mixed   profiles/mvm_v8_batch_kernel_bench.json, stochastic profiles/mvm_v8_batch_st_kernel_bench.json
//   8-bit   profiles/m8_mvm_batch_kernel_bench.json, stochastic profiles/m8_mvm_batch_st_kernel_bench.json: at 2, 4 and 8 vectors the
//           batched launch beat the single calls by more than their spread in every row -- 65536^2 and 32768^2 (streaming), fused at
//           8192 x 4096 (cache-resident) and at 65536^2, the IHT loop at N = 8192, either rounding.  Not measured: groups of 3 and 5-7,
//           matrices between 32 MiB and 1 GiB or below 32 MiB.
// The transposed families have rules of their own (MvmT4Batch::batched_by_rule, mvm_t4_batch.h; MvmT8Batch::batched_by_rule, mvm_t8_batch.h;
// M8TBatch::batched_by_rule, matrix8_t_batch.h).
template <class F>
static inline bool mvm_batch_selected(uint64_t g, uint64_t rows, uint64_t cols, bool fused, bool stochastic)
{
    if (g < 2 && !stochastic) return false;
    const int force = mvm_batch_forced();
    return force >= 0 ? force != 0 : F::batched_by_rule(g, rows, cols, fused, stochastic);
}

// the vectors of a batch call (host arrays of device pointers) in the kernel's terms: r / sr NULL = the mvm result is not stored (fused
// form only); qu == NULL = plain mvm, else r2 = a * mvm + qu behind it
struct MvmBatchVectors {
    const int8_t *const *x;
    const float *const *sx;
    int8_t *const *r;
    float *const *sr;
    const int8_t *const *qu;
    const float *const *su;
    float a;
    int8_t *const *r2;
    float *const *sr2;
    MvmBatchVectors from(uint64_t j0) const
    {
        return {x + j0, sx + j0, r ? r + j0 : nullptr, r ? sr + j0 : nullptr, qu ? qu + j0 : nullptr, qu ? su + j0 : nullptr, a,
                qu ? r2 + j0 : nullptr, qu ? sr2 + j0 : nullptr};
    }
};

// the draws of a batched launch on the host side: rng == NULL = rounding disabled
struct MvmBatchDraws {
    uint64_t *rng;
    uint64_t base, stride, commit;
};

template <class T>
static inline void mvm_batch_slot(T *&slot, const void *p) { slot = (T *)p; }      // the cast into the family's Args / Fuse

// one launch for the first g <= NV vectors of v
template <class F, int NV>
static int mvm_batch_launch(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t g, const MvmBatchVectors &v,
                            const MvmBatchDraws &dr, hipStream_t st)
{
    typename F::template Args<NV> arg;
    typename F::template Fuse<NV> fuse;
    for (uint64_t i = 0; i < NV; i++) {
        const bool in = i < g;
        mvm_batch_slot(arg.x[i], in ? v.x[i] : nullptr);
        arg.sx[i] = in ? v.sx[i] : nullptr;
        mvm_batch_slot(arg.r[i], in && v.r ? v.r[i] : nullptr);
        arg.sr[i] = in && v.r ? v.sr[i] : nullptr;
        mvm_batch_slot(fuse.qu[i], in && v.qu ? v.qu[i] : nullptr);
        fuse.su[i] = in && v.qu ? v.su[i] : nullptr;
        mvm_batch_slot(fuse.r2[i], in && v.qu ? v.r2[i] : nullptr);
        fuse.sr2[i] = in && v.qu ? v.sr2[i] : nullptr;
    }
    fuse.a = v.a;
    MvmBatchRng rs = {nullptr, 0, nullptr, 0, 0, 0};
    if (dr.rng) {
        RngTables T = {nullptr, nullptr, nullptr};
        int rc = clv_rng_tables(&T);
        if (rc) return rc;
        // every launch takes a number of its own, committing or not: it is what picks the slot to read
        rs = MvmBatchRng{dr.rng, clv_rng_seq_for(dr.rng, st), T.pow_rows, dr.base, dr.stride, dr.commit};
    }
    const dim3 grid = F::grid(rows, cols);
    const uint8_t *Au = (const uint8_t *)A;
    const int nv = (int)g;
    // nontemporal loads by the rule of the single calls: once the matrix cannot live in the 256 MiB Infinity Cache
    const bool nt = F::matrix_bytes(rows, cols) > (256ull << 20), fused = v.qu != nullptr, st_ = dr.rng != nullptr;
    switch (4 * nt + 2 * fused + st_) {
    case 7: F::template launch<NV, true, true, true>(grid, st, Au, sA, rows, cols, nv, arg, fuse, rs); break;
    case 6: F::template launch<NV, true, true, false>(grid, st, Au, sA, rows, cols, nv, arg, fuse, rs); break;
    case 5: F::template launch<NV, true, false, true>(grid, st, Au, sA, rows, cols, nv, arg, fuse, rs); break;
    case 4: F::template launch<NV, true, false, false>(grid, st, Au, sA, rows, cols, nv, arg, fuse, rs); break;
    case 3: F::template launch<NV, false, true, true>(grid, st, Au, sA, rows, cols, nv, arg, fuse, rs); break;
    case 2: F::template launch<NV, false, true, false>(grid, st, Au, sA, rows, cols, nv, arg, fuse, rs); break;
    case 1: F::template launch<NV, false, false, true>(grid, st, Au, sA, rows, cols, nv, arg, fuse, rs); break;
    default: F::template launch<NV, false, false, false>(grid, st, Au, sA, rows, cols, nv, arg, fuse, rs); break;
    }
    CLV_LAUNCH_CHECK();
    clv_internal_mvm_batch_count();
    return CLV_OK;
}

// a group of g <= CLM4_MVM_BATCH_MAX vectors on the smallest instantiation that holds it
template <class F>
static int mvm_batch_launch_group(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t g, const MvmBatchVectors &v,
                                  const MvmBatchDraws &dr, hipStream_t st)
{
    return g <= 2   ? mvm_batch_launch<F, 2>(A, sA, rows, cols, g, v, dr, st)
           : g <= 4 ? mvm_batch_launch<F, 4>(A, sA, rows, cols, g, v, dr, st)
                    : mvm_batch_launch<F, 8>(A, sA, rows, cols, g, v, dr, st);
}

// The checked arguments of the family's mvm batch call (qu == NULL) / fused batch call on the stream, group by group.  With an rng every
// group starts at the state the group before it left (G = output blocks): a batched group's windows lie 2 G (fused: 4 G) draws apart from position 0 and its
// launch commits all of them, a forwarded group's single calls advance the state themselves -- so the two kinds mix freely.
template <class F>
static int mvm_batch_run(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const MvmBatchVectors &v, uint64_t *rng,
                         void *stream)
{
    const uint64_t per_vector = (v.qu ? 4ull : 2ull) * (F::r_len(rows, cols) / 64);
    for (uint64_t j0 = 0; j0 < nvec; j0 += CLM4_MVM_BATCH_MAX) {
        const uint64_t g = nvec - j0 < CLM4_MVM_BATCH_MAX ? nvec - j0 : CLM4_MVM_BATCH_MAX;
        int rc = CLV_OK;
        if (!mvm_batch_selected<F>(g, rows, cols, v.qu != nullptr, rng != nullptr)) {
            for (uint64_t j = j0; j < j0 + g && !rc; j++)
                rc = v.qu ? F::scale_and_add(A, sA, rows, cols, v.x[j], v.sx[j], v.qu[j], v.su[j], v.a, v.r ? v.r[j] : nullptr,
                                             v.r ? v.sr[j] : nullptr, v.r2[j], v.sr2[j], rng, stream)
                          : F::mvm(A, sA, rows, cols, v.x[j], v.sx[j], v.r[j], v.sr[j], rng, stream);
        } else {
            rc = mvm_batch_launch_group<F>(A, sA, rows, cols, g, v.from(j0), MvmBatchDraws{rng, 0, per_vector, g * per_vector}, as_stream(stream));
        }
        if (rc) return rc;
    }
    return CLV_OK;
}

// The positioned form: vector j's window begins draw_base + j * draw_stride draws behind the state the call finds, across groups too;
// only the last group's launch commits.  Always the batched kernel (a window that is not where a single call would draw cannot be
// forwarded).  rng == NULL: the deterministic kernel, the positions unused.  The caller has checked the positions (mvm_batch_check_draws).
template <class F>
static int mvm_batch_at(const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const MvmBatchVectors &v, uint64_t *rng,
                        uint64_t draw_base, uint64_t draw_stride, uint64_t commit_draws, void *stream)
{
    for (uint64_t j0 = 0; j0 < nvec; j0 += CLM4_MVM_BATCH_MAX) {
        const uint64_t g = nvec - j0 < CLM4_MVM_BATCH_MAX ? nvec - j0 : CLM4_MVM_BATCH_MAX;
        const bool last = j0 + g == nvec;
        int rc = mvm_batch_launch_group<F>(A, sA, rows, cols, g, v.from(j0),
                                           MvmBatchDraws{rng, draw_base + j0 * draw_stride, draw_stride, last ? commit_draws : 0}, as_stream(stream));
        if (rc) return rc;
    }
    return CLV_OK;
}

// the positions of a *_mvm_batch_at call with a generator: everything below 2^55, the exponents the jump-ahead has table levels for.
// rows = the elements of a result, F::r_len(rows, cols)
static inline int mvm_batch_check_draws(const char *fn, uint64_t rows, uint64_t nvec, uint64_t draw_base, uint64_t draw_stride, uint64_t commit_draws)
{
    CLV_REQUIRE(commit_draws < (1ull << (RNG_POW_LEVELS - 1)), "%s: commit_draws=%llu must stay below 2^55", fn, (unsigned long long)commit_draws);
    const uint64_t bad = clv_internal_first_bad_window(nvec, draw_base, draw_stride, 2 * (rows / 64));
    CLV_REQUIRE(bad == nvec, "%s: the draws of vector %llu (draw_base=%llu, draw_stride=%llu) do not stay below 2^55", fn, (unsigned long long)bad,
                (unsigned long long)draw_base, (unsigned long long)draw_stride);
    return CLV_OK;
}

// every check of the family's three mvm batch calls, before any device work.  r / sr: the call's result; t / st_: the fused call's
// optional mvm result
template <class F>
static int mvm_batch_check_args(const char *fn, const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                                const float *const *sx, const int8_t *const *qu, const float *const *su, int8_t *const *t, float *const *st_,
                                int8_t *const *r, float *const *sr, bool fused)
{
    // a NULL vector array is reported as such, not as one of the single call's pointers
    int rc = F::check_matrix(fn, A, sA, rows, cols);
    if (rc) return rc;
    if (!nvec) return CLV_OK;
    CLV_REQUIRE(x && sx && r && sr && (!fused || (qu && su)), "%s: null pointer array", fn);
    CLV_REQUIRE((t == nullptr) == (st_ == nullptr), "%s: t and st must both be given or both be NULL", fn);
    for (uint64_t j = 0; j < nvec; j++)
        CLV_REQUIRE(x[j] && sx[j] && r[j] && sr[j] && (!fused || (qu[j] && su[j])) && (!t || (t[j] && st_[j])), "%s: null pointer in vector %llu", fn,
                    (unsigned long long)j);
    if (F::result_may_not_alias_x(fused))
        for (uint64_t j = 0; j < nvec; j++)
            CLV_REQUIRE((const void *)r[j] != (const void *)x[j] && (const void *)sr[j] != (const void *)sx[j],
                        "%s: the result of vector %llu must not alias the vector being multiplied", fn, (unsigned long long)j);
    std::vector<ClvRange> rg;
    rg.reserve(8 * nvec + 2);
    const uint64_t sc = sizeof(float), xl = F::x_len(rows, cols), rl = F::r_len(rows, cols), xb = F::vector_bytes(xl), rb = F::vector_bytes(rl);
    rg.push_back(clv_range(A, F::matrix_bytes(rows, cols), false, ~0ull, "A"));
    rg.push_back(clv_range(sA, (rows / 64) * (cols / 64) * sc, false, ~0ull, "sA"));
    for (uint64_t j = 0; j < nvec; j++) {
        rg.push_back(clv_range(x[j], xb, false, j, "x"));
        rg.push_back(clv_range(sx[j], xl / 64 * sc, false, j, "sx"));
        rg.push_back(clv_range(r[j], rb, true, j, "r"));
        rg.push_back(clv_range(sr[j], rl / 64 * sc, true, j, "sr"));
        if (fused) {
            // the in-place form r[j] == qu[j], sr[j] == su[j]: the result IS the input, only the workgroup that owns a block touches it in either
            const bool in_place = (const void *)r[j] == (const void *)qu[j] && (const void *)sr[j] == (const void *)su[j];
            if (!in_place) {
                rg.push_back(clv_range(qu[j], rb, false, j, "qu"));
                rg.push_back(clv_range(su[j], rl / 64 * sc, false, j, "su"));
            }
        }
        if (t) {
            rg.push_back(clv_range(t[j], rb, true, j, "t"));
            rg.push_back(clv_range(st_[j], rl / 64 * sc, true, j, "st"));
        }
    }
    return clv_internal_check_ranges(fn, rg);
}

// ---- the bodies of a family's three extern "C" mvm batch entry points; fn = the name of the entry point that was called -----------------
// *_batch: r[j] = quantize(A x[j]) (the transposed families: A' x[j]); one vector is the single call
template <class F>
static int mvm_batch_entry(const char *fn, const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                           const float *const *sx, int8_t *const *r, float *const *sr, uint64_t *rng, void *stream)
{
    int rc = mvm_batch_check_args<F>(fn, A, sA, rows, cols, nvec, x, sx, nullptr, nullptr, nullptr, nullptr, r, sr, false);
    if (rc) return rc;
    if (F::nothing_to_do(nvec, rows, cols)) return CLV_OK;
    if (nvec == 1) return F::mvm(A, sA, rows, cols, x[0], sx[0], r[0], sr[0], rng, stream);
    return mvm_batch_run<F>(A, sA, rows, cols, nvec, {x, sx, r, sr, nullptr, nullptr, 0.0f, nullptr, nullptr}, rng, stream);
}

// *_batch_at: the same with the place of every vector's draws chosen by the caller; without an rng it is the plain call, fn_plain
template <class F>
static int mvm_batch_at_entry(const char *fn, const char *fn_plain, const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec,
                              const int8_t *const *x, const float *const *sx, int8_t *const *r, float *const *sr, uint64_t *rng, uint64_t draw_base,
                              uint64_t draw_stride, uint64_t commit_draws, void *stream)
{
    int rc = mvm_batch_check_args<F>(fn, A, sA, rows, cols, nvec, x, sx, nullptr, nullptr, nullptr, nullptr, r, sr, false);
    if (rc) return rc;
    if (!rng) return mvm_batch_entry<F>(fn_plain, A, sA, rows, cols, nvec, x, sx, r, sr, nullptr, stream);
    rc = mvm_batch_check_draws(fn, F::r_len(rows, cols), nvec, draw_base, draw_stride, commit_draws);
    if (rc) return rc;
    if (F::nothing_to_do(nvec, rows, cols)) return CLV_OK;
    return mvm_batch_at<F>(A, sA, rows, cols, nvec, {x, sx, r, sr, nullptr, nullptr, 0.0f, nullptr, nullptr}, rng, draw_base, draw_stride,
                           commit_draws, stream);
}

// *_scale_and_add_batch: t[j] = quantize(A x[j]) (stored if t != NULL), r[j] = quantize(qu[j] + a * t[j]); one vector is the single call
template <class F>
static int mvm_batch_fused_entry(const char *fn, const int8_t *A, const float *sA, uint64_t rows, uint64_t cols, uint64_t nvec, const int8_t *const *x,
                                 const float *const *sx, const int8_t *const *qu, const float *const *su, float a, int8_t *const *t,
                                 float *const *st_, int8_t *const *r, float *const *sr, uint64_t *rng, void *stream)
{
    int rc = mvm_batch_check_args<F>(fn, A, sA, rows, cols, nvec, x, sx, qu, su, t, st_, r, sr, true);
    if (rc) return rc;
    if (F::nothing_to_do(nvec, rows, cols)) return CLV_OK;
    if (nvec == 1)
        return F::scale_and_add(A, sA, rows, cols, x[0], sx[0], qu[0], su[0], a, t ? t[0] : nullptr, t ? st_[0] : nullptr, r[0], sr[0], rng, stream);
    return mvm_batch_run<F>(A, sA, rows, cols, nvec, {x, sx, t, st_, qu, su, a, r, sr}, rng, stream);
}

// Q_IHT / Q_GD for nvec signals with one Phi: the loop of the family's single call F::iht with every step batched.  Arrays are HOST arrays
// of nvec device pointers.  Bit-identical to F::iht per vector (where that takes a persistent kernel: it equals the launch-per-step loop
// bit for bit).  FT = the family that takes step 2, t3 = Phi' t2: F itself on the held PhiT, or the transposed family on Phi's own bytes
// (PhiT / sPhiT are then NULL and unused, the single call is FT::iht_one_matrix, which never takes a persistent kernel).
template <class F, class FT = F>
static int mvm_batch_iht(const char *fn, const int8_t *Phi, const float *sPhi, const int8_t *PhiT, const float *sPhiT, uint64_t m, uint64_t n,
                         uint64_t nvec, int8_t *const *x, float *const *sx, uint64_t x_len, const int8_t *const *y, const float *const *sy,
                         int8_t *const *t1, float *const *st1, int8_t *const *t2, float *const *st2, int8_t *const *t3, float *const *st3,
                         uint64_t iterations, uint64_t K, float mu, int threshold, uint64_t *rng, void *stream)
{
    constexpr bool one_matrix = !std::is_same<F, FT>::value;
    CLV_REQUIRE(Phi && sPhi && (one_matrix || (PhiT && sPhiT)), "%s: null pointer", fn);
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
        const uint64_t sc = sizeof(float), tiles = (m / 64) * (n / 64), mb = F::vector_bytes(m), nb = F::vector_bytes(n);
        rg.push_back(clv_range(Phi, F::matrix_bytes(m, n), false, ~0ull, "Phi"));
        rg.push_back(clv_range(sPhi, tiles * sc, false, ~0ull, "sPhi"));
        if (!one_matrix) {
            rg.push_back(clv_range(PhiT, F::matrix_bytes(m, n), false, ~0ull, "PhiT"));
            rg.push_back(clv_range(sPhiT, tiles * sc, false, ~0ull, "sPhiT"));
        }
        for (uint64_t j = 0; j < nvec; j++) {
            rg.push_back(clv_range(y[j], mb, false, j, "y"));
            rg.push_back(clv_range(sy[j], m / 64 * sc, false, j, "sy"));
            rg.push_back(clv_range(x[j], nb, true, j, "x"));
            rg.push_back(clv_range(sx[j], n / 64 * sc, true, j, "sx"));
            rg.push_back(clv_range(t1[j], mb, true, j, "t1"));
            rg.push_back(clv_range(st1[j], m / 64 * sc, true, j, "st1"));
            rg.push_back(clv_range(t2[j], mb, true, j, "t2"));
            rg.push_back(clv_range(st2[j], m / 64 * sc, true, j, "st2"));
            rg.push_back(clv_range(t3[j], nb, true, j, "t3"));
            rg.push_back(clv_range(st3[j], n / 64 * sc, true, j, "st3"));
        }
        int rc = clv_internal_check_ranges(fn, rg);
        if (rc) return rc;
    }
    // Which groups run the batched loop: groups of two or more over a matrix that is not empty, unless the family measured its single calls
    // faster for such a group (F::iht_prefers_single).  CLV_MVM_BATCH = 1 / 0 forces one or the other.
    // The draws keep the order of the single calls, all iterations of vector 0 first: one iteration draws P = 4 (m / 64) + 4 (n / 64), so
    // vector j of a group has its Phi window of iteration `it` at (j * iterations + it) * P and its PhiT window 4 (m / 64) further on; only
    // the group's last launch commits, all g * iterations * P.
    const int force = mvm_batch_forced();
    const uint64_t P = 4 * (m / 64) + 4 * (n / 64);
    const int mode = threshold == 2 ? CLV_THRESHOLD_REFERENCE : CLV_THRESHOLD_FAST;
    for (uint64_t j0 = 0; j0 < nvec; j0 += CLM4_MVM_BATCH_MAX) {
        const uint64_t g = nvec - j0 < CLM4_MVM_BATCH_MAX ? nvec - j0 : CLM4_MVM_BATCH_MAX;
        bool batched = g >= 2 && m && n && force != 0 && (force == 1 || !FT::iht_prefers_single(m, n, iterations, threshold, rng != nullptr, g));
        if (rng && g * P && iterations > ((1ull << 55) - 1) / (g * P)) batched = false;      // positions beyond the jump-ahead tables
        if (!batched) {
            for (uint64_t j = j0; j < j0 + g; j++) {
                int rc;
                if constexpr (one_matrix)
                    rc = FT::iht_one_matrix(Phi, sPhi, m, n, x[j], sx[j], x_len, y[j], sy[j], t1[j], st1[j], t2[j], st2[j], t3[j], st3[j], iterations, K, mu,
                                            threshold, rng, stream);
                else
                    rc = F::iht(Phi, sPhi, PhiT, sPhiT, m, n, x[j], sx[j], x_len, y[j], sy[j], t1[j], st1[j], t2[j], st2[j], t3[j], st3[j], iterations, K,
                                mu, threshold, rng, stream);
                if (rc) return rc;
            }
            continue;
        }
        for (uint64_t j = j0; j < j0 + g; j++) {
            int rc = F::clear(x[j], sx[j], n, as_stream(stream));      // x.clear()
            if (rc) return rc;
        }
        const uint64_t stride = iterations * P;
        const MvmBatchVectors step1 = {x + j0, sx + j0, t1 + j0, st1 + j0, y + j0, sy + j0, -1.0f, t2 + j0, st2 + j0};
        const MvmBatchVectors step2 = {t2 + j0, st2 + j0, t3 + j0, st3 + j0, x + j0, sx + j0, mu, x + j0, sx + j0};
        for (uint64_t it = 0; it < iterations; it++) {
            // t1 = Phi * x, t2 = y - t1;  t3 = Phi' * t2, x += mu * t3;  keep the K largest: three launches for the group
            const uint64_t commit = it + 1 == iterations ? g * stride : 0;
            int rc = mvm_batch_at<F>(Phi, sPhi, m, n, g, step1, rng, it * P, stride, 0, stream);
            if (!rc)
                rc = one_matrix ? mvm_batch_at<FT>(Phi, sPhi, m, n, g, step2, rng, it * P + 4 * (m / 64), stride, commit, stream)
                                : mvm_batch_at<F>(PhiT, sPhiT, n, m, g, step2, rng, it * P + 4 * (m / 64), stride, commit, stream);
            if (!rc && threshold) rc = F::threshold_batch(x + j0, sx + j0, g, x_len, n, K, mode, stream);
            if (rc) return rc;
        }
    }
    return CLV_OK;
}
