// validate_grid_wide.cpp -- the reference's validation harness for the three wider containers, CloverVector16, CloverMatrix8 and
// CloverMatrix16, which it instantiates for bit counts 8 and 16 as well (test/validate/02_vector.cpp:579-636, 03_matrix.cpp:598-629):
//   vector16  02_vector.cpp:111-553 at 16 bits.  The device sees n_pad only (threshold also n), so not every n: for each n_pad = 128,
//             256 ... 2048 the five n = n_pad - 127, n_pad - 64, n_pad - 63, n_pad - 1, n_pad (80 sizes): the tail at the start, in the
//             middle and at the end of the last 128 elements, for every block count the reference covers
//   matrix8 / matrix16  03_matrix.cpp:38-573 at 8 / 16 bits: every (128 i) x (128 j), i, j = 1 ... 10, and three ragged shapes the
//             constructors accept, (100, 200), (129, 127), (1000, 72), compared at the padded size
// Each relation has the device method on one side and its scalar host twin on the other, at the reference's strictness; "exact" is == on
// get() values and memcmp of getData() (for CloverMatrix8 / CloverVector8 the scales behind them too).  Built with
// -DCLOVER_STOCHASTIC_ROUNDING_DISABLED=1 as the reference's exact checks require; every pointer is taken AFTER the device operation it
// reads, so the same text is right in the -DCLOVER_HIP_EXPLICIT_SYNC build.
//   validate_grid_wide <vector16|matrix8|matrix16> [a-b] [dir [corners]]
// a-b: grid rows i = a ... b only (the ragged shapes go with the row range that contains 10).  dir: also run mvm on NON-INTEGER data
// (setRandomFloats(-1, 1)) at the four corner shapes of the grid and write operands and results there -- integer data make every order of
// summation give the same bits, which is this harness's (and the reference's) blind spot; the Python side compares those bytes with the
// restatements.  "corners" after dir: only that.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "CloverMatrix16.h"
#include "CloverMatrix8.h"
#include "CloverVector16.h"
#include "CloverVector8.h"

static int failures = 0;
static void expect(bool ok, const char *what, uint64_t a, uint64_t b)
{
    if (!ok) {
        if (failures < 40) std::printf("FAILED %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
        failures++;
    }
}

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// ---- byte equality of two containers of one class
static bool same_bytes(const CloverVector16 &a, const CloverVector16 &b) { return !std::memcmp(a.getData(), b.getData(), a.getBytes()); }
static bool same_bytes(const CloverVector8 &a, const CloverVector8 &b)
{
    return !std::memcmp(a.getData(), b.getData(), a.size_pad()) && !std::memcmp(a.getScales(), b.getScales(), a.size_pad() / 64 * sizeof(float));
}
static bool same_bytes(const CloverMatrix16 &a, const CloverMatrix16 &b) { return !std::memcmp(a.getData(), b.getData(), a.getBytes()); }
static bool same_bytes(const CloverMatrix8 &a, const CloverMatrix8 &b)      // values, then the grid of tile scales behind them
{
    return !std::memcmp(a.getData(), b.getData(), a.getRows() * a.getCols()) &&
           !std::memcmp(a.getScales(), b.getScales(), (a.getRows() / 64) * (a.getCols() / 64) * sizeof(float));
}

// ------------------------------------------------------------------------------------------------ vector16
template <class QVector>
static void threshold_relation(const CloverVector32 &src, uint64_t n, const char *what)      // 02_vector.cpp:449-553
{
    const uint64_t k = 64;
    CloverVector32 v(n), r(n);
    QVector q(n);
    q.quantize(src);
    QVector copy(q);
    copy.restore(v);
    q.threshold(k);
    q.restore(r);
    for (uint64_t i = n; i < q.size_pad(); i++) expect(q.getData()[i] == 0, "padding after threshold", n, i);
    auto by_mag = [](float a, float b) { return std::fabs(a) > std::fabs(b); };
    std::sort(v.getData(), v.getData() + n, by_mag);
    std::sort(r.getData(), r.getData() + n, by_mag);
    for (uint64_t i = 0; i < k; i++) {
        const float a = std::fabs(v.get(i)), b = std::fabs(r.get(i));
        expect(a == b || std::fabs(a - b) / std::max(a, b) <= 0.1f, what, n, i);       // the reference allows 10 %; equality holds here
    }
    for (uint64_t i = k; i < n; i++) expect(r.get(i) == 0.0f, "threshold keeps at most k", n, i);
}

// the reference's containers keep their padding zero; dot and the next quantize depend on it
static void padding_is_zero(const CloverVector16 &v, const char *what)
{
    const uint16_t *p = v.getData();
    for (uint64_t i = v.size(); i < v.size_pad(); i++) expect(p[i] == 0x0000, what, v.size(), i);
}

static void vector16_size(uint64_t n)
{
    CloverVector32 x(n), y(n), z(n), r1(n), r2(n);
    x.setRandomInteger(10, 1000 + n);
    y.setRandomInteger(7, 2000 + n);
    z.setRandomInteger(7, 3000 + n);
    CloverVector16 q(n), qp(n), qs(n);
    // the destinations' padding starts out NON-zero (setBits reaches all size_pad() elements, CloverVector16.h:114-117): quantize converts
    // all size_pad() elements of a zero-padded source, so it has to come out zero
    for (uint64_t i = n; i < q.size_pad(); i++) { q.setBits(i, 0x3C00); qp.setBits(i, 0x3C00); qs.setBits(i, 0x3C00); }
    q.quantize(x);
    qp.quantize_parallel(x);
    qs.quantize_scalar(x);
    padding_is_zero(q, "padding after quantize");
    padding_is_zero(qp, "padding after quantize_parallel");
    padding_is_zero(qs, "padding after quantize_scalar");
    for (uint64_t i = 0; i < n; i++) {
        expect(q.get(i) == qs.get(i), "quantize vs quantize_scalar", n, i);                                              // :111-144
        expect(qp.get(i) == qs.get(i), "quantize_parallel vs quantize_scalar", n, i);                                    // :146-179
    }
    expect(same_bytes(q, qs) && same_bytes(qp, qs), "quantize == quantize_parallel == quantize_scalar (bytes)", n, 0);
    q.restore(r1);
    q.restore_scalar(r2);
    for (uint64_t i = 0; i < n; i++) expect(r1.get(i) == r2.get(i), "restore vs restore_scalar", n, i);                  // :223-256
    expect(!std::memcmp(r1.getData(), r2.getData(), r1.getBytes()), "restore vs restore_scalar (bytes)", n, 0);
    CloverVector16 qa(n), qb(n);
    qa.quantize(y);
    qa.restore(r1);
    for (uint64_t i = 0; i < n; i++) expect(std::fabs(y.get(i) - r1.get(i)) <= 1.0f, "quantize -> restore consistency", n, i);   // :181-221
    qb.quantize(z);
    // :258-339: the reference's 0.02 absolute.  And more: the data are integers below 2^11, so every product and every partial sum is an
    // integer below 2^24 -- exact in fp32 in ANY order -- and the three forms must agree bit for bit
    const float ds = qa.dot_scalar(qb), dd = qa.dot(qb), dp = qa.dot_parallel(qb);
    expect(std::fabs(dd - ds) <= 0.02f, "dot vs dot_scalar", n, 0);
    expect(std::fabs(dp - ds) <= 0.02f, "dot_parallel vs dot_scalar", n, 0);
    expect(bits(dd) == bits(ds) && bits(dp) == bits(ds), "dot == dot_parallel == dot_scalar (bits, integer data)", n, bits(dd));
    CloverVector32 w(n);
    w.setRandomInteger(40, 4000 + n);
    CloverVector16 u(n);
    u.quantize(w);
    CloverVector16 s1(u), s2(u), s3(u), s4(n), s5(n), s6(n);
    for (uint64_t i = n; i < s4.size_pad(); i++) { s4.setBits(i, 0x3C00); s6.setBits(i, 0x3C00); }
    s1.scaleAndAdd(q, 0.5f);
    s2.scaleAndAdd_scalar(q, 0.5f);
    s3.scaleAndAdd_parallel(q, 0.5f);
    u.scaleAndAdd(q, 0.5f, s4);
    u.scaleAndAdd_scalar(q, 0.5f, s5);
    u.scaleAndAdd_parallel(q, 0.5f, s6);
    padding_is_zero(s1, "padding after scaleAndAdd (in place)");
    padding_is_zero(s3, "padding after scaleAndAdd_parallel (in place)");
    padding_is_zero(s4, "padding after scaleAndAdd (3 operands)");
    padding_is_zero(s6, "padding after scaleAndAdd_parallel (3 operands)");
    for (uint64_t i = 0; i < n; i++) {
        expect(s1.get(i) == s2.get(i), "scaleAndAdd vs scalar (in place)", n, i);                                        // :341-393
        expect(s3.get(i) == s2.get(i), "scaleAndAdd_parallel vs scalar", n, i);                                          // :395-447
        expect(s4.get(i) == s5.get(i), "scaleAndAdd vs scalar (3 operands)", n, i);
        expect(s6.get(i) == s5.get(i), "scaleAndAdd_parallel vs scalar (3 operands)", n, i);
    }
    expect(same_bytes(s1, s2) && same_bytes(s3, s2) && same_bytes(s4, s5) && same_bytes(s6, s5), "scaleAndAdd forms (bytes)", n, 0);
    clover_hip::set_threshold_mode(CLV_THRESHOLD_FAST);                                                                  // :449-553, both tie rules
    threshold_relation<CloverVector16>(w, n, "threshold: sorted magnitudes");
    clover_hip::set_threshold_mode(CLV_THRESHOLD_REFERENCE);
    threshold_relation<CloverVector16>(w, n, "threshold (reference order): sorted magnitudes");
}

static void vector16()
{
    for (uint64_t n_pad = 128; n_pad <= 2048; n_pad += 128) {
        const uint64_t tails[5] = {n_pad - 127, n_pad - 64, n_pad - 63, n_pad - 1, n_pad};
        for (int t = 0; t < 5; t++) vector16_size(tails[t]);
    }
}

// ------------------------------------------------------------------------------------------------ matrix8 / matrix16
// restore exists as a device / scalar pair on the 8-bit class only
static void restore_relation(const CloverMatrix8 &q, uint64_t M, uint64_t N)
{
    CloverMatrix32 R1(M, N), R2(M, N);
    q.restore(R1);
    q.restore_scalar(R2);
    expect(!std::memcmp(R1.getData(), R2.getData(), M * N * sizeof(float)), "matrix restore vs restore_scalar", M, N);
    for (uint64_t i = 0; i < M; i += 37)
        for (uint64_t j = 0; j < N; j += 1) expect(R1.get(i, j) == q.get(i, j), "matrix restore vs get", i, j);
}
static void restore_relation(const CloverMatrix16 &, uint64_t, uint64_t) {}

// m x n logical elements of integers in [-max, max], the padding zero
static void fill_integers(CloverMatrix32 &A, uint64_t m, uint64_t n, float max_value, uint64_t seed)
{
    CloverVector32 src(m * n);
    src.setRandomInteger(max_value, seed);
    A.clear();
    const float *s = src.getData();
    float *a = A.getData();
    for (uint64_t i = 0; i < m; i++) std::memcpy(a + i * A.getCols(), s + i * n, n * sizeof(float));
}

template <class QMatrix, class QVector>
static void matrix_shape(uint64_t m, uint64_t n, uint64_t seed)
{
    CloverMatrix32 A(m, n);
    const uint64_t M = A.getRows(), N = A.getCols();
    fill_integers(A, m, n, 10, 77 * seed + 1);
    QMatrix qA(m, n), qS(m, n);
    qA.quantize(A);
    qS.quantize_scalar(A);
    for (uint64_t i = 0; i < M; i++)
        for (uint64_t j = 0; j < N; j++) expect(qA.get(i, j) == qS.get(i, j), "matrix quantize vs quantize_scalar", i, j);       // :38-96
    expect(same_bytes(qA, qS), "matrix quantize vs quantize_scalar (bytes)", M, N);
    for (uint64_t i = 0; i < M; i++)                                     // ragged: the padded rows and columns come out zero
        for (uint64_t j = (i < m ? n : 0); j < N; j++) expect(qA.getData()[i * N + j] == 0 && qA.get(i, j) == 0.0f, "matrix padding after quantize", i, j);
    restore_relation(qA, M, N);
    {
        CloverMatrix32 A7(m, n);
        fill_integers(A7, m, n, 7, 99 * seed + 2);
        QMatrix q7(m, n);
        q7.quantize(A7);
        for (uint64_t i = 0; i < M; i++)
            for (uint64_t j = 0; j < N; j++) expect(std::fabs(A7.get(i, j) - q7.get(i, j)) <= 1.0f, "matrix consistency", i, j);   // :99-151
    }
    // mvm == mvm_parallel == mvm_scalar with a quantized vector of the class's own width: EXACT, as validate_matrix_MVM demands with
    // rounding disabled (:248-326, :495-573).  8-bit: mvm_scalar is the reference's dot order per row and the scalar quantiser.  f16: the
    // kernel's 32 chains and the scalar twin's one running sum are different orders, but the data are integers (|A|, |x| <= 10, N <= 1280):
    // every product and partial sum is an integer below 2^24, every fp32 sum is exact in any order, and both round the same fp32 value.
    CloverVector32 x(N);
    x.setRandomInteger(10, 5 * seed + 3);
    QVector qx(N), r(M), rp(M), rs(M);
    qx.quantize(x);
    qA.mvm(qx, r);
    qA.mvm_parallel(qx, rp);
    qA.mvm_scalar(qx, rs);
    for (uint64_t k = 0; k < M; k++) {
        expect(r.get(k) == rs.get(k), "mvm vs mvm_scalar", M, k);
        expect(rp.get(k) == rs.get(k), "mvm_parallel vs mvm_scalar", M, k);
    }
    expect(same_bytes(r, rs) && same_bytes(rp, rs), "mvm == mvm_parallel == mvm_scalar (bytes)", M, N);
    // fp32 vector (:419-491): |delta| <= 0.01 against the scalar loop (a double accumulation); mvm == mvm_parallel exactly
    CloverVector32 xs(N), y32(M), y32p(M), y32s(M);
    for (uint64_t j = 0; j < N; j++) xs.set(j, x.get(j) * 0.001f);
    qA.mvm(xs, y32);
    qA.mvm_parallel(xs, y32p);
    qA.mvm_scalar(xs, y32s);
    for (uint64_t k = 0; k < M; k++) expect(std::fabs(y32.get(k) - y32s.get(k)) <= 0.01f, "fp32-vector mvm vs mvm_scalar", M, k);
    expect(!std::memcmp(y32.getData(), y32p.getData(), M * sizeof(float)), "fp32-vector mvm vs mvm_parallel (bytes)", M, N);
    // transpose (:153-246)
    QMatrix T(n, m), Tp(n, m), Ts(n, m);
    qA.transpose(T);
    qA.transpose_parallel(Tp);
    qA.transpose_scalar(Ts);
    for (uint64_t i = 0; i < M; i++)
        for (uint64_t j = 0; j < N; j++) expect(qA.get(i, j) == T.get(j, i), "transpose", i, j);
    expect(same_bytes(T, Ts), "transpose vs transpose_scalar (bytes, scale tiles)", M, N);
    expect(same_bytes(Tp, Ts), "transpose_parallel vs transpose_scalar (bytes, scale tiles)", M, N);
    for (uint64_t j = 0; j < N; j++)
        for (uint64_t i = (j < n ? m : 0); i < M; i++) expect(T.getData()[j * M + i] == 0 && T.get(j, i) == 0.0f, "matrix padding after transpose", j, i);
}

template <class QMatrix, class QVector>
static void matrix_grid(uint64_t first, uint64_t last)
{
    for (uint64_t bi = first; bi <= last; bi++)
        for (uint64_t bj = 1; bj <= 10; bj++) matrix_shape<QMatrix, QVector>(128 * bi, 128 * bj, 10 * bi + bj);
    if (first <= 10 && last >= 10) {
        matrix_shape<QMatrix, QVector>(100, 200, 201);
        matrix_shape<QMatrix, QVector>(129, 127, 202);
        matrix_shape<QMatrix, QVector>(1000, 72, 203);
    }
}

// ---- non-integer data at the four corner shapes, for the byte comparison with the restatements
static void write_file(const std::string &path, const void *a, size_t na, const void *b = nullptr, size_t nb = 0)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(a, 1, na, f) != na || (nb && std::fwrite(b, 1, nb, f) != nb)) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); std::exit(2); }
    std::fclose(f);
}
static void dump(const std::string &path, const CloverVector16 &v) { write_file(path, v.getData(), v.getBytes()); }
static void dump(const std::string &path, const CloverVector8 &v) { write_file(path, v.getData(), v.size_pad(), v.getScales(), v.size_pad() / 64 * sizeof(float)); }
static void dump(const std::string &path, const CloverMatrix16 &A) { write_file(path, A.getData(), A.getBytes()); }
static void dump(const std::string &path, const CloverMatrix8 &A)
{
    write_file(path, A.getData(), A.getRows() * A.getCols(), A.getScales(), (A.getRows() / 64) * (A.getCols() / 64) * sizeof(float));
}

template <class QMatrix, class QVector>
static void corners(const std::string &dir)
{
    const uint64_t shapes[4][2] = {{128, 128}, {128, 1280}, {1280, 128}, {1280, 1280}};
    for (int s = 0; s < 4; s++) {
        const uint64_t M = shapes[s][0], N = shapes[s][1];
        const std::string base = dir + "/" + std::to_string(M) + "x" + std::to_string(N) + "_";
        CloverMatrix32 A(M, N);
        CloverVector32 x(N), f(M), fp(M), fs(M);
        A.setRandomFloats(-1.0f, 1.0f, 31 + s);
        x.setRandomFloats(-1.0f, 1.0f, 41 + s);
        QMatrix qA(M, N);
        QVector qx(N), r(M), rp(M), rs(M);
        qA.quantize(A);
        qx.quantize(x);
        qA.mvm(qx, r);
        qA.mvm_parallel(qx, rp);
        qA.mvm_scalar(qx, rs);
        qA.mvm(x, f);
        qA.mvm_parallel(x, fp);
        qA.mvm_scalar(x, fs);
        expect(same_bytes(r, rp), "corner shape: mvm vs mvm_parallel (bytes)", M, N);
        expect(!std::memcmp(f.getData(), fp.getData(), M * sizeof(float)), "corner shape: fp32-vector mvm vs mvm_parallel (bytes)", M, N);
        write_file(base + "A.f32", A.getData(), M * N * sizeof(float));
        write_file(base + "x.f32", x.getData(), N * sizeof(float));
        dump(base + "qA.bin", qA);
        dump(base + "qx.bin", qx);
        dump(base + "r.bin", r);
        dump(base + "rs.bin", rs);
        write_file(base + "f.f32", f.getData(), M * sizeof(float));
        write_file(base + "fs.f32", fs.getData(), M * sizeof(float));
    }
}

int main(int argc, char **argv)
{
    int ndev = 0;
    if (clv_device_count(&ndev) != CLV_OK || ndev == 0) { std::printf("no_device\n"); return 0; }
    const std::string family = argc > 1 ? argv[1] : "";
    uint64_t first = 1, last = 10;
    std::string dir;
    bool only_corners = false;
    for (int a = 2; a < argc; a++) {
        unsigned long long lo, hi;
        char tail;
        if (std::sscanf(argv[a], "%llu-%llu%c", &lo, &hi, &tail) == 2) { first = lo; last = hi; }
        else if (!std::strcmp(argv[a], "corners")) only_corners = true;
        else dir = argv[a];
    }
    if ((family != "vector16" && family != "matrix8" && family != "matrix16") || first < 1 || last > 10 || first > last || (only_corners && dir.empty())) {
        std::fprintf(stderr, "usage: %s vector16|matrix8|matrix16 [a-b] [dir [corners]]\n", argv[0]);
        return 2;
    }
    const auto t0 = std::chrono::steady_clock::now();
    if (family == "vector16") vector16();
    if (family == "matrix8" && !only_corners) matrix_grid<CloverMatrix8, CloverVector8>(first, last);
    if (family == "matrix16" && !only_corners) matrix_grid<CloverMatrix16, CloverVector16>(first, last);
    const auto t1 = std::chrono::steady_clock::now();
    if (family == "matrix8" && !dir.empty()) corners<CloverMatrix8, CloverVector8>(dir);
    if (family == "matrix16" && !dir.empty()) corners<CloverMatrix16, CloverVector16>(dir);
    const auto t2 = std::chrono::steady_clock::now();
    std::printf("%s_s=%.2f corners_s=%.2f\n", family.c_str(), std::chrono::duration<double>(t1 - t0).count(), std::chrono::duration<double>(t2 - t1).count());
    std::printf(failures ? "validate grid wide FAILED (%d)\n" : "validate grid wide ok\n", failures);
    return failures ? 1 : 0;
}
