// matrix8_dropin.cpp -- a client of include/CloverMatrix8.h written with the reference's method names (tests/test_matrix8.py).
//   matrix8_dropin <dir> <iht|gd> <m> <n> <iterations> <K> <mu>
//   matrix8_dropin <dir> ragged <m> <n>
// reads <dir>/phi.f32 (m x n) and <dir>/y.f32 (m), checks mvm == mvm_parallel == mvm_scalar for 8-bit and fp32 vectors (rounding
// disabled: validate/03_matrix.cpp does the same for CloverMatrix4), runs Q_IHT<CloverMatrix8, CloverVector8> or Q_GD<...> through
// the generic templates of CloverIHT.h and writes Phi, PhiT, y, x, t1, t2, t3 (values then scales) to <dir>/<name>.bin.
// ragged: a CloverMatrix8(m, n) with m, n not multiples of 128, from <dir>/phi.f32 (m x n) and <dir>/x.f32 (n): writes Phi, PhiT, the
// 8-bit mvm r1 and the fp32 mvm (<dir>/f1.f32), all at the padded size.
#include <CloverIHT.h>
#include <CloverMatrix8.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static std::vector<float> read_f32(const std::string &path, size_t n)
{
    std::vector<float> v(n);
    FILE *f = fopen(path.c_str(), "rb");
    if (!f || fread(v.data(), sizeof(float), n, f) != n) { fprintf(stderr, "cannot read %s\n", path.c_str()); exit(2); }
    fclose(f);
    return v;
}

static void write_bytes(const std::string &path, const void *a, size_t na, const void *b, size_t nb)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(a, 1, na, f) != na || fwrite(b, 1, nb, f) != nb) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(2); }
    fclose(f);
}

static void dump(const std::string &dir, const char *name, const CloverVector8 &v)
{
    write_bytes(dir + "/" + name + ".bin", v.getData(), v.size_pad(), v.getScales(), v.size_pad() / 64 * sizeof(float));
}

static void dump(const std::string &dir, const char *name, const CloverMatrix8 &A)
{
    write_bytes(dir + "/" + name + ".bin", A.getData(), A.getRows() * A.getCols(), A.getScales(),
                (A.getRows() / 64) * (A.getCols() / 64) * sizeof(float));
}

static bool same8(const CloverVector8 &a, const CloverVector8 &b)
{
    return !memcmp(a.getData(), b.getData(), a.size_pad()) && !memcmp(a.getScales(), b.getScales(), a.size_pad() / 64 * sizeof(float));
}

static int ragged(const std::string &dir, uint64_t m, uint64_t n)
{
    const std::vector<float> phi = read_f32(dir + "/phi.f32", m * n), xv = read_f32(dir + "/x.f32", n);
    CloverMatrix8 Phi(m, n), PhiT(n, m);
    const uint64_t rows = Phi.getRows(), cols = Phi.getCols();
    CloverMatrix32 Phi32(m, n);
    for (uint64_t i = 0; i < rows; i++)
        for (uint64_t j = 0; j < cols; j++) Phi32.set(i, j, i < m && j < n ? phi[i * n + j] : 0.0f);
    CloverVector32 x32(cols);
    for (uint64_t j = 0; j < cols; j++) x32.set(j, j < n ? xv[j] : 0.0f);
    Phi.quantize(Phi32);
    Phi.transpose(PhiT);
    CloverVector8 xq(x32), r1(rows);
    CloverVector32 f1(rows);
    Phi.mvm(xq, r1);
    Phi.mvm(x32, f1);
    dump(dir, "phi", Phi);
    dump(dir, "phit", PhiT);
    dump(dir, "xq", xq);
    dump(dir, "r1", r1);
    write_bytes(dir + "/f1.f32", f1.getData(), rows * sizeof(float), f1.getData(), 0);
    printf("rows=%llu cols=%llu done\n", (unsigned long long)rows, (unsigned long long)cols);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[2], "ragged")) return ragged(argv[1], strtoull(argv[3], 0, 10), strtoull(argv[4], 0, 10));
    if (argc != 8) { fprintf(stderr, "usage: %s dir iht|gd m n iterations K mu\n", argv[0]); return 2; }
    const std::string dir = argv[1], mode = argv[2];
    const uint64_t m = strtoull(argv[3], 0, 10), n = strtoull(argv[4], 0, 10), iterations = strtoull(argv[5], 0, 10),
                   K = strtoull(argv[6], 0, 10);
    const float mu = strtof(argv[7], 0);

    const std::vector<float> phi = read_f32(dir + "/phi.f32", m * n), yv = read_f32(dir + "/y.f32", m);
    CloverMatrix32 Phi32(m, n);
    for (uint64_t i = 0; i < m; i++)
        for (uint64_t j = 0; j < n; j++) Phi32.set(i, j, phi[i * n + j]);
    CloverVector32 y32(m), x32(n);
    for (uint64_t i = 0; i < m; i++) y32.set(i, yv[i]);
    for (uint64_t j = 0; j < n; j++) x32.set(j, phi[j] - phi[n + j]);

    CloverMatrix8 Phi(m, n), PhiT(n, m);
    Phi.quantize(Phi32);
    Phi.transpose(PhiT);
    CloverVector8 y(y32), xq(x32);

    // mvm == mvm_parallel == mvm_scalar (8-bit) and mvm == mvm_parallel (fp32)
    CloverVector8 r1(m), r2(m), r3(m);
    Phi.mvm(xq, r1);
    Phi.mvm_parallel(xq, r2);
    Phi.mvm_scalar(xq, r3);
    CloverVector32 f1(m), f2(m);
    Phi.mvm(x32, f1);
    Phi.mvm_parallel(x32, f2);
    printf("mvm_equal=%d mvm_f32_equal=%d\n", (int)(same8(r1, r2) && same8(r1, r3)), (int)!memcmp(f1.getData(), f2.getData(), m * sizeof(float)));
    dump(dir, "xq", xq);
    dump(dir, "r1", r1);

    CloverVector8 x(n), t1(m), t2(m), t3(n);
    if (mode == "iht") Q_IHT<CloverMatrix8, CloverVector8>(Phi, PhiT, x, y, t1, t2, t3, iterations, K, mu);
    else Q_GD<CloverMatrix8, CloverVector8>(Phi, PhiT, x, y, t1, t2, t3, iterations, mu);
    dump(dir, "phi", Phi);
    dump(dir, "phit", PhiT);
    dump(dir, "y", y);
    dump(dir, "x", x);
    dump(dir, "t1", t1);
    dump(dir, "t2", t2);
    dump(dir, "t3", t3);
    printf("done\n");
    return 0;
}
