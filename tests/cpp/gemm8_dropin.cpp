// gemm8_dropin.cpp -- a client of CloverMatrix8::gemm and CloverMatrix4::gemm(const CloverMatrix8 &, ...) (tests/test_gemm8.py).
//   gemm8_dropin <dir> <M> <N> <K>
// reads <dir>/a.f32 (M x K) and <dir>/b.f32 (N x K), quantizes A into a CloverMatrix8 and a CloverMatrix4 and B into a CloverMatrix8,
// calls both gemm methods and writes what the driver compares: the three images (<dir>/a8.bin, a4.bin, b8.bin: values then scales), the
// three restored matrices (ra8.f32, ra4.f32, rb8.f32) and the two products (c88.f32, c48.f32).
#include <CloverMatrix4.h>
#include <CloverMatrix8.h>

#include <cstdio>
#include <cstdlib>
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

static void fill(CloverMatrix32 &m, const std::vector<float> &v, uint64_t rows, uint64_t cols)
{
    for (uint64_t i = 0; i < rows; i++)
        for (uint64_t j = 0; j < cols; j++) m.set(i, j, v[i * cols + j]);
}

static void dump(const std::string &path, const CloverMatrix32 &m)
{
    write_bytes(path, m.getData(), m.getRows() * m.getCols() * sizeof(float), m.getData(), 0);
}

int main(int argc, char **argv)
{
    if (argc != 5) { fprintf(stderr, "usage: %s dir M N K\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    const uint64_t M = strtoull(argv[2], 0, 10), N = strtoull(argv[3], 0, 10), K = strtoull(argv[4], 0, 10);
    if (M % 128 || N % 128 || K % 128) { fprintf(stderr, "M, N and K are multiples of 128 here\n"); return 2; }

    CloverMatrix32 A32(M, K), B32(N, K), RA8(M, K), RA4(M, K), RB8(N, K), C88(M, N), C48(M, N);
    fill(A32, read_f32(dir + "/a.f32", M * K), M, K);
    fill(B32, read_f32(dir + "/b.f32", N * K), N, K);

    CloverMatrix8 A8(M, K), B8(N, K);
    CloverMatrix4 A4(M, K);
    A8.quantize(A32);
    A4.quantize(A32);
    B8.quantize(B32);

    A8.gemm(B8, C88);
    A4.gemm(B8, C48);

    A8.restore(RA8);
    A4.restore(RA4);
    B8.restore(RB8);

    const size_t tiles_a = (M / 64) * (K / 64) * sizeof(float), tiles_b = (N / 64) * (K / 64) * sizeof(float);
    write_bytes(dir + "/a8.bin", A8.getData(), M * K, A8.getScales(), tiles_a);
    write_bytes(dir + "/a4.bin", A4.getData(), M * K / 2, A4.getScales(), tiles_a);
    write_bytes(dir + "/b8.bin", B8.getData(), N * K, B8.getScales(), tiles_b);
    dump(dir + "/ra8.f32", RA8);
    dump(dir + "/ra4.f32", RA4);
    dump(dir + "/rb8.f32", RB8);
    dump(dir + "/c88.f32", C88);
    dump(dir + "/c48.f32", C48);
    printf("M=%llu N=%llu K=%llu done\n", (unsigned long long)M, (unsigned long long)N, (unsigned long long)K);
    return 0;
}
