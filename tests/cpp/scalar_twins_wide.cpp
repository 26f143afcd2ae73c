// scalar_twins_wide.cpp -- the host `_scalar` methods of CloverMatrix8, CloverMatrix16 and CloverVector16 on inputs read from files, their
// results written to files: tests/test_validate_grid_wide.py compares them with the restatements the GPU tests check the kernels against
// (tests/matrix8_restate.c, tests/half16_restate.c).  Only host methods are called, so the program links with tests/cpp/fake_clv.c and
// needs no device.
//   scalar_twins_wide m8  <dir> <rows> <cols>   A.f32 (rows x cols), x.f32 (cols)   -> q.bin (values, scales), r.f32 (restore_scalar),
//                                                                                      t.bin (transpose_scalar), f.f32 (mvm_scalar, fp32 vector)
//   scalar_twins_wide m16 <dir> <rows> <cols>   A.f32, x.f32                        -> q.bin, t.bin, xq.bin, r.bin (mvm_scalar, f16 vector), f.f32
//   scalar_twins_wide v16 <dir> <n> <a>         x.f32 (n), u.bin, v.bin (n_pad binary16 patterns each)
//                                               -> q.bin, r.f32, s3.bin (u.scaleAndAdd_scalar(v, a, result)), s2.bin (in place); prints dot=<hex>
// Not here: CloverMatrix8::mvm_scalar with a CloverVector8.  The reference defines it through CloverVector8::dot on row views
// (CloverMatrix8.h:480-548), and so does the header: it runs on the device and is compared in the GPU part of the same test file.
// CloverVector16 has no host form of threshold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "CloverMatrix16.h"
#include "CloverMatrix8.h"
#include "CloverVector16.h"

template <class T>
static std::vector<T> read_file(const std::string &path, size_t n)
{
    std::vector<T> v(n);
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f || std::fread(v.data(), sizeof(T), n, f) != n) { std::fprintf(stderr, "cannot read %s\n", path.c_str()); std::exit(2); }
    std::fclose(f);
    return v;
}

static void write_file(const std::string &path, const void *a, size_t na, const void *b = nullptr, size_t nb = 0)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(a, 1, na, f) != na || (nb && std::fwrite(b, 1, nb, f) != nb)) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); std::exit(2); }
    std::fclose(f);
}

static void load(CloverMatrix32 &A, CloverVector32 &x, const std::string &dir, uint64_t rows, uint64_t cols)
{
    const std::vector<float> a = read_file<float>(dir + "/A.f32", rows * cols), xv = read_file<float>(dir + "/x.f32", cols);
    std::memcpy(A.getData(), a.data(), rows * cols * sizeof(float));
    std::memcpy(x.getData(), xv.data(), cols * sizeof(float));
}

static int m8(const std::string &dir, uint64_t rows, uint64_t cols)
{
    CloverMatrix32 A(rows, cols), R(rows, cols);
    CloverVector32 x(cols), f(rows);
    load(A, x, dir, rows, cols);
    CloverMatrix8 q(rows, cols), t(cols, rows);
    q.quantize_scalar(A);
    q.restore_scalar(R);
    q.transpose_scalar(t);
    q.mvm_scalar(x, f);
    const uint64_t tiles = (rows / 64) * (cols / 64) * sizeof(float);
    write_file(dir + "/q.bin", q.getData(), rows * cols, q.getScales(), tiles);
    write_file(dir + "/r.f32", R.getData(), rows * cols * sizeof(float));
    write_file(dir + "/t.bin", t.getData(), rows * cols, t.getScales(), tiles);
    write_file(dir + "/f.f32", f.getData(), rows * sizeof(float));
    return 0;
}

static int m16(const std::string &dir, uint64_t rows, uint64_t cols)
{
    CloverMatrix32 A(rows, cols);
    CloverVector32 x(cols), f(rows);
    load(A, x, dir, rows, cols);
    CloverMatrix16 q(rows, cols), t(cols, rows);
    CloverVector16 xq(cols), r(rows);
    q.quantize_scalar(A);
    q.transpose_scalar(t);
    xq.quantize_scalar(x);
    q.mvm_scalar(xq, r);
    q.mvm_scalar(x, f);
    write_file(dir + "/q.bin", q.getData(), q.getBytes());
    write_file(dir + "/t.bin", t.getData(), t.getBytes());
    write_file(dir + "/xq.bin", xq.getData(), xq.getBytes());
    write_file(dir + "/r.bin", r.getData(), r.getBytes());
    write_file(dir + "/f.f32", f.getData(), rows * sizeof(float));
    return 0;
}

static int v16(const std::string &dir, uint64_t n, float a)
{
    CloverVector32 x(n), R(n);
    const uint64_t n_pad = x.size_pad();
    const std::vector<float> xv = read_file<float>(dir + "/x.f32", n);
    const std::vector<uint16_t> ub = read_file<uint16_t>(dir + "/u.bin", n_pad), vb = read_file<uint16_t>(dir + "/v.bin", n_pad);
    std::memcpy(x.getData(), xv.data(), n * sizeof(float));
    CloverVector16 q(n), u(n), v(n), s3(n);
    std::memcpy(u.getData(), ub.data(), n_pad * sizeof(uint16_t));
    std::memcpy(v.getData(), vb.data(), n_pad * sizeof(uint16_t));
    q.quantize_scalar(x);
    q.restore_scalar(R);
    u.scaleAndAdd_scalar(v, a, s3);
    const float d = u.dot_scalar(v);
    CloverVector16 s2(u);
    s2.scaleAndAdd_scalar(v, a);
    write_file(dir + "/q.bin", q.getData(), q.getBytes());
    write_file(dir + "/r.f32", R.getData(), n_pad * sizeof(float));
    write_file(dir + "/s3.bin", s3.getData(), s3.getBytes());
    write_file(dir + "/s2.bin", s2.getData(), s2.getBytes());
    uint32_t db;
    std::memcpy(&db, &d, 4);
    std::printf("dot=%08x\n", db);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 5) {
        const std::string what = argv[1], dir = argv[2];
        int rc = 2;
        if (what == "m8") rc = m8(dir, std::strtoull(argv[3], 0, 10), std::strtoull(argv[4], 0, 10));
        else if (what == "m16") rc = m16(dir, std::strtoull(argv[3], 0, 10), std::strtoull(argv[4], 0, 10));
        else if (what == "v16") rc = v16(dir, std::strtoull(argv[3], 0, 10), std::strtof(argv[4], 0));
        if (rc == 0) std::printf("scalar twins wide done\n");
        if (rc != 2) return rc;
    }
    std::fprintf(stderr, "usage: %s m8|m16 dir rows cols | v16 dir n a\n", argv[0]);
    return 2;
}
