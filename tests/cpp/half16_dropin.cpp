// half16_dropin.cpp -- a client of include/CloverVector16.h / CloverMatrix16.h written with the reference's method names
// (tests/test_half16_dropin.py).
//   half16_dropin <dir> <iht|gd> <m> <n> <iterations> <K> <mu>
// reads <dir>/phi.f32 (m x n) and <dir>/y.f32 (m); checks mvm == mvm_parallel for both vector types and that the non-owning view
// constructor writes through; writes the f16 and scalar forms of mvm / dot for the caller to compare; runs
// Q_IHT<CloverMatrix16, CloverVector16> or Q_GD<...> through the generic templates of CloverIHT.h and writes Phi, PhiT, y, x, t1, t2, t3
// (raw uint16) to <dir>/<name>.bin.
#include <CloverIHT.h>
#include <CloverMatrix16.h>
#include <CloverVector16.h>

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

static void write_bytes(const std::string &path, const void *a, size_t na)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(a, 1, na, f) != na) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(2); }
    fclose(f);
}

static void dump(const std::string &dir, const char *name, const CloverVector16 &v) { write_bytes(dir + "/" + name + ".bin", v.getData(), v.getBytes()); }
static void dump(const std::string &dir, const char *name, const CloverMatrix16 &A) { write_bytes(dir + "/" + name + ".bin", A.getData(), A.getBytes()); }
static bool same16(const CloverVector16 &a, const CloverVector16 &b) { return !memcmp(a.getData(), b.getData(), a.getBytes()); }
static unsigned bits_of(float f) { unsigned u; memcpy(&u, &f, 4); return u; }

int main(int argc, char **argv)
{
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

    CloverMatrix16 Phi(m, n), PhiT(n, m);
    Phi.quantize(Phi32);
    Phi.transpose(PhiT);
    CloverVector16 y(y32), xq(x32);
    if (Phi.getBitsLength() != 16 || xq.getBitsLength() != 16 || xq.getBytes() != 2 * xq.size_pad()) return 3;

    // mvm == mvm_parallel (f16 and fp32 vectors); the scalar forms go to the caller
    CloverVector16 r1(m), r2(m), r3(m);
    Phi.mvm(xq, r1);
    Phi.mvm_parallel(xq, r2);
    Phi.mvm_scalar(xq, r3);
    CloverVector32 f1(m), f2(m), f3(m);
    Phi.mvm(x32, f1);
    Phi.mvm_parallel(x32, f2);
    Phi.mvm_scalar(x32, f3);
    printf("mvm_equal=%d mvm_f32_equal=%d\n", (int)same16(r1, r2), (int)!memcmp(f1.getData(), f2.getData(), m * sizeof(float)));
    dump(dir, "xq", xq);
    dump(dir, "r1", r1);
    dump(dir, "r3_scalar", r3);
    write_bytes(dir + "/f1.f32", f1.getData(), m * sizeof(float));
    write_bytes(dir + "/f3_scalar.f32", f3.getData(), m * sizeof(float));
    CloverVector16 col0(y32);                       // a second vector of m elements for the dots
    printf("dot=%08x dot_parallel=%08x dot_scalar=%08x\n", bits_of(r1.dot(col0)), bits_of(r1.dot_parallel(col0)), bits_of(r1.dot_scalar(col0)));

    // element accessors and the scalar twins of the vector methods
    CloverVector16 s1(n), s2(n), s3(n);
    s1.quantize_scalar(x32);
    xq.scaleAndAdd(s1, 0.37f, s2);
    xq.scaleAndAdd_scalar(s1, 0.37f, s3);
    CloverVector32 back(n), back2(n);
    xq.restore(back);
    xq.restore_scalar(back2);
    bool acc_ok = same16(s1, xq) && same16(s2, s3) && !memcmp(back.getData(), back2.getData(), n * sizeof(float));
    for (uint64_t j = 0; j < n && j < 300; j++) {
        acc_ok = acc_ok && bits_of(xq.get(j)) == bits_of(back.get(j)) && xq.getAbs(j) == (back.get(j) < 0 ? -back.get(j) : back.get(j));
        s3.set(j, x32.get(j));
        acc_ok = acc_ok && s3.getBits(j) == xq.getBits(j);
    }
    CloverMatrix16 Ps(m, n), PTs(n, m);
    Ps.quantize_scalar(Phi32);
    Ps.transpose_scalar(PTs);
    acc_ok = acc_ok && !memcmp(Ps.getData(), Phi.getData(), Phi.getBytes()) && !memcmp(PTs.getData(), PhiT.getData(), PhiT.getBytes());
    acc_ok = acc_ok && bits_of(Phi.get(1, 2)) == bits_of(clover_hip::half::to_f32(Phi.getData()[Phi.getCols() + 2]));
    printf("scalar_twins_equal=%d\n", (int)acc_ok);

    // the non-owning view writes through to the caller's memory
    std::vector<uint16_t> mine(xq.size_pad(), 0xFFFF);
    {
        CloverVector16 view(n, mine.data());
        view.quantize(x32);
        view.scaleAndAdd(xq, 1.0f);                 // 2 x, in place, on the device
        view.toHost();
    }
    CloverVector16 twice(n);
    xq.scaleAndAdd(xq, 1.0f, twice);
    printf("view_writes_through=%d\n", (int)!memcmp(mine.data(), twice.getData(), twice.getBytes()));

    // threshold_min_heap with the caller's heap
    {
        CloverVector16 h(xq);
        std::vector<CloverVector16::idx_t> heap(K ? K : 1);
        h.threshold_min_heap(heap.data(), K ? K : 1);
        std::vector<uint32_t> out;
        for (size_t i = 0; i < heap.size(); i++) { out.push_back(bits_of(heap[i].value)); out.push_back((uint32_t)heap[i].idx); out.push_back((uint32_t)heap[i].bits.i); }
        write_bytes(dir + "/heap.bin", out.data(), out.size() * 4);
        dump(dir, "thr", h);
    }

    CloverVector16 x(n), t1(m), t2(m), t3(n);
    if (mode == "iht") Q_IHT<CloverMatrix16, CloverVector16>(Phi, PhiT, x, y, t1, t2, t3, iterations, K, mu);
    else Q_GD<CloverMatrix16, CloverVector16>(Phi, PhiT, x, y, t1, t2, t3, iterations, mu);
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
