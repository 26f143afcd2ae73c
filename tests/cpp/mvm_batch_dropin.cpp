// mvm_batch_dropin.cpp -- the batch methods of the containers against their single-call partners (tests/test_mvm_batch_dropin.py), built with
// -DCLOVER_STOCHASTIC_ROUNDING_DISABLED in the tracked and the -DCLOVER_HIP_EXPLICIT_SYNC builds.
//   mvm_batch_dropin <dir> <m> <n> <count> <iterations> <K> <mu>
// reads <dir>/phi.f32 (m x n) and <dir>/ys.f32 (count x m); with Phi = quantize(phi), PhiT its transpose and y[j] = quantize(ys[j]) it checks on
// the host-visible bytes (values and scales) that
//   mvm_batch              == mvm per vector
//   mvm_scaleAndAdd_batch  == mvm_scaleAndAdd per vector (both overloads)
//   threshold_batch        == threshold per vector
//   Q_IHT_batch / Q_GD_batch == Q_IHT / Q_GD per vector (x, t1, t2, t3)
// prints <name>_equal=0|1 for each, kept_pointer=0|1 (host pointers taken with getData() BEFORE a batch call show its results after it in
// the tracked build; the explicit-sync build takes them again), and writes the restored x of the IHT run to <dir>/x<j>.f32.
#include <CloverIHT.h>
#include <CloverMatrix4.h>
#include <CloverVector4.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
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

static bool same4(const CloverVector4 &a, const CloverVector4 &b)
{
    return a.size_pad() == b.size_pad() && !memcmp(a.getData(), b.getData(), a.size_pad() / 2) &&
           !memcmp(a.getScales(), b.getScales(), a.size_pad() / 64 * sizeof(float));
}

typedef std::vector<std::unique_ptr<CloverVector4> > Vecs;

static Vecs make(uint64_t count, uint64_t n)
{
    Vecs v;
    for (uint64_t j = 0; j < count; j++) v.emplace_back(new CloverVector4(n));
    return v;
}
static std::vector<CloverVector4 *> ptrs(const Vecs &v)
{
    std::vector<CloverVector4 *> p;
    for (const auto &e : v) p.push_back(e.get());
    return p;
}
static std::vector<const CloverVector4 *> cptrs(const Vecs &v)
{
    std::vector<const CloverVector4 *> p;
    for (const auto &e : v) p.push_back(e.get());
    return p;
}
static bool all_same(const Vecs &a, const Vecs &b)
{
    bool ok = a.size() == b.size();
    for (size_t j = 0; ok && j < a.size(); j++) ok = same4(*a[j], *b[j]);
    return ok;
}

int main(int argc, char **argv)
{
    if (argc != 8) { fprintf(stderr, "usage: %s dir m n count iterations K mu\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    const uint64_t m = strtoull(argv[2], 0, 10), n = strtoull(argv[3], 0, 10), count = strtoull(argv[4], 0, 10),
                   iterations = strtoull(argv[5], 0, 10), K = strtoull(argv[6], 0, 10);
    const float mu = strtof(argv[7], 0);

    const std::vector<float> phi = read_f32(dir + "/phi.f32", m * n), ys = read_f32(dir + "/ys.f32", count * m);
    CloverMatrix32 Phi32(m, n);
    for (uint64_t i = 0; i < m; i++)
        for (uint64_t j = 0; j < n; j++) Phi32.set(i, j, phi[i * n + j]);
    CloverMatrix4 Phi(m, n), PhiT(n, m);
    Phi.quantize(Phi32);
    Phi.transpose(PhiT);
    Vecs y = make(count, m), xq = make(count, n);
    for (uint64_t j = 0; j < count; j++) {
        CloverVector32 y32(m), x32(n);
        for (uint64_t i = 0; i < m; i++) y32.set(i, ys[j * m + i]);
        for (uint64_t i = 0; i < n; i++) x32.set(i, phi[(2 * j % m) * n + i] - phi[((2 * j + 1) % m) * n + i]);
        y[j]->quantize(y32);
        xq[j]->quantize(x32);
    }
    bool kept = true;

    // mvm_batch against mvm
    {
        Vecs one = make(count, m), many = make(count, m);
        for (uint64_t j = 0; j < count; j++) Phi.mvm(*xq[j], *one[j]);
        const int8_t *p0 = many[0]->getData();
        const float *s0 = many[0]->getScales();
        const std::vector<const CloverVector4 *> px = cptrs(xq);
        const std::vector<CloverVector4 *> pr = ptrs(many);
        Phi.mvm_batch(px.data(), pr.data(), count);
#ifdef CLOVER_HIP_EXPLICIT_SYNC
        p0 = many[0]->getData();
        s0 = many[0]->getScales();
#endif
        kept = kept && !memcmp(p0, one[0]->getData(), m / 2) && !memcmp(s0, one[0]->getScales(), m / 64 * sizeof(float));
        printf("mvm_batch_equal=%d\n", (int)all_same(one, many));
    }
    // mvm_scaleAndAdd_batch against mvm_scaleAndAdd, out of place and in place
    {
        Vecs t1 = make(count, m), r1 = make(count, m), t2 = make(count, m), r2 = make(count, m);
        for (uint64_t j = 0; j < count; j++) Phi.mvm_scaleAndAdd(*xq[j], *y[j], -1.0f, *t1[j], *r1[j]);
        const int8_t *p0 = r2[count - 1]->getData();
        const std::vector<const CloverVector4 *> px = cptrs(xq), pu = cptrs(y);
        const std::vector<CloverVector4 *> pt = ptrs(t2), pr = ptrs(r2);
        Phi.mvm_scaleAndAdd_batch(px.data(), pu.data(), -1.0f, pt.data(), pr.data(), count);
#ifdef CLOVER_HIP_EXPLICIT_SYNC
        p0 = r2[count - 1]->getData();
#endif
        kept = kept && !memcmp(p0, r1[count - 1]->getData(), m / 2);
        printf("mvm_scaleAndAdd_batch_equal=%d\n", (int)(all_same(t1, t2) && all_same(r1, r2)));

        Vecs u1, u2, s1 = make(count, n), s2 = make(count, n);
        for (uint64_t j = 0; j < count; j++) { u1.emplace_back(new CloverVector4(*xq[j])); u2.emplace_back(new CloverVector4(*xq[j])); }
        for (uint64_t j = 0; j < count; j++) PhiT.mvm_scaleAndAdd(*r1[j], *u1[j], 0.37f, *s1[j]);
        const int8_t *pu0 = u2[0]->getData();
        const std::vector<const CloverVector4 *> pr1 = cptrs(r1);
        const std::vector<CloverVector4 *> pu2 = ptrs(u2), ps2 = ptrs(s2);
        PhiT.mvm_scaleAndAdd_batch(pr1.data(), pu2.data(), 0.37f, ps2.data(), count);
#ifdef CLOVER_HIP_EXPLICIT_SYNC
        pu0 = u2[0]->getData();
#endif
        kept = kept && !memcmp(pu0, u1[0]->getData(), n / 2);
        printf("mvm_scaleAndAdd_batch_in_place_equal=%d\n", (int)(all_same(u1, u2) && all_same(s1, s2) && !same4(*u1[0], *xq[0])));
    }
    // threshold_batch against threshold
    {
        Vecs a, b;
        for (uint64_t j = 0; j < count; j++) { a.emplace_back(new CloverVector4(*xq[j])); b.emplace_back(new CloverVector4(*xq[j])); }
        for (uint64_t j = 0; j < count; j++) a[j]->threshold(K);
        const int8_t *p0 = b[0]->getData();
        const std::vector<CloverVector4 *> pb = ptrs(b);
        CloverVector4::threshold_batch(pb.data(), count, K);
#ifdef CLOVER_HIP_EXPLICIT_SYNC
        p0 = b[0]->getData();
#endif
        kept = kept && !memcmp(p0, a[0]->getData(), n / 2);
        printf("threshold_batch_equal=%d\n", (int)(all_same(a, b) && !same4(*a[0], *xq[0])));
    }
    // Q_IHT_batch / Q_GD_batch against Q_IHT / Q_GD per vector
    for (int gd = 0; gd < 2; gd++) {
        Vecs x1 = make(count, n), a1 = make(count, m), b1 = make(count, m), c1 = make(count, n);
        Vecs x2 = make(count, n), a2 = make(count, m), b2 = make(count, m), c2 = make(count, n);
        for (uint64_t j = 0; j < count; j++) {
            if (gd) Q_GD(Phi, PhiT, *x1[j], *y[j], *a1[j], *b1[j], *c1[j], iterations, mu);
            else Q_IHT(Phi, PhiT, *x1[j], *y[j], *a1[j], *b1[j], *c1[j], iterations, K, mu);
        }
        const int8_t *p0 = x2[0]->getData();
        const std::vector<CloverVector4 *> px = ptrs(x2), py = ptrs(y), pa = ptrs(a2), pb = ptrs(b2), pc = ptrs(c2);
        if (gd) Q_GD_batch(Phi, PhiT, px.data(), py.data(), pa.data(), pb.data(), pc.data(), count, iterations, mu);
        else Q_IHT_batch(Phi, PhiT, px.data(), py.data(), pa.data(), pb.data(), pc.data(), count, iterations, K, mu);
#ifdef CLOVER_HIP_EXPLICIT_SYNC
        p0 = x2[0]->getData();
#endif
        kept = kept && !memcmp(p0, x1[0]->getData(), n / 2);
        printf("%s_equal=%d\n", gd ? "Q_GD_batch" : "Q_IHT_batch", (int)(all_same(x1, x2) && all_same(a1, a2) && all_same(b1, b2) && all_same(c1, c2)));
        if (!gd)
            for (uint64_t j = 0; j < count; j++) {
                CloverVector32 back(n);
                x2[j]->restore(back);
                write_bytes(dir + "/x" + std::to_string(j) + ".f32", back.getData(), n * sizeof(float));
            }
    }
    printf("kept_pointer=%d\ndone\n", (int)kept);
    return 0;
}
