// m8_mvm_transposed_dropin.cpp -- the one-matrix methods of CloverMatrix8 against their stored-transpose partners
// (tests/test_m8_mvm_transposed_dropin.py), built with -DCLOVER_STOCHASTIC_ROUNDING_DISABLED in the tracked and the
// -DCLOVER_HIP_EXPLICIT_SYNC builds, and without it (stochastic rounding, the reference's default).
//   m8_mvm_transposed_dropin <dir> <m> <n> <iterations> <K> <mu>
// reads <dir>/phi.f32 (m x n) and <dir>/y.f32 (m); with Phi = quantize(phi), PhiT its transpose and y = quantize8(y) it checks on the
// host-visible bytes (values and scales) that
//   Phi.mvm_transposed               == PhiT.mvm
//   Phi.mvm_transposed_scaleAndAdd   == PhiT.mvm_scaleAndAdd (both overloads)
//   Q_IHT_one_matrix / Q_GD_one_matrix == Q_IHT / Q_GD (x, t1, t2, t3)
// With stochastic rounding every object draws from its own generator, so either side of a comparison starts from the same keys (seed());
// the gradient step of the one-matrix loop draws from Phi's generator where the two-matrix loop draws from PhiT's, so there the loops are
// compared with the same steps composed from method calls: mvm, scaleAndAdd, mvm_transposed, scaleAndAdd, threshold.
// prints <name>_equal=0|1 for each and kept_pointer=0|1 (host pointers taken with getData() BEFORE a call show its results after it in the
// tracked build; the explicit-sync build takes them again).
#include <CloverIHT.h>
#include <CloverMatrix8.h>
#include <CloverVector8.h>

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

static bool same8(const CloverVector8 &a, const CloverVector8 &b)
{
    return a.size_pad() == b.size_pad() && !memcmp(a.getData(), b.getData(), a.size_pad()) &&
           !memcmp(a.getScales(), b.getScales(), a.size_pad() / 64 * sizeof(float));
}

static bool any_nonzero(const CloverVector8 &a)
{
    const int8_t *p = a.getData();
    for (uint64_t i = 0; i < a.size_pad(); i++)
        if (p[i]) return true;
    return false;
}

// the same keys for both matrices and for every vector that draws: either side of a comparison walks the same streams
static void seed(CloverMatrix8 &Phi, CloverMatrix8 &PhiT, CloverVector8 &a, CloverVector8 &b)
{
    Phi.seedRandomKeys(11, 12);
    PhiT.seedRandomKeys(11, 12);
    a.seedRandomKeys(21, 22);
    b.seedRandomKeys(31, 32);
}

int main(int argc, char **argv)
{
    if (argc != 7) { fprintf(stderr, "usage: %s dir m n iterations K mu\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    const uint64_t m = strtoull(argv[2], 0, 10), n = strtoull(argv[3], 0, 10), iterations = strtoull(argv[4], 0, 10), K = strtoull(argv[5], 0, 10);
    const float mu = strtof(argv[6], 0);

    const std::vector<float> phi = read_f32(dir + "/phi.f32", m * n), ys = read_f32(dir + "/y.f32", m);
    CloverMatrix32 Phi32(m, n);
    for (uint64_t i = 0; i < m; i++)
        for (uint64_t j = 0; j < n; j++) Phi32.set(i, j, phi[i * n + j]);
    CloverMatrix8 Phi(m, n), PhiT(n, m);
    Phi.seedRandomKeys(1, 2);
    Phi.quantize(Phi32);
    Phi.transpose(PhiT);
    CloverVector8 y(m), u(n);
    {
        CloverVector32 y32(m), u32(n);
        for (uint64_t i = 0; i < m; i++) y32.set(i, ys[i]);
        for (uint64_t i = 0; i < n; i++) u32.set(i, phi[i] - phi[n + i]);
        y.seedRandomKeys(3, 4);
        u.seedRandomKeys(5, 6);
        y.quantize(y32);
        u.quantize(u32);
    }
    bool kept = true;

    // mvm_transposed against transpose + mvm
    {
        CloverVector8 one(n), two(n);
        seed(Phi, PhiT, y, u);
        PhiT.mvm(y, one);
        const int8_t *p0 = two.getData();
        const float *s0 = two.getScales();
        Phi.mvm_transposed(y, two);
#ifdef CLOVER_HIP_EXPLICIT_SYNC
        p0 = two.getData();
        s0 = two.getScales();
#endif
        kept = kept && !memcmp(p0, one.getData(), n) && !memcmp(s0, one.getScales(), n / 64 * sizeof(float));
        printf("mvm_transposed_equal=%d\n", (int)(same8(one, two) && any_nonzero(one)));
    }
    // mvm_transposed_scaleAndAdd against mvm_scaleAndAdd on the stored transpose, out of place and in place
    {
        CloverVector8 t1(n), r1(n), t2(n), r2(n);
        seed(Phi, PhiT, y, u);
        PhiT.mvm_scaleAndAdd(y, u, 0.37f, t1, r1);
        const int8_t *p0 = r2.getData();
        seed(Phi, PhiT, y, u);
        Phi.mvm_transposed_scaleAndAdd(y, u, 0.37f, t2, r2);
#ifdef CLOVER_HIP_EXPLICIT_SYNC
        p0 = r2.getData();
#endif
        kept = kept && !memcmp(p0, r1.getData(), n);
        printf("mvm_transposed_scaleAndAdd_equal=%d\n", (int)(same8(t1, t2) && same8(r1, r2) && !same8(r1, u)));

        CloverVector8 u1(u), u2(u), s1(n), s2(n);
        seed(Phi, PhiT, u1, u2);
        u2.seedRandomKeys(21, 22);
        PhiT.mvm_scaleAndAdd(y, u1, 0.37f, s1);
        const int8_t *pu = u2.getData();
        Phi.mvm_transposed_scaleAndAdd(y, u2, 0.37f, s2);
#ifdef CLOVER_HIP_EXPLICIT_SYNC
        pu = u2.getData();
#endif
        kept = kept && !memcmp(pu, u1.getData(), n);
        printf("mvm_transposed_scaleAndAdd_in_place_equal=%d\n", (int)(same8(u1, u2) && same8(s1, s2) && !same8(u1, u)));
    }
    // Q_IHT_one_matrix / Q_GD_one_matrix against Q_IHT / Q_GD (stochastic: against the steps composed from method calls)
    for (int gd = 0; gd < 2; gd++) {
        CloverVector8 x1(n), a1(m), b1(m), c1(n), x2(n), a2(m), b2(m), c2(n), y1(y), y2(y);
        seed(Phi, PhiT, x1, y1);
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
        if (gd) Q_GD(Phi, PhiT, x1, y1, a1, b1, c1, iterations, mu);
        else Q_IHT(Phi, PhiT, x1, y1, a1, b1, c1, iterations, K, mu);
#else
        x1.clear();
        for (uint64_t i = 0; i < iterations; i++) {
            Phi.mvm(x1, a1);
            y1.scaleAndAdd(a1, -1.0f, b1);
            Phi.mvm_transposed(b1, c1);
            x1.scaleAndAdd(c1, mu);
            if (!gd) x1.threshold_parallel(K);
        }
#endif
        const int8_t *p0 = x2.getData();
        seed(Phi, PhiT, x2, y2);
        if (gd) Q_GD_one_matrix(Phi, x2, y2, a2, b2, c2, iterations, mu);
        else Q_IHT_one_matrix(Phi, x2, y2, a2, b2, c2, iterations, K, mu);
#ifdef CLOVER_HIP_EXPLICIT_SYNC
        p0 = x2.getData();
#endif
        kept = kept && !memcmp(p0, x1.getData(), n);
        printf("%s_equal=%d\n", gd ? "Q_GD_one_matrix" : "Q_IHT_one_matrix",
               (int)(same8(x1, x2) && same8(a1, a2) && same8(b1, b2) && same8(c1, c2) && any_nonzero(x1)));
    }
    printf("kept_pointer=%d\ndone\n", (int)kept);
    return 0;
}
