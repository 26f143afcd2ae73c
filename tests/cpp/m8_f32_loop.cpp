// m8_f32_loop.cpp -- CloverMatrix8 on CloverVector32 vectors through the headers (tests/test_m8_f32_dropin.py), built with
// -DCLOVER_FP32_ON_DEVICE, with the default exactness (the reference's threshold) and with -DCLOVER_FAST.
//   m8_f32_loop <m> <n> <iterations> <K> <mu>
// On data of its own (a fixed generator), with one Phi (m x n) and PhiT = Phi.transpose_parallel(), it runs
//   mvm:    CloverMatrix8::mvm_transposed against PhiT.mvm;
//   pair:   mvm_scaleAndAdd (both overloads) against mvm + scaleAndAdd, mvm_transposed_scaleAndAdd against PhiT.mvm_scaleAndAdd;
//   iht:    the Q_IHT overload against the five method calls written out on the same containers;
//   gd:     the Q_GD overload against the four method calls;
//   iht1:   Q_IHT_one_matrix against Q_IHT with PhiT;
//   gd1:    Q_GD_one_matrix against Q_GD with PhiT;
// and prints one digest (FNV-1a over the bits of every vector) per side: the two of a line are equal.
#include <CloverIHT.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>

static uint64_t fnv(uint64_t h, const void *p, size_t n)
{
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001B3ull;
    return h;
}

static uint64_t digest(uint64_t h, const CloverVector32 &v) { return fnv(h, v.getData(), v.size_pad() * sizeof(float)); }
static uint64_t digest4(const CloverVector32 &a, const CloverVector32 &b, const CloverVector32 &c, const CloverVector32 &d)
{
    return digest(digest(digest(digest(0xCBF29CE484222325ull, a), b), c), d);
}

static float next_unit(uint64_t &s)          // (-1, 1), 24 bits
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((int64_t)(s >> 40) - (1 << 23)) / (float)(1 << 23);
}

static void fill(CloverVector32 &v, uint64_t &seed, float amp)
{
    for (uint64_t i = 0; i < v.size(); i++) v.set(i, next_unit(seed) * amp);
}

static void line(const char *name, uint64_t fused, uint64_t written_out)
{
    printf("%s fused=%016llx written_out=%016llx\n", name, (unsigned long long)fused, (unsigned long long)written_out);
}

// the generic templates' bodies (01_measure.h:923-946, 999-1021), written out
static void loop_written_out(CloverMatrix8 &Phi, CloverMatrix8 &PhiT, CloverVector32 &x, CloverVector32 &y, CloverVector32 &t1, CloverVector32 &t2,
                             CloverVector32 &t3, uint64_t iterations, uint64_t K, float mu, bool threshold)
{
    x.clear();
    for (uint64_t i = 0; i < iterations; i++) {
        Phi.mvm_parallel(x, t1);
        y.scaleAndAdd_parallel(t1, -1, t2);
        PhiT.mvm_parallel(t2, t3);
        x.scaleAndAdd_parallel(t3, mu);
        if (threshold) x.threshold_parallel(K);
    }
}

int main(int argc, char **argv)
{
    if (argc != 6) { fprintf(stderr, "usage: %s m n iterations K mu\n", argv[0]); return 2; }
    const uint64_t m = strtoull(argv[1], 0, 10), n = strtoull(argv[2], 0, 10), iterations = strtoull(argv[3], 0, 10), K = strtoull(argv[4], 0, 10);
    const float mu = strtof(argv[5], 0);

    uint64_t seed = 2026;
    const float scale = 1.0f / sqrtf((float)m);                      // Phi entries ~ U(-1, 1) / sqrt(m): the iterates stay finite at mu = 0.5
    CloverMatrix32 Phi32(m, n);
    for (uint64_t i = 0; i < m; i++)
        for (uint64_t j = 0; j < n; j++) Phi32.set(i, j, next_unit(seed) * scale);
    CloverMatrix8 Phi(m, n), PhiT(n, m);
    Phi.quantize(Phi32);
    Phi.transpose_parallel(PhiT);
    CloverVector32 y(m), v(m), w(n), u(n), um(m);
    fill(y, seed, 3.0f);
    fill(v, seed, 2.0f);
    fill(w, seed, 2.0f);
    fill(u, seed, 1.0f);
    fill(um, seed, 1.0f);

    {   // mvm
        CloverVector32 r1(n), r2(n), r3(n);
        Phi.mvm_transposed(v, r1);
        Phi.mvm_transposed_parallel(v, r3);
        PhiT.mvm(v, r2);
        line("mvm", digest(digest(1, r1), r3), digest(digest(1, r2), r2));
    }
    {   // pair: row-major (t = Phi w, r = um - 0.75 t; then in place with 0.5) and transposed (t = Phi' v, r = u - 0.75 t; in place)
        CloverVector32 t1(m), r1(m), t2(m), r2(m), tc(m), td(m), u1(um), u2(um);
        Phi.mvm_scaleAndAdd(w, um, -0.75f, t1, r1);
        Phi.mvm(w, t2);
        um.scaleAndAdd(t2, -0.75f, r2);
        Phi.mvm_scaleAndAdd(w, u1, 0.5f, tc);
        Phi.mvm(w, td);
        u2.scaleAndAdd(td, 0.5f);
        CloverVector32 a1(n), b1(n), a2(n), b2(n), ac(n), ad(n), v1(u), v2(u);
        Phi.mvm_transposed_scaleAndAdd(v, u, -0.75f, a1, b1);
        PhiT.mvm_scaleAndAdd(v, u, -0.75f, a2, b2);
        Phi.mvm_transposed_scaleAndAdd(v, v1, 0.5f, ac);
        PhiT.mvm_scaleAndAdd(v, v2, 0.5f, ad);
        line("pair", digest4(t1, r1, tc, u1) ^ digest4(a1, b1, ac, v1), digest4(t2, r2, td, u2) ^ digest4(a2, b2, ad, v2));
    }
    uint64_t iht_digest = 0, nz = 0;
    {   // iht
        CloverVector32 x(n), t1(m), t2(m), t3(n), hx(n), h1(m), h2(m), h3(n);
        Q_IHT(Phi, PhiT, x, y, t1, t2, t3, iterations, K, mu);
        loop_written_out(Phi, PhiT, hx, y, h1, h2, h3, iterations, K, mu, true);
        for (uint64_t i = 0; i < n; i++) nz += x.get(i) != 0.0f;
        iht_digest = digest4(x, t1, t2, t3);
        line("iht", iht_digest, digest4(hx, h1, h2, h3));
        CloverVector32 ox(n), o1(m), o2(m), o3(n);
        Q_IHT_one_matrix(Phi, ox, y, o1, o2, o3, iterations, K, mu);
        line("iht1", digest4(ox, o1, o2, o3), iht_digest);
    }
    {   // gd
        CloverVector32 x(n), t1(m), t2(m), t3(n), hx(n), h1(m), h2(m), h3(n);
        Q_GD(Phi, PhiT, x, y, t1, t2, t3, iterations, mu);
        loop_written_out(Phi, PhiT, hx, y, h1, h2, h3, iterations, 0, mu, false);
        const uint64_t gd = digest4(x, t1, t2, t3);
        line("gd", gd, digest4(hx, h1, h2, h3));
        CloverVector32 ox(n), o1(m), o2(m), o3(n);
        Q_GD_one_matrix(Phi, ox, y, o1, o2, o3, iterations, mu);
        line("gd1", digest4(ox, o1, o2, o3), gd);
        printf("gd_differs_from_iht=%d\n", gd != iht_digest);
    }
    printf("nonzero=%llu\ndone\n", (unsigned long long)nz);
    return 0;
}
