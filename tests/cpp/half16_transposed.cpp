// half16_transposed.cpp -- the transposed half-precision methods through the headers (tests/test_f16_mvm_transposed_dropin.py), built in
// the tracked and the -DCLOVER_HIP_EXPLICIT_SYNC builds, with the default exactness (the reference's threshold) and with -DCLOVER_FAST.
//   half16_transposed <m> <n> <iterations> <K> <mu>
// On data of its own (a fixed generator), with one Phi (m x n) and PhiT = Phi.transpose(), it runs
//   mvm:    CloverMatrix16::mvm_transposed against PhiT.mvm, CloverVector16 and CloverVector32;
//   pair:   mvm_transposed_scaleAndAdd (both overloads) against PhiT.mvm_scaleAndAdd;
//   loop:   iht_loop_one_matrix against iht_loop with PhiT;
//   iht:    Q_IHT_one_matrix against Q_IHT with PhiT;
//   gd:     Q_GD_one_matrix against Q_GD with PhiT;
// and prints one digest (FNV-1a over the bits of every vector) per side: the two of a line are equal.
#include <CloverIHT.h>
#include <CloverMatrix16.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>

static uint64_t fnv(uint64_t h, const void *p, size_t n)
{
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001B3ull;
    return h;
}

static uint64_t digest(uint64_t h, const CloverVector16 &v) { return fnv(h, v.getData(), v.getBytes()); }
static uint64_t digest4(const CloverVector16 &a, const CloverVector16 &b, const CloverVector16 &c, const CloverVector16 &d)
{
    return digest(digest(digest(digest(0xCBF29CE484222325ull, a), b), c), d);
}

static float next_unit(uint64_t &s)          // (-1, 1), 24 bits
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((int64_t)(s >> 40) - (1 << 23)) / (float)(1 << 23);
}

static void fill(CloverVector16 &v, uint64_t &seed, float amp)
{
    CloverVector32 t(v.size());
    for (uint64_t i = 0; i < v.size(); i++) t.set(i, next_unit(seed) * amp);
    v.quantize(t);
}

static void line(const char *name, uint64_t one, uint64_t two)
{
    printf("%s one_matrix=%016llx two_matrices=%016llx\n", name, (unsigned long long)one, (unsigned long long)two);
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
    CloverMatrix16 Phi(m, n), PhiT(n, m);
    Phi.quantize(Phi32);
    Phi.transpose(PhiT);
    CloverVector16 y(m), v(m), u(n);
    fill(y, seed, 3.0f);
    fill(v, seed, 2.0f);
    fill(u, seed, 1.0f);

    {   // mvm: f16 vectors, then fp32 vectors
        CloverVector16 r1(n), r2(n);
        Phi.mvm_transposed(v, r1);
        PhiT.mvm(v, r2);
        CloverVector32 vf(m), f1(n), f2(n);
        for (uint64_t i = 0; i < m; i++) vf.set(i, next_unit(seed) * 2.0f);
        Phi.mvm_transposed(vf, f1);
        PhiT.mvm(vf, f2);
        line("mvm", fnv(digest(1, r1), f1.getData(), n * sizeof(float)), fnv(digest(1, r2), f2.getData(), n * sizeof(float)));
    }
    {   // pair: t = Phi' v, r = u - 0.75 t; then in place with 0.5
        CloverVector16 t1(n), r1(n), t2(n), r2(n), tc(n), td(n), u1(u), u2(u);
        Phi.mvm_transposed_scaleAndAdd(v, u, -0.75f, t1, r1);
        PhiT.mvm_scaleAndAdd(v, u, -0.75f, t2, r2);
        Phi.mvm_transposed_scaleAndAdd(v, u1, 0.5f, tc);
        PhiT.mvm_scaleAndAdd(v, u2, 0.5f, td);
        line("pair", digest4(t1, r1, tc, u1), digest4(t2, r2, td, u2));
    }
    {   // loop
        CloverVector16 x(n), t1(m), t2(m), t3(n), hx(n), h1(m), h2(m), h3(n);
        Phi.iht_loop_one_matrix(x, y, t1, t2, t3, iterations, K, mu, true);
        Phi.iht_loop(PhiT, hx, y, h1, h2, h3, iterations, K, mu, true);
        line("loop", digest4(x, t1, t2, t3), digest4(hx, h1, h2, h3));
    }
    uint64_t iht_digest = 0, nz = 0;
    {   // iht
        CloverVector16 x(n), t1(m), t2(m), t3(n), hx(n), h1(m), h2(m), h3(n);
        Q_IHT_one_matrix(Phi, x, y, t1, t2, t3, iterations, K, mu);
        Q_IHT(Phi, PhiT, hx, y, h1, h2, h3, iterations, K, mu);
        for (uint64_t i = 0; i < n; i++) nz += (x.getData()[i] & 0x7FFF) != 0;
        iht_digest = digest4(x, t1, t2, t3);
        line("iht", iht_digest, digest4(hx, h1, h2, h3));
    }
    {   // gd
        CloverVector16 x(n), t1(m), t2(m), t3(n), hx(n), h1(m), h2(m), h3(n);
        Q_GD_one_matrix(Phi, x, y, t1, t2, t3, iterations, mu);
        Q_GD(Phi, PhiT, hx, y, h1, h2, h3, iterations, mu);
        const uint64_t gd = digest4(x, t1, t2, t3);
        line("gd", gd, digest4(hx, h1, h2, h3));
        printf("gd_differs_from_iht=%d\n", gd != iht_digest);
    }
    printf("nonzero=%llu\ndone\n", (unsigned long long)nz);
    return 0;
}
