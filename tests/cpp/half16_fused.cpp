// half16_fused.cpp -- the fused half-precision loop machinery through the headers (tests/test_half16_fused.py), built in the tracked and
// the -DCLOVER_HIP_EXPLICIT_SYNC builds, with the default exactness (the reference's threshold) and with -DCLOVER_FAST.
//   half16_fused <m> <n> <iterations> <K> <mu>
// On data of its own (a fixed generator) it runs
//   pair:  CloverMatrix16::mvm_scaleAndAdd (both overloads) against mvm + scaleAndAdd;
//   iht:   Q_IHT<CloverMatrix16, CloverVector16> (the specialisation of CloverIHT.h, template arguments spelled out) against the five
//          method calls written out by hand;
//   gd:    Q_GD(Phi, PhiT, ...) (template arguments deduced) against the four method calls;
// and prints one digest (FNV-1a over the bits of x, t1, t2, t3) per side: the two lines of a pair are equal.
// kept_pointer: a host pointer taken from x.getData() before the specialised loop shows the loop's result after it (tracked build; the
// explicit-sync build re-takes the pointer, which is that build's rule).
#include <CloverIHT.h>
#include <CloverMatrix16.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static uint64_t fnv(uint64_t h, const void *p, size_t n)
{
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001B3ull;
    return h;
}

static uint64_t digest(const CloverVector16 &x, const CloverVector16 &t1, const CloverVector16 &t2, const CloverVector16 &t3)
{
    uint64_t h = 0xCBF29CE484222325ull;
    const CloverVector16 *v[4] = {&x, &t1, &t2, &t3};
    for (int i = 0; i < 4; i++) h = fnv(h, v[i]->getData(), v[i]->getBytes());
    return h;
}

static float next_unit(uint64_t &s)          // (-1, 1), 24 bits
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((int64_t)(s >> 40) - (1 << 23)) / (float)(1 << 23);
}

int main(int argc, char **argv)
{
    if (argc != 6) { fprintf(stderr, "usage: %s m n iterations K mu\n", argv[0]); return 2; }
    const uint64_t m = strtoull(argv[1], 0, 10), n = strtoull(argv[2], 0, 10), iterations = strtoull(argv[3], 0, 10), K = strtoull(argv[4], 0, 10);
    const float mu = strtof(argv[5], 0);

    uint64_t seed = 2024;
    const float scale = 1.0f / sqrtf((float)m);                      // Phi entries ~ U(-1, 1) / sqrt(m): the iterates stay finite at mu = 0.5
    CloverMatrix32 Phi32(m, n);
    for (uint64_t i = 0; i < m; i++)
        for (uint64_t j = 0; j < n; j++) Phi32.set(i, j, next_unit(seed) * scale);
    CloverVector32 y32(m), u32(m), x32(n);
    for (uint64_t i = 0; i < m; i++) { y32.set(i, next_unit(seed) * 3.0f); u32.set(i, next_unit(seed)); }
    for (uint64_t j = 0; j < n; j++) x32.set(j, next_unit(seed) * 2.0f);
    CloverMatrix16 Phi(m, n), PhiT(n, m);
    Phi.quantize(Phi32);
    Phi.transpose(PhiT);
    CloverVector16 y(y32), xq(x32);

    {   // pair: t = Phi xq, r = u - 0.75 t; then in place
        CloverVector16 u(u32), ta(m), ra(m), tb(m), rb(m);
        Phi.mvm_scaleAndAdd(xq, u, -0.75f, ta, ra);
        Phi.mvm(xq, tb);
        u.scaleAndAdd(tb, -0.75f, rb);
        CloverVector16 ua(u32), ub(u32), tc(m), td(m);
        Phi.mvm_scaleAndAdd(xq, ua, 0.5f, tc);
        Phi.mvm(xq, td);
        ub.scaleAndAdd(td, 0.5f);
        printf("pair fused=%016llx separate=%016llx\n", (unsigned long long)digest(ta, ra, tc, ua), (unsigned long long)digest(tb, rb, td, ub));
    }

    int kept = 1;
    {
        CloverVector16 x(n), t1(m), t2(m), t3(n);
        const uint16_t *px = x.getData();
        Q_IHT<CloverMatrix16, CloverVector16>(Phi, PhiT, x, y, t1, t2, t3, iterations, K, mu);
#ifdef CLOVER_HIP_EXPLICIT_SYNC
        px = x.getData();
#endif
        CloverVector16 hx(n), h1(m), h2(m), h3(n);
        hx.clear();
        for (uint64_t it = 0; it < iterations; it++) {
            Phi.mvm_parallel(hx, h1);
            y.scaleAndAdd_parallel(h1, -1.0f, h2);
            PhiT.mvm_parallel(h2, h3);
            hx.scaleAndAdd_parallel(h3, mu);
            hx.threshold_parallel(K);
        }
        kept = !memcmp(px, hx.getData(), n * sizeof(uint16_t));
        uint64_t nz = 0;
        for (uint64_t j = 0; j < n; j++) nz += (px[j] & 0x7FFF) != 0;
        printf("iht spec=%016llx hand=%016llx nonzero=%llu\n", (unsigned long long)digest(x, t1, t2, t3), (unsigned long long)digest(hx, h1, h2, h3),
               (unsigned long long)nz);
    }
    {
        CloverVector16 x(n), t1(m), t2(m), t3(n);
        Q_GD(Phi, PhiT, x, y, t1, t2, t3, iterations, mu);
        CloverVector16 hx(n), h1(m), h2(m), h3(n);
        hx.clear();
        for (uint64_t it = 0; it < iterations; it++) {
            Phi.mvm_parallel(hx, h1);
            y.scaleAndAdd_parallel(h1, -1.0f, h2);
            PhiT.mvm_parallel(h2, h3);
            hx.scaleAndAdd_parallel(h3, mu);
        }
        printf("gd spec=%016llx hand=%016llx\n", (unsigned long long)digest(x, t1, t2, t3), (unsigned long long)digest(hx, h1, h2, h3));
    }
    printf("kept_pointer=%d\ndone\n", kept);
    return 0;
}
