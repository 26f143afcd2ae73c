// half16_transposed_batch.cpp -- the batched transposed half-precision methods through the headers
// (tests/test_f16_mvm_transposed_batch_dropin.py), built in the tracked and the -DCLOVER_HIP_EXPLICIT_SYNC builds, with the default
// exactness (the reference's threshold) and with -DCLOVER_FAST.
//   half16_transposed_batch <m> <n> <count> <iterations> <K> <mu>
// On data of its own (a fixed generator), for `count` signals with ONE Phi (m x n) and no stored transpose, it runs
//   mvm:    CloverMatrix16::mvm_transposed_batch against mvm_transposed per vector;
//   pair:   mvm_transposed_scaleAndAdd_batch (both overloads) against mvm_transposed_scaleAndAdd per vector;
//   loop:   iht_loop_batch_one_matrix against iht_loop_one_matrix per signal;
//   iht:    Q_IHT_batch_one_matrix against the five method calls written out by hand per signal (Phi' t2 by mvm_transposed);
//   gd:     Q_GD_batch_one_matrix against the four method calls per signal;
// and prints one digest (FNV-1a over the bits of every vector of every signal) per side: the two of a line are equal.
#include <CloverIHT.h>
#include <CloverMatrix16.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

static uint64_t fnv(uint64_t h, const void *p, size_t n)
{
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001B3ull;
    return h;
}

typedef std::vector<CloverVector16 *> Vecs;

static Vecs make(uint64_t count, uint64_t n)
{
    Vecs v;
    for (uint64_t j = 0; j < count; j++) v.push_back(new CloverVector16(n));
    return v;
}

static uint64_t digest(uint64_t h, const Vecs &v)
{
    for (size_t j = 0; j < v.size(); j++) h = fnv(h, v[j]->getData(), v[j]->getBytes());
    return h;
}
static uint64_t digest4(const Vecs &a, const Vecs &b, const Vecs &c, const Vecs &d)
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

static void line(const char *name, uint64_t batch, uint64_t single)
{
    printf("%s batch=%016llx single=%016llx\n", name, (unsigned long long)batch, (unsigned long long)single);
}

int main(int argc, char **argv)
{
    if (argc != 7) { fprintf(stderr, "usage: %s m n count iterations K mu\n", argv[0]); return 2; }
    const uint64_t m = strtoull(argv[1], 0, 10), n = strtoull(argv[2], 0, 10), count = strtoull(argv[3], 0, 10),
                   iterations = strtoull(argv[4], 0, 10), K = strtoull(argv[5], 0, 10);
    const float mu = strtof(argv[6], 0);

    uint64_t seed = 2026;
    const float scale = 1.0f / sqrtf((float)m);                      // Phi entries ~ U(-1, 1) / sqrt(m): the iterates stay finite at mu = 0.5
    CloverMatrix32 Phi32(m, n);
    for (uint64_t i = 0; i < m; i++)
        for (uint64_t j = 0; j < n; j++) Phi32.set(i, j, next_unit(seed) * scale);
    CloverMatrix16 Phi(m, n);
    Phi.quantize(Phi32);
    Vecs y = make(count, m), u = make(count, n);
    for (uint64_t j = 0; j < count; j++) { fill(*y[j], seed, 3.0f); fill(*u[j], seed, 1.0f); }

    {   // mvm: Phi' y
        Vecs rb = make(count, n), rs = make(count, n);
        Phi.mvm_transposed_batch(y.data(), rb.data(), count);
        for (uint64_t j = 0; j < count; j++) Phi.mvm_transposed(*y[j], *rs[j]);
        line("mvm", digest(1, rb), digest(1, rs));
    }
    {   // pair: t = Phi' y, r = u - 0.75 t; then in place with 0.5
        Vecs tb = make(count, n), rb = make(count, n), ts = make(count, n), rs = make(count, n);
        Phi.mvm_transposed_scaleAndAdd_batch(y.data(), u.data(), -0.75f, tb.data(), rb.data(), count);
        for (uint64_t j = 0; j < count; j++) Phi.mvm_transposed_scaleAndAdd(*y[j], *u[j], -0.75f, *ts[j], *rs[j]);
        Vecs ub, us, tc = make(count, n), td = make(count, n);
        for (uint64_t j = 0; j < count; j++) { ub.push_back(new CloverVector16(*u[j])); us.push_back(new CloverVector16(*u[j])); }
        Phi.mvm_transposed_scaleAndAdd_batch(y.data(), ub.data(), 0.5f, tc.data(), count);
        for (uint64_t j = 0; j < count; j++) Phi.mvm_transposed_scaleAndAdd(*y[j], *us[j], 0.5f, *td[j]);
        line("pair", digest4(tb, rb, tc, ub), digest4(ts, rs, td, us));
    }
    {   // loop
        Vecs x = make(count, n), t1 = make(count, m), t2 = make(count, m), t3 = make(count, n);
        Vecs hx = make(count, n), h1 = make(count, m), h2 = make(count, m), h3 = make(count, n);
        Phi.iht_loop_batch_one_matrix(x.data(), y.data(), t1.data(), t2.data(), t3.data(), count, iterations, K, mu, true);
        for (uint64_t j = 0; j < count; j++) Phi.iht_loop_one_matrix(*hx[j], *y[j], *h1[j], *h2[j], *h3[j], iterations, K, mu, true);
        line("loop", digest4(x, t1, t2, t3), digest4(hx, h1, h2, h3));
    }
    uint64_t iht_digest = 0, nz = 0;
    {   // iht
        Vecs x = make(count, n), t1 = make(count, m), t2 = make(count, m), t3 = make(count, n);
        Vecs hx = make(count, n), h1 = make(count, m), h2 = make(count, m), h3 = make(count, n);
        Q_IHT_batch_one_matrix(Phi, x.data(), y.data(), t1.data(), t2.data(), t3.data(), count, iterations, K, mu);
        for (uint64_t j = 0; j < count; j++) {
            hx[j]->clear();
            for (uint64_t it = 0; it < iterations; it++) {
                Phi.mvm_parallel(*hx[j], *h1[j]);
                y[j]->scaleAndAdd_parallel(*h1[j], -1.0f, *h2[j]);
                Phi.mvm_transposed(*h2[j], *h3[j]);
                hx[j]->scaleAndAdd_parallel(*h3[j], mu);
                hx[j]->threshold_parallel(K);
            }
            for (uint64_t i = 0; i < n; i++) nz += (x[j]->getData()[i] & 0x7FFF) != 0;
        }
        iht_digest = digest4(x, t1, t2, t3);
        line("iht", iht_digest, digest4(hx, h1, h2, h3));
    }
    {   // gd
        Vecs x = make(count, n), t1 = make(count, m), t2 = make(count, m), t3 = make(count, n);
        Vecs hx = make(count, n), h1 = make(count, m), h2 = make(count, m), h3 = make(count, n);
        Q_GD_batch_one_matrix(Phi, x.data(), y.data(), t1.data(), t2.data(), t3.data(), count, iterations, mu);
        for (uint64_t j = 0; j < count; j++) {
            hx[j]->clear();
            for (uint64_t it = 0; it < iterations; it++) {
                Phi.mvm_parallel(*hx[j], *h1[j]);
                y[j]->scaleAndAdd_parallel(*h1[j], -1.0f, *h2[j]);
                Phi.mvm_transposed(*h2[j], *h3[j]);
                hx[j]->scaleAndAdd_parallel(*h3[j], mu);
            }
        }
        const uint64_t gd = digest4(x, t1, t2, t3);
        line("gd", gd, digest4(hx, h1, h2, h3));
        printf("gd_differs_from_iht=%d\n", gd != iht_digest);
    }
    printf("nonzero=%llu\nlaunches=%llu\ndone\n", (unsigned long long)nz, (unsigned long long)clv_mvm_batch_launches());
    return 0;
}
