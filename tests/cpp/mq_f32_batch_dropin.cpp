// mq_f32_batch_dropin.cpp -- several CloverVector32 signals with one CloverMatrix4 / CloverMatrix8 through the headers
// (tests/test_mq_f32_batch_dropin.py), built with -DCLOVER_FP32_ON_DEVICE.
//   mq_f32_batch_dropin <m> <n> <iterations> <K> <mu>
// For both matrix widths, on data of its own (a fixed generator), with one Phi (m x n), PhiT = Phi.transpose_parallel() and three signals:
//   iht:  Q_IHT_batch against three Q_IHT calls;          gd:   Q_GD_batch against three Q_GD calls;
//   mvm:  mvm_batch against three mvm_parallel calls;     pair: mvm_scaleAndAdd_batch (both overloads) against three mvm_scaleAndAdd
// and prints one digest (FNV-1a over the bits of every vector of every signal) per side: the two of a line are equal.
#include <CloverIHT.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>

static const uint64_t SIGNALS = 3;

static uint64_t fnv(uint64_t h, const void *p, size_t n)
{
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001B3ull;
    return h;
}
static uint64_t digest(uint64_t h, CloverVector32 *const *v)
{
    for (uint64_t j = 0; j < SIGNALS; j++) h = fnv(h, v[j]->getData(), v[j]->size_pad() * sizeof(float));
    return h;
}
static float next_unit(uint64_t &s)          // (-1, 1), 24 bits
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((int64_t)(s >> 40) - (1 << 23)) / (float)(1 << 23);
}
static void line(const char *width, const char *name, uint64_t batch, uint64_t single)
{
    printf("%s_%s batch=%016llx single=%016llx\n", width, name, (unsigned long long)batch, (unsigned long long)single);
}

struct Signals {      // SIGNALS vectors of one length, as the batch methods take them
    CloverVector32 *v[SIGNALS];
    explicit Signals(uint64_t n) { for (uint64_t j = 0; j < SIGNALS; j++) v[j] = new CloverVector32(n); }
    ~Signals() { for (uint64_t j = 0; j < SIGNALS; j++) delete v[j]; }
    void fill(uint64_t &seed, float amp)
    {
        for (uint64_t j = 0; j < SIGNALS; j++)
            for (uint64_t i = 0; i < v[j]->size(); i++) v[j]->set(i, next_unit(seed) * amp);
    }
    void copy(const Signals &o)
    {
        for (uint64_t j = 0; j < SIGNALS; j++)
            for (uint64_t i = 0; i < v[j]->size(); i++) v[j]->set(i, o.v[j]->get(i));
    }
};

template <class M>
static void run(const char *width, const CloverMatrix32 &Phi32, uint64_t m, uint64_t n, uint64_t iterations, uint64_t K, float mu)
{
    M Phi(m, n), PhiT(n, m);
    Phi.quantize(Phi32);
    Phi.transpose_parallel(PhiT);
    uint64_t seed = 77;
    Signals y(m), xs(n), u0(m);
    y.fill(seed, 3.0f);
    xs.fill(seed, 2.0f);
    u0.fill(seed, 1.0f);
    for (int gd = 0; gd < 2; gd++) {
        Signals x(n), t1(m), t2(m), t3(n), X(n), T1(m), T2(m), T3(n);
        if (gd) Q_GD_batch(Phi, PhiT, x.v, y.v, t1.v, t2.v, t3.v, SIGNALS, iterations, mu);
        else Q_IHT_batch(Phi, PhiT, x.v, y.v, t1.v, t2.v, t3.v, SIGNALS, iterations, K, mu);
        for (uint64_t j = 0; j < SIGNALS; j++) {
            if (gd) Q_GD(Phi, PhiT, *X.v[j], *y.v[j], *T1.v[j], *T2.v[j], *T3.v[j], iterations, mu);
            else Q_IHT(Phi, PhiT, *X.v[j], *y.v[j], *T1.v[j], *T2.v[j], *T3.v[j], iterations, K, mu);
        }
        line(width, gd ? "gd" : "iht", digest(digest(digest(digest(0xCBF29CE484222325ull, x.v), t1.v), t2.v), t3.v),
             digest(digest(digest(digest(0xCBF29CE484222325ull, X.v), T1.v), T2.v), T3.v));
        if (!gd) {
            uint64_t nz = 0;
            for (uint64_t i = 0; i < n; i++) nz += x.v[0]->get(i) != 0.0f;
            printf("%s_nonzero=%llu\n", width, (unsigned long long)nz);
        }
    }
    {
        Signals r(m), R(m);
        Phi.mvm_batch(xs.v, r.v, SIGNALS);
        for (uint64_t j = 0; j < SIGNALS; j++) Phi.mvm_parallel(*xs.v[j], *R.v[j]);
        line(width, "mvm", digest(0xCBF29CE484222325ull, r.v), digest(0xCBF29CE484222325ull, R.v));
    }
    {
        Signals t(m), r(m), ui(m), T(m), R(m), UI(m);
        ui.copy(u0);
        UI.copy(u0);
        Phi.mvm_scaleAndAdd_batch(xs.v, u0.v, 0.37f, t.v, r.v, SIGNALS);
        Phi.mvm_scaleAndAdd_batch(xs.v, ui.v, 0.37f, t.v, SIGNALS);                       // in place
        for (uint64_t j = 0; j < SIGNALS; j++) {
            Phi.mvm_scaleAndAdd(*xs.v[j], *u0.v[j], 0.37f, *T.v[j], *R.v[j]);
            Phi.mvm_scaleAndAdd(*xs.v[j], *UI.v[j], 0.37f, *T.v[j]);
        }
        line(width, "pair", digest(digest(digest(0xCBF29CE484222325ull, t.v), r.v), ui.v), digest(digest(digest(0xCBF29CE484222325ull, T.v), R.v), UI.v));
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
    run<CloverMatrix4>("m4", Phi32, m, n, iterations, K, mu);
    run<CloverMatrix8>("m8", Phi32, m, n, iterations, K, mu);
    printf("done\n");
    return 0;
}
