// mvm_transposed_batch_dropin.cpp -- the batched transposed methods of one matrix class with one vector class (mvm_transposed_batch,
// mvm_transposed_batch_at through Q_IHT_batch_one_matrix, mvm_transposed_scaleAndAdd_batch in both forms, iht_loop_batch_one_matrix,
// Q_IHT_batch_one_matrix / Q_GD_batch_one_matrix of CloverIHT.h) against the loops of their single-call partners, in BOTH rounding builds
// -- with and without -DCLOVER_STOCHASTIC_ROUNDING_DISABLED -- each tracked and with -DCLOVER_HIP_EXPLICIT_SYNC.  The classes come from
// the command line: -DDROPIN_MATRIX=CloverMatrix4 -DDROPIN_VECTOR=CloverVector4 (tests/test_mvm_transposed_batch_dropin.py),
// CloverMatrix4 with CloverVector8 (tests/test_mvm_v8_transposed_batch_dropin.py), CloverMatrix8 with CloverVector8
// (tests/test_m8_mvm_transposed_batch_dropin.py).
//   mvm_transposed_batch_dropin <dir> <m> <n> <count> <iterations> <K> <mu>
// reads <dir>/phi.f32 (m x n) and <dir>/ys.f32 (count x m).  Two sets of objects ("one": the single methods, "many": the batch methods)
// get the same keys with setRandomKeys -- matrices and vectors -- before every comparison; checked on the host-visible bytes:
//   mvm_transposed_batch              == mvm_transposed per vector
//   mvm_transposed_scaleAndAdd_batch  == mvm_transposed_scaleAndAdd per vector (both overloads)
//   Q_IHT_batch_one_matrix / Q_GD_batch_one_matrix == Q_IHT_one_matrix / Q_GD_one_matrix per signal (x, t1, t2, t3)
// and after each the keys of the matrices are equal (and, with stochastic rounding, have moved).  Prints <name>_equal=0|1,
// <name>_keys_equal=0|1, launches_rose=0|1 (clv_mvm_batch_launches went up over the batch calls) and single_side_launches.
#include <CloverIHT.h>      // every matrix and vector class

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#if !defined(DROPIN_MATRIX) || !defined(DROPIN_VECTOR)
#error "compile with -DDROPIN_MATRIX=<matrix class> -DDROPIN_VECTOR=<vector class>"
#endif
typedef DROPIN_MATRIX Matrix;
typedef DROPIN_VECTOR Vector;

static std::vector<float> read_f32(const std::string &path, size_t n)
{
    std::vector<float> v(n);
    FILE *f = fopen(path.c_str(), "rb");
    if (!f || fread(v.data(), sizeof(float), n, f) != n) { fprintf(stderr, "cannot read %s\n", path.c_str()); exit(2); }
    fclose(f);
    return v;
}

// the bytes of n values
static uint64_t value_bytes(const Vector &v, uint64_t n) { return n * v.getBitsLength() / 8; }
static bool same(const Vector &a, const Vector &b)
{
    return a.size_pad() == b.size_pad() && !memcmp(a.getData(), b.getData(), value_bytes(a, a.size_pad())) &&
           !memcmp(a.getScales(), b.getScales(), a.size_pad() / 64 * sizeof(float));
}

typedef std::vector<std::unique_ptr<Vector> > Vecs;

static Vecs make(uint64_t count, uint64_t n)
{
    Vecs v;
    for (uint64_t j = 0; j < count; j++) v.emplace_back(new Vector(n));
    return v;
}
static Vecs copies(const Vecs &src)
{
    Vecs v;
    for (const auto &e : src) v.emplace_back(new Vector(*e));
    return v;
}
static std::vector<Vector *> ptrs(const Vecs &v)
{
    std::vector<Vector *> p;
    for (const auto &e : v) p.push_back(e.get());
    return p;
}
static std::vector<const Vector *> cptrs(const Vecs &v)
{
    std::vector<const Vector *> p;
    for (const auto &e : v) p.push_back(e.get());
    return p;
}
static bool all_same(const Vecs &a, const Vecs &b)
{
    bool ok = a.size() == b.size();
    for (size_t j = 0; ok && j < a.size(); j++) ok = same(*a[j], *b[j]);
    return ok;
}
// object `id` of either side gets the same keys
static void keys_for(uint64_t id, uint64_t k1[4], uint64_t k2[4])
{
    for (int l = 0; l < 4; l++) {
        k1[l] = 0x9E3779B97F4A7C15ull * (8 * id + l + 1) ^ 0x1234567ull;
        k2[l] = 0xBF58476D1CE4E5B9ull * (8 * id + l + 5) ^ 0x7654321ull;
    }
}
static void key_vectors(Vecs &v, uint64_t first_id)
{
    for (size_t j = 0; j < v.size(); j++) {
        uint64_t k1[4], k2[4];
        keys_for(first_id + j, k1, k2);
        v[j]->setRandomKeys(k1, k2);
    }
}
static void key_matrix(Matrix &M, uint64_t id)
{
    uint64_t k1[4], k2[4];
    keys_for(id, k1, k2);
    M.setRandomKeys(k1, k2);
}
static bool same_keys(const Matrix &A, const Matrix &B, uint64_t id)
{
    uint64_t a1[4], a2[4], b1[4], b2[4], f1[4], f2[4];
    A.getRandomKeys(a1, a2);
    B.getRandomKeys(b1, b2);
    keys_for(id, f1, f2);
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
    (void)f2;
    return !memcmp(a1, b1, sizeof a1) && !memcmp(a2, b2, sizeof a2);                                         // equal (nothing draws)
#else
    return !memcmp(a1, b1, sizeof a1) && !memcmp(a2, b2, sizeof a2) && memcmp(a2, f2, sizeof a2) != 0;       // equal, and used
#endif
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
    // the same matrix image on both sides: quantised (stochastically) from the same keys.  No transpose exists on either side.
    Matrix Phi1(m, n), Phi2(m, n);
    key_matrix(Phi1, 1);
    key_matrix(Phi2, 1);
    Phi1.quantize(Phi32);
    Phi2.quantize(Phi32);
    Vecs y = make(count, m), xq = make(count, n);
    key_vectors(y, 100);
    key_vectors(xq, 200);
    for (uint64_t j = 0; j < count; j++) {
        CloverVector32 y32(m), x32(n);
        for (uint64_t i = 0; i < m; i++) y32.set(i, ys[j * m + i]);
        for (uint64_t i = 0; i < n; i++) x32.set(i, phi[(2 * j % m) * n + i] - phi[((2 * j + 1) % m) * n + i]);
        y[j]->quantize(y32);
        xq[j]->quantize(x32);
    }
    const uint64_t launches0 = clv_mvm_batch_launches();
    uint64_t single_side_launches = 0;

    // mvm_transposed_batch against mvm_transposed: y[j] has m elements, the results n
    {
        Vecs one = make(count, n), many = make(count, n);
        key_matrix(Phi1, 2);
        key_matrix(Phi2, 2);
        uint64_t c = clv_mvm_batch_launches();
        for (uint64_t j = 0; j < count; j++) Phi1.mvm_transposed(*y[j], *one[j]);
        single_side_launches += clv_mvm_batch_launches() - c;
        const std::vector<const Vector *> px = cptrs(y);
        const std::vector<Vector *> pr = ptrs(many);
        Phi2.mvm_transposed_batch(px.data(), pr.data(), count);
        bool nonzero = false;
        for (uint64_t i = 0; i < value_bytes(*one[0], n); i++) nonzero = nonzero || one[0]->getData()[i] != 0;
        printf("mvm_transposed_batch_equal=%d\nmvm_transposed_batch_keys_equal=%d\n", (int)(all_same(one, many) && nonzero), (int)same_keys(Phi1, Phi2, 2));
    }
    // mvm_transposed_scaleAndAdd_batch against mvm_transposed_scaleAndAdd, out of place and in place
    {
        Vecs u1 = copies(xq), u2 = copies(xq);
        Vecs t1 = make(count, n), r1 = make(count, n), t2 = make(count, n), r2 = make(count, n);
        key_matrix(Phi1, 3);
        key_matrix(Phi2, 3);
        key_vectors(u1, 300);
        key_vectors(u2, 300);
        uint64_t c = clv_mvm_batch_launches();
        for (uint64_t j = 0; j < count; j++) Phi1.mvm_transposed_scaleAndAdd(*y[j], *u1[j], 0.37f, *t1[j], *r1[j]);
        single_side_launches += clv_mvm_batch_launches() - c;
        const std::vector<const Vector *> px = cptrs(y), pu = cptrs(u2);
        const std::vector<Vector *> pt = ptrs(t2), pr = ptrs(r2);
        Phi2.mvm_transposed_scaleAndAdd_batch(px.data(), pu.data(), 0.37f, pt.data(), pr.data(), count);
        printf("mvm_transposed_scaleAndAdd_batch_equal=%d\nmvm_transposed_scaleAndAdd_batch_keys_equal=%d\n",
               (int)(all_same(t1, t2) && all_same(r1, r2) && all_same(u1, u2)), (int)same_keys(Phi1, Phi2, 3));

        Vecs v1 = copies(xq), v2 = copies(xq), s1 = make(count, n), s2 = make(count, n);
        key_matrix(Phi1, 4);
        key_matrix(Phi2, 4);
        key_vectors(v1, 400);
        key_vectors(v2, 400);
        c = clv_mvm_batch_launches();
        for (uint64_t j = 0; j < count; j++) Phi1.mvm_transposed_scaleAndAdd(*y[j], *v1[j], 0.37f, *s1[j]);
        single_side_launches += clv_mvm_batch_launches() - c;
        const std::vector<Vector *> pv2 = ptrs(v2), ps2 = ptrs(s2);
        Phi2.mvm_transposed_scaleAndAdd_batch(px.data(), pv2.data(), 0.37f, ps2.data(), count);
        printf("mvm_transposed_scaleAndAdd_batch_in_place_equal=%d\nmvm_transposed_scaleAndAdd_batch_in_place_keys_equal=%d\n",
               (int)(all_same(v1, v2) && all_same(s1, s2) && !same(*v1[0], *xq[0])), (int)same_keys(Phi1, Phi2, 4));
    }
    // Q_IHT_batch_one_matrix / Q_GD_batch_one_matrix against Q_IHT_one_matrix / Q_GD_one_matrix per signal
    for (int gd = 0; gd < 2; gd++) {
        Vecs y1 = copies(y), y2 = copies(y);
        Vecs x1 = make(count, n), a1 = make(count, m), b1 = make(count, m), c1 = make(count, n);
        Vecs x2 = make(count, n), a2 = make(count, m), b2 = make(count, m), c2 = make(count, n);
        key_matrix(Phi1, 5 + gd);
        key_matrix(Phi2, 5 + gd);
        key_vectors(y1, 500);
        key_vectors(y2, 500);
        key_vectors(x1, 600);
        key_vectors(x2, 600);
        uint64_t c = clv_mvm_batch_launches();
        for (uint64_t j = 0; j < count; j++) {
            if (gd) Q_GD_one_matrix(Phi1, *x1[j], *y1[j], *a1[j], *b1[j], *c1[j], iterations, mu);
            else Q_IHT_one_matrix(Phi1, *x1[j], *y1[j], *a1[j], *b1[j], *c1[j], iterations, K, mu);
        }
        single_side_launches += clv_mvm_batch_launches() - c;
        const std::vector<Vector *> px = ptrs(x2), py = ptrs(y2), pa = ptrs(a2), pb = ptrs(b2), pc = ptrs(c2);
        if (gd) Q_GD_batch_one_matrix(Phi2, px.data(), py.data(), pa.data(), pb.data(), pc.data(), count, iterations, mu);
        else Q_IHT_batch_one_matrix(Phi2, px.data(), py.data(), pa.data(), pb.data(), pc.data(), count, iterations, K, mu);
        const char *name = gd ? "Q_GD_batch_one_matrix" : "Q_IHT_batch_one_matrix";
        bool nonzero = false;
        for (uint64_t i = 0; i < value_bytes(*x1[0], n); i++) nonzero = nonzero || x1[0]->getData()[i] != 0;
        printf("%s_equal=%d\n%s_keys_equal=%d\n", name, (int)(all_same(x1, x2) && all_same(a1, a2) && all_same(b1, b2) && all_same(c1, c2) && nonzero), name,
               (int)same_keys(Phi1, Phi2, 5 + gd));
    }
    printf("launches_rose=%d\nsingle_side_launches=%llu\ndone\n", (int)(clv_mvm_batch_launches() > launches0), (unsigned long long)single_side_launches);
    return 0;
}
