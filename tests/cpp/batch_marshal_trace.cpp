// batch_marshal_trace.cpp -- every public batch method of CloverMatrix4 and CloverMatrix8 called once against tests/cpp/fake_clv_batch.c
// (no GPU): the fake prints each C call's name and scalar arguments and writes, into the first value and scale of every output, a number
// made of the first value and scale of that vector's inputs; this client tags every vector and both matrices with numbers of their own and
// prints what the host sees of every output afterwards, with the copy counts of the fake.  The whole output is the trace that
// tests/test_batch_marshalling_cpu.py compares with tests/traces/: it changes when a pointer lands in another slot, rows and cols swap
// (128 x 256), an output is not committed or an input is mapped for writing -- and not with the order in which one call's inputs are mapped.
#include <cstdio>
#include <memory>
#include <vector>

#include <CloverMatrix4.h>
#include <CloverMatrix8.h>
#include <CloverVector4.h>
#include <CloverVector8.h>

extern "C" int fake_copies_d2h, fake_copies_h2d;

static const uint64_t ROWS = 128, COLS = 256, COUNT = 3;
enum Role { X = 1, U, T, R, Y, T1, T2, T3 };

// COUNT vectors of one role, each tagged in its first value and first scale
template <class V>
struct Vecs {
    std::vector<std::unique_ptr<V> > own;
    std::vector<V *> p;
    std::vector<const V *> cp;
    Vecs(uint64_t n, Role role)
    {
        for (uint64_t j = 0; j < COUNT; j++) {
            own.emplace_back(new V(n));
            own[j]->getData()[0] = (int8_t)(8 * role + j + 1);
            own[j]->getScales()[0] = 4.0f * role + j + 0.5f;
            p.push_back(own[j].get());
            cp.push_back(own[j].get());
        }
    }
};

template <class M>
static void tag_matrix(M &A, int8_t value, float scale)
{
    A.getData()[0] = value;
    A.getScales()[0] = scale;
}

static void copies(const char *when) { std::printf("  copies %s: h2d=%d d2h=%d\n", when, fake_copies_h2d, fake_copies_d2h); }

template <class V>
static void show(const char *role, const Vecs<V> &v)
{
    for (uint64_t j = 0; j < COUNT; j++) std::printf("  %s[%d] q=%d s=%.4f\n", role, (int)j, (int)v.p[j]->getData()[0], v.p[j]->getScales()[0]);
}

template <class M, class V>
static void run(const char *name, int8_t tag)
{
    std::printf("==== %s\n", name);
    M A(ROWS, COLS), AT(COLS, ROWS);
    tag_matrix(A, tag, tag + 0.5f);
    tag_matrix(AT, (int8_t)(tag + 1), tag + 1.5f);
    for (int transposed = 0; transposed < 2; transposed++) {
        const uint64_t x_len = transposed ? ROWS : COLS, r_len = transposed ? COLS : ROWS;
        const char *dir = transposed ? "mvm_transposed" : "mvm";
        {
            std::printf("-- %s_batch\n", dir);
            Vecs<V> x(x_len, X), r(r_len, R);
            if (transposed) A.mvm_transposed_batch(x.cp.data(), r.p.data(), COUNT);
            else A.mvm_batch(x.cp.data(), r.p.data(), COUNT);
            copies("after the call");
            show("r", r);
            copies("after the reads");
        }
        {
            std::printf("-- %s_batch_at\n", dir);
            Vecs<V> x(x_len, X), r(r_len, R);
            if (transposed) A.mvm_transposed_batch_at(x.cp.data(), r.p.data(), COUNT, 5, 7, 11);
            else A.mvm_batch_at(x.cp.data(), r.p.data(), COUNT, 5, 7, 11);
            copies("after the call");
            show("r", r);
            copies("after the reads");
        }
        {
            std::printf("-- %s_scaleAndAdd_batch\n", dir);
            Vecs<V> x(x_len, X), u(r_len, U), t(r_len, T), r(r_len, R);
            if (transposed) A.mvm_transposed_scaleAndAdd_batch(x.cp.data(), u.cp.data(), -1.0f, t.p.data(), r.p.data(), COUNT);
            else A.mvm_scaleAndAdd_batch(x.cp.data(), u.cp.data(), -1.0f, t.p.data(), r.p.data(), COUNT);
            copies("after the call");
            show("t", t);
            show("r", r);
            show("u", u);
            copies("after the reads");
        }
        {
            std::printf("-- %s_scaleAndAdd_batch in place\n", dir);
            Vecs<V> x(x_len, X), u(r_len, U), t(r_len, T);
            if (transposed) A.mvm_transposed_scaleAndAdd_batch(x.cp.data(), u.p.data(), 0.75f, t.p.data(), COUNT);
            else A.mvm_scaleAndAdd_batch(x.cp.data(), u.p.data(), 0.75f, t.p.data(), COUNT);
            copies("after the call");
            show("t", t);
            show("u", u);
            copies("after the reads");
        }
    }
#ifdef CLOVER_STOCHASTIC_ROUNDING_DISABLED
    for (int one_matrix = 0; one_matrix < 2; one_matrix++)
        for (uint64_t iterations = 0; iterations <= 2; iterations += 2) {
            std::printf("-- iht_loop_batch%s iterations=%d\n", one_matrix ? "_one_matrix" : "", (int)iterations);
            Vecs<V> x(COLS - 9, X), y(ROWS, Y), t1(ROWS, T1), t2(ROWS, T2), t3(COLS, T3);
            const bool with_threshold = iterations != 0;
            if (one_matrix) A.iht_loop_batch_one_matrix(x.p.data(), y.cp.data(), t1.p.data(), t2.p.data(), t3.p.data(), COUNT, iterations, 24, 0.005f, with_threshold);
            else A.iht_loop_batch(AT, x.p.data(), y.cp.data(), t1.p.data(), t2.p.data(), t3.p.data(), COUNT, iterations, 24, 0.005f, with_threshold);
            copies("after the call");
            show("x", x);
            show("t1", t1);
            show("t2", t2);
            show("t3", t3);
            copies("after the reads");
        }
#endif
}

int main()
{
    run<CloverMatrix4, CloverVector4>("CloverMatrix4 x CloverVector4", 10);
    run<CloverMatrix4, CloverVector8>("CloverMatrix4 x CloverVector8", 20);
    run<CloverMatrix8, CloverVector8>("CloverMatrix8 x CloverVector8", 30);
    std::printf("done\n");
    return 0;
}
