// coherence_wide.cpp -- cases 1-5 of pointer_coherence.cpp for CloverVector16, CloverMatrix8 and CloverMatrix16: a getData() (8-bit:
// and getScales()) pointer taken BEFORE a device operation reads that operation's result, a raw write through it reaches the next device
// operation, a copy does not alias, and CloverVector16(n, ptr) aliases the caller's memory in both directions -- also as the result of
// CloverMatrix16::mvm.  In the reference these hold trivially (one copy: CloverVector16.h:67-71, :119-122); here page tracking provides
// them.  Built -DCLOVER_HIP_EXPLICIT_SYNC the same program RE-TAKES each pointer after the device operation and checks the same values:
// that build's one rule (clover_device.h, tests/cpp/explicit_sync.cpp).  Sizes 128 ... 1280.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "CloverMatrix16.h"
#include "CloverMatrix8.h"
#include "CloverVector16.h"
#include "CloverVector8.h"

static int failures = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) { if (failures < 40) std::printf("FAILED line %d (n=%llu): %s\n", __LINE__, (unsigned long long)size_now, #cond); failures++; } \
    } while (0)
static uint64_t size_now = 0;

#ifdef CLOVER_HIP_EXPLICIT_SYNC
#define RETAKE(p, expr) p = (expr)          /* explicit residency: the pointer is taken again after the device operation */
#else
#define RETAKE(p, expr) (void)0             /* page tracking: the pointer from before the operation stays current */
#endif

static const uint16_t H1 = 0x3C00, H2 = 0x4000, H3 = 0x4200, H4 = 0x4400, H6 = 0x4600, H10 = 0x4900;      // 1, 2, 3, 4, 6, 10 as binary16

template <class T>
static bool all_equal(const T *p, uint64_t n, T v)
{
    for (uint64_t i = 0; i < n; i++) if (p[i] != v) return false;
    return true;
}

static void fill(CloverVector32 &v, float value) { for (uint64_t i = 0; i < v.size(); i++) v.set(i, value); }
static void fill(CloverMatrix32 &A, float value)
{
    for (uint64_t i = 0; i < A.getRows(); i++) for (uint64_t j = 0; j < A.getCols(); j++) A.set(i, j, value);
}

static void vector16(uint64_t n)
{
    size_now = n;
    CloverVector32 two(n), four(n), one(n), ramp(n);
    fill(two, 2.0f);
    fill(four, 4.0f);
    fill(one, 1.0f);
    for (uint64_t i = 0; i < n; i++) ramp.set(i, (float)(i + 1));          // distinct integers <= 1280: exact in binary16
    CloverVector16 v(n), w(n), ones(n);
    uint16_t *p = v.getData();                                             // taken BEFORE the device writes the vector
    w.quantize(four);
    ones.quantize(one);
    // 1. reads through a pointer kept across device operations
    v.quantize(two);
    RETAKE(p, v.getData());
    EXPECT(all_equal(p, n, H2));
    v.scaleAndAdd(w, 0.5f);                                                // 2 + 0.5 * 4
    RETAKE(p, v.getData());
    EXPECT(all_equal(p, n, H4));
    v.quantize(ramp);
    v.threshold(64);                                                       // the 64 largest are the last 64
    RETAKE(p, v.getData());
    EXPECT(all_equal(p, n - 64, (uint16_t)0) && p[n - 64] != 0 && p[n - 1] != 0 && v.get(n - 1) == (float)n);
    {
        CloverMatrix32 D(n, n);
        D.clear();
        for (uint64_t i = 0; i < n; i++) D.set(i, i, 2.0f);
        CloverMatrix16 qD(n, n);
        qD.quantize(D);
        CloverVector16 three(n);
        for (uint64_t i = 0; i < n; i++) three.set(i, 3.0f);
        qD.mvm(three, v);                                                  // mvm INTO the object whose pointer is kept: 2 I * 3
        RETAKE(p, v.getData());
        EXPECT(all_equal(p, n, H6));
    }
    // 2. a raw write through the kept pointer is seen by the next device operation
    v.quantize(two);
    EXPECT(v.dot(ones) == 2.0f * n);
    RETAKE(p, v.getData());
    p[0] = H10;                                                            // 2 -> 10
    p[n - 1] = H4;                                                         // 2 -> 4
    EXPECT(v.dot(ones) == 2.0f * n + 10.0f);
    EXPECT(v.dot_parallel(ones) == 2.0f * n + 10.0f && v.dot_scalar(ones) == 2.0f * n + 10.0f);
    // ... and the other way round again
    v.quantize(two);
    RETAKE(p, v.getData());
    EXPECT(p[0] == H2 && p[n - 1] == H2);
    // 3. a copy does not alias: neither a device operation on the copy nor a raw write through its pointer reaches the original
    {
        CloverVector16 c(v);
        uint16_t *pc = c.getData();
        EXPECT(pc != p && all_equal(pc, n, H2));
        c.scaleAndAdd(w, 0.5f);
        RETAKE(pc, c.getData());
        RETAKE(p, v.getData());
        EXPECT(all_equal(pc, n, H4) && all_equal(p, n, H2));
        pc[1] = H10;
        EXPECT(v.dot(ones) == 2.0f * n && c.dot(ones) == 4.0f * n + 6.0f);
        RETAKE(p, v.getData());
        p[2] = H1;
        EXPECT(c.dot(ones) == 4.0f * n + 6.0f && v.dot(ones) == 2.0f * n - 1.0f);
    }
    // 4. CloverVector16(n, ptr) over plain caller memory: device results land in the caller's array, the caller's writes reach the device
    {
        std::vector<uint16_t> user(n, 0x5555);
        CloverVector16 view(n, user.data());
        view.quantize(two);
        EXPECT(all_equal(user.data(), n, H2));
        user[3] = H10;
        EXPECT(view.dot(ones) == 2.0f * n + 8.0f);
        view.scaleAndAdd(w, 0.5f);
        EXPECT(user[3] == 0x4A00 && user[0] == H4 && user[n - 1] == H4);   // 10 + 2 = 12
        view.threshold(1);
        EXPECT(user[3] == 0x4A00 && user[0] == 0 && user[n - 1] == 0);
        // the view as the RESULT of CloverMatrix16::mvm, both vector types of operand
        CloverMatrix32 D(n, n);
        D.clear();
        for (uint64_t i = 0; i < n; i++) D.set(i, i, 3.0f);
        CloverMatrix16 qD(n, n);
        qD.quantize(D);
        qD.mvm(ones, view);
        EXPECT(all_equal(user.data(), n, H3));
        qD.mvm_parallel(w, view);
        EXPECT(all_equal(user.data(), n, (uint16_t)0x4A00));
        std::vector<float> user32(n, -1.0f);
        CloverVector32 view32(n, user32.data());
        qD.mvm(two, view32);
        EXPECT(all_equal(user32.data(), n, 6.0f));
    }
    // 5. a view over another container's pointer aliases that container
    {
        v.quantize(two);
        CloverVector16 alias(n, v.getData());
        alias.quantize(four);                                              // writes "through" v's storage
        RETAKE(p, v.getData());
        EXPECT(p[0] == H4 && v.get(n - 1) == 4.0f && v.dot(ones) == 4.0f * n);
    }
}

static void matrix8(uint64_t m, uint64_t n)
{
    size_now = m * 10000 + n;
    const uint64_t vb = m / 64, hb = n / 64;
    CloverMatrix32 A(m, n), B(m, n);
    fill(A, 4.0f);                                                         // 127 / 4 is exact: every byte is 127
    for (uint64_t i = 0; i < m; i++) for (uint64_t j = 0; j < n; j++) B.set(i, j, (float)(1 + (i >> 6) + 32 * (j >> 6)));      // one value per tile
    CloverMatrix8 q(m, n), T(n, m);
    int8_t *pd = q.getData(), *pt = T.getData();                           // taken BEFORE the device writes the matrices
    float *ps = q.getScales(), *pts = T.getScales();
    // 1. quantize, then transpose INTO the object whose pointers are kept
    q.quantize(A);
    RETAKE(pd, q.getData());
    RETAKE(ps, q.getScales());
    EXPECT(all_equal(pd, m * n, (int8_t)127) && all_equal(ps, vb * hb, 4.0f));
    q.quantize(B);
    RETAKE(pd, q.getData());
    RETAKE(ps, q.getScales());
    EXPECT(pd[0] == 127 && pd[m * n - 1] >= 126 && ps[0] == 1.0f && ps[vb * hb - 1] == (float)(vb + 32 * (hb - 1)));
    q.transpose(T);
    RETAKE(pt, T.getData());
    RETAKE(pts, T.getScales());
    RETAKE(pd, q.getData());
    bool scales_ok = true, values_ok = true;
    for (uint64_t bi = 0; bi < vb; bi++) for (uint64_t bj = 0; bj < hb; bj++) scales_ok = scales_ok && pts[bj * vb + bi] == (float)(1 + bi + 32 * bj);
    for (uint64_t i = 0; i < m; i++) for (uint64_t j = 0; j < n; j++) values_ok = values_ok && pt[j * m + i] == pd[i * n + j];
    EXPECT(values_ok && scales_ok);
    // mvm into an 8-bit vector whose pointers are kept
    q.quantize(A);
    CloverVector32 one(n), y(m), y2(m);
    fill(one, 1.0f);
    CloverVector8 x8(one), r8(m);
    int8_t *pr = r8.getData();
    float *prs = r8.getScales();
    q.mvm(x8, r8);                                                         // every row: 4 n, to within the rounding of the block factors
    RETAKE(pr, r8.getData());
    RETAKE(prs, r8.getScales());
    EXPECT(all_equal(pr, m, pr[0]) && pr[0] >= 126 && std::fabs(prs[0] - 4.0f * n) <= 1e-3f * n && prs[vb - 1] == prs[0]);
    // 2. raw writes through the kept pointers reach the next device operation: tile (0, 0) gets scale 8, then value bytes -127
    q.mvm(one, y);
    RETAKE(ps, q.getScales());
    ps[0] = 8.0f;
    q.mvm(one, y2);
    EXPECT(std::fabs(y.get(0) - 4.0f * n) <= 1e-3f * n && std::fabs(y2.get(0) - (4.0f * n + 256.0f)) <= 1e-3f * n);
    EXPECT(std::fabs(y2.get(63) - y2.get(0)) <= 1e-3f && std::fabs(y2.get(64) - 4.0f * n) <= 1e-3f * n);
    RETAKE(pd, q.getData());
    for (uint64_t j = 0; j < 64; j++) pd[j] = -127;                        // row 0 of tile (0, 0): +8 -> -8 each
    q.mvm(one, y2);
    EXPECT(std::fabs(y2.get(0) - (4.0f * n - 768.0f)) <= 1e-3f * n && std::fabs(y2.get(1) - (4.0f * n + 256.0f)) <= 1e-3f * n);
    // ... and the other way round again
    q.quantize(A);
    RETAKE(pd, q.getData());
    RETAKE(ps, q.getScales());
    EXPECT(pd[0] == 127 && ps[0] == 4.0f);
}

static void matrix16(uint64_t m, uint64_t n)
{
    size_now = m * 10000 + n;
    CloverMatrix32 A(m, n), B(m, n);
    fill(A, 3.0f);
    for (uint64_t i = 0; i < m; i++) for (uint64_t j = 0; j < n; j++) B.set(i, j, (float)((i % 32) * 64 + (j % 64)));          // integers < 2048
    CloverMatrix16 q(m, n), T(n, m);
    uint16_t *pd = q.getData(), *pt = T.getData();
    // 1. quantize, then transpose INTO the object whose pointer is kept
    q.quantize(A);
    RETAKE(pd, q.getData());
    EXPECT(all_equal(pd, m * n, H3));
    q.quantize(B);
    q.transpose(T);
    RETAKE(pd, q.getData());
    RETAKE(pt, T.getData());
    bool ok = true;
    for (uint64_t i = 0; i < m; i++) for (uint64_t j = 0; j < n; j++) ok = ok && pt[j * m + i] == pd[i * n + j] && q.get(i, j) == B.get(i, j);
    EXPECT(ok && T.get(n - 1, m - 1) == B.get(m - 1, n - 1));
    // mvm into a CloverVector16 whose pointer is kept
    q.quantize(A);
    CloverVector32 one(n), y(m), y2(m);
    fill(one, 1.0f);
    CloverVector16 x16(one), r16(m);
    uint16_t *pr = r16.getData();
    q.mvm(x16, r16);                                                       // every row: 3 n <= 3840, a multiple of 2 below 4096: exact
    RETAKE(pr, r16.getData());
    EXPECT(r16.get(0) == 3.0f * n && all_equal(pr, m, pr[0]));
    // 2. a raw write through the kept pointer reaches the next device operation
    q.mvm(one, y);
    RETAKE(pd, q.getData());
    pd[0] = H10;                                                           // 3 -> 10
    pd[(m - 1) * n + n - 1] = H1;                                          // 3 -> 1
    q.mvm(one, y2);
    EXPECT(y.get(0) == 3.0f * n && y2.get(0) == 3.0f * n + 7.0f && y2.get(m - 1) == 3.0f * n - 2.0f && y2.get(1) == 3.0f * n);
    q.mvm(x16, r16);
    RETAKE(pr, r16.getData());
    EXPECT(r16.get(m - 1) == 3.0f * n - 2.0f && pr[1] == pr[2]);
    // ... and the other way round again
    q.quantize(A);
    RETAKE(pd, q.getData());
    EXPECT(pd[0] == H3 && pd[(m - 1) * n + n - 1] == H3);
}

int main()
{
    int ndev = 0;
    if (clv_device_count(&ndev) != CLV_OK || ndev == 0) { std::printf("no_device\n"); return 0; }
    const uint64_t sizes[3] = {128, 640, 1280};
    for (int i = 0; i < 3; i++) vector16(sizes[i]);
    const uint64_t shapes[3][2] = {{128, 128}, {256, 1280}, {1280, 384}};
    for (int i = 0; i < 3; i++) {
        matrix8(shapes[i][0], shapes[i][1]);
        matrix16(shapes[i][0], shapes[i][1]);
    }
#ifdef CLOVER_HIP_EXPLICIT_SYNC
    std::printf("build=explicit\n");
#else
    std::printf("build=tracked untracked_blocks=%llu\n", (unsigned long long)clover_hip::untracked_blocks());
#endif
    std::printf(failures ? "coherence wide FAILED (%d)\n" : "coherence wide ok\n", failures);
    return failures ? 1 : 0;
}
