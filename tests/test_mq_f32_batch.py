"""The batched fp32-vector calls of include/clover_hip_batch_f32.h on the GPU, both matrix widths, bit for bit against the CPU references:
oracle.m4_mvm_f32 / m8.mvm_f32, rf.scale_and_add and the helpers' loop_reference (tests/m4_f32_helpers.py, tests/m8_f32_helpers.py).  The
helpers' data makes a wrong chain order visible: normal-distributed x, full-range bytes / nibbles, tile scales that differ per tile.

- products: (128, 128) one chunk; (256, 640) a ragged last round of loads; (128, chunk + 128) the second staging of x, the chunk read from
  the header; (192, 256) a 64-row shard.  nvec 1 (the single call), 2, 3, 5, 8 (absent slots of the 4- and 8-vector instantiations) and
  9 (a full group plus a forwarded remainder); a vector of its own per slot;
- fused: with t, without t, in place, a from {-1, 0.37}, and the "cancel" u on slot 1 (a single-rounding fma leaves the rounding error);
- the scale edges of the helpers' edge_problem(), used row-major; the loop on LOOP_SHAPES for 3 and 8 signals and the three thresholds;
- CLV_MVM_BATCH = 1 / 0: same bytes, the launch counter moves under 1 only; a fused call captured and replayed twice; the argument checks.

The cases of a width run as loops inside one test item per kind (the whole file takes about a second): a failing assertion names its
shape, vector count and slot."""
import re

import numpy as np
import pytest

import m4_f32_helpers as h4
import m8_f32_helpers as h8
from capture_helpers import fresh_graph
from clover_amd.build import repo_root
from fp32_helpers import rf  # noqa: F401  (fixture)
from matrix8_helpers import m8  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

HEADER = (repo_root() / "include" / "clover_hip_batch_f32.h").read_text()
CHUNK = int(re.search(r"#define\s+CLMQ_F32_BATCH_CHUNK\s+(\d+)", HEADER).group(1))
SHAPES = [(128, 128), (256, 640), (128, CHUNK + 128), (192, 256)]
NVECS = [1, 2, 3, 5, 8, 9]
same = h4.same


@pytest.fixture(autouse=True)
def batched(monkeypatch):
    """every group of two or more on the batched kernel, whatever the measured rule says about these small shapes"""
    monkeypatch.setenv("CLV_MVM_BATCH", "1")


class Width:
    """the helpers, the CPU product and the binding methods of one matrix width"""

    def __init__(self, bits, hip, oracle, m8):  # noqa: F811
        self.bits, self.h, self.hip = bits, (h4 if bits == 4 else h8), hip
        self.product = oracle.m4_mvm_f32 if bits == 4 else m8.mvm_f32
        self.quantize = oracle.m4_quantize if bits == 4 else m8.quantize
        self.transpose = oracle.m4_transpose if bits == 4 else m8.transpose
        self.ref = oracle if bits == 4 else m8
        self._refs = {}

    def call(self, name):
        return getattr(self.hip, f"m{self.bits}_{name}")

    def lib(self, name):
        return getattr(self.hip.lib, f"clm{self.bits}_{name}"), f"clm{self.bits}_{name}"

    def problem(self, rows, cols):
        """(qA, sA, nine x, nine u, nine products) of one shape, computed once"""
        if (rows, cols) not in self._refs:
            qA, sA = self.h.problem(rows, cols)[:2]
            rng = np.random.default_rng(rows + cols)
            xs, us = [self.h.vector(rng, cols) for _ in range(9)], [self.h.vector(rng, rows) for _ in range(9)]
            self._refs[rows, cols] = (qA, sA, xs, us, [self.product(qA, sA, rows, cols, x) for x in xs])
        return self._refs[rows, cols]


@pytest.fixture(scope="module", params=[4, 8], ids=["m4", "m8"])
def w(request, hip, oracle, m8):  # noqa: F811
    return Width(request.param, hip, oracle, m8)


def test_products_equal_the_cpu_product_per_slot(w, rf):  # noqa: F811
    assert CHUNK % 128 == 0 and CHUNK <= 4096 and (128, CHUNK + 128) in SHAPES
    for rows, cols in SHAPES:
        qA, sA, xs, _, want = w.problem(rows, cols)
        dq, ds = w.hip.to_device(qA), w.hip.to_device(sA)
        assert not same(want[0], want[1])
        for nvec in NVECS:
            got = w.call("mvm_f32_batch")(dq, ds, rows, cols, xs[:nvec])
            for j in range(nvec):
                assert same(got[j], want[j]), (rows, cols, nvec, j, np.count_nonzero(got[j].view(np.uint32) != want[j].view(np.uint32)))
    scale_edges_row_major(w, rf)


def test_fused_step_equals_the_product_then_scale_and_add(w, rf):  # noqa: F811
    for rows, cols in SHAPES[:3]:
        for nvec in (2, 8):
            fused_step(w, rf, rows, cols, nvec)


def fused_step(w, rf, rows, cols, nvec):  # noqa: F811
    qA, sA, xs, us, d = w.problem(rows, cols)
    dq, ds = w.hip.to_device(qA), w.hip.to_device(sA)
    fused = w.call("mvm_f32_scale_and_add_batch")
    for a in w.h.A_VALUES:
        u = [v.copy() for v in us[:nvec]]
        u[1] = w.h.cancel_u(d[1], a)                   # fma(d, a, u) is then the rounding error of the product and nothing else
        want = [rf.scale_and_add(u[j], d[j], a) for j in range(nvec)]
        if a != -1.0:
            assert np.count_nonzero(want[1]) > rows // 4, "the rounding error of the product is there to be seen"
        for in_place, want_t in ((False, True), (False, False), (True, True)):
            got = fused(dq, ds, rows, cols, xs[:nvec], [v.copy() for v in u], a, in_place=in_place, want_t=want_t)
            for j in range(nvec):
                assert (got[j][0] is None) if not want_t else same(got[j][0], d[j]), (rows, cols, nvec, a, in_place, want_t, j)
                assert same(got[j][1], want[j]), (rows, cols, nvec, a, in_place, want_t, j)


def scale_edges_row_major(w, rf):  # noqa: F811
    rows, cols, qA, sA, _, huge, tiny = w.h.edge_problem()
    rng = np.random.default_rng(5)
    xs = [w.h.vector(rng, cols) for _ in range(3)]
    for x in xs:
        for _, ct, _ in huge:
            x[64 * ct:64 * ct + 64] *= np.float32(1e-30)
    want = [w.product(qA, sA, rows, cols, x) for x in xs]
    got = w.call("mvm_f32_batch")(qA, sA, rows, cols, xs)
    u = np.full(rows, 0.25, np.float32)
    fused = w.call("mvm_f32_scale_and_add_batch")(qA, sA, rows, cols, xs, [u] * 3, 0.37)
    for j in range(3):
        fin = np.isfinite(want[j])
        assert np.array_equal(np.isfinite(got[j]), fin) and same(got[j][fin], want[j][fin])
        assert np.array_equal(np.isnan(got[j]), np.isnan(want[j])) and same(got[j][~fin & ~np.isnan(want[j])], want[j][~fin & ~np.isnan(want[j])])
        assert same(fused[j][0][fin], want[j][fin]) and same(fused[j][1][fin], rf.scale_and_add(u, want[j], 0.37)[fin])
    assert fin.sum() > rows // 2


_LOOPS = {}


def _loop(w, rf, m, n, thr):  # noqa: F811
    """the problem, its stored transpose, eight signals and their reference loops, once per (width, shape, threshold)"""
    key = (w.bits, m, n, thr)
    if key not in _LOOPS:
        qPhi, sPhi, y, mu = w.h.loop_problem(w.ref, m, n, False)
        qT, sT = w.transpose(qPhi, sPhi, m, n)
        ys = [rf.scale_and_add(y, np.roll(y, j), 0.25 * j) for j in range(8)]
        wants = [w.h.loop_reference(w.ref, rf, qPhi, sPhi, m, n, yj, 2, n // 8, mu, thr, n - 64, lambda t2: w.product(qT, sT, n, m, t2)) for yj in ys]
        _LOOPS[key] = (qPhi, sPhi, qT, sT, ys, float(mu), wants)
    return _LOOPS[key]


def test_the_loop_equals_the_five_calls_one_by_one_per_signal(w, rf):  # noqa: F811
    for m, n in h4.LOOP_SHAPES:
        for thr in (0, 1, 2):                                   # GD, FAST, REFERENCE
            qPhi, sPhi, qT, sT, ys, mu, wants = _loop(w, rf, m, n, thr)
            for nsig in (3, 8):
                got = w.call("iht_f32_batch")(qPhi, sPhi, qT, sT, m, n, ys[:nsig], 2, n // 8, mu, thr, x_len=n - 64, prefill=0x55)
                for j in range(nsig):
                    for k in ("x", "t1", "t2", "t3"):
                        assert same(got[j][k], wants[j][k]), (m, n, thr, nsig, j, k, np.count_nonzero(got[j][k] != wants[j][k]))


@pytest.fixture(scope="module")
def widths(hip, oracle, m8):  # noqa: F811
    return [Width(bits, hip, oracle, m8) for bits in (4, 8)]


def test_forced_dispatch_and_capture_give_the_same_bytes(widths, rf, monkeypatch):  # noqa: F811
    for w in widths:
        for fused in (False, True):
            forced_dispatch(w, rf, monkeypatch, fused)
        captured_fused_call(w)


def forced_dispatch(w, rf, monkeypatch, fused):  # noqa: F811
    rows, cols = 256, 640
    qA, sA, xs, us, d = w.problem(rows, cols)
    count = w.hip.lib.clv_mvm_batch_launches
    moved, out = {}, {}
    for force in ("1", "0"):
        monkeypatch.setenv("CLV_MVM_BATCH", force)
        before = count()
        if fused:
            out[force] = [r2 for _, r2 in w.call("mvm_f32_scale_and_add_batch")(qA, sA, rows, cols, xs[:5], us[:5], 0.37)]
        else:
            out[force] = w.call("mvm_f32_batch")(qA, sA, rows, cols, xs[:5])
        moved[force] = count() - before
    assert moved == {"1": 1, "0": 0}, (w.bits, fused)
    monkeypatch.setenv("CLV_MVM_BATCH", "1")
    for j in range(5):
        assert same(out["1"][j], out["0"][j]) and same(out["0"][j], rf.scale_and_add(us[j], d[j], 0.37) if fused else d[j])


def captured_fused_call(w):
    rows, cols, nvec = 256, 640, 3
    hip, (fn, _) = w.hip, w.lib("mvm_f32_scale_and_add_batch")
    qA, sA, xs, us, _ = w.problem(rows, cols)
    eager = w.call("mvm_f32_scale_and_add_batch")(qA, sA, rows, cols, xs[:nvec], us[:nvec], 0.37)
    dq, ds = hip.to_device(qA), hip.to_device(sA)
    dx, du = [hip.to_device(x) for x in xs[:nvec]], [hip.to_device(u) for u in us[:nvec]]
    dt, dr = [hip.alloc(4 * rows) for _ in range(nvec)], [hip.alloc(4 * rows) for _ in range(nvec)]
    pa = hip.ptr_array
    g = fresh_graph(hip.lib)
    try:
        g.capture(lambda stream: hip.check(fn(dq.ptr, ds.ptr, rows, cols, nvec, pa(dx), pa(du), 0.37, pa(dt), pa(dr), stream)))
        for _ in range(2):
            for b in dt + dr:
                hip.check(hip.lib.clv_memset(b.ptr, 0xEE, b.nbytes, None))
            hip.sync()
            g.replay()
            for j in range(nvec):
                assert same(dt[j].download(np.float32), eager[j][0]) and same(dr[j].download(np.float32), eager[j][1]), j
    finally:
        g.close(hip.lib)


def test_bad_arguments_are_refused_by_name_and_the_empty_call_is_ok(widths):
    for w in widths:
        bad_arguments(w)


def bad_arguments(w):
    rows, cols = 128, 128
    hip, (fn, name) = w.hip, w.lib("mvm_f32_batch")
    qA, sA, xs, _, _ = w.problem(rows, cols)
    dq, ds = hip.to_device(qA), hip.to_device(sA)
    x, r = [hip.alloc(4 * cols + 16) for _ in range(2)], [hip.alloc(4 * rows) for _ in range(2)]
    pa = hip.ptr_array
    bad = {"a NULL entry": (pa([x[0], None]), pa(r)),
           "a misaligned x": (pa([x[0], x[1].ptr + 4]), pa(r)),
           "an output over another vector's input": (pa(x), pa([r[0], x[0]]))}
    for what, (px, pr) in bad.items():
        assert fn(dq.ptr, ds.ptr, rows, cols, 2, px, pr, None) == -1, what                    # CLV_ERR_INVALID
        assert name in hip.lib.clv_last_error().decode(), what
    # the other two entry points answer under their own names: a NULL entry of u, a misaligned x[1] of the loop
    (fused, fname), (loop, lname) = w.lib("mvm_f32_scale_and_add_batch"), w.lib("iht_f32_batch")
    assert fused(dq.ptr, ds.ptr, rows, cols, 2, pa(x), pa([r[0], None]), 0.37, None, pa(r), None) == -1
    assert fname in hip.lib.clv_last_error().decode()
    v = [hip.alloc(4 * 128 + 16) for _ in range(10)]
    assert loop(dq.ptr, ds.ptr, dq.ptr, ds.ptr, 128, 128, 2, pa([v[0], v[1].ptr + 4]), 128, pa(v[2:4]), pa(v[4:6]), pa(v[6:8]), pa(v[8:10]), 1, 16, 0.5, 0,
                None) == -1
    assert lname in hip.lib.clv_last_error().decode()
    before = hip.lib.clv_mvm_batch_launches()
    for nvec, rr, cc in ((0, rows, cols), (2, 0, cols), (2, rows, 0)):
        assert fn(dq.ptr, ds.ptr, rr, cc, nvec, pa(x), pa(r), None) == 0
    assert hip.lib.clv_mvm_batch_launches() == before
