"""k_m4_mvm_cu<G, FUSE> (matrix4.hip): one workgroup of 256 G threads per CU, G consecutive 64-row groups on one LDS image of x.

launch_mvm takes it for a streaming matrix (rows cols / 2 > T = 256 MiB) without a generator whose row groups number more than 2 and
at most 4 per CU: G = ceil((rows / 64) / CUs), grid = ceil((rows / 64) / G).  Every case asserts that predicate on its shape with the
device's CU count first, so it cannot pass on another kernel.  The streaming-instantiation map of test_streaming_instantiations.py
continues here:

matrix4.hip:
- k_m4_mvm_cu<4, false> (no generator, 3 CUs < rows / 64 <= 4 CUs): test_whole_result_equals_the_shards[g4_ragged],
  test_sampled_groups_against_the_oracle[g4_ragged], test_rowdots_equal_the_shards, test_capture_and_replay; at 65536 x 65536 also
  test_gpu_large.py::test_c3_mvm_65536_sampled_and_sharded
- k_m4_mvm_cu<3, false> (2 CUs < rows / 64 <= 3 CUs): the same two tests with [g3] and [two_chunks]
- k_m4_mvm_cu<4, true>: test_fused_equals_mvm_then_scale_and_add[...]
- k_m4_mvm_cu<3, true>: test_streaming_instantiations.py::test_m4_mvm_fused_four_wave_streaming (513 row groups)
- k_m4_mvm64<8, true, false, *> keeps the launches with more than 4 row groups per CU (test_gpu_large.py's C5 case)

The whole packed result is compared, byte for byte, with clm4_mvm on row shards of at most 512 row groups at pointer offsets.  512 row
groups are at most 2 per CU, so the launcher never gives a shard to k_m4_mvm_cu: it runs the eight-wave k_m4_mvm64<16, true, ..., 8>
where the shard itself exceeds 256 MiB (two_chunks) and the cached k_m4_mvm64<8, false, ...> below that, both unchanged code.
Sampled row groups -- group 0, the last one and a seeded pick from each of the G slots of a workgroup -- are compared with the scalar
oracle.  No tolerance anywhere: the chains of a row never leave its lane.  Matrices are filled on the device and never downloaded
whole."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

T = 256 << 20
A_FUSED = -0.37
SHAPES = {
    "g4_ragged": (64 * 1021, 8320, 4),           # 1021 row groups: 256 workgroups, the last one holds one live group
    "g3": (64 * 768, 11264, 3),
    "two_chunks": (64 * 513, 65536 + 128, 3),    # a second x chunk of 128 columns: the chunk loop's barriers, the ragged chunk
}


def same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


def ok(rc):
    assert rc == 0, f"HIP runtime call failed: {rc}"


def assert_selects_mvm_cu(hip, rows, cols, G):
    """launch_mvm's predicate for k_m4_mvm_cu<G, *>, on this device"""
    cus = hip.device_info()["compute_units"]
    groups = rows // 64
    assert rows % 64 == 0 and cols % 128 == 0
    assert rows * (cols // 2) > T, "not a streaming matrix"
    assert 2 * cus < groups <= 4 * cus, f"{groups} row groups on {cus} CUs: another kernel"
    assert -(-groups // cus) == G


def sharded(hip, call, rows, cols, A, sA):
    """call(A shard, sA shard, first row, shard rows) on shards of at most 512 row groups"""
    hb = cols // 64
    for g0 in range(0, rows // 64, 512):
        n = min(512, rows // 64 - g0)
        call(A.ptr + g0 * 64 * (cols // 2), sA.ptr + g0 * hb * 4, g0 * 64, n * 64)


class Case:
    def __init__(self, hip, name):
        self.name = name
        self.rows, self.cols, self.G = rows, cols, G = SHAPES[name]
        assert_selects_mvm_cu(hip, rows, cols, G)
        L = hip.lib
        seed = 0x700 + 16 * list(SHAPES).index(name)
        self.A, self.sA = hip.alloc(rows * cols // 2), hip.alloc((rows // 64) * (cols // 64) * 4)
        self.x, self.sx = hip.alloc(cols // 2), hip.alloc(cols // 16)
        hip.check(L.clv_fill_random_nibbles(self.A.ptr, self.A.nbytes, seed, 0, None))
        hip.check(L.clv_fill_random_scales(self.sA.ptr, self.sA.nbytes // 4, seed + 1, 0, None))
        hip.check(L.clv_fill_random_nibbles(self.x.ptr, self.x.nbytes, seed + 2, 0, None))
        hip.check(L.clv_fill_random_scales(self.sx.ptr, self.sx.nbytes // 4, seed + 3, 0, None))
        # the whole call: k_m4_mvm_cu.  The result buffers start from a pattern, so that a row group nobody wrote shows
        self.r, self.sr = hip.alloc(rows // 2), hip.alloc(rows // 16)
        for d in (self.r, self.sr):
            hip.check(L.clv_memset(d.ptr, 0x5A, d.nbytes, None))
        hip.check(L.clm4_mvm(self.A.ptr, self.sA.ptr, rows, cols, self.x.ptr, self.sx.ptr, self.r.ptr, self.sr.ptr, None, None))
        self.r_h, self.sr_h = self.r.download(np.uint8), self.sr.download(np.float32)


@pytest.fixture(scope="module")
def cases(hip):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(hip, name)
        return made[name]
    yield get
    made.clear()


@pytest.mark.parametrize("name", list(SHAPES))
def test_whole_result_equals_the_shards(hip, cases, name):
    c = cases(name)
    rows, cols = c.rows, c.cols
    parts_r, parts_s = [], []

    def call(pA, psA, row0, n):
        rk, srk = hip.alloc(n // 2), hip.alloc(n // 16)
        hip.check(hip.lib.clm4_mvm(pA, psA, n, cols, c.x.ptr, c.sx.ptr, rk.ptr, srk.ptr, None, None))
        parts_r.append(rk.download(np.uint8))
        parts_s.append(srk.download(np.float32))
    sharded(hip, call, rows, cols, c.A, c.sA)
    want_r, want_s = np.concatenate(parts_r), np.concatenate(parts_s)
    assert want_r.size == rows // 2 and want_s.size == rows // 64
    assert same(c.r_h, want_r), np.flatnonzero(c.r_h != want_r)[:8] // 32
    assert same(c.sr_h, want_s), np.flatnonzero(c.sr_h.view(np.uint32) != want_s.view(np.uint32))[:8]
    assert len(set(c.r_h[::97].tolist())) > 16            # not a constant


@pytest.mark.parametrize("name", list(SHAPES))
def test_sampled_groups_against_the_oracle(hip, oracle, cases, name):
    c = cases(name)
    rows, cols, G = c.rows, c.cols, c.G
    groups, hb = rows // 64, cols // 64
    rng = np.random.default_rng(groups)
    full = groups // G                                  # workgroups whose G slots are all live
    picks = sorted({0, groups - 1} | {int(rng.integers(0, full)) * G + slot for slot in range(G)})
    assert {g % G for g in picks} == set(range(G))
    qx, sxh = c.x.download(np.uint8), c.sx.download(np.float32)
    for g in picks:
        blk = np.empty(64 * cols // 2, np.uint8)
        hip.check(hip.lib.clv_memcpy_d2h(blk.ctypes.data, c.A.ptr + g * 64 * (cols // 2), blk.nbytes, None))
        sblk = np.empty(hb, np.float32)
        hip.check(hip.lib.clv_memcpy_d2h(sblk.ctypes.data, c.sA.ptr + g * hb * 4, sblk.nbytes, None))
        d = oracle.m4_rowdots(blk, sblk, 64, cols, qx, sxh)
        ro, sro = oracle.v4_quantize(np.concatenate([d, np.zeros(64, np.float32)]))
        assert same(c.r_h[g * 32:(g + 1) * 32], ro[:32]) and bits(c.sr_h[g]) == bits(sro[0]), g


def test_rowdots_equal_the_shards(hip, cases):
    c = cases("g4_ragged")
    rows, cols = c.rows, c.cols
    d = hip.alloc(rows * 4)
    hip.check(hip.lib.clv_memset(d.ptr, 0x5A, d.nbytes, None))
    hip.check(hip.lib.clm4_rowdots(c.A.ptr, c.sA.ptr, rows, cols, c.x.ptr, c.sx.ptr, d.ptr, None))
    parts = []

    def call(pA, psA, row0, n):
        dk = hip.alloc(n * 4)
        hip.check(hip.lib.clm4_rowdots(pA, psA, n, cols, c.x.ptr, c.sx.ptr, dk.ptr, None))
        parts.append(dk.download(np.uint32))
    sharded(hip, call, rows, cols, c.A, c.sA)
    got, want = d.download(np.uint32), np.concatenate(parts)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert np.unique(got).size > rows // 2


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("want_t", [True, False], ids=["t", "no_t"])
def test_fused_equals_mvm_then_scale_and_add(hip, cases, want_t, in_place):
    """clm4_mvm_scale_and_add on k_m4_mvm_cu<4, true> against clm4_mvm (the case's whole result, itself compared with the shards)
    followed by clv4_scale_and_add.  rows is no multiple of 128, which clv4_scale_and_add wants: its operands carry one more block of
    zeros (blocks do not meet in a deterministic scaleAndAdd), the fused call sees the first rows / 64 blocks only"""
    c = cases("g4_ragged")
    L = hip.lib
    rows, cols = c.rows, c.cols
    n_pad = rows + 64
    assert n_pad % 128 == 0

    def padded(seed=None, src=None):
        q, s = hip.alloc(n_pad // 2), hip.alloc(n_pad // 16)
        for d in (q, s):
            hip.check(L.clv_memset(d.ptr, 0, d.nbytes, None))
        if seed is not None:
            hip.check(L.clv_fill_random_nibbles(q.ptr, rows // 2, seed, 0, None))
            hip.check(L.clv_fill_random_scales(s.ptr, rows // 64, seed + 1, 0, None))
        return q, s
    u, v, want = padded(seed=0x7A0), padded(), padded()
    hip.check(L.clv_memcpy_d2d(v[0].ptr, c.r.ptr, rows // 2, None))
    hip.check(L.clv_memcpy_d2d(v[1].ptr, c.sr.ptr, rows // 16, None))
    hip.check(L.clv4_scale_and_add(u[0].ptr, u[1].ptr, v[0].ptr, v[1].ptr, A_FUSED, n_pad, want[0].ptr, want[1].ptr, None, None))
    want_r, want_s = want[0].download(np.uint8, rows // 2), want[1].download(np.float32, rows // 64)
    u_h = u[0].download(np.uint8, rows // 2)

    t = (hip.alloc(rows // 2), hip.alloc(rows // 16)) if want_t else None
    r2 = u if in_place else (hip.alloc(rows // 2), hip.alloc(rows // 16))
    hip.check(L.clm4_mvm_scale_and_add(c.A.ptr, c.sA.ptr, rows, cols, c.x.ptr, c.sx.ptr, u[0].ptr, u[1].ptr, A_FUSED,
                                       t[0].ptr if t else None, t[1].ptr if t else None, r2[0].ptr, r2[1].ptr, None, None))
    assert same(r2[0].download(np.uint8, rows // 2), want_r) and same(r2[1].download(np.float32, rows // 64), want_s)
    if t:
        assert same(t[0].download(np.uint8), c.r_h) and same(t[1].download(np.float32), c.sr_h)
    if not in_place:
        assert same(u[0].download(np.uint8, rows // 2), u_h), "u was written"
    assert not same(want_r, u_h)


def test_capture_and_replay(hip, cases):
    """nothing is allocated or set per call: the launch captures into a graph and two replays give the eager bytes"""
    c = cases("g4_ragged")
    L = hip.lib
    rt = C.CDLL("libamdhip64.so")
    rows, cols = c.rows, c.cols
    r, sr = hip.alloc(rows // 2), hip.alloc(rows // 16)
    stream, graph, gexec = C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(rt.hipStreamCreate(C.byref(stream)))
    ok(rt.hipStreamBeginCapture(stream, 0))
    hip.check(L.clm4_mvm(c.A.ptr, c.sA.ptr, rows, cols, c.x.ptr, c.sx.ptr, r.ptr, sr.ptr, None, stream))
    ok(rt.hipStreamEndCapture(stream, C.byref(graph)))
    ok(rt.hipGraphInstantiate(C.byref(gexec), graph, None, None, 0))
    for rep in range(2):
        for d in (r, sr):
            hip.check(L.clv_memset(d.ptr, 0x5A, d.nbytes, None))
        hip.sync()
        ok(rt.hipGraphLaunch(gexec, stream))
        ok(rt.hipStreamSynchronize(stream))
        assert same(r.download(np.uint8), c.r_h) and same(sr.download(np.float32), c.sr_h), rep
    ok(rt.hipGraphExecDestroy(gexec))
    ok(rt.hipGraphDestroy(graph))
    ok(rt.hipStreamDestroy(stream))
