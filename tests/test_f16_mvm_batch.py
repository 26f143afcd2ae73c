"""clm_f16_mvm_batch and clm_f16_mvm_scale_and_add_batch (include/clover_hip_batch_f16.h) on the GPU: one pass over a CloverMatrix16 for up
to eight CloverVector16.  Every comparison is on uint16 bit patterns (the project's standing exception: where the reference is a NaN the
result has to be a NaN); there is no tolerance.

The reference side is never the new code: each vector's result equals the single calls clm_f16_mvm / clm_f16_mvm_scale_and_add made on
that vector, and the CPU restatement (tests/half16_restate.c) -- at the large shapes the restatement is computed for ONE vector of the
call and the single GPU calls carry the others.

Shapes: those of test_half16_fused.py plus the batch kernel's own chunk edges.  x is staged 512 columns per wave of the workgroup: 512 in
the 16-row form, 2048 in the 64-row form (rows / 64 >= 2 x 256 CUs)."""
import numpy as np
import pytest

from f16_batch_helpers import KINDS, SCALES, _check_kind, _operands, forced, pa, same16
from half16_helpers import rh, rhp  # noqa: F401

NVECS = [1, 2, 3, 4, 5, 8, 9, 17]                # every instantiation full and partly filled; a remainder group
ENVS = [None, "1", "0"]
SHAPES = [(8, 128),          # one-wave workgroup, mostly tail rows; one tail loop of four steps
          (24, 256),         # exactly one full step of eight (NV = 2, 4)
          (100, 384),        # full step + tail steps, ragged rows
          (24, 512),         # exactly one staged chunk of the 16-row form
          (40, 640),         # a chunk plus 128 columns
          (32808, 128)]      # the 64-row form with a 40-row tail
WIDE_CHUNK = (32776, 2048 + 128)                 # the 64-row form: one chunk of 2048 columns plus 128
STREAMING = [(16440, 8320), (32808, 4224)]       # one per workgroup form, both just past the 256 MiB nontemporal rule
NVMAX = max(NVECS)


def vectors(kind, rows, cols, count):
    """A and `count` pairs (x, u) of the kind that differ from one another: rotations of the kind's own x and u, so that each keeps what
    makes the kind (the magnitudes of `subnormal`, the positive x of `overflow`, the -0.0 at even places of `negzero`)"""
    A, x, u = _operands(kind, rows, cols)
    xs = [np.roll(x, 7 * j) for j in range(count)]
    us = [np.roll(u, 2 * j) for j in range(count)]
    assert all(not np.array_equal(xs[0], v) for v in xs[1:])
    return A, xs, us


class Group:
    """the operands of one matrix on the device: uploaded once, the outputs overwritten with 0xEE before every call"""

    def __init__(self, hip, A, rows, cols, xs, us):
        self.hip, self.L, self.rows, self.cols = hip, hip.lib, rows, cols
        self.dA = hip.to_device(A)
        self.us = us
        self.dx, self.du = [hip.to_device(x) for x in xs], [hip.to_device(u) for u in us]
        self.dt, self.dr = [hip.alloc(2 * rows) for _ in xs], [hip.alloc(2 * rows) for _ in xs]

    def _reset(self, n, in_place):
        for j in range(n):
            self.hip.check(self.L.clv_memset(self.dt[j].ptr, 0xEE, 2 * self.rows, None))
            if in_place:
                self.dr[j].upload(self.us[j])
            else:
                self.hip.check(self.L.clv_memset(self.dr[j].ptr, 0xEE, 2 * self.rows, None))

    def _get(self, bufs, n):
        return [b.download(np.uint16, self.rows) for b in bufs[:n]]

    def single_mvm(self, n):
        self._reset(n, False)
        for j in range(n):
            self.hip.check(self.L.clm_f16_mvm(self.dA.ptr, self.rows, self.cols, self.dx[j].ptr, self.dt[j].ptr, None))
        return self._get(self.dt, n)

    def single_fused(self, n, a):
        self._reset(n, False)
        for j in range(n):
            self.hip.check(self.L.clm_f16_mvm_scale_and_add(self.dA.ptr, self.rows, self.cols, self.dx[j].ptr, self.du[j].ptr, a, self.dt[j].ptr,
                                                            self.dr[j].ptr, None))
        return self._get(self.dt, n), self._get(self.dr, n)

    def batch_mvm(self, n):
        self._reset(n, False)
        before = self.L.clv_mvm_batch_launches()
        self.hip.check(self.L.clm_f16_mvm_batch(self.dA.ptr, self.rows, self.cols, n, pa(self.dx[:n]), pa(self.dt[:n]), None))
        return self._get(self.dt, n), self.L.clv_mvm_batch_launches() - before

    def batch_fused(self, n, a, want_t, in_place):
        """(t or None, r, batched launches); in place: r[j] is a buffer that holds u[j]"""
        self._reset(n, in_place)
        u = self.dr if in_place else self.du
        before = self.L.clv_mvm_batch_launches()
        self.hip.check(self.L.clm_f16_mvm_scale_and_add_batch(self.dA.ptr, self.rows, self.cols, n, pa(self.dx[:n]), pa(u[:n]), a,
                                                              pa(self.dt[:n]) if want_t else None, pa(self.dr[:n]), None))
        launches = self.L.clv_mvm_batch_launches() - before
        t = self._get(self.dt, n)
        if not want_t:
            assert all(np.all(v == 0xEEEE) for v in t), "t was written by a call that was given none"
        return (t if want_t else None), self._get(self.dr, n), launches


def want_launches(env, nvec, streaming=False):
    """forced: a call of two or more vectors is ceil(nvec / 8) batched launches; forwarded: none; unset, the measured rule: every group of
    two or more over a matrix above 256 MiB, of three or more over a smaller one"""
    if nvec == 1 or env == "0":
        return 0
    return (nvec + 7) // 8 if env == "1" else nvec // 8 + (nvec % 8 >= (2 if streaming else 3))


def all_same(got, want, what):
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert same16(g, w), (what, "vector", j, np.flatnonzero(g != w)[:8])


def check_calls(G, nvecs, envs, t_ref, r_ref, variants):
    """every (nvec, CLV_MVM_BATCH) on the plain call and on the fused call's `variants` (a, want_t, in_place): the bits of the single
    calls (t_ref[j], r_ref[a][j]) and the launch counter"""
    streaming = G.rows * G.cols * 2 > 256 << 20
    for env in envs:
        with forced(env):
            for nvec in nvecs:
                r, launches = G.batch_mvm(nvec)
                all_same(r, t_ref[:nvec], ("plain", env, nvec))
                assert launches == want_launches(env, nvec, streaming), ("plain", env, nvec, launches)
                for a, want_t, in_place in variants:
                    t, r, launches = G.batch_fused(nvec, a, want_t, in_place)
                    all_same(r, r_ref[a][:nvec], ("fused r", env, nvec, a, want_t, in_place))
                    if want_t:
                        all_same(t, t_ref[:nvec], ("fused t", env, nvec, a, in_place))
                    assert launches == want_launches(env, nvec, streaming), ("fused", env, nvec, launches)


ALL_VARIANTS = [(a, want_t, in_place) for a in SCALES for want_t in (True, False) for in_place in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_batch_equals_the_single_calls_and_the_restatement(hip, rh, rhp, shape):  # noqa: F811
    rows, cols = shape
    small = rows * cols <= 1 << 22
    for kind in (KINDS if small else KINDS[:1]):
        A, xs, us = vectors(kind, rows, cols, NVMAX)
        G = Group(hip, A, rows, cols, xs, us)
        t_ref = G.single_mvm(NVMAX)
        r_ref = {}
        for a in SCALES:
            t_again, r_ref[a] = G.single_fused(NVMAX, a)
            all_same(t_again, t_ref, ("the two single calls", a))
        # the restatement: every vector at the small shapes, one vector of the call at the large one
        for j in (range(NVMAX) if small and rows * cols <= 1 << 16 else (0,)):
            t_cpu = (rh if rows * cols <= 1 << 20 else rhp).mvm(A, rows, cols, xs[j])
            assert same16(t_ref[j], t_cpu), (kind, j)
            r_cpu = {a: rh.scale_and_add(us[j], t_cpu, np.float32(a)) for a in SCALES}
            for a in SCALES:
                assert same16(r_ref[a][j], r_cpu[a]), (kind, j, a)
            if j == 0:
                _check_kind(kind, t_cpu, r_cpu)
        check_calls(G, NVECS, ENVS, t_ref, r_ref, ALL_VARIANTS)


@pytest.mark.gpu
def test_gpu_batch_wide_form_across_a_chunk_edge(hip, rhp):  # noqa: F811
    """the 64-row form stages 2048 columns at a time: one chunk plus 128 columns, with 2, 5 and 8 vectors (every instantiation)"""
    rows, cols = WIDE_CHUNK
    A, xs, us = vectors("uniform", rows, cols, 8)
    G = Group(hip, A, rows, cols, xs, us)
    t_ref = G.single_mvm(8)
    t_again, r = G.single_fused(8, -1.0)
    all_same(t_again, t_ref, "the two single calls")
    t_cpu = rhp.mvm(A, rows, cols, xs[3])
    assert same16(t_ref[3], t_cpu) and same16(r[3], rhp.scale_and_add(us[3], t_cpu, np.float32(-1.0)))
    check_calls(G, [2, 5, 8], ["1"], t_ref, {-1.0: r}, [(-1.0, True, False), (-1.0, False, True)])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", STREAMING, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_batch_streaming_loads(hip, rhp, shape):  # noqa: F811
    rows, cols = shape
    assert rows * cols * 2 > 256 << 20
    A, xs, us = vectors("uniform", rows, cols, 8)
    G = Group(hip, A, rows, cols, xs, us)
    t_ref = G.single_mvm(8)
    t_again, r = G.single_fused(8, 0.5)
    all_same(t_again, t_ref, "the two single calls")
    t_cpu = rhp.mvm(A, rows, cols, xs[1])
    assert same16(t_ref[1], t_cpu) and same16(r[1], rhp.scale_and_add(us[1], t_cpu, np.float32(0.5)))
    check_calls(G, [2, 8], ["1", None], t_ref, {0.5: r}, [(0.5, True, False), (0.5, False, True)])


@pytest.mark.gpu
@pytest.mark.parametrize("k", [16, 40])
def test_gpu_batch_on_row_shards_at_pointer_offsets(hip, rh, k):  # noqa: F811
    """A + k cols, u[j] + k, t[j] + k, r[j] + k: the shard's rows equal the whole-matrix call's, the rows before it keep their prefill"""
    rows, cols, a, nvec = 100, 384, -1.0, 3
    A, xs, us = vectors("uniform", rows, cols, nvec)
    G = Group(hip, A, rows, cols, xs, us)
    t_full = G.single_mvm(nvec)
    _, r_full = G.single_fused(nvec, a)
    assert same16(t_full[0], rh.mvm(A, rows, cols, xs[0]))
    L = hip.lib
    with forced("1"):
        G._reset(nvec, False)
        off = lambda bufs: pa([b.ptr + 2 * k for b in bufs[:nvec]])  # noqa: E731
        hip.check(L.clm_f16_mvm_batch(G.dA.ptr + 2 * k * cols, rows - k, cols, nvec, pa(G.dx[:nvec]), off(G.dt), None))
        for j, t in enumerate(G._get(G.dt, nvec)):
            assert same16(t[k:], t_full[j][k:]) and np.all(t[:k] == 0xEEEE), ("plain", j)
        G._reset(nvec, False)
        hip.check(L.clm_f16_mvm_scale_and_add_batch(G.dA.ptr + 2 * k * cols, rows - k, cols, nvec, pa(G.dx[:nvec]), off(G.du), a, off(G.dt),
                                                    off(G.dr), None))
        for j, (t, r) in enumerate(zip(G._get(G.dt, nvec), G._get(G.dr, nvec))):
            assert same16(t[k:], t_full[j][k:]) and same16(r[k:], r_full[j][k:]), ("fused", j)
            assert np.all(t[:k] == 0xEEEE) and np.all(r[:k] == 0xEEEE), ("fused", j)


@pytest.mark.gpu
def test_gpu_batch_methods_of_the_binding(hip, rh):  # noqa: F811
    """CloverHip.mf16_mvm_batch / mf16_mvm_scale_and_add_batch: lists in, lists out, the restatement's bits"""
    rows, cols = 100, 384
    A, xs, us = vectors("uniform", rows, cols, 5)
    t_cpu = [rh.mvm(A, rows, cols, x) for x in xs]
    all_same(hip.mf16_mvm_batch(A, rows, cols, xs), t_cpu, "mf16_mvm_batch")
    for in_place, want_t in ((False, True), (True, False)):
        out = hip.mf16_mvm_scale_and_add_batch(A, rows, cols, xs, us, 0.5, in_place=in_place, want_t=want_t)
        all_same([r for _, r in out], [rh.scale_and_add(u, t, np.float32(0.5)) for u, t in zip(us, t_cpu)], "mf16_mvm_scale_and_add_batch")
        if want_t:
            all_same([t for t, _ in out], t_cpu, "mf16_mvm_scale_and_add_batch t")
