"""clm_f16_mvm_transposed_batch and clm_f16_mvm_transposed_scale_and_add_batch (include/clover_hip_batch_f16_t.h) on the GPU: one pass over
a CloverMatrix16's own bytes for up to eight CloverVector16, r[j] = f16(A' x[j]).  Every comparison is on uint16 bit patterns (where the
reference is a NaN the result has to be a NaN); there is no tolerance.

The reference side is never the new code.  Each vector's result equals (1) the single transposed calls clm_f16_mvm_transposed /
clm_f16_mvm_transposed_scale_and_add made on that vector, (2) the CPU restatement's column walk (tests/half16_t_restate.c) for the first
and the last vector of a shape, and (3) clm_f16_mvm_batch / clm_f16_mvm_scale_and_add_batch on the device-made clm_f16_transpose(A).

Shapes (rows x cols; tests/f16_transposed_batch_data.py reads F16TB_COLS, F16TB_U and F16TB_CHUNK from clover_amd/csrc/half16_t_batch.hip):
  128 x 128, 256 x 128, 128 x 256, 384 x 640    BASIC: every nvec of NVECS under every CLV_MVM_BATCH; non-square both ways, so that a
                                                product that forgets to transpose fails
  128 ... 1024 rows x 128                       one set, one round, a round plus a set, a partial set, two rounds for U in {1, 2, 4, 8}
  W - 128 (if positive), W, W + 128, 2 W + 128 columns at 128 and 256 rows, for every strip width W
                                                the masked last workgroup (strips wider than 128 columns) and several workgroups
  C - 128, C, C + 128, 2 C + 128 rows x 128     the x re-staging barriers, for every chunk C
  C + round + 128 rows, three workgroups        a multiple of neither the chunk nor the round
The edge shapes run forced (CLV_MVM_BATCH=1) with 2, 3, 5 and 8 vectors: every instantiation, full and partly filled.  The data cancels
across chains (f16_transposed_data.py), so a wrong summation order shows in the f16 bits; test_f16_mvm_transposed_batch_cpu.py asserts that
it does for every shape and vector here.  The nontemporal instantiations run at 8192 x 16512 against the device pair only: the launcher
has no switch that forces them at a small shape."""
import numpy as np
import pytest

from f16_batch_helpers import SCALES, _check_kind, _operands, forced, pa, same16
from f16_transposed_batch_data import EDGE_NVECS, EDGES, NVECS, count_for, u_of, x_of
from f16_transposed_data import A_VALUES, BASIC, NT_SHAPE, ZERO_COLUMN, big_matrix, case, vector_cols, vector_rows
from f16_transposed_helpers import rt  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ENVS = [None, "1", "0"]
# The dispatch rule with CLV_MVM_BATCH unset (F16TBatch::batched_by_rule, half16_t_batch.hip), from profiles/f16_mvm_transposed_batch_kernel_bench.json
# and profiles/f16_mvm_transposed_batch_groups_kernel_bench.json: every group of 2 ... 8 beat the single transposed calls by more than
# their spread, over a streaming matrix (2.0 x at two vectors) and over a cache-resident one (1.11 x at two vectors).  The smallest
# group that runs batched, by size class; None would mean that the class forwards every group to the single calls
UNSET_MIN_GROUP = {"streaming": 2, "resident": 2}


def want_launches(env, nvec, streaming=False):
    """forced: a call of two or more vectors is ceil(nvec / 8) batched launches; forwarded and one vector: none; unset: the measured rule"""
    if nvec == 1 or env == "0":
        return 0
    if env == "1":
        return (nvec + 7) // 8
    g_min = UNSET_MIN_GROUP["streaming" if streaming else "resident"]
    return 0 if g_min is None else nvec // 8 * (8 >= g_min) + (nvec % 8 >= g_min)


class Group:
    """one matrix and its vectors on the device: uploaded once, the outputs overwritten with 0xEE before every call.  A is rows x cols:
    every x has `rows` elements, u / t / r `cols`"""

    def __init__(self, hip, dA, rows, cols, xs, us):
        self.hip, self.L, self.rows, self.cols, self.dA, self.us = hip, hip.lib, rows, cols, dA, us
        self.dx, self.du = [hip.to_device(x) for x in xs], [hip.to_device(u) for u in us]
        self.dt, self.dr = [hip.alloc(2 * cols) for _ in xs], [hip.alloc(2 * cols) for _ in xs]

    def _reset(self, n, in_place):
        for j in range(n):
            self.hip.check(self.L.clv_memset(self.dt[j].ptr, 0xEE, 2 * self.cols, None))
            if in_place:
                self.dr[j].upload(self.us[j])
            else:
                self.hip.check(self.L.clv_memset(self.dr[j].ptr, 0xEE, 2 * self.cols, None))

    def _get(self, bufs, n):
        return [b.download(np.uint16, self.cols) for b in bufs[:n]]

    def single_mvm(self, n):
        self._reset(n, False)
        for j in range(n):
            self.hip.check(self.L.clm_f16_mvm_transposed(self.dA.ptr, self.rows, self.cols, self.dx[j].ptr, self.dt[j].ptr, None))
        return self._get(self.dt, n)

    def single_fused(self, n, a):
        self._reset(n, False)
        for j in range(n):
            self.hip.check(self.L.clm_f16_mvm_transposed_scale_and_add(self.dA.ptr, self.rows, self.cols, self.dx[j].ptr, self.du[j].ptr, a,
                                                                       self.dt[j].ptr, self.dr[j].ptr, None))
        return self._get(self.dt, n), self._get(self.dr, n)

    def held(self, dAt, n, a=None):
        """the row-major batch on the stored transpose dAt (cols x rows), forced batched: t, or (t, r) of the fused call"""
        self._reset(n, False)
        with forced("1"):
            if a is None:
                self.hip.check(self.L.clm_f16_mvm_batch(dAt.ptr, self.cols, self.rows, n, pa(self.dx[:n]), pa(self.dt[:n]), None))
                return self._get(self.dt, n)
            self.hip.check(self.L.clm_f16_mvm_scale_and_add_batch(dAt.ptr, self.cols, self.rows, n, pa(self.dx[:n]), pa(self.du[:n]), a,
                                                                  pa(self.dt[:n]), pa(self.dr[:n]), None))
        return self._get(self.dt, n), self._get(self.dr, n)

    def batch_mvm(self, n):
        self._reset(n, False)
        before = self.L.clv_mvm_batch_launches()
        self.hip.check(self.L.clm_f16_mvm_transposed_batch(self.dA.ptr, self.rows, self.cols, n, pa(self.dx[:n]), pa(self.dt[:n]), None))
        return self._get(self.dt, n), self.L.clv_mvm_batch_launches() - before

    def batch_fused(self, n, a, form):
        """(t or None, r, batched launches); form: "t", "no_t" or "in_place" (r[j] is a buffer that holds u[j]; t stored)"""
        in_place, want_t = form == "in_place", form != "no_t"
        self._reset(n, in_place)
        u = self.dr if in_place else self.du
        before = self.L.clv_mvm_batch_launches()
        self.hip.check(self.L.clm_f16_mvm_transposed_scale_and_add_batch(self.dA.ptr, self.rows, self.cols, n, pa(self.dx[:n]), pa(u[:n]), a,
                                                                         pa(self.dt[:n]) if want_t else None, pa(self.dr[:n]), None))
        launches = self.L.clv_mvm_batch_launches() - before
        t = self._get(self.dt, n)
        if not want_t:
            assert all(np.all(v == 0xEEEE) for v in t), "t was written by a call that was given none"
        return (t if want_t else None), self._get(self.dr, n), launches


def all_same(got, want, what):
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert same16(g, w), (what, "vector", j, np.flatnonzero(g != w)[:8])


class Refs:
    """a shape's references, computed once: the single transposed calls per vector (t[j], r[a][j]), held to the restatement for the first
    and the last vector and to the row-major batch on the device-made transpose for all of them"""

    def __init__(self, hip, rt, rows, cols):  # noqa: F811
        S, n = case(rows, cols), count_for((rows, cols))
        xs, us = [x_of(rows, cols, j) for j in range(n)], [u_of(rows, cols, j) for j in range(n)]
        dA, dAt = hip.to_device(S.A), hip.alloc(2 * rows * cols)
        hip.check(hip.lib.clm_f16_transpose(dA.ptr, rows, cols, dAt.ptr, None))
        assert rt.is_transpose(S.A, rows, cols, dAt.download(np.uint16, rows * cols))
        G = self.G = Group(hip, dA, rows, cols, xs, us)
        self.t, self.r = G.single_mvm(n), {}
        for a in A_VALUES:
            t_again, self.r[a] = G.single_fused(n, a)
            all_same(t_again, self.t, ("the two single calls", a))
            t_held, r_held = G.held(dAt, n, a)
            all_same(t_held, self.t, ("clm_f16_mvm_scale_and_add_batch on the stored transpose, t", a))
            all_same(r_held, self.r[a], ("clm_f16_mvm_scale_and_add_batch on the stored transpose, r", a))
        all_same(G.held(dAt, n), self.t, "clm_f16_mvm_batch on the stored transpose")
        for j in (0, n - 1):
            assert same16(self.t[j], rt.mvm_transposed(S.A, rows, cols, xs[j])), ("the restatement", j)
            for a in A_VALUES:
                t_cpu, r_cpu = rt.mvm_transposed_scale_and_add(S.A, rows, cols, xs[j], us[j], a)
                assert same16(self.t[j], t_cpu) and same16(self.r[a][j], r_cpu), ("the restatement, fused", j, a)
        for j in range(n):
            assert self.t[j][ZERO_COLUMN] == 0 and np.count_nonzero(self.t[j]) > cols // 2, ("the zero column is +0", j)
            assert j == 0 or not np.array_equal(self.t[j], self.t[0])


_refs = {}


def refs(hip, rt, rows, cols):  # noqa: F811
    if (rows, cols) not in _refs:
        _refs[(rows, cols)] = Refs(hip, rt, rows, cols)
    return _refs[(rows, cols)]


def check_calls(G, nvecs, env, t_ref, r_ref, variants, streaming=False):
    """every nvec on the plain call and on the fused call's `variants` (a, form) under one CLV_MVM_BATCH: the bits of the single calls
    (t_ref[j], r_ref[a][j]) and the launch counter"""
    with forced(env):
        for nvec in nvecs:
            r, launches = G.batch_mvm(nvec)
            all_same(r, t_ref[:nvec], ("plain", env, nvec))
            assert launches == want_launches(env, nvec, streaming), ("plain", env, nvec, launches)
            for a, form in variants:
                t, r, launches = G.batch_fused(nvec, a, form)
                all_same(r, r_ref[a][:nvec], ("fused r", env, nvec, a, form))
                if t is not None:
                    all_same(t, t_ref[:nvec], ("fused t", env, nvec, a, form))
                assert launches == want_launches(env, nvec, streaming), ("fused", env, nvec, a, form, launches)


FORMS = ("t", "no_t", "in_place")
ALL_VARIANTS = [(a, form) for a in A_VALUES for form in FORMS]
# every form once, both values of a
SOME_VARIANTS = [(A_VALUES[0], "t"), (A_VALUES[1], "no_t"), (A_VALUES[0], "in_place")]


@pytest.mark.parametrize("env", ENVS, ids=lambda e: f"batch={e}")
@pytest.mark.parametrize("rows,cols", BASIC, ids=lambda v: str(v))
def test_batch_equals_the_single_calls_the_restatement_and_the_held_transpose(hip, rt, rows, cols, env):  # noqa: F811
    R = refs(hip, rt, rows, cols)
    check_calls(R.G, NVECS, env, R.t, R.r, ALL_VARIANTS if env == "1" else SOME_VARIANTS)


@pytest.mark.parametrize("rows,cols", EDGES, ids=lambda v: str(v))
def test_batched_kernel_on_its_edge_shapes(hip, rt, rows, cols):  # noqa: F811
    R = refs(hip, rt, rows, cols)
    check_calls(R.G, EDGE_NVECS, "1", R.t, R.r, SOME_VARIANTS)


@pytest.mark.parametrize("kind", ["subnormal", "overflow", "negzero"])
def test_edge_values_with_the_roles_of_rows_and_columns_exchanged(hip, rt, kind):  # noqa: F811
    """the operand kinds of the row-major tests at 256 x 128: their 128 x 256 matrix is A', so A' x is their product -- f16 subnormal
    results, sums beyond 65520 (+-inf, and NaN from inf - inf in the epilogue), -0.0 from fma(+0, -1, -0)"""
    rows, cols, n = 256, 128, 8
    At, x, u = _operands(kind, cols, rows)
    A = np.ascontiguousarray(At.reshape(cols, rows).T).reshape(-1)
    xs, us = [np.roll(x, 7 * j) for j in range(n)], [np.roll(u, 2 * j) for j in range(n)]
    G = Group(hip, hip.to_device(A), rows, cols, xs, us)
    t_ref, r_ref = G.single_mvm(n), {}
    for a in SCALES:
        t_again, r_ref[a] = G.single_fused(n, a)
        all_same(t_again, t_ref, ("the two single calls", a))
    dAt = hip.to_device(At)
    all_same(G.held(dAt, n), t_ref, "clm_f16_mvm_batch on the stored transpose")
    for j in (0, n - 1):
        t_cpu = rt.mvm_transposed(A, rows, cols, xs[j])
        assert same16(t_ref[j], t_cpu) and same16(t_cpu, rt.mvm(At, cols, rows, xs[j])), (kind, j)
        r_cpu = {a: rt.scale_and_add(us[j], t_cpu, np.float32(a)) for a in SCALES}
        for a in SCALES:
            assert same16(r_ref[a][j], r_cpu[a]), (kind, j, a)
        if j == 0:
            _check_kind(kind, t_cpu, r_cpu)
    check_calls(G, EDGE_NVECS, "1", t_ref, r_ref, [(SCALES[0], "t"), (SCALES[1], "no_t"), (SCALES[2], "in_place")])


def test_the_nontemporal_instantiations(hip):
    """k_f16_mvm_t_batch<NV, true, FUSE> for NV = 2, 4 (three vectors) and 8, plain and fused, forced and under the unset rule.  The
    references are the row-major batch on the stored transpose and the single transposed calls"""
    L = hip.lib
    rows, cols = NT_SHAPE
    rng = np.random.default_rng(rows + cols + 1)
    dA, dAt = hip.to_device(big_matrix(rng, rows, cols)), hip.alloc(2 * rows * cols)
    hip.check(L.clm_f16_transpose(dA.ptr, rows, cols, dAt.ptr, None))
    n, a = 8, A_VALUES[0]
    G = Group(hip, dA, rows, cols, [vector_rows(rng, rows) for _ in range(n)], [vector_cols(rng, cols) for _ in range(n)])
    t_ref, r_ref = G.held(dAt, n, a)
    del dAt
    t_single, r_single = G.single_fused(n, a)
    all_same(t_single, t_ref, "the single transposed calls, t")
    all_same(r_single, r_ref, "the single transposed calls, r")
    assert all(np.count_nonzero(t) > cols // 2 and t[ZERO_COLUMN] == 0 for t in t_ref)
    check_calls(G, [2, 3, 8], "1", t_ref, {a: r_ref}, [(a, "t"), (a, "in_place")], streaming=True)
    check_calls(G, [2, 8], None, t_ref, {a: r_ref}, [(a, "no_t")], streaming=True)


def test_the_methods_of_the_binding(hip, rt):  # noqa: F811
    """CloverHip.mf16_mvm_transposed_batch / mf16_mvm_transposed_scale_and_add_batch: lists in, lists out, the bits of the references;
    the matrix as a host array and as an uploaded DevBuf"""
    rows, cols = 384, 640
    R = refs(hip, rt, rows, cols)
    S = case(rows, cols)
    xs, us = [x_of(rows, cols, j) for j in range(5)], [u_of(rows, cols, j) for j in range(5)]
    with forced("1"):
        all_same(hip.mf16_mvm_transposed_batch(S.A, rows, cols, xs), R.t[:5], "mf16_mvm_transposed_batch")
        all_same(hip.mf16_mvm_transposed_batch(R.G.dA, rows, cols, xs), R.t[:5], "mf16_mvm_transposed_batch on a DevBuf")
        for in_place, want_t in ((False, True), (True, False)):
            out = hip.mf16_mvm_transposed_scale_and_add_batch(R.G.dA, rows, cols, xs, us, A_VALUES[0], in_place=in_place, want_t=want_t)
            all_same([r for _, r in out], R.r[A_VALUES[0]][:5], "mf16_mvm_transposed_scale_and_add_batch")
            if want_t:
                all_same([t for t, _ in out], R.t[:5], "mf16_mvm_transposed_scale_and_add_batch t")
            else:
                assert all(np.all(t == 0xEEEE) for t, _ in out), "t was written by a call that was given none"
