"""The batch calls WITH a generator on the GPU: k_m4_mvm_batch<., ., ., ., ST = true> (clover_amd/csrc/mvm_batch4.hip) reads the matrix once
for a group of vectors and places every vector's draws where the sequence of single calls has them.

The reference side is never the new kernel.  It is (a) the CPU oracle run in stream order with ONE OrcRng -- oracle.m4_mvm(..., rng), then
oracle.v4_scale_and_add(..., rng) per vector -- with Oracle.rng_keys for the state, and (b) the existing single device calls (clm4_mvm,
clm4_mvm_scale_and_add, clm4_iht) on one device state.  For clm4_mvm_batch_at the generator is moved to a vector's window on the test side:
small positions by burning oracle.rng_draw, large ones by a 64 x 64 GF(2) power of the generator's step (gf2.advance_keys, checked against
burnt draws in test_mvm_batch_stochastic_cpu.py), loaded into the device state with clv_rng_set.

Shapes (G = rows / 64 row groups; C = MVMB_CHUNK): (64, 128) G = 1, windows 2 or 4 draws apart; (192, 256) G = 3, exponents that are no powers
of two, a row count that is no multiple of 128; (128, C + 128) x re-staged once; (4096, 131072 + 128) just over 256 MiB, the nontemporal
instantiation, against the single device calls only.  nvec: 2; 3 and 5 (masked slots); 8; 9 and 17 (full passes plus a remainder of 1: the
state is handed from launch to launch; forced, the remainder runs on the batched kernel too).  Vector 1 is all zero, vector 2 repeats vector 0's
pointers (test_mvm_batch.Shape).  Every case runs with CLV_MVM_BATCH=1, the first two shapes with the measured rule as well."""
import ctypes as C

import numpy as np
import pytest

import gf2
import test_guard_bands as gb
from oracle.binding import Oracle, OrcRng
from test_mvm_batch import CHUNK, KEYS, NVMAX, assert_same_vectors, batch_kernel, get, iht_data, iht_read, iht_run, pa, pairs, same, shape

SHAPES = [(64, 128), (192, 256), (128, CHUNK + 128)]
NVECS = (2, 3, 5, 8, 9, 17)
A_FUSED = 0.37


def set_state(hip, st, keys):
    hip.check(hip.lib.clv_rng_set(st.ptr, (C.c_uint64 * 4)(*[int(v) for v in keys[0]]), (C.c_uint64 * 4)(*[int(v) for v in keys[1]]), None))


def orng_at(keys):
    r = OrcRng()
    r.s0[:] = [int(v) for v in keys[0]]
    r.s1[:] = [int(v) for v in keys[1]]
    return r


def moved(oracle, keys, e):
    """the keys `e` draws further on: burnt draws where that is quick, the GF(2) power beyond"""
    if e > 4096:
        return gf2.advance_keys(keys, e)
    r = orng_at(keys)
    for _ in range(e):
        oracle.rng_draw(r)
    return Oracle.rng_keys(r)


def keys_equal(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


class Stochastic:
    """per shape, once: the oracle sequence and the single device calls for NVMAX vectors from KEYS, plain and fused, with the state after
    every vector"""

    def __init__(self, hip, oracle, rows, cols):
        L = hip.lib
        S = self.S = shape(hip, oracle, rows, cols)
        self.fresh = Oracle.rng_keys(oracle.rng(*KEYS))
        o = oracle.rng(*KEYS)
        self.o_mvm, self.o_mvm_keys = [], []
        for x in S.x:
            self.o_mvm.append(oracle.m4_mvm(S.qA, S.sA, rows, cols, *x, o))
            self.o_mvm_keys.append(Oracle.rng_keys(o))
        o = oracle.rng(*KEYS)
        self.o_t, self.o_r, self.o_fused_keys = [], [], []
        for x, u in zip(S.x, S.u):
            t = oracle.m4_mvm(S.qA, S.sA, rows, cols, *x, o)
            self.o_t.append(t)
            self.o_r.append(oracle.v4_scale_and_add(*u, *t, A_FUSED, o))
            self.o_fused_keys.append(Oracle.rng_keys(o))
        st = hip.new_rng(*KEYS)
        out = pairs(hip, NVMAX, rows)
        self.d_mvm_keys = []
        for (dq, ds), (r, sr) in zip(S.dx, out):
            hip.check(L.clm4_mvm(S.dA.ptr, S.dsA.ptr, rows, cols, dq.ptr, ds.ptr, r.ptr, sr.ptr, st.ptr, None))
            self.d_mvm_keys.append(hip.rng_get(st))
        self.d_mvm = [get(p, rows) for p in out]
        st = hip.new_rng(*KEYS)
        t, r = pairs(hip, NVMAX, rows), pairs(hip, NVMAX, rows)
        self.d_fused_keys = []
        for j in range(NVMAX):
            hip.check(L.clm4_mvm_scale_and_add(S.dA.ptr, S.dsA.ptr, rows, cols, S.dx[j][0].ptr, S.dx[j][1].ptr, S.du[j][0].ptr, S.du[j][1].ptr, A_FUSED,
                                               t[j][0].ptr, t[j][1].ptr, r[j][0].ptr, r[j][1].ptr, st.ptr, None))
            self.d_fused_keys.append(hip.rng_get(st))
        self.d_t, self.d_r = [get(p, rows) for p in t], [get(p, rows) for p in r]


_st = {}


def stochastic(hip, oracle, rows, cols):
    if (rows, cols) not in _st:
        _st[(rows, cols)] = Stochastic(hip, oracle, rows, cols)
    return _st[(rows, cols)]


def eq(p, q):
    return same(p[0], q[0]) and same(p[1], q[1])


CONTIG = [(r, c, nv, "1") for r, c in SHAPES for nv in NVECS] + [(r, c, nv, None) for r, c in SHAPES[:2] for nv in NVECS]


# ---------------------------------------------------------------- contiguous windows: the two existing calls
@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,nvec,force", CONTIG)
def test_stochastic_mvm_batch_equals_the_oracle_sequence_and_the_single_calls(hip, oracle, rows, cols, nvec, force):
    T = stochastic(hip, oracle, rows, cols)
    S = T.S
    st, out = hip.new_rng(*KEYS), pairs(hip, nvec, rows)
    with batch_kernel(force):
        hip.check(hip.lib.clm4_mvm_batch(S.dA.ptr, S.dsA.ptr, rows, cols, nvec, pa([d[0] for d in S.dx[:nvec]]), pa([d[1] for d in S.dx[:nvec]]),
                                         pa([o[0] for o in out]), pa([o[1] for o in out]), st.ptr, None))
    hip.sync()
    for j in range(nvec):
        got = get(out[j], rows)
        assert eq(T.d_mvm[j], T.o_mvm[j]), f"clm4_mvm itself differs from the oracle, vector {j}"
        assert eq(got, T.o_mvm[j]), f"vector {j} differs from the oracle sequence"
        assert eq(got, T.d_mvm[j]), f"vector {j} differs from the single calls"
    keys = hip.rng_get(st)
    assert keys_equal(keys, T.o_mvm_keys[nvec - 1]), "the state left behind differs from the oracle's"
    assert keys_equal(keys, T.d_mvm_keys[nvec - 1]), "the state left behind differs from the single calls'"
    assert not keys_equal(keys, T.fresh)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,nvec,force", CONTIG)
def test_stochastic_fused_batch_equals_the_oracle_sequence_and_the_single_calls(hip, oracle, rows, cols, nvec, force):
    """t stored, t not stored, in place: r is the same in all three"""
    T = stochastic(hip, oracle, rows, cols)
    S, L = T.S, hip.lib
    dx = S.dx[:nvec]
    for with_t, in_place in ((True, False), (False, False), (True, True)):
        u = pairs(hip, nvec, rows)
        for (wq, ws), (pq, ps) in zip(u, S.du):
            hip.check(L.clv_memcpy_d2d(wq.ptr, pq.ptr, rows // 2, None))
            hip.check(L.clv_memcpy_d2d(ws.ptr, ps.ptr, rows // 16, None))
        t = pairs(hip, nvec, rows) if with_t else None
        r = u if in_place else pairs(hip, nvec, rows)
        st = hip.new_rng(*KEYS)
        with batch_kernel(force):
            hip.check(L.clm4_mvm_scale_and_add_batch(S.dA.ptr, S.dsA.ptr, rows, cols, nvec, pa([d[0] for d in dx]), pa([d[1] for d in dx]),
                                                     pa([d[0] for d in u]), pa([d[1] for d in u]), A_FUSED, pa([d[0] for d in t]) if t else None,
                                                     pa([d[1] for d in t]) if t else None, pa([d[0] for d in r]), pa([d[1] for d in r]), st.ptr, None))
        hip.sync()
        what = f"t={with_t} in_place={in_place}"
        for j in range(nvec):
            got = get(r[j], rows)
            assert eq(got, T.o_r[j]), f"{what}: r of vector {j} against the oracle sequence"
            assert eq(got, T.d_r[j]), f"{what}: r of vector {j} against the single calls"
            if with_t:
                gt = get(t[j], rows)
                assert eq(gt, T.o_t[j]) and eq(gt, T.d_t[j]), f"{what}: t of vector {j}"
            if not in_place:
                assert eq(get(u[j], rows), S.u[j]), f"{what}: u of vector {j} was written"
        keys = hip.rng_get(st)
        assert keys_equal(keys, T.o_fused_keys[nvec - 1]) and keys_equal(keys, T.d_fused_keys[nvec - 1]), f"{what}: the state left behind"


@pytest.mark.gpu
@pytest.mark.parametrize("nvec", [3, 8])
def test_stochastic_batch_beyond_the_infinity_cache(hip, nvec):
    """4096 x (131072 + 128): just over 256 MiB, the nontemporal instantiation with ST; against the single device calls on the same buffers"""
    L = hip.lib
    rows, cols = 4096, 131072 + 128
    dA, dsA = hip.alloc(rows * cols // 2), hip.alloc((rows // 64) * (cols // 64) * 4)
    hip.check(L.clv_fill_random_nibbles(dA.ptr, dA.nbytes, 11, 0, None))
    hip.check(L.clv_fill_random_scales(dsA.ptr, dsA.nbytes // 4, 12, 0, None))
    dx, du = pairs(hip, nvec, cols), pairs(hip, nvec, rows)
    for j, ((q, s), (uq, us)) in enumerate(zip(dx, du)):
        hip.check(L.clv_fill_random_nibbles(q.ptr, q.nbytes, 100 + j, 0, None))
        hip.check(L.clv_fill_random_scales(s.ptr, s.nbytes // 4, 200 + j, 0, None))
        hip.check(L.clv_fill_random_nibbles(uq.ptr, uq.nbytes, 300 + j, 0, None))
        hip.check(L.clv_fill_random_scales(us.ptr, us.nbytes // 4, 400 + j, 0, None))
    launches = L.clv_mvm_batch_launches()
    res = []
    for batch in (False, True):
        st = hip.new_rng(*KEYS)
        r, t, r2 = pairs(hip, nvec, rows), pairs(hip, nvec, rows), pairs(hip, nvec, rows)
        if batch:
            with batch_kernel("1"):
                hip.check(L.clm4_mvm_batch(dA.ptr, dsA.ptr, rows, cols, nvec, pa([d[0] for d in dx]), pa([d[1] for d in dx]), pa([d[0] for d in r]),
                                           pa([d[1] for d in r]), st.ptr, None))
                hip.check(L.clm4_mvm_scale_and_add_batch(dA.ptr, dsA.ptr, rows, cols, nvec, pa([d[0] for d in dx]), pa([d[1] for d in dx]),
                                                         pa([d[0] for d in du]), pa([d[1] for d in du]), -1.0, pa([d[0] for d in t]), pa([d[1] for d in t]),
                                                         pa([d[0] for d in r2]), pa([d[1] for d in r2]), st.ptr, None))
        else:
            for j in range(nvec):
                hip.check(L.clm4_mvm(dA.ptr, dsA.ptr, rows, cols, dx[j][0].ptr, dx[j][1].ptr, r[j][0].ptr, r[j][1].ptr, st.ptr, None))
            for j in range(nvec):
                hip.check(L.clm4_mvm_scale_and_add(dA.ptr, dsA.ptr, rows, cols, dx[j][0].ptr, dx[j][1].ptr, du[j][0].ptr, du[j][1].ptr, -1.0, t[j][0].ptr,
                                                   t[j][1].ptr, r2[j][0].ptr, r2[j][1].ptr, st.ptr, None))
        hip.sync()
        res.append(({k: [get(p, rows) for p in v] for k, v in dict(r=r, t=t, r2=r2).items()}, hip.rng_get(st)))
    assert L.clv_mvm_batch_launches() - launches == 2
    assert_same_vectors(res[1][0], res[0][0], "beyond the cache:")
    assert keys_equal(res[1][1], res[0][1]), "the state left behind"
    assert np.any(res[0][0]["r"][0][0]) and not eq(res[0][0]["r"][0], res[0][0]["t"][0]), "the two calls drew the same noise"


# ---------------------------------------------------------------- clm4_mvm_batch_at
def at_call(hip, T, rows, cols, nvec, st, base, stride, commit):
    S = T.S
    out = pairs(hip, nvec, rows)
    rc = hip.lib.clm4_mvm_batch_at(S.dA.ptr, S.dsA.ptr, rows, cols, nvec, pa([d[0] for d in S.dx[:nvec]]), pa([d[1] for d in S.dx[:nvec]]),
                                   pa([o[0] for o in out]), pa([o[1] for o in out]), st.ptr if st else None, base, stride, commit, None)
    return rc, out


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("nvec", NVECS)
def test_batch_at_with_the_windows_of_the_contiguous_call_is_the_contiguous_call(hip, oracle, rows, cols, nvec):
    T = stochastic(hip, oracle, rows, cols)
    G = rows // 64
    st = hip.new_rng(*KEYS)
    with batch_kernel("1"):
        rc, out = at_call(hip, T, rows, cols, nvec, st, 0, 2 * G, nvec * 2 * G)
    hip.check(rc)
    hip.sync()
    for j in range(nvec):
        assert eq(get(out[j], rows), T.o_mvm[j]) and eq(get(out[j], rows), T.d_mvm[j]), j
    assert keys_equal(hip.rng_get(st), T.o_mvm_keys[nvec - 1])


def windows(G):
    """(base, stride, commit): every vector on the same draws and the state untouched; odd positions and a commit unrelated to the windows;
    bases that need the table rounds of the jump-ahead beyond 8 and beyond 16 bits, up to bit 54"""
    return [(0, 0, 0), (7, 2 * G + 3, 5), ((1 << 33) + 12345, 2 * G, (1 << 20) + 1), (1 << 54, 1, (1 << 54) + 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,force", [(r, c, "1") for r, c in SHAPES] + [(r, c, None) for r, c in SHAPES[:2]] + [(192, 256, "0")])
@pytest.mark.parametrize("nvec", [1, 3, 9])
def test_batch_at_places_every_window_where_it_is_told(hip, oracle, rows, cols, nvec, force):
    """vector j against the oracle and against clm4_mvm, each on a generator moved to base + j * stride on the test side; the state
    afterwards is the initial one moved by commit.  nvec = 1 with a non-zero base is among them.  CLV_MVM_BATCH=0 changes nothing: the
    positioned call always runs the batched kernel."""
    T = stochastic(hip, oracle, rows, cols)
    S, L = T.S, hip.lib
    for base, stride, commit in windows(rows // 64):
        st = hip.new_rng(*KEYS)
        before = L.clv_mvm_batch_launches()
        with batch_kernel(force):
            rc, out = at_call(hip, T, rows, cols, nvec, st, base, stride, commit)
        hip.check(rc)
        hip.sync()
        assert L.clv_mvm_batch_launches() - before == (nvec + 7) // 8, "the positioned call did not run the batched kernel"
        what = f"(base, stride, commit) = ({base}, {stride}, {commit})"
        assert keys_equal(hip.rng_get(st), moved(oracle, T.fresh, commit)), f"{what}: the state left behind"
        one, single = hip.new_rng(*KEYS), pairs(hip, 1, rows)[0]
        for j in range(nvec):
            at = moved(oracle, T.fresh, base + j * stride)
            want = oracle.m4_mvm(S.qA, S.sA, rows, cols, *S.x[j], orng_at(at))
            set_state(hip, one, at)
            hip.check(L.clm4_mvm(S.dA.ptr, S.dsA.ptr, rows, cols, S.dx[j][0].ptr, S.dx[j][1].ptr, single[0].ptr, single[1].ptr, one.ptr, None))
            hip.sync()
            got = get(out[j], rows)
            assert eq(got, want), f"{what}: vector {j} against the oracle at its window"
            assert eq(got, get(single, rows)), f"{what}: vector {j} against clm4_mvm at its window"
            if (base, stride) == (0, 0):
                assert eq(got, T.o_mvm[0]) or j, "stride 0: vector 0 is the first single call from the fresh state"


@pytest.mark.gpu
def test_batch_at_without_a_generator_is_the_deterministic_call_and_a_position_beyond_the_tables_is_refused(hip, oracle):
    rows, cols, nvec = 192, 256, 5
    T = stochastic(hip, oracle, rows, cols)
    rc, out = at_call(hip, T, rows, cols, nvec, None, 1 << 60, 1 << 60, 1 << 60)      # ignored without an rng
    hip.check(rc)
    hip.sync()
    for j in range(nvec):
        assert eq(get(out[j], rows), T.S.single[j]), j
    st = hip.new_rng(*KEYS)
    before = hip.lib.clv_mvm_batch_launches()
    for base, stride, commit in (((1 << 55) - 5, 0, 0), (0, 1 << 53, 0), (0, 6, 1 << 55), ((1 << 64) - 1, (1 << 64) - 1, 0)):
        rc, out = at_call(hip, T, rows, cols, nvec, st, base, stride, commit)
        assert rc == -1 and b"clm4_mvm_batch_at" in hip.lib.clv_last_error() and b"2^55" in hip.lib.clv_last_error(), (base, stride, commit)
        hip.sync()
        assert all(np.all(get(o, rows)[0] == 0x5A) for o in out), "a refused call wrote a result"
    assert hip.lib.clv_mvm_batch_launches() == before, "a refused call launched"
    assert keys_equal(hip.rng_get(st), T.fresh)


# ---------------------------------------------------------------- the launch counter
@pytest.mark.gpu
def test_the_launch_counter_sees_the_one_pass_kernel(hip, oracle):
    """17 vectors with a generator under CLV_MVM_BATCH=1: launches for 8, 8 and 1 vectors (forced, the remainder of one runs on the batched
    kernel too, so that every hand-over of the state is from one batched launch to the next); under CLV_MVM_BATCH=0 none"""
    rows, cols, nvec = 192, 256, 17
    T = stochastic(hip, oracle, rows, cols)
    S, L = T.S, hip.lib
    for force, want in (("1", 3), ("0", 0)):
        st, out = hip.new_rng(*KEYS), pairs(hip, nvec, rows)
        before = L.clv_mvm_batch_launches()
        with batch_kernel(force):
            hip.check(L.clm4_mvm_batch(S.dA.ptr, S.dsA.ptr, rows, cols, nvec, pa([d[0] for d in S.dx[:nvec]]), pa([d[1] for d in S.dx[:nvec]]),
                                       pa([o[0] for o in out]), pa([o[1] for o in out]), st.ptr, None))
        hip.sync()
        assert L.clv_mvm_batch_launches() - before == want, force
        assert keys_equal(hip.rng_get(st), T.o_mvm_keys[nvec - 1])
        assert all(eq(get(out[j], rows), T.o_mvm[j]) for j in range(nvec))


# ---------------------------------------------------------------- IHT / GD with a generator
@pytest.mark.gpu
@pytest.mark.parametrize("m,n", [(128, 256), (256, 384), (384, 256)])
@pytest.mark.parametrize("nvec", [2, 5, 8, 9])
def test_stochastic_iht_batch_equals_clm4_iht_per_vector_in_order(hip, oracle, m, n, nvec):
    """three iterations, thresholds none / FAST / REFERENCE, CLV_MVM_BATCH=1: x, t1 .. t3 and the state equal clm4_iht for vector 0, then
    1, ... on one state.  nvec = 5, one group: 2 batched launches per iteration.  Also with the measured rule (nvec = 8 is the full group it
    batches where a single call takes the persistent kernel)."""
    mats, dy = iht_data(hip, oracle, m, n, nvec)
    L = hip.lib
    for thr in (0, 1, 2):
        st1 = hip.new_rng(*KEYS)
        v1, lens = iht_run(hip, mats, dy, m, n, thr, batch=False, rng=st1)
        hip.sync()
        one, keys1 = iht_read(v1, lens), hip.rng_get(st1)
        for force in ("1", None):                                            # None: the measured rule, whatever it picks per group
            st2 = hip.new_rng(*KEYS)
            before = L.clv_mvm_batch_launches()
            with batch_kernel(force):
                v2, _ = iht_run(hip, mats, dy, m, n, thr, batch=True, rng=st2)
            hip.sync()
            if nvec == 5 and force:
                assert L.clv_mvm_batch_launches() - before == 6
            assert_same_vectors(iht_read(v2, lens), one, f"threshold={thr} CLV_MVM_BATCH={force}:")
            assert keys_equal(hip.rng_get(st2), keys1), f"threshold={thr} CLV_MVM_BATCH={force}: the state left behind"
        assert any(np.any(x[0]) for x in one["x"]), "the loop left every x zero: the comparison shows nothing"
        assert not keys_equal(keys1, Oracle.rng_keys(oracle.rng(*KEYS)))
    st = hip.new_rng(*KEYS)
    with batch_kernel("1"):
        iht_run(hip, mats, dy, m, n, 1, batch=True, rng=st, iters=0)
    hip.sync()
    assert keys_equal(hip.rng_get(st), Oracle.rng_keys(oracle.rng(*KEYS))), "no iterations: nothing drawn, nothing committed"


# ---------------------------------------------------------------- graph capture
@pytest.mark.gpu
def test_a_stochastic_batch_call_captures_into_a_graph_when_the_state_is_in_graph_mode(hip, oracle):
    """clm4_mvm_batch, nvec = 5, captured once after a warm-up call and replayed twice on changed inputs: every replay equals the eager
    single calls that continue the same stream on a second state"""
    L = hip.lib
    rt = C.CDLL("libamdhip64.so")
    stream, graph, gexec = C.c_void_p(), C.c_void_p(), C.c_void_p()

    def ok(rc):
        assert rc == 0, f"HIP runtime call failed: {rc}"
    rows, cols, nvec = 192, 256, 5
    S = shape(hip, oracle, rows, cols)
    dx, out = pairs(hip, nvec, cols), pairs(hip, nvec, rows)
    captured, eager = hip.new_rng(*KEYS), hip.new_rng(*KEYS)

    def fill(seed):
        for j, (q, s) in enumerate(dx):
            hip.check(L.clv_fill_random_nibbles(q.ptr, q.nbytes, seed + 2 * j, 0, None))
            hip.check(L.clv_fill_random_scales(s.ptr, s.nbytes // 4, seed + 2 * j + 1, 0, None))
        hip.sync()

    def enqueue(st):
        hip.check(L.clm4_mvm_batch(S.dA.ptr, S.dsA.ptr, rows, cols, nvec, pa([d[0] for d in dx]), pa([d[1] for d in dx]), pa([o[0] for o in out]),
                                   pa([o[1] for o in out]), captured.ptr, st))

    def singles():
        want = pairs(hip, nvec, rows)
        for j in range(nvec):
            hip.check(L.clm4_mvm(S.dA.ptr, S.dsA.ptr, rows, cols, dx[j][0].ptr, dx[j][1].ptr, want[j][0].ptr, want[j][1].ptr, eager.ptr, None))
        hip.sync()
        return [get(p, rows) for p in want]

    with batch_kernel("1"):
        fill(1)
        ok(rt.hipStreamCreate(C.byref(stream)))
        hip.check(L.clv_rng_graph_mode(captured.ptr, 1, stream))
        enqueue(stream)                                                     # warm-up outside the capture
        ok(rt.hipStreamSynchronize(stream))
        want = singles()
        assert all(eq(get(o, rows), w) for o, w in zip(out, want)), "the warm-up call"
        ok(rt.hipStreamBeginCapture(stream, 0))
        enqueue(stream)
        ok(rt.hipStreamEndCapture(stream, C.byref(graph)))
        ok(rt.hipGraphInstantiate(C.byref(gexec), graph, None, None, 0))
        seen = []
        for rep in range(2):
            fill(50 + 10 * rep)
            ok(rt.hipGraphLaunch(gexec, stream))
            ok(rt.hipStreamSynchronize(stream))
            got, want = [get(o, rows) for o in out], singles()
            for j in range(nvec):
                assert eq(got[j], want[j]), f"replay {rep}: vector {j}"
            seen.append(got)
        assert not eq(seen[0][0], seen[1][0]), "the replays saw the same inputs"
        hip.check(L.clv_rng_graph_mode(captured.ptr, 0, stream))
        assert keys_equal(hip.rng_get(captured), hip.rng_get(eager)), "the state after two replays"
        ok(rt.hipGraphExecDestroy(gexec))
        ok(rt.hipGraphDestroy(graph))
        ok(rt.hipStreamDestroy(stream))


# ---------------------------------------------------------------- guard bands: the two new entry points in test_guard_bands' table
GB_ENV = {"CLV_MVM_BATCH": "1"}


def _gb_at(rows, cols, nvec, st):
    """deterministic: the positions are ignored; stochastic: windows at 3 + j (2 G + 1), the state moved by 5"""
    def build(R):
        orc = R.oracle
        G = rows // 64
        base, stride, commit = (3, 2 * G + 1, 5) if st else (1 << 60, 1 << 60, 1 << 60)
        qA, sA = gb.m4(rows * cols + 61, rows, cols)
        regs, want = [("A", "input", qA), ("sA", "input", sA)] + ([("rng", "state", None)] if st else []), {}
        for j in range(nvec):
            qx, sx = gb.v4(cols + 70 + j, cols)
            o = None
            if st:
                o = orc.rng(*gb.KEYS)
                for _ in range(base + j * stride):
                    orc.rng_draw(o)
            r = orc.m4_mvm(qA, sA, rows, cols, qx, sx, o)
            regs += [(f"x{j}", "input", qx), (f"sx{j}", "input", sx), (f"r{j}", "output", rows // 2), (f"sr{j}", "output", rows // 16)]
            want.update({f"r{j}": r[0], f"sr{j}": r[1]})
        after = None
        if st:
            after = orc.rng(*gb.KEYS)
            for _ in range(commit):
                orc.rng_draw(after)

        def call(L, p):
            a = lambda name: pa([p[f"{name}{j}"] for j in range(nvec)])  # noqa: E731
            return L.clm4_mvm_batch_at(p["A"], p["sA"], rows, cols, nvec, a("x"), a("sx"), a("r"), a("sr"), p.get("rng"), base, stride, commit, None)
        return gb.Case(regs, call, want, orng=after, env=GB_ENV)
    return build


def _gb_counter(rows, cols, nvec):
    """the counter is read around a stochastic clm4_mvm_batch in the arena: one more batched launch, the call's ranges and nothing else"""
    def build(R):
        orc = R.oracle
        qA, sA = gb.m4(rows * cols + 62, rows, cols)
        regs, want, o = [("A", "input", qA), ("sA", "input", sA), ("rng", "state", None)], {}, orc.rng(*gb.KEYS)
        for j in range(nvec):
            qx, sx = gb.v4(cols + 80 + j, cols)
            r = orc.m4_mvm(qA, sA, rows, cols, qx, sx, o)
            regs += [(f"x{j}", "input", qx), (f"sx{j}", "input", sx), (f"r{j}", "output", rows // 2), (f"sr{j}", "output", rows // 16)]
            want.update({f"r{j}": r[0], f"sr{j}": r[1]})

        def call(L, p):
            a = lambda name: pa([p[f"{name}{j}"] for j in range(nvec)])  # noqa: E731
            before = L.clv_mvm_batch_launches()
            rc = L.clm4_mvm_batch(p["A"], p["sA"], rows, cols, nvec, a("x"), a("sx"), a("r"), a("sr"), p["rng"], None)
            assert L.clv_mvm_batch_launches() - before == 1, "the call did not take the batched kernel"
            return rc
        return gb.Case(regs, call, want, orng=o, env=GB_ENV)
    return build


ST_CASES = [("clm4_mvm_batch_at 192x640 nvec=3 rounding disabled", _gb_at(192, 640, 3, False)),
            ("clm4_mvm_batch_at 192x640 nvec=3 stochastic", _gb_at(192, 640, 3, True)),
            (f"clm4_mvm_batch_at 64x{CHUNK + 128} nvec=9 stochastic", _gb_at(64, CHUNK + 128, 9, True)),
            ("clv_mvm_batch_launches around a stochastic clm4_mvm_batch 192x640 nvec=5", _gb_counter(192, 640, 5))]
for _name, _build in ST_CASES:
    if _name not in gb.CASES:                 # the coverage test of test_guard_bands.py reads its table when it runs, after every module is imported
        gb.case(_name)(_build)


@pytest.fixture(scope="module")
def refs(oracle):
    return gb.Refs(oracle, None, None)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, _ in ST_CASES])
def test_the_new_calls_write_their_outputs_and_nothing_else(hip, refs, name):
    gb.run_case(hip, dict(ST_CASES)[name](refs))
