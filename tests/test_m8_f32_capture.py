"""The five calls of include/clover_hip_m8_f32.h captured into a hipGraph and replayed on changed inputs (tests/capture_helpers.py): two
replays give the bits of the CPU reference (m8.mvm_f32 on m8.transpose, rf.scale_and_add, the composed loop of
tests/m8_f32_helpers.py).  The products take no workspace and keep no state; the loops are captured as GD and with the FAST threshold
within one workgroup (n <= 16384) -- nothing to allocate under capture.  The REFERENCE threshold takes the stream's scratch: captured as a
first call on a stream it is refused with the advice clm_f32_iht's rule gives, before anything is enqueued, and the capture still ends
well.  One case per name of SIGNATURES_M8_F32."""
import numpy as np
import pytest

from capture_helpers import fresh_graph
from clover_amd.lib_binding import SIGNATURES_M8_F32
from fp32_helpers import rf  # noqa: F401  (fixture)
from m8_f32_helpers import COLS, loop_problem, loop_reference, matrix, same, vector
from matrix8_helpers import m8  # noqa: F401  (fixture)

ROWS, COLS_ = 384, COLS + 128       # twelve 32-row blocks, two workgroups
M, N, ITERS, K = 128, 256, 2, 32
A = 0.37


def _run(hip, inputs, outputs, sets, wants, enqueue, keep=()):
    """inputs: device buffers the sets are uploaded into (a set = one array per buffer); outputs: buffers overwritten with 0xEE before
    every run except those of `keep` (in/out vectors, which are inputs too).  The graph is captured on set 0 and replayed on sets 1 and 2:
    the reference bits of each"""
    L = hip.lib

    def load(i):
        for b, a in zip(inputs, sets[i]):
            b.upload(a)
        for b in outputs:
            if b not in keep:
                hip.check(L.clv_memset(b.ptr, 0xEE, b.nbytes, None))
        hip.sync()
    g = fresh_graph(L)
    try:
        load(0)
        g.capture(enqueue)
        assert not all(same(a, b) for a, b in zip(wants[1], wants[2])), "the sets give the same results: a replay would show nothing"
        for i in (1, 2):
            load(i)
            g.replay()
            for j, (b, want) in enumerate(zip(outputs, wants[i])):
                got = b.download(np.float32)
                assert same(got, want), (i, j, np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:8])
    finally:
        g.close(L)


def _product_case(hip, m8, rf, fn):  # noqa: F811
    rngs = [np.random.default_rng(s) for s in (11, 12, 13)]
    qA, sA = matrix(rngs[0], ROWS, COLS_)
    dq, ds = hip.to_device(qA), hip.to_device(sA)
    transposed = "transposed" in fn
    nin, nout = (ROWS, COLS_) if transposed else (COLS_, ROWS)
    if transposed:
        qT, sT = m8.transpose(qA, sA, ROWS, COLS_)

    def product(x):
        return m8.mvm_f32(qT, sT, COLS_, ROWS, x) if transposed else m8.mvm_f32(qA, sA, ROWS, COLS_, x)
    dx = hip.alloc(4 * nin)
    if fn == "clm8_mvm_f32_transposed":
        dr = hip.alloc(4 * nout)
        sets = [[vector(r, nin)] for r in rngs]
        wants = [[product(s[0])] for s in sets]
        _run(hip, [dx], [dr], sets, wants, lambda stream: hip.check(hip.lib.clm8_mvm_f32_transposed(dq.ptr, ds.ptr, ROWS, COLS_, dx.ptr, dr.ptr, stream)))
        return
    du, dt = hip.alloc(4 * nout), hip.alloc(4 * nout)
    sets = [[vector(r, nin), vector(r, nout)] for r in rngs]
    wants = [[product(s[0]), rf.scale_and_add(s[1], product(s[0]), A)] for s in sets]
    # in place: r2 == u, an input and an output of every run
    _run(hip, [dx, du], [dt, du], sets, wants,
         lambda stream: hip.check(getattr(hip.lib, fn)(dq.ptr, ds.ptr, ROWS, COLS_, dx.ptr, du.ptr, A, dt.ptr, du.ptr, stream)), keep=[du])


def _loop_buffers(hip, m8):
    qPhi, sPhi, y, mu = loop_problem(m8, M, N, False)
    qT, sT = m8.transpose(qPhi, sPhi, M, N)
    d = [hip.to_device(a) for a in (qPhi, sPhi, qT, sT)]
    v = {k: hip.alloc(4 * ln) for k, ln in dict(x=N, t1=M, t2=M, t3=N).items()}
    return qPhi, sPhi, qT, sT, y, mu, d, v


def _loop_call(hip, fn, d, v, dy, mu, thr, stream):
    tail = (M, N, v["x"].ptr, N - 64, dy.ptr, v["t1"].ptr, v["t2"].ptr, v["t3"].ptr, ITERS, K, float(mu), thr, stream)
    if fn == "clm8_iht_f32":
        return hip.lib.clm8_iht_f32(d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, *tail)
    return hip.lib.clm8_iht_f32_one_matrix(d[0].ptr, d[1].ptr, *tail)


def _loop_case(hip, m8, rf, fn, thr):  # noqa: F811
    qPhi, sPhi, qT, sT, y, mu, d, v = _loop_buffers(hip, m8)
    dy = hip.alloc(4 * M)
    sets = [[rf.scale_and_add(y, np.roll(y, s), 0.25 * s)] for s in (1, 2, 3)]
    wants = []
    for (ys,) in sets:
        w = loop_reference(m8, rf, qPhi, sPhi, M, N, ys, ITERS, K, mu, thr, N - 64, lambda t2: m8.mvm_f32(qT, sT, N, M, t2))
        wants.append([w[k] for k in v])
    _run(hip, [dy], list(v.values()), sets, wants, lambda stream: hip.check(_loop_call(hip, fn, d, v, dy, mu, thr, stream)))


CASES = {"clm8_mvm_f32_scale_and_add": [lambda *a: _product_case(*a, "clm8_mvm_f32_scale_and_add")],
         "clm8_mvm_f32_transposed": [lambda *a: _product_case(*a, "clm8_mvm_f32_transposed")],
         "clm8_mvm_f32_transposed_scale_and_add": [lambda *a: _product_case(*a, "clm8_mvm_f32_transposed_scale_and_add")],
         "clm8_iht_f32": [lambda *a: _loop_case(*a, "clm8_iht_f32", 0), lambda *a: _loop_case(*a, "clm8_iht_f32", 1)],                  # GD, FAST
         "clm8_iht_f32_one_matrix": [lambda *a: _loop_case(*a, "clm8_iht_f32_one_matrix", 0), lambda *a: _loop_case(*a, "clm8_iht_f32_one_matrix", 1)]}


def test_every_entry_point_of_the_table_has_a_case():
    assert set(CASES) == set(SIGNATURES_M8_F32)


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", [(n, k) for n in sorted(CASES) for k in range(len(CASES[n]))])
def test_gpu_captured_call_replays_to_the_reference_bits(hip, m8, rf, name, k):  # noqa: F811
    CASES[name][k](hip, m8, rf)


@pytest.mark.gpu
@pytest.mark.parametrize("fn", ["clm8_iht_f32", "clm8_iht_f32_one_matrix"])
def test_gpu_the_reference_threshold_loop_as_a_first_call_under_capture_is_refused_with_advice(hip, m8, rf, fn):  # noqa: F811
    """REFERENCE takes the stream's scratch (first call outside a capture, as clm_f32_iht documents): a capturing stream that has none gets
    CLV_ERR_INVALID and the advice from the threshold step before it allocates; the capture ends well, and the same call made eagerly
    afterwards gives the reference bits"""
    L = hip.lib
    qPhi, sPhi, qT, sT, y, mu, d, v = _loop_buffers(hip, m8)
    dy = hip.to_device(y)
    g = fresh_graph(L)
    try:
        g.begin()
        rc = _loop_call(hip, fn, d, v, dy, mu, 2, g.stream)
        message = L.clv_last_error().decode()
        end = g.end()
        print(fn, "REFERENCE as a first call under capture: rc", rc, "| message:", message, "| hipStreamEndCapture:", end)
        assert rc == -1, (rc, message)                                             # CLV_ERR_INVALID
        assert "before hipStreamBeginCapture" in message
        assert end == 0
        hip.check(_loop_call(hip, fn, d, v, dy, mu, 2, g.stream))
        g.sync()
        want = loop_reference(m8, rf, qPhi, sPhi, M, N, y, ITERS, K, mu, 2, N - 64, lambda t2: m8.mvm_f32(qT, sT, N, M, t2))
        for k, b in v.items():
            assert same(b.download(np.float32), want[k]), k
    finally:
        g.close(L)
