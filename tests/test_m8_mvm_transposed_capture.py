"""The deterministic transposed CloverMatrix8 calls and the deterministic one-matrix loop capture into a hipGraph -- nothing is allocated
during a call, one stream, no parallel branches -- and replay to the bytes of the eager call; with an rng the call behaves as clm8_mvm
does: on a state in graph mode (clv_rng_graph_mode) every replay takes the NEXT draws of the stream, which is the restatement's walk with
mvm on the stored transpose."""
import ctypes as C

import numpy as np
import pytest

from matrix8_helpers import m8  # noqa: F401  (fixture)
from test_m8_mvm_transposed import A_FUSED, C_, KEYS, eq, keys_equal, matrix, shape, vector

pytestmark = pytest.mark.gpu


def ok(rc):
    assert rc == 0, f"HIP runtime call failed: {rc}"


def fresh(hip, n):
    q, s = hip.alloc(n), hip.alloc(n // 16)
    for d in (q, s):
        hip.check(hip.lib.clv_memset(d.ptr, 0x5A, d.nbytes, None))
    return q, s


def get(pair, n):
    return pair[0].download(np.int8, n), pair[1].download(np.float32, n // 64)


@pytest.mark.parametrize("rows,cols", [(C_ + 128, 128), (384, 640)], ids=lambda v: str(v))
def test_the_deterministic_calls_capture_and_replay(hip, oracle, m8, rows, cols):  # noqa: F811
    L = hip.lib
    rt = C.CDLL("libamdhip64.so")
    S = shape(hip, oracle, m8, rows, cols)
    dx, dsx, du, dsu = (hip.to_device(v) for v in (*S.x, *S.u))
    r1, t, r2 = fresh(hip, cols), fresh(hip, cols), fresh(hip, cols)
    eager = hip.m8_mvm_transposed(S.dA, S.dsA, rows, cols, *S.x)
    eager_f = hip.m8_mvm_transposed_scale_and_add(S.dA, S.dsA, rows, cols, *S.x, *S.u, A_FUSED)
    stream, graph, gexec = C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(rt.hipStreamCreate(C.byref(stream)))
    ok(rt.hipStreamBeginCapture(stream, 0))
    hip.check(L.clm8_mvm_transposed(S.dA.ptr, S.dsA.ptr, rows, cols, dx.ptr, dsx.ptr, r1[0].ptr, r1[1].ptr, None, stream))
    hip.check(L.clm8_mvm_transposed_scale_and_add(S.dA.ptr, S.dsA.ptr, rows, cols, dx.ptr, dsx.ptr, du.ptr, dsu.ptr, A_FUSED, t[0].ptr, t[1].ptr,
                                                  r2[0].ptr, r2[1].ptr, None, stream))
    ok(rt.hipStreamEndCapture(stream, C.byref(graph)))
    ok(rt.hipGraphInstantiate(C.byref(gexec), graph, None, None, 0))
    for rep in range(2):
        for d in (*r1, *t, *r2):
            hip.check(L.clv_memset(d.ptr, 0x5A, d.nbytes, None))
        hip.sync()
        assert np.all(get(r1, cols)[0] == 0x5A)
        ok(rt.hipGraphLaunch(gexec, stream))
        ok(rt.hipStreamSynchronize(stream))
        assert eq(get(r1, cols), eager) and eq(get(r1, cols), S.cpu_t), rep
        assert eq(get(t, cols), eager_f[0:2]) and eq(get(r2, cols), eager_f[2:4]) and eq(get(r2, cols), S.cpu_r), rep
    ok(rt.hipGraphExecDestroy(gexec))
    ok(rt.hipGraphDestroy(graph))
    ok(rt.hipStreamDestroy(stream))


@pytest.mark.parametrize("threshold", [0, 1], ids=["GD", "IHT_FAST"])
def test_the_deterministic_one_matrix_loop_captures_and_replays(hip, threshold):
    L = hip.lib
    rt = C.CDLL("libamdhip64.so")
    m, n, iters = 384, 640, 3
    rng = np.random.default_rng(m * 7 + n)
    Phi = matrix(rng, m, n)
    y = vector(rng, m)
    args = dict(iterations=iters, K=n // 4, mu=0.0002, threshold=threshold, x_len=n - 5)
    eager = hip.m8_iht(*Phi, None, None, m, n, *y, **args)
    b = [hip.to_device(v) for v in (*Phi, *y)]
    lens = {"x": n, "t1": m, "t2": m, "t3": n}
    v = {k: fresh(hip, ln) for k, ln in lens.items()}
    stream, graph, gexec = C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(rt.hipStreamCreate(C.byref(stream)))
    # one ordinary call on the stream before the capture: the threshold's per-stream scratch is allocated by the first call there
    call = lambda: L.clm8_iht_one_matrix(b[0].ptr, b[1].ptr, m, n, v["x"][0].ptr, v["x"][1].ptr, n - 5, b[2].ptr, b[3].ptr, v["t1"][0].ptr,  # noqa: E731
                                         v["t1"][1].ptr, v["t2"][0].ptr, v["t2"][1].ptr, v["t3"][0].ptr, v["t3"][1].ptr, iters, n // 4, 0.0002,
                                         threshold, None, stream)
    hip.check(call())
    ok(rt.hipStreamSynchronize(stream))
    ok(rt.hipStreamBeginCapture(stream, 0))
    hip.check(call())
    ok(rt.hipStreamEndCapture(stream, C.byref(graph)))
    ok(rt.hipGraphInstantiate(C.byref(gexec), graph, None, None, 0))
    for rep in range(2):
        for pair in v.values():
            for d in pair:
                hip.check(L.clv_memset(d.ptr, 0x5A, d.nbytes, None))
        hip.sync()
        ok(rt.hipGraphLaunch(gexec, stream))
        ok(rt.hipStreamSynchronize(stream))
        for k, ln in lens.items():
            assert eq(get(v[k], ln), eager[k]), (k, rep)
    assert np.any(eager["x"][0])
    ok(rt.hipGraphExecDestroy(gexec))
    ok(rt.hipGraphDestroy(graph))
    ok(rt.hipStreamDestroy(stream))


@pytest.mark.parametrize("rows,cols", [(C_ + 128, 128), (384, 640)], ids=lambda v: str(v))
def test_a_captured_call_with_an_rng_walks_the_stream_as_clm8_mvm_does(hip, oracle, m8, rows, cols):  # noqa: F811
    L = hip.lib
    rt = C.CDLL("libamdhip64.so")
    S = shape(hip, oracle, m8, rows, cols)
    dx, dsx = hip.to_device(S.x[0]), hip.to_device(S.x[1])
    r = fresh(hip, cols)
    st, o = hip.new_rng(*KEYS), oracle.rng(*KEYS)
    # an ordinary call first: the generator tables are built outside the capture
    hip.check(L.clm8_mvm_transposed(S.dA.ptr, S.dsA.ptr, rows, cols, dx.ptr, dsx.ptr, r[0].ptr, r[1].ptr, st.ptr, None))
    hip.sync()
    assert eq(get(r, cols), m8.mvm(*S.At, cols, rows, *S.x, o))
    hip.check(L.clv_rng_graph_mode(st.ptr, 1, None))
    hip.sync()
    stream, graph, gexec = C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(rt.hipStreamCreate(C.byref(stream)))
    ok(rt.hipStreamBeginCapture(stream, 0))
    hip.check(L.clm8_mvm_transposed(S.dA.ptr, S.dsA.ptr, rows, cols, dx.ptr, dsx.ptr, r[0].ptr, r[1].ptr, st.ptr, stream))
    ok(rt.hipStreamEndCapture(stream, C.byref(graph)))
    ok(rt.hipGraphInstantiate(C.byref(gexec), graph, None, None, 0))
    for rep in range(2):
        ok(rt.hipGraphLaunch(gexec, stream))
        ok(rt.hipStreamSynchronize(stream))
        assert eq(get(r, cols), m8.mvm(*S.At, cols, rows, *S.x, o)), rep
    ok(rt.hipGraphExecDestroy(gexec))
    ok(rt.hipGraphDestroy(graph))
    ok(rt.hipStreamDestroy(stream))
    assert keys_equal(hip, st, o, oracle)
    hip.check(L.clv_rng_graph_mode(st.ptr, 0, None))
