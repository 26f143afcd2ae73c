"""The deterministic transposed mixed calls capture into a hipGraph -- nothing is allocated during a call, one stream, no parallel branches
-- and replay to the bytes of the eager call; with an rng the call behaves as clm4_mvm_v8 does: on a state in graph mode
(clv_rng_graph_mode) every replay takes the NEXT draws of the stream, which is the oracle's walk with m4_mvm_v8 on the stored transpose."""
import ctypes as C

import numpy as np
import pytest

from test_mvm_v8_transposed import A_FUSED, C_, KEYS, eq, keys_equal, shape

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
def test_the_deterministic_calls_capture_and_replay(hip, oracle, rows, cols):
    L = hip.lib
    rt = C.CDLL("libamdhip64.so")
    S = shape(hip, oracle, rows, cols)
    dx, dsx, du, dsu = (hip.to_device(v) for v in (*S.x, *S.u))
    r1, t, r2 = fresh(hip, cols), fresh(hip, cols), fresh(hip, cols)
    eager = hip.m4_mvm_v8_transposed(S.dA, S.dsA, rows, cols, *S.x)
    eager_f = hip.m4_mvm_v8_transposed_scale_and_add(S.dA, S.dsA, rows, cols, *S.x, *S.u, A_FUSED)
    stream, graph, gexec = C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(rt.hipStreamCreate(C.byref(stream)))
    ok(rt.hipStreamBeginCapture(stream, 0))
    hip.check(L.clm4_mvm_v8_transposed(S.dA.ptr, S.dsA.ptr, rows, cols, dx.ptr, dsx.ptr, r1[0].ptr, r1[1].ptr, None, stream))
    hip.check(L.clm4_mvm_v8_transposed_scale_and_add(S.dA.ptr, S.dsA.ptr, rows, cols, dx.ptr, dsx.ptr, du.ptr, dsu.ptr, A_FUSED, t[0].ptr, t[1].ptr,
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


@pytest.mark.parametrize("rows,cols", [(C_ + 128, 128), (384, 640)], ids=lambda v: str(v))
def test_a_captured_call_with_an_rng_walks_the_stream_as_clm4_mvm_v8_does(hip, oracle, rows, cols):
    L = hip.lib
    rt = C.CDLL("libamdhip64.so")
    S = shape(hip, oracle, rows, cols)
    dx, dsx = hip.to_device(S.x[0]), hip.to_device(S.x[1])
    r = fresh(hip, cols)
    st, o = hip.new_rng(*KEYS), oracle.rng(*KEYS)
    # an ordinary call first: the generator tables are built outside the capture
    hip.check(L.clm4_mvm_v8_transposed(S.dA.ptr, S.dsA.ptr, rows, cols, dx.ptr, dsx.ptr, r[0].ptr, r[1].ptr, st.ptr, None))
    hip.sync()
    assert eq(get(r, cols), oracle.m4_mvm_v8(*S.At, cols, rows, *S.x, o))
    hip.check(L.clv_rng_graph_mode(st.ptr, 1, None))
    hip.sync()
    stream, graph, gexec = C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(rt.hipStreamCreate(C.byref(stream)))
    ok(rt.hipStreamBeginCapture(stream, 0))
    hip.check(L.clm4_mvm_v8_transposed(S.dA.ptr, S.dsA.ptr, rows, cols, dx.ptr, dsx.ptr, r[0].ptr, r[1].ptr, st.ptr, stream))
    ok(rt.hipStreamEndCapture(stream, C.byref(graph)))
    ok(rt.hipGraphInstantiate(C.byref(gexec), graph, None, None, 0))
    for rep in range(2):
        ok(rt.hipGraphLaunch(gexec, stream))
        ok(rt.hipStreamSynchronize(stream))
        assert eq(get(r, cols), oracle.m4_mvm_v8(*S.At, cols, rows, *S.x, o)), rep
    ok(rt.hipGraphExecDestroy(gexec))
    ok(rt.hipGraphDestroy(graph))
    ok(rt.hipStreamDestroy(stream))
    assert keys_equal(hip, st, o, oracle)
    hip.check(L.clv_rng_graph_mode(st.ptr, 0, None))
