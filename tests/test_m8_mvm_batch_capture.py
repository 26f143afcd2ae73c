"""A deterministic clm8_mvm_scale_and_add_batch captures into a hipGraph: no pointer table on the device, nothing allocated during the
call.  nvec = 8 (a full pass) on a shape of more than one LDS chunk; captured once after a warm-up call outside the capture, replayed twice
with the outputs cleared in between; every replay equals the eager single calls and the CPU."""
import ctypes as C

import numpy as np
import pytest

from matrix8_helpers import m8  # noqa: F401
from test_m8_mvm_batch import CHUNK, eq, get8, pairs8, shape
from test_mvm_batch import batch_kernel, pa


@pytest.mark.gpu
def test_the_fused_m8_batch_call_captures_into_a_graph(hip, m8, oracle):  # noqa: F811
    L = hip.lib
    rt = C.CDLL("libamdhip64.so")
    stream, graph, gexec = C.c_void_p(), C.c_void_p(), C.c_void_p()

    def ok(rc):
        assert rc == 0, f"HIP runtime call failed: {rc}"
    rows, cols, nvec = 64, CHUNK + 128, 8
    S = shape(hip, m8, rows, cols)
    du = S.du[:nvec]
    t, r = pairs8(hip, nvec, rows), pairs8(hip, nvec, rows)
    want_t = S.cpu[:nvec]
    want_r = [oracle.v8_scale_and_add(*S.u[j], *S.cpu[j], -1.0) for j in range(nvec)]
    wt, wr = pairs8(hip, nvec, rows), pairs8(hip, nvec, rows)
    for j in range(nvec):
        hip.check(L.clm8_mvm_scale_and_add(S.dA.ptr, S.dsA.ptr, rows, cols, S.dx[j][0].ptr, S.dx[j][1].ptr, du[j][0].ptr, du[j][1].ptr, -1.0,
                                           wt[j][0].ptr, wt[j][1].ptr, wr[j][0].ptr, wr[j][1].ptr, None, None))
    hip.sync()
    single_t, single_r = [get8(p, rows) for p in wt], [get8(p, rows) for p in wr]

    def enqueue(st):
        hip.check(L.clm8_mvm_scale_and_add_batch(S.dA.ptr, S.dsA.ptr, rows, cols, nvec, *S.xs(nvec), pa([d[0] for d in du]), pa([d[1] for d in du]),
                                                 -1.0, pa([d[0] for d in t]), pa([d[1] for d in t]), pa([d[0] for d in r]), pa([d[1] for d in r]),
                                                 None, st))

    def clear():
        for q, s in t + r:
            hip.check(L.clv_memset(q.ptr, 0x5A, rows, None))
            hip.check(L.clv_memset(s.ptr, 0x5A, rows // 16, None))
        hip.sync()
        assert np.all(get8(r[0], rows)[0] == 0x5A)

    def check(what):
        for j in range(nvec):
            gt, gr = get8(t[j], rows), get8(r[j], rows)
            assert eq(gt, single_t[j]) and eq(gr, single_r[j]), f"{what}: vector {j} against the single calls"
            assert eq(gt, want_t[j]) and eq(gr, want_r[j]), f"{what}: vector {j} against the CPU"

    with batch_kernel("1"):
        ok(rt.hipStreamCreate(C.byref(stream)))
        enqueue(stream)                                                     # warm-up outside the capture
        ok(rt.hipStreamSynchronize(stream))
        check("the warm-up call")
        before = L.clv_mvm_batch_launches()
        ok(rt.hipStreamBeginCapture(stream, 0))
        enqueue(stream)
        ok(rt.hipStreamEndCapture(stream, C.byref(graph)))
        assert L.clv_mvm_batch_launches() - before == 1, "the captured call did not take the batched kernel"
        ok(rt.hipGraphInstantiate(C.byref(gexec), graph, None, None, 0))
        for rep in range(2):
            clear()
            ok(rt.hipGraphLaunch(gexec, stream))
            ok(rt.hipStreamSynchronize(stream))
            check(f"replay {rep}")
        ok(rt.hipGraphExecDestroy(gexec))
        ok(rt.hipGraphDestroy(graph))
        ok(rt.hipStreamDestroy(stream))
