"""Stochastic calls inside a hipGraph (clv_rng_graph_mode).  A state in graph mode keeps its launch stamps on the device (a one-thread
tick kernel in front of every stochastic kernel), so the calls can be captured once and replayed: every replay consumes the NEXT part
of the XORShift stream -- the same nibbles as the same calls issued one after another, i.e. as the reference's sequential methods on one
object (CloverVector4.h:690-734, 1196-1478) -- checked against the oracle walking the stream."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


@pytest.mark.parametrize("n", [4096, 1 << 18])
def test_captured_stochastic_calls_walk_the_stream_on_every_replay(hip, oracle, n):
    lib = hip.lib
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * 3).astype(np.float32)
    xd = hip.to_device(x)
    q, s = hip.alloc(n // 2), hip.alloc(n // 16)
    q2, s2 = hip.alloc(n // 2), hip.alloc(n // 16)
    st = hip.new_rng(12345, 67890)
    orng = oracle.rng(12345, 67890)
    # an ordinary (host-stamped) call first: builds the generator tables outside the capture and moves the stream on
    hip.check(lib.clv4_quantize(xd.ptr, n, q.ptr, s.ptr, st.ptr, None))
    hip.sync()
    oq, osc = oracle.v4_quantize(x, orng)
    assert same(q.download(np.uint8), oq)
    hip.check(lib.clv_rng_graph_mode(st.ptr, 1, None))
    hip.sync()
    # the HIP graph API straight from the runtime the library is linked against (no torch: a second HIP runtime in the process is not needed)
    rt = C.CDLL("libamdhip64.so")
    stream, graph, gexec = C.c_void_p(), C.c_void_p(), C.c_void_p()

    def ok(rc):
        assert rc == 0, f"HIP runtime call failed: {rc}"
    ok(rt.hipStreamCreate(C.byref(stream)))
    ok(rt.hipStreamBeginCapture(stream, 0))                                       # hipStreamCaptureModeGlobal
    hip.check(lib.clv4_quantize(xd.ptr, n, q.ptr, s.ptr, st.ptr, stream))
    hip.check(lib.clv4_scale_and_add(q.ptr, s.ptr, q.ptr, s.ptr, 0.5, n, q2.ptr, s2.ptr, st.ptr, stream))
    ok(rt.hipStreamEndCapture(stream, C.byref(graph)))
    ok(rt.hipGraphInstantiate(C.byref(gexec), graph, None, None, 0))
    for rep in range(3):
        ok(rt.hipGraphLaunch(gexec, stream))
        ok(rt.hipStreamSynchronize(stream))
        oq, osc = oracle.v4_quantize(x, orng)
        o2, os2 = oracle.v4_scale_and_add(oq, osc, oq, osc, 0.5, orng)
        assert same(q.download(np.uint8), oq) and same(s.download(np.float32), osc), rep
        assert same(q2.download(np.uint8), o2) and same(s2.download(np.float32), os2), rep
    ok(rt.hipGraphExecDestroy(gexec))
    ok(rt.hipGraphDestroy(graph))
    ok(rt.hipStreamDestroy(stream))
    # the state is where 1 + 3 x 2 sequential calls leave it, and ordinary calls continue from there after leaving graph mode
    k1, k2 = hip.rng_get(st)
    ok1, ok2 = oracle.rng_keys(orng)
    assert np.array_equal(k1, ok1) and np.array_equal(k2, ok2)
    hip.check(lib.clv_rng_graph_mode(st.ptr, 0, None))
    hip.check(lib.clv4_quantize(xd.ptr, n, q.ptr, s.ptr, st.ptr, None))
    hip.sync()
    oq, _ = oracle.v4_quantize(x, orng)
    assert same(q.download(np.uint8), oq)


@pytest.mark.parametrize("n", [128, 8192, 1 << 20, (1 << 24) + 256])
def test_captured_dot_fast_replays(hip, oracle, n):
    """round 5: clv4_dot FAST is ONE launch whose workgroups hand their partials to a collector workgroup through slots that must be zero
    when the kernel starts (clv_internal_sync_slots) -- the collector clears what it read.  Captured once, replayed on changing operands:
    every replay must find clean slots and give the bits of an ordinary call (and of the two-launch form: same fixed tree)."""
    from clover_amd.lib_binding import DOT_FAST
    lib = hip.lib
    rng = np.random.default_rng(n)
    rt = C.CDLL("libamdhip64.so")
    stream, graph, gexec = C.c_void_p(), C.c_void_p(), C.c_void_p()

    def ok(rc):
        assert rc == 0, f"HIP runtime call failed: {rc}"
    ok(rt.hipStreamCreate(C.byref(stream)))
    qa, sa, qb, sb = hip.alloc(n // 2), hip.alloc(n // 16), hip.alloc(n // 2), hip.alloc(n // 16)
    out = hip.alloc(8)

    def fill(seed):
        hip.check(lib.clv_fill_random_nibbles(qa.ptr, qa.nbytes, seed, 0, stream))
        hip.check(lib.clv_fill_random_nibbles(qb.ptr, qb.nbytes, seed + 1, 0, stream))
        hip.check(lib.clv_fill_random_scales(sa.ptr, sa.nbytes // 4, seed + 2, 0, stream))
        hip.check(lib.clv_fill_random_scales(sb.ptr, sb.nbytes // 4, seed + 3, 0, stream))
    fill(1)
    # one ordinary call on this stream first: the slots and the scratch of (device, stream) are allocated outside the capture
    hip.check(lib.clv4_dot(qa.ptr, sa.ptr, qb.ptr, sb.ptr, n, DOT_FAST, out.ptr, None, stream))
    ok(rt.hipStreamSynchronize(stream))
    ok(rt.hipStreamBeginCapture(stream, 0))
    hip.check(lib.clv4_dot(qa.ptr, sa.ptr, qb.ptr, sb.ptr, n, DOT_FAST, out.ptr, None, stream))
    ok(rt.hipStreamEndCapture(stream, C.byref(graph)))
    ok(rt.hipGraphInstantiate(C.byref(gexec), graph, None, None, 0))
    for rep in range(4):
        fill(10 * rep + int(rng.integers(1, 1000)))
        ok(rt.hipGraphLaunch(gexec, stream))
        ok(rt.hipStreamSynchronize(stream))
        got = out.download(np.uint32)[0]
        hip.check(lib.clv4_dot(qa.ptr, sa.ptr, qb.ptr, sb.ptr, n, DOT_FAST, out.ptr + 4, None, stream))
        ok(rt.hipStreamSynchronize(stream))
        plain = out.download(np.uint32)[1]
        assert got == plain, (rep, hex(got), hex(plain))
        d64 = oracle.v4_dot_f64(qa.download(np.uint8), sa.download(np.float32), qb.download(np.uint8), sb.download(np.float32))
        mag = float(np.abs(np.float32(0)) + abs(d64))
        assert abs(float(np.array([got], np.uint32).view(np.float32)[0]) - d64) <= 2e-5 * max(mag, 1.0) + 2e-6 * n
    ok(rt.hipGraphExecDestroy(gexec))
    ok(rt.hipGraphDestroy(graph))
    ok(rt.hipStreamDestroy(stream))


def test_captured_matrix_stochastic_calls_walk_the_stream_on_every_replay(hip, oracle, tmp_path_factory):
    """one stochastic call of each matrix-level entry and of the 8-bit vector calls, captured into ONE linear stream on one state in
    graph mode: clm8_quantize, clm8_mvm, clm4_quantize (its public entry always has rows / 64 >= 2: the <2> strip kernel, sequence
    number in the argument list), clm4_mvm, clm4_mvm_v8, clm4_mvm_scale_and_add, clv8_quantize, clv8_scale_and_add.  Every replay gives
    the next part of the oracle's walk, and ordinary calls continue from where the replays left the state.  (The persistent one-launch
    form of clm4_iht* is not captured: its workgroups spin-wait on each other and need to be co-resident; tests/test_capture_base.py
    captures the launch-per-step loops, CLV_IHT_PERSISTENT=0.  The large-n threshold, whose middle launch is persistent too, IS captured:
    tests/test_threshold_large3.py and the first-large rows of tests/test_capture_base.py.)"""
    from conftest import random_packed
    from matrix8_helpers import build_restate
    m8 = build_restate(tmp_path_factory.getbasetemp(), parallel=False)
    lib = hip.lib
    rows, cols = 256, 512
    rng = np.random.default_rng(88)
    A = (rng.standard_normal((rows, cols)) * 2).astype(np.float32)
    q8A, s8A = m8.quantize(A)
    q4A, _ = random_packed(rng, rows * cols)
    s4A = rng.uniform(0.5, 2, size=(rows // 64) * (cols // 64)).astype(np.float32)
    (q4x, s4x), (q4u, s4u) = random_packed(rng, cols), random_packed(rng, rows)
    x = (rng.standard_normal(cols) * 3).astype(np.float32)
    q8x, s8x = oracle.v8_quantize(x)
    q8u, s8u = oracle.v8_quantize((rng.standard_normal(cols) * 3).astype(np.float32))
    d = {k: hip.to_device(v) for k, v in dict(A=A, q8A=q8A, s8A=s8A, q4A=q4A, s4A=s4A, q4x=q4x, s4x=s4x, q4u=q4u, s4u=s4u, x=x, q8x=q8x,
                                                  s8x=s8x, q8u=q8u, s8u=s8u).items()}
    n_tiles = (rows // 64) * (cols // 64)
    out = dict(m8q=(rows * cols, 4 * n_tiles), m8r=(rows, rows // 16), m4q=(rows * cols // 2, 4 * n_tiles), m4r=(rows // 2, rows // 16),
               m4r8=(rows, rows // 16), m4t=(rows // 2, rows // 16), m4sa=(rows // 2, rows // 16), v8q=(cols, cols // 16), v8sa=(cols, cols // 16))
    o = {k: (hip.alloc(a), hip.alloc(b)) for k, (a, b) in out.items()}
    st = hip.new_rng(2718, 2818)
    orng = oracle.rng(2718, 2818)

    def enqueue(stream):
        hip.check(lib.clm8_quantize(d["A"].ptr, rows, cols, o["m8q"][0].ptr, o["m8q"][1].ptr, st.ptr, stream))
        hip.check(lib.clm8_mvm(d["q8A"].ptr, d["s8A"].ptr, rows, cols, d["q8x"].ptr, d["s8x"].ptr, o["m8r"][0].ptr, o["m8r"][1].ptr, st.ptr, stream))
        hip.check(lib.clm4_quantize(d["A"].ptr, rows, cols, o["m4q"][0].ptr, o["m4q"][1].ptr, st.ptr, stream))
        hip.check(lib.clm4_mvm(d["q4A"].ptr, d["s4A"].ptr, rows, cols, d["q4x"].ptr, d["s4x"].ptr, o["m4r"][0].ptr, o["m4r"][1].ptr, st.ptr, stream))
        hip.check(lib.clm4_mvm_v8(d["q4A"].ptr, d["s4A"].ptr, rows, cols, d["q8x"].ptr, d["s8x"].ptr, o["m4r8"][0].ptr, o["m4r8"][1].ptr,
                                  st.ptr, stream))
        hip.check(lib.clm4_mvm_scale_and_add(d["q4A"].ptr, d["s4A"].ptr, rows, cols, d["q4x"].ptr, d["s4x"].ptr, d["q4u"].ptr, d["s4u"].ptr,
                                             -0.37, o["m4t"][0].ptr, o["m4t"][1].ptr, o["m4sa"][0].ptr, o["m4sa"][1].ptr, st.ptr, stream))
        hip.check(lib.clv8_quantize(d["x"].ptr, cols, o["v8q"][0].ptr, o["v8q"][1].ptr, st.ptr, stream))
        hip.check(lib.clv8_scale_and_add(d["q8u"].ptr, d["s8u"].ptr, d["q8x"].ptr, d["s8x"].ptr, 0.625, cols, o["v8sa"][0].ptr,
                                         o["v8sa"][1].ptr, st.ptr, stream))

    def check(rep):
        def got(k, dt_q):
            return o[k][0].download(dt_q), o[k][1].download(np.float32)
        want = {}
        want["m8q"] = m8.quantize(A, orng)
        want["m8r"] = m8.mvm(q8A, s8A, rows, cols, q8x, s8x, orng)
        want["m4q"] = oracle.m4_quantize(A, orng)
        want["m4r"] = oracle.m4_mvm(q4A, s4A, rows, cols, q4x, s4x, orng)
        want["m4r8"] = oracle.m4_mvm_v8(q4A, s4A, rows, cols, q8x, s8x, orng)
        want["m4t"] = oracle.m4_mvm(q4A, s4A, rows, cols, q4x, s4x, orng)
        want["m4sa"] = oracle.v4_scale_and_add(q4u, s4u, *want["m4t"], -0.37, orng)
        want["v8q"] = oracle.v8_quantize(x, orng)
        want["v8sa"] = oracle.v8_scale_and_add(q8u, s8u, q8x, s8x, 0.625, orng)
        for k, (wq, ws) in want.items():
            gq, gs = got(k, np.asarray(wq).dtype)
            assert same(gq, wq) and same(gs, ws), (rep, k)

    # ordinary (host-stamped) calls first: the generator tables and any per-stream state are built outside the capture
    enqueue(None)
    hip.sync()
    check("ordinary")
    hip.check(lib.clv_rng_graph_mode(st.ptr, 1, None))
    hip.sync()
    rt = C.CDLL("libamdhip64.so")
    stream, graph, gexec = C.c_void_p(), C.c_void_p(), C.c_void_p()

    def ok(rc):
        assert rc == 0, f"HIP runtime call failed: {rc}"
    ok(rt.hipStreamCreate(C.byref(stream)))
    ok(rt.hipStreamBeginCapture(stream, 0))
    enqueue(stream)
    ok(rt.hipStreamEndCapture(stream, C.byref(graph)))
    ok(rt.hipGraphInstantiate(C.byref(gexec), graph, None, None, 0))
    for rep in range(3):
        ok(rt.hipGraphLaunch(gexec, stream))
        ok(rt.hipStreamSynchronize(stream))
        check(rep)
    ok(rt.hipGraphExecDestroy(gexec))
    ok(rt.hipGraphDestroy(graph))
    ok(rt.hipStreamDestroy(stream))
    k1, k2 = hip.rng_get(st)
    ok1, ok2 = oracle.rng_keys(orng)
    assert np.array_equal(k1, ok1) and np.array_equal(k2, ok2)
    hip.check(lib.clv_rng_graph_mode(st.ptr, 0, None))
    enqueue(None)
    hip.sync()
    check("after")
