"""Every entry point of include/clover_hip_fp32.h captured once into a hipGraph and replayed on changing operands: the replay equals the
eager call bit for bit.  The calls only enqueue; what they need from the library (the stream's scratch, the hand-over slots of dot FAST)
is allocated by one ordinary call on the stream before the capture, as for the other widths.  Every call is a sequence of launches on one
stream: the graphs are linear."""
import numpy as np
import pytest

from clover_amd.lib_binding import DOT_EXACT, DOT_FAST, SIGNATURES_FP32, THRESHOLD_FAST, THRESHOLD_REFERENCE
from capture_helpers import Graph, ok
from fp32_helpers import iht_problem, make_ops, threshold_data

pytestmark = pytest.mark.gpu


N, ROWS, COLS, K = 8192 + 128, 256, 512, 700
NBIG = 16384 + 128                                                            # beyond the one-workgroup threshold
M_IHT, N_IHT = 128, 256


def _cases(hip):
    """name -> (input arrays per seed, enqueue(bufs, out, stream), output bytes)"""
    L = hip.lib

    def vec(seed):
        return make_ops("magnitudes", 1, N, seed)[:2]

    def mat(seed):
        A, x, _ = make_ops("magnitudes", ROWS, COLS, seed)
        return A, x, make_ops("magnitudes", 1, ROWS, seed + 100)[0]

    def tied(n_pad):
        return lambda seed: (threshold_data("ties", n_pad, seed),)

    def thr(mode, n_pad):
        def run(b, out, s):                                            # in place: work on a copy of the input
            hip.check(L.clv_memcpy_d2d(out.ptr, b[0].ptr, 4 * n_pad, s))
            hip.check(L.clv_f32_threshold_mode(out.ptr, n_pad - 100, n_pad, K, mode, None, s))
        return run

    def fused(b, out, s):                                              # out = [t | r2]
        hip.check(L.clm_f32_mvm_scale_and_add(b[0].ptr, ROWS, COLS, b[1].ptr, b[2].ptr, 0.37, out.ptr, out.ptr + 4 * ROWS, s))

    def problem(seed):
        return iht_problem(M_IHT, N_IHT, seed)[:3]

    def iht(threshold):
        def run(b, out, s):                                            # out = [x | t1 | t2 | t3]
            p = out.ptr
            hip.check(L.clm_f32_iht(b[0].ptr, b[1].ptr, M_IHT, N_IHT, p, N_IHT - 10, b[2].ptr, p + 4 * N_IHT, p + 4 * (N_IHT + M_IHT),
                                    p + 4 * (N_IHT + 2 * M_IHT), 3, 32, 0.5, threshold, s))
        return run

    return {
        "clv_f32_scale_and_add": (vec, lambda b, out, s: hip.check(L.clv_f32_scale_and_add(b[0].ptr, b[1].ptr, 0.37, N, out.ptr, s)), 4 * N),
        "clv_f32_dot exact": (vec, lambda b, out, s: hip.check(L.clv_f32_dot(b[0].ptr, b[1].ptr, N, DOT_EXACT, out.ptr, None, s)), 4),
        "clv_f32_dot fast": (vec, lambda b, out, s: hip.check(L.clv_f32_dot(b[0].ptr, b[1].ptr, N, DOT_FAST, out.ptr, None, s)), 4),
        "clv_f32_threshold_mode fast": (tied(N), thr(THRESHOLD_FAST, N), 4 * N),
        "clv_f32_threshold_mode fast large": (tied(NBIG), thr(THRESHOLD_FAST, NBIG), 4 * NBIG),
        "clv_f32_threshold_mode reference": (tied(N), thr(THRESHOLD_REFERENCE, N), 4 * N),
        "clm_f32_mvm": (mat, lambda b, out, s: hip.check(L.clm_f32_mvm(b[0].ptr, ROWS, COLS, b[1].ptr, out.ptr, s)), 4 * ROWS),
        "clm_f32_mvm_scale_and_add": (mat, fused, 8 * ROWS),
        "clm_f32_transpose": (mat, lambda b, out, s: hip.check(L.clm_f32_transpose(b[0].ptr, ROWS, COLS, out.ptr, s)), 4 * ROWS * COLS),
        "clm_f32_iht gd": (problem, iht(0), 8 * (M_IHT + N_IHT)),
        "clm_f32_iht fast": (problem, iht(1), 8 * (M_IHT + N_IHT)),
        "clm_f32_iht reference": (problem, iht(2), 8 * (M_IHT + N_IHT)),
    }


CASES = ["clv_f32_scale_and_add", "clv_f32_dot exact", "clv_f32_dot fast", "clv_f32_threshold_mode fast", "clv_f32_threshold_mode fast large",
         "clv_f32_threshold_mode reference", "clm_f32_mvm", "clm_f32_mvm_scale_and_add", "clm_f32_transpose", "clm_f32_iht gd", "clm_f32_iht fast",
         "clm_f32_iht reference"]


@pytest.mark.parametrize("name", CASES)
def test_captured_call_replays_to_the_eager_bits(hip, name):
    make, enqueue, nbytes = _cases(hip)[name]
    first = make(1)
    bufs = [hip.to_device(a) for a in first]
    out, eager = hip.alloc(nbytes), hip.alloc(nbytes)
    g = Graph()
    g.capture(lambda s: enqueue(bufs, out, s))
    results = []
    for rep in range(3):
        for b, a in zip(bufs, make(10 + rep)):
            b.upload(a, g.stream)
        hip.check(hip.lib.clv_memset(out.ptr, 0xA5, nbytes, g.stream))
        g.replay()
        got = out.download(np.uint8)
        enqueue(bufs, eager, g.stream)
        ok(g.rt.hipStreamSynchronize(g.stream))
        assert np.array_equal(got, eager.download(np.uint8)), (name, rep)
        results.append(got)
    assert not np.array_equal(results[0], results[1])                  # the replays did compute from the new operands
    g.close(hip.lib)                                                   # the stream's scratch goes with it


def test_the_case_list_covers_every_fp32_entry_point():
    entries = {n for n in SIGNATURES_FP32 if not n.endswith("workspace_bytes")}
    assert entries == {c.split()[0] for c in CASES}
