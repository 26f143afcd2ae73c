"""Every half-precision entry point captured once into a hipGraph and replayed on changing operands: the replay equals the eager call bit
for bit.  The calls only enqueue; what they need from the library (the stream's scratch, the hand-over slots of dot FAST) is allocated by
one ordinary call on the stream before the capture, as for the other widths."""
import numpy as np
import pytest

from clover_amd.lib_binding import DOT_EXACT, DOT_FAST, THRESHOLD_FAST, THRESHOLD_REFERENCE
from capture_helpers import Graph, ok
from half16_helpers import random_f16_bits

pytestmark = pytest.mark.gpu


N, ROWS, COLS, K = 8192 + 128, 192, 512, 700


def _cases(hip):
    """name -> (input arrays per seed, enqueue(bufs, out, stream), output bytes)"""
    L = hip.lib

    def vec(seed):
        rng = np.random.default_rng(seed)
        return random_f16_bits(rng, N, -4, 4, 0.05), random_f16_bits(rng, N, -4, 4, 0.05)

    def f32vec(seed):
        return ((np.random.default_rng(seed).normal(size=N) * 3).astype(np.float32),)

    def mat(seed):
        rng = np.random.default_rng(seed)
        return random_f16_bits(rng, ROWS * COLS, -4, 4, 0.05), random_f16_bits(rng, COLS, -4, 4, 0.05)

    def mat32(seed):
        rng = np.random.default_rng(seed)
        return random_f16_bits(rng, ROWS * COLS, -4, 4, 0.05), rng.normal(size=COLS).astype(np.float32)

    def fmat(seed):
        return ((np.random.default_rng(seed).normal(size=128 * 256) * 3).astype(np.float32),)

    def tied(seed):
        rng = np.random.default_rng(seed)
        h = random_f16_bits(rng, N, -3, 3)
        h[rng.integers(0, N, size=N // 2)] = np.float16(1.5).view(np.uint16)
        return (h,)

    def thr(mode):
        def run(b, out, s):                                            # in place: work on a copy of the input
            hip.check(L.clv_memcpy_d2d(out.ptr, b[0].ptr, 2 * N, s))
            hip.check(L.clv_f16_threshold_mode(out.ptr, N - 100, N, K, mode, None, s))
        return run

    def thr_heap(b, out, s):
        hip.check(L.clv_memcpy_d2d(out.ptr, b[0].ptr, 2 * N, s))
        hip.check(L.clv_f16_threshold_heap(out.ptr, N - 100, N, K, out.ptr + 2 * N, None, s))

    return {
        "clv_f16_quantize": (f32vec, lambda b, out, s: hip.check(L.clv_f16_quantize(b[0].ptr, N, out.ptr, s)), 2 * N),
        "clv_f16_restore": (vec, lambda b, out, s: hip.check(L.clv_f16_restore(b[0].ptr, N, out.ptr, s)), 4 * N),
        "clv_f16_scale_and_add": (vec, lambda b, out, s: hip.check(L.clv_f16_scale_and_add(b[0].ptr, b[1].ptr, 0.37, N, out.ptr, s)), 2 * N),
        "clv_f16_dot exact": (vec, lambda b, out, s: hip.check(L.clv_f16_dot(b[0].ptr, b[1].ptr, N, DOT_EXACT, out.ptr, None, s)), 4),
        "clv_f16_dot fast": (vec, lambda b, out, s: hip.check(L.clv_f16_dot(b[0].ptr, b[1].ptr, N, DOT_FAST, out.ptr, None, s)), 4),
        "clv_f16_threshold_mode fast": (tied, thr(THRESHOLD_FAST), 2 * N),
        "clv_f16_threshold_mode reference": (tied, thr(THRESHOLD_REFERENCE), 2 * N),
        "clv_f16_threshold_heap": (tied, thr_heap, 2 * N + 8 * K),
        "clm_f16_quantize": (fmat, lambda b, out, s: hip.check(L.clm_f16_quantize(b[0].ptr, 128, 256, out.ptr, s)), 2 * 128 * 256),
        "clm_f16_mvm": (mat, lambda b, out, s: hip.check(L.clm_f16_mvm(b[0].ptr, ROWS, COLS, b[1].ptr, out.ptr, s)), 2 * ROWS),
        "clm_f16_mvm_f32": (mat32, lambda b, out, s: hip.check(L.clm_f16_mvm_f32(b[0].ptr, ROWS, COLS, b[1].ptr, out.ptr, s)), 4 * ROWS),
        "clm_f16_transpose": (mat, lambda b, out, s: hip.check(L.clm_f16_transpose(b[0].ptr, ROWS, COLS, out.ptr, s)), 2 * ROWS * COLS),
    }


CASES = ["clv_f16_quantize", "clv_f16_restore", "clv_f16_scale_and_add", "clv_f16_dot exact", "clv_f16_dot fast", "clv_f16_threshold_mode fast",
         "clv_f16_threshold_mode reference", "clv_f16_threshold_heap", "clm_f16_quantize", "clm_f16_mvm", "clm_f16_mvm_f32", "clm_f16_transpose"]


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


def test_the_case_list_covers_every_f16_entry_point():
    from clover_amd.lib_binding import SIGNATURES
    entries = {n for n in SIGNATURES if "_f16_" in n and not n.endswith("workspace_bytes")}
    assert entries == {c.split()[0] for c in CASES}
