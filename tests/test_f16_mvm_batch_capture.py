"""The four batched half-precision calls (include/clover_hip_batch_f16.h) captured into a hipGraph and replayed on changed inputs
(tests/capture_helpers.py): the replay equals the eager call on the same inputs, bit for bit.  The calls run the batched kernel
(CLV_MVM_BATCH=1); the threshold cases are FAST within one workgroup -- no workspace, nothing to allocate under capture.  One case per
name of SIGNATURES_BATCH_F16."""
import numpy as np
import pytest

from capture_helpers import fresh_graph
from clover_amd.lib_binding import SIGNATURES_BATCH_F16, THRESHOLD_FAST
from f16_batch_helpers import MU, _iht_problem, forced, pa, same16
from half16_helpers import random_f16_bits, rh  # noqa: F401

NVEC = 5


def _bits(seed, n):
    return random_f16_bits(np.random.default_rng(seed), n, -3, 3, 0.05)


def _run(hip, inputs, outputs, sets, enqueue, keep=()):
    """inputs: device buffers the sets are uploaded into (a set = one array per buffer); outputs: buffers overwritten with 0xEE before
    every run, except those of `keep` (in/out vectors, which are inputs too).  For every set: the eager call on the default stream, then
    the replay of the graph captured on the first set -- the same bits"""
    L = hip.lib

    def load(i):
        for b, a in zip(inputs, sets[i]):
            b.upload(a)
        for b in outputs:
            if b not in keep:
                hip.check(L.clv_memset(b.ptr, 0xEE, b.nbytes, None))
        hip.sync()

    def read():
        return [b.download(np.uint16) for b in outputs]
    with forced("1"):
        g = fresh_graph(L)
        try:
            load(0)
            before = L.clv_mvm_batch_launches()
            g.capture(enqueue)
            counted = L.clv_mvm_batch_launches() - before
            eager = []
            for i in range(len(sets)):
                load(i)
                enqueue(None)
                hip.sync()
                eager.append(read())
            assert not all(np.array_equal(a, b) for a, b in zip(eager[0], eager[1])), "the sets give the same results: a replay would show nothing"
            for i in range(len(sets)):
                load(i)
                g.replay()
                for j, (got, want) in enumerate(zip(read(), eager[i])):
                    assert same16(got, want), (i, j, np.flatnonzero(got != want)[:8])
        finally:
            g.close(L)
    return counted


def _mvm_case(hip, fused):
    rows, cols = 100, 640
    dA = hip.to_device(_bits(1, rows * cols))
    dx = [hip.alloc(2 * cols) for _ in range(NVEC)]
    du = [hip.alloc(2 * rows) for _ in range(NVEC)]
    dt = [hip.alloc(2 * rows) for _ in range(NVEC)]
    dr = [hip.alloc(2 * rows) for _ in range(NVEC)]
    sets = [[_bits(10 * s + j, cols) for j in range(NVEC)] + [_bits(100 * s + j, rows) for j in range(NVEC)] for s in (1, 2, 3)]

    def enqueue(stream):
        if fused:
            hip.check(hip.lib.clm_f16_mvm_scale_and_add_batch(dA.ptr, rows, cols, NVEC, pa(dx), pa(du), -1.0, pa(dt), pa(dr), stream))
        else:
            hip.check(hip.lib.clm_f16_mvm_batch(dA.ptr, rows, cols, NVEC, pa(dx), pa(dr), stream))
    # an ordinary call and the captured one: two batched launches were counted, the replays count nothing
    assert _run(hip, dx + du, (dt + dr) if fused else dr, sets, enqueue) == 2


def _threshold_case(hip):
    n, n_pad, k = 1000, 1024, 250
    dh = [hip.alloc(2 * n_pad) for _ in range(NVEC)]
    sets = [[_bits(7 * s + j, n_pad) for j in range(NVEC)] for s in (1, 2, 3)]
    _run(hip, dh, dh, sets, lambda stream: hip.check(hip.lib.clv_f16_threshold_batch(pa(dh), NVEC, n, n_pad, k, THRESHOLD_FAST, stream)), keep=dh)


def _iht_case(hip, R):
    m, n, iters, K = 128, 256, 2, 32
    Phi, PhiT, y = _iht_problem(R, m, n)
    d = [hip.to_device(v) for v in (Phi, PhiT)]
    dy = [hip.alloc(2 * m) for _ in range(NVEC)]
    v = {k: [hip.alloc(2 * ln) for _ in range(NVEC)] for k, ln in dict(x=n, t1=m, t2=m, t3=n).items()}
    sets = [[R.scale_and_add(y, np.roll(y, s + j), np.float32(0.25 * (j + 1))) for j in range(NVEC)] for s in (1, 2, 3)]

    def enqueue(stream):
        hip.check(hip.lib.clm_f16_iht_batch(d[0].ptr, d[1].ptr, m, n, NVEC, pa(v["x"]), n, pa(dy), pa(v["t1"]), pa(v["t2"]), pa(v["t3"]), iters, K, MU,
                                            1, stream))
    assert _run(hip, dy, v["x"] + v["t1"] + v["t2"] + v["t3"], sets, enqueue) == 2 * 2 * iters


CASES = {"clm_f16_mvm_batch": lambda hip, R: _mvm_case(hip, False),
         "clm_f16_mvm_scale_and_add_batch": lambda hip, R: _mvm_case(hip, True),
         "clv_f16_threshold_batch": lambda hip, R: _threshold_case(hip),
         "clm_f16_iht_batch": _iht_case}


def test_every_entry_point_of_the_table_has_a_case():
    assert set(CASES) == set(SIGNATURES_BATCH_F16)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_captured_batch_call_replays_on_changed_inputs(hip, rh, name):  # noqa: F811
    CASES[name](hip, rh)
