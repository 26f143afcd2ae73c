"""The four transposed half-precision calls (include/clover_hip_f16_t.h) captured into a hipGraph and replayed on changed inputs
(tests/capture_helpers.py): the replay equals the eager call on the same inputs, bit for bit.  The loop is captured as GD and with the
FAST threshold within one workgroup (n <= 32768) -- no workspace, nothing to allocate under capture.  One case per name of
SIGNATURES_F16_T."""
import numpy as np
import pytest

from capture_helpers import fresh_graph
from clover_amd.lib_binding import SIGNATURES_F16_T
from f16_batch_helpers import MU, _iht_problem
from f16_transposed_data import COLS, matrix, vector_cols, vector_rows, vector_rows_f32
from f16_transposed_helpers import same
from half16_helpers import rh  # noqa: F401  (fixture)

ROWS, COLS_ = 384, COLS + 128       # twelve 32-row blocks, two workgroups


def _run(hip, inputs, outputs, sets, enqueue, keep=()):
    """inputs: device buffers the sets are uploaded into (a set = one array per buffer); outputs: (buffer, dtype), overwritten with 0xEE
    before every run except those of `keep` (in/out vectors, which are inputs too).  For every set: the eager call on the default stream,
    then the replay of the graph captured on the first set -- the same bits"""
    L = hip.lib

    def load(i):
        for b, a in zip(inputs, sets[i]):
            b.upload(a)
        for b, _ in outputs:
            if b not in keep:
                hip.check(L.clv_memset(b.ptr, 0xEE, b.nbytes, None))
        hip.sync()

    def read():
        return [b.download(dt) for b, dt in outputs]
    g = fresh_graph(L)
    try:
        load(0)
        g.capture(enqueue)
        eager = []
        for i in range(len(sets)):
            load(i)
            enqueue(None)
            hip.sync()
            eager.append(read())
        assert not all(same(a, b) for a, b in zip(eager[0], eager[1])), "the sets give the same results: a replay would show nothing"
        for i in range(len(sets)):
            load(i)
            g.replay()
            for j, (got, want) in enumerate(zip(read(), eager[i])):
                assert same(got, want), (i, j, np.flatnonzero(got != want)[:8])
                assert not np.all(got.view(np.uint8) == 0xEE), (i, j, "the replay wrote nothing")
    finally:
        g.close(L)


def _mvt_case(hip, R, f32):
    rngs = [np.random.default_rng(s) for s in (1, 2, 3)]
    dA = hip.to_device(matrix(rngs[0], ROWS, COLS_))
    eb, dt = (4, np.float32) if f32 else (2, np.uint16)
    dx, dr = hip.alloc(eb * ROWS), hip.alloc(eb * COLS_)
    sets = [[(vector_rows_f32 if f32 else vector_rows)(r, ROWS)] for r in rngs]
    fn = hip.lib.clm_f16_mvm_f32_transposed if f32 else hip.lib.clm_f16_mvm_transposed
    _run(hip, [dx], [(dr, dt)], sets, lambda stream: hip.check(fn(dA.ptr, ROWS, COLS_, dx.ptr, dr.ptr, stream)))


def _fused_case(hip, R):
    rngs = [np.random.default_rng(s) for s in (4, 5, 6)]
    dA = hip.to_device(matrix(rngs[0], ROWS, COLS_))
    dx, du, dt = hip.alloc(2 * ROWS), hip.alloc(2 * COLS_), hip.alloc(2 * COLS_)
    sets = [[vector_rows(r, ROWS), vector_cols(r, COLS_)] for r in rngs]
    # in place: r == u, an input and an output of every run
    _run(hip, [dx, du], [(dt, np.uint16), (du, np.uint16)], sets,
         lambda stream: hip.check(hip.lib.clm_f16_mvm_transposed_scale_and_add(dA.ptr, ROWS, COLS_, dx.ptr, du.ptr, 0.37, dt.ptr, du.ptr, stream)), keep=[du])


def _iht_case(hip, R, thr):
    m, n, iters, K = 128, 256, 2, 32
    Phi, _, y = _iht_problem(R, m, n)
    dPhi, dy = hip.to_device(Phi), hip.alloc(2 * m)
    v = {k: hip.alloc(2 * ln) for k, ln in dict(x=n, t1=m, t2=m, t3=n).items()}
    sets = [[R.scale_and_add(y, np.roll(y, s), np.float32(0.25 * s))] for s in (1, 2, 3)]
    _run(hip, [dy], [(b, np.uint16) for b in v.values()], sets,
         lambda stream: hip.check(hip.lib.clm_f16_iht_one_matrix(dPhi.ptr, m, n, v["x"].ptr, n, dy.ptr, v["t1"].ptr, v["t2"].ptr, v["t3"].ptr, iters,
                                                                 K, MU, thr, stream)))


CASES = {"clm_f16_mvm_transposed": [lambda hip, R: _mvt_case(hip, R, False)],
         "clm_f16_mvm_f32_transposed": [lambda hip, R: _mvt_case(hip, R, True)],
         "clm_f16_mvm_transposed_scale_and_add": [_fused_case],
         "clm_f16_iht_one_matrix": [lambda hip, R: _iht_case(hip, R, 0), lambda hip, R: _iht_case(hip, R, 1)]}      # GD, FAST


def test_every_entry_point_of_the_table_has_a_case():
    assert set(CASES) == set(SIGNATURES_F16_T)


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", [(n, k) for n in sorted(CASES) for k in range(len(CASES[n]))])
def test_gpu_captured_transposed_call_replays_on_changed_inputs(hip, rh, name, k):  # noqa: F811
    CASES[name][k](hip, rh)
