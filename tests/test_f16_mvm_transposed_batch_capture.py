"""The three batched transposed half-precision calls (include/clover_hip_batch_f16_t.h) captured into a hipGraph and replayed on changed
inputs (tests/capture_helpers.py): the replay equals the eager call on the same inputs, bit for bit.  The calls run the batched kernel
(CLV_MVM_BATCH=1, five vectors: a partly filled group).  The loop is captured where clm_f16_iht_batch captures: as GD and with the FAST
threshold within one workgroup (n <= 32768) -- no workspace, nothing to allocate under capture.  One case per name of
SIGNATURES_BATCH_F16_T."""
import numpy as np
import pytest

from capture_helpers import fresh_graph
from clover_amd.lib_binding import SIGNATURES_BATCH_F16_T
from f16_batch_helpers import MU, _iht_problem, forced, pa, same16
from f16_transposed_batch_data import WIDTHS
from f16_transposed_data import matrix, vector_cols, vector_rows
from half16_helpers import rh  # noqa: F401  (fixture)

NVEC = 5
ROWS, COLS_ = 384, max(WIDTHS) + 128        # twelve 32-row blocks, two workgroups or more


def _run(hip, inputs, outputs, sets, enqueue, keep=()):
    """inputs: device buffers the sets are uploaded into (a set = one array per buffer); outputs: buffers overwritten with 0xEE before
    every run, except those of `keep` (in/out vectors, which are inputs too).  For every set: the eager call on the default stream, then
    the replay of the graph captured on the first set -- the same bits.  Returns the batched launches counted by fresh_graph's capture
    (an ordinary call, then the recorded one)"""
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
                    assert not np.all(got == 0xEEEE), (i, j, "the replay wrote nothing")
        finally:
            g.close(L)
    return counted


def _mvm_case(hip, R, fused):
    rngs = [np.random.default_rng(s) for s in (11, 12, 13)]
    dA = hip.to_device(matrix(rngs[0], ROWS, COLS_))
    dx = [hip.alloc(2 * ROWS) for _ in range(NVEC)]
    du = [hip.alloc(2 * COLS_) for _ in range(NVEC)]
    dt = [hip.alloc(2 * COLS_) for _ in range(NVEC)]
    sets = [[vector_rows(r, ROWS) for _ in range(NVEC)] + [vector_cols(r, COLS_) for _ in range(NVEC)] for r in rngs]

    def enqueue(stream):
        if fused:       # in place: r[j] == u[j], an input and an output of every run
            hip.check(hip.lib.clm_f16_mvm_transposed_scale_and_add_batch(dA.ptr, ROWS, COLS_, NVEC, pa(dx), pa(du), 0.37, pa(dt), pa(du), stream))
        else:
            hip.check(hip.lib.clm_f16_mvm_transposed_batch(dA.ptr, ROWS, COLS_, NVEC, pa(dx), pa(dt), stream))
    # an ordinary call and the captured one: two batched launches were counted, the replays count nothing
    assert _run(hip, dx + du, (dt + du) if fused else dt, sets, enqueue, keep=du if fused else ()) == 2


def _iht_case(hip, R, thr):
    m, n, iters, K = 128, 256, 2, 32
    Phi, _, y = _iht_problem(R, m, n)
    dPhi = hip.to_device(Phi)
    dy = [hip.alloc(2 * m) for _ in range(NVEC)]
    v = {k: [hip.alloc(2 * ln) for _ in range(NVEC)] for k, ln in dict(x=n, t1=m, t2=m, t3=n).items()}
    sets = [[R.scale_and_add(y, np.roll(y, s + j), np.float32(0.25 * (j + 1))) for j in range(NVEC)] for s in (1, 2, 3)]

    def enqueue(stream):
        hip.check(hip.lib.clm_f16_iht_batch_one_matrix(dPhi.ptr, m, n, NVEC, pa(v["x"]), n, pa(dy), pa(v["t1"]), pa(v["t2"]), pa(v["t3"]), iters, K,
                                                       MU, thr, stream))
    assert _run(hip, dy, v["x"] + v["t1"] + v["t2"] + v["t3"], sets, enqueue) == 2 * 2 * iters


CASES = {"clm_f16_mvm_transposed_batch": [lambda hip, R: _mvm_case(hip, R, False)],
         "clm_f16_mvm_transposed_scale_and_add_batch": [lambda hip, R: _mvm_case(hip, R, True)],
         "clm_f16_iht_batch_one_matrix": [lambda hip, R: _iht_case(hip, R, 0), lambda hip, R: _iht_case(hip, R, 1)]}      # GD, FAST


def test_every_entry_point_of_the_table_has_a_case():
    assert set(CASES) == set(SIGNATURES_BATCH_F16_T)


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", [(n, k) for n in sorted(CASES) for k in range(len(CASES[n]))])
def test_gpu_captured_batched_transposed_call_replays_on_changed_inputs(hip, rh, name, k):  # noqa: F811
    CASES[name][k](hip, rh)
