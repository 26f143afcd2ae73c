"""clm8_iht_f32 and clm8_iht_f32_one_matrix (include/clover_hip_m8_f32.h) on the GPU: Q_IHT / Q_GD of <CloverMatrix8, CloverVector32> in
one call.  x, t1, t2 and t3 equal the Python composition of the five calls (tests/m8_f32_helpers.py loop_reference: m8.mvm_f32 of
tests/matrix8_helpers.py, rf.scale_and_add, the lowest-index model for FAST, rf.threshold for REFERENCE; tests/test_m8_f32_cpu.py shows
it is the same with Phi' stored and through the column walk), and the one-matrix loop equals the two-matrix loop called with
PhiT = clm8_transpose(Phi).

(m, n) from {(128, 256), (256, 384), (384, 128)}, 3 iterations, threshold 0 / 1 / 2, K = n / 8 and -- on iht_problem(..., ties=True) data
re-quantized to 8 bits -- a K at which the first cut falls among equal magnitudes; x_len = n - 64; x and the temporaries prefilled with
0x55; iterations == 0."""
import numpy as np
import pytest

from fp32_helpers import rf  # noqa: F401  (fixture)
from m8_f32_helpers import LOOP_SHAPES, loop_problem, loop_reference, same, tie_K
from matrix8_helpers import m8  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ITERS = 3


@pytest.fixture(scope="module")
def problems(m8, rf):  # noqa: F811
    """(m, n, ties) -> the problem, the restatement's transpose and K, once"""
    out = {}
    for m, n in LOOP_SHAPES:
        for ties in (False, True):
            qPhi, sPhi, y, mu = loop_problem(m8, m, n, ties)
            qT, sT = m8.transpose(qPhi, sPhi, m, n)
            K = tie_K(m8, rf, qPhi, sPhi, qT, sT, m, n, y, mu, n - 64) if ties else n // 8
            out[m, n, ties] = (qPhi, sPhi, qT, sT, y, mu, K)
    return out


@pytest.mark.parametrize("thr", [0, 1, 2], ids=["gd", "fast", "reference"])
@pytest.mark.parametrize("ties", [False, True], ids=["K=n/8", "tie"])
@pytest.mark.parametrize("m,n", LOOP_SHAPES, ids=lambda v: str(v))
def test_both_loops_equal_the_five_calls_one_by_one(hip, m8, rf, problems, m, n, ties, thr):  # noqa: F811
    qPhi, sPhi, qT, sT, y, mu, K = problems[m, n, ties]
    x_len = n - 64
    want = loop_reference(m8, rf, qPhi, sPhi, m, n, y, ITERS, K, mu, thr, x_len, lambda t2: m8.mvm_f32(qT, sT, n, m, t2))
    two = hip.m8_iht_f32(qPhi, sPhi, qT, sT, m, n, y, ITERS, K, float(mu), thr, x_len=x_len, prefill=0x55)
    dT = hip.m8_transpose(qPhi, sPhi, m, n)
    assert same(dT[0], qT) and same(dT[1], sT)
    one = hip.m8_iht_f32_one_matrix(qPhi, sPhi, m, n, y, ITERS, K, float(mu), thr, x_len=x_len, prefill=0x55)
    for k in ("x", "t1", "t2", "t3"):
        assert same(two[k], want[k]), ("two matrices", k, np.count_nonzero(two[k] != want[k]))
        assert same(one[k], two[k]), ("one matrix", k, np.count_nonzero(one[k] != two[k]))
    if thr:
        assert 0 < np.count_nonzero(want["x"][:x_len]) <= K


@pytest.mark.parametrize("m,n", LOOP_SHAPES[:2], ids=lambda v: str(v))
def test_no_iterations_clear_x_and_touch_nothing_else(hip, problems, m, n):
    qPhi, sPhi, qT, sT, y, mu, K = problems[m, n, False]
    for out in (hip.m8_iht_f32(qPhi, sPhi, qT, sT, m, n, y, 0, K, float(mu), 1, x_len=n - 64, prefill=0x55),
                hip.m8_iht_f32_one_matrix(qPhi, sPhi, m, n, y, 0, K, float(mu), 2, x_len=n - 64, prefill=0x55)):
        assert out["x"].view(np.uint8).max() == 0, "x.clear() runs over all n values"
        for k in ("t1", "t2", "t3"):
            assert np.all(out[k].view(np.uint8) == 0x55), k
