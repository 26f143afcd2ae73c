"""clm_f16_iht_one_matrix (include/clover_hip_f16_t.h) on the GPU: the half-precision Q_IHT / Q_GD loop that holds ONE matrix.  x, t1, t2
and t3 equal, bit for bit, clm_f16_iht called with PhiT = clm_f16_transpose(Phi), and the loop composed call by call from the calls of
clover_hip.h on that stored transpose (clear, then per iteration the two fused calls and the threshold).  GD, the FAST and the REFERENCE
threshold; x_len = n and n - 5; three iterations; a call of 0 iterations clears x and touches nothing else.

The problem (f16_batch_helpers._iht_problem): Phi ~ U(-1, 1) / sqrt(m), y = Phi x_true for a sparse x_true, mu = 0.5: the iterates stay
finite and do not die out."""
import numpy as np
import pytest

from clover_amd.lib_binding import THRESHOLD_FAST, THRESHOLD_REFERENCE
from f16_batch_helpers import MU, _iht_problem
from f16_transposed_data import IHT_SHAPES
from f16_transposed_helpers import same
from half16_helpers import rh  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ITERS = 3
NAMES = ("x", "t1", "t2", "t3")
MODES = {"GD": 0, "FAST": 1, "REFERENCE": 2}


def composed_loop(hip, dPhi, dPhiT, m, n, y, iterations, K, mu, threshold, x_len, prefill=0x55):
    """clm_f16_iht's loop call by call from clover_hip.h on the stored transpose"""
    L = hip.lib
    dy = hip.to_device(y)
    lens = {"x": n, "t1": m, "t2": m, "t3": n}
    v = {}
    for name, ln in lens.items():
        v[name] = hip.alloc(2 * ln)
        hip.check(L.clv_memset(v[name].ptr, prefill, v[name].nbytes, None))
    v["x"] = hip.to_device(np.zeros(n, np.uint16))                        # x.clear()
    for _ in range(iterations):
        hip.check(L.clm_f16_mvm_scale_and_add(dPhi.ptr, m, n, v["x"].ptr, dy.ptr, -1.0, v["t1"].ptr, v["t2"].ptr, None))
        hip.check(L.clm_f16_mvm_scale_and_add(dPhiT.ptr, n, m, v["t2"].ptr, v["x"].ptr, mu, v["t3"].ptr, v["x"].ptr, None))
        if threshold:
            hip.check(L.clv_f16_threshold_mode(v["x"].ptr, x_len, n, K, THRESHOLD_REFERENCE if threshold == 2 else THRESHOLD_FAST, None, None))
    return {name: v[name].download(np.uint16, ln) for name, ln in lens.items()}


@pytest.mark.parametrize("short", [False, True], ids=["x_len=n", "x_len=n-5"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m,n", IHT_SHAPES, ids=lambda v: str(v))
def test_the_one_matrix_loop_equals_the_two_matrix_loop(hip, rh, m, n, mode, short):  # noqa: F811
    Phi, PhiT_cpu, y = _iht_problem(rh, m, n)
    PhiT = hip.mf16_transpose(Phi, m, n)
    assert same(PhiT, PhiT_cpu)
    x_len = n - 5 if short else n
    args = dict(iterations=ITERS, K=x_len // 8, mu=MU, threshold=MODES[mode], x_len=x_len)
    dPhi, dPhiT = hip.to_device(Phi), hip.to_device(PhiT)
    two = hip.mf16_iht(Phi, PhiT, m, n, y, **args)
    one = hip.mf16_iht_one_matrix(dPhi, m, n, y, **args)
    step = composed_loop(hip, dPhi, dPhiT, m, n, y, **args)
    for name in NAMES:
        assert same(one[name], two[name]), (name, "against clm_f16_iht with the stored transpose")
        assert same(one[name], step[name]), (name, "against the loop composed call by call")
    assert np.any(one["x"] & 0x7FFF) and np.any(one["t3"] & 0x7FFF) and not np.any(one["x"] & 0x7C00 == 0x7C00)
    if MODES[mode]:
        assert np.count_nonzero(one["x"][:x_len] & 0x7FFF) <= x_len // 8


@pytest.mark.parametrize("mode", MODES)
def test_a_call_of_no_iterations_clears_x_only(hip, rh, mode):  # noqa: F811
    m, n = IHT_SHAPES[0]
    Phi, _, y = _iht_problem(rh, m, n)
    got = hip.mf16_iht_one_matrix(Phi, m, n, y, 0, n // 8, MU, MODES[mode], prefill=0x55)
    assert not got["x"].any()
    for name in ("t1", "t2", "t3"):
        assert np.all(got[name] == 0x5555), name


def test_every_call_starts_from_a_cleared_x(hip, rh):  # noqa: F811
    """two iterations, then three on the SAME buffers: the second call equals a fresh call of three"""
    m, n = IHT_SHAPES[2]
    Phi, _, y = _iht_problem(rh, m, n)
    L = hip.lib
    dPhi, dy = hip.to_device(Phi), hip.to_device(y)
    lens = dict(x=n, t1=m, t2=m, t3=n)
    v = {k: hip.alloc(2 * ln) for k, ln in lens.items()}
    for iters in (2, 3):
        hip.check(L.clm_f16_iht_one_matrix(dPhi.ptr, m, n, v["x"].ptr, n, dy.ptr, v["t1"].ptr, v["t2"].ptr, v["t3"].ptr, iters, n // 8, MU, 1, None))
    want = hip.mf16_iht_one_matrix(dPhi, m, n, y, 3, n // 8, MU, 1)
    for k, ln in lens.items():
        assert same(v[k].download(np.uint16, ln), want[k]), k
