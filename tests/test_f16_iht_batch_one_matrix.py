"""clm_f16_iht_batch_one_matrix (include/clover_hip_batch_f16_t.h) on the GPU: the half-precision Q_IHT / Q_GD loop for several signals
that holds ONE matrix -- per iteration and group t1 = Phi x, t2 = y - t1 as one row-major batched launch and t3 = Phi' t2, x += mu t3 as one
batched transposed launch on the same Phi.  x, t1, t2 and t3 of every signal equal, bit for bit, three references that are not the new
code: clm_f16_iht_one_matrix on that signal, clm_f16_iht_batch with a stored transpose, and (first and last signal) the CPU loop over the
restatement with the column walk of tests/half16_t_restate.c for Phi' t2.  x is cleared on every call; the batched launches are counted
per iteration and group."""
import numpy as np
import pytest

from f16_batch_helpers import IHT_SHAPES, MU, _iht_problem, _modes, forced, pa, same16
from f16_transposed_helpers import rt  # noqa: F401  (fixture)
from test_f16_mvm_transposed_batch import UNSET_MIN_GROUP
from test_half16 import lowest_index_threshold

pytestmark = pytest.mark.gpu

ITERS = (0, 1, 3)
NVECS = (3, 9)
NAMES = ("x", "t1", "t2", "t3")
_LOOPS = {}


def _signals(R, m, n, count):
    """Phi, its transpose and `count` measurements that differ from one another: y_j = f16(y + 0.25 j roll(y, j))"""
    Phi, PhiT, y = _iht_problem(R, m, n)
    return Phi, PhiT, [y if j == 0 else R.scale_and_add(y, np.roll(y, j), np.float32(0.25 * j)) for j in range(count)]


def _cpu_loop(R, m, n, x_len, K, thr, j, iters):
    """the loop over the restatement for signal j with ONE matrix (Phi' t2 by the column walk), computed once per case"""
    key = (m, n, x_len, K, thr, j)
    if key not in _LOOPS:
        Phi, _, ys = _signals(R, m, n, max(NVECS))
        x, out = np.zeros(n, np.uint16), {0: dict(x=np.zeros(n, np.uint16))}
        for it in range(1, max(ITERS) + 1):
            t1 = R.mvm(Phi, m, n, x)
            t2 = R.scale_and_add(ys[j], t1, np.float32(-1.0))
            t3 = R.mvm_transposed(Phi, m, n, t2)
            x = R.scale_and_add(x, t3, np.float32(MU))
            if thr:
                x = R.threshold(x, x_len, K) if thr == 2 else lowest_index_threshold(x, x_len, K)
            out[it] = dict(x=x, t1=t1, t2=t2, t3=t3)
        _LOOPS[key] = out
    return _LOOPS[key][iters]


def want_groups(env, nvec):
    """groups of a call that run batched: forced all (a remainder group of one too), forwarded none, unset the measured rule of the
    cache-resident class (these matrices are far below 256 MiB)"""
    if env == "0":
        return 0
    if env == "1":
        return (nvec + 7) // 8
    g_min = UNSET_MIN_GROUP["resident"]
    return 0 if g_min is None else nvec // 8 * (8 >= g_min) + (nvec % 8 >= g_min)


@pytest.mark.parametrize("mode", range(3), ids=["gd", "fast", "reference"])
@pytest.mark.parametrize("shape", IHT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_batch_one_matrix_equals_the_single_loop_the_held_transpose_and_the_cpu_loop(hip, rt, shape, mode):  # noqa: F811
    m, n, x_len = shape
    name, thr, K = _modes(x_len)[mode]
    Phi, PhiT, ys = _signals(rt, m, n, max(NVECS))
    dPhi, dPhiT = hip.to_device(Phi), hip.to_device(PhiT)
    L = hip.lib
    for iters in ITERS:
        single = [hip.mf16_iht_one_matrix(dPhi, m, n, y, iters, K, MU, thr, x_len=x_len, prefill=0x55) for y in ys]
        with forced("1"):
            held = hip.mf16_iht_batch(dPhi, dPhiT, m, n, ys, iters, K, MU, thr, x_len=x_len, prefill=0x55)
        for j in range(max(NVECS)):
            for k in NAMES:
                assert same16(single[j][k], held[j][k]), (name, iters, j, k, "clm_f16_iht_batch with the stored transpose")
        for j in (0, max(NVECS) - 1):                                # the CPU loop for the first and the last signal
            for k in NAMES:
                if iters or k == "x":
                    assert same16(single[j][k], _cpu_loop(rt, m, n, x_len, K, thr, j, iters)[k]), (name, iters, j, k, "cpu")
        for nvec in NVECS:
            for env in ("1", "0", None):
                with forced(env):
                    before = L.clv_mvm_batch_launches()
                    got = hip.mf16_iht_batch_one_matrix(dPhi, m, n, ys[:nvec], iters, K, MU, thr, x_len=x_len, prefill=0x55)
                    launches = L.clv_mvm_batch_launches() - before
                assert launches == 2 * iters * want_groups(env, nvec), (name, iters, nvec, env, launches)
                for j in range(nvec):
                    for k in NAMES:
                        if iters == 0 and k != "x":
                            assert np.all(got[j][k] == 0x5555), (name, nvec, env, j, k)      # untouched: the prefill
                        else:
                            assert same16(got[j][k], single[j][k]), (name, iters, nvec, env, j, k, np.flatnonzero(got[j][k] != single[j][k])[:8])
                    if iters == 0:
                        assert not got[j]["x"].any()
        if iters == max(ITERS):
            assert all(np.any(s["x"] & 0x7FFF) and np.any(s["t3"] & 0x7FFF) for s in single), "the iterates do not die out"


@pytest.mark.parametrize("mode", range(3), ids=["gd", "fast", "reference"])
def test_batch_one_matrix_clears_x_on_every_call(hip, rt, mode):  # noqa: F811
    """two iterations, then three, then none on the SAME buffers: every call starts from x = 0, so each equals the single call of its own
    iteration count; a call of 0 iterations clears every x and leaves t1..t3 as they were"""
    m, n, x_len = IHT_SHAPES[2]
    name, thr, K = _modes(x_len)[mode]
    nvec = 3
    Phi, _, ys = _signals(rt, m, n, nvec)
    dPhi = hip.to_device(Phi)
    dy = [hip.to_device(y) for y in ys]
    lens = dict(x=n, t1=m, t2=m, t3=n)
    v = {k: [hip.alloc(2 * ln) for _ in range(nvec)] for k, ln in lens.items()}
    last = None
    with forced("1"):
        for iters in (2, 3, 0):
            hip.check(hip.lib.clm_f16_iht_batch_one_matrix(dPhi.ptr, m, n, nvec, pa(v["x"]), x_len, pa(dy), pa(v["t1"]), pa(v["t2"]), pa(v["t3"]),
                                                           iters, K, MU, thr, None))
            fresh = [hip.mf16_iht_one_matrix(dPhi, m, n, y, iters, K, MU, thr, x_len=x_len) for y in ys] if iters else None
            for j in range(nvec):
                want = fresh[j] if iters else dict(last[j], x=np.zeros(n, np.uint16))
                for k, ln in lens.items():
                    assert same16(v[k][j].download(np.uint16, ln), want[k]), (name, iters, j, k)
            if iters:
                last = fresh
