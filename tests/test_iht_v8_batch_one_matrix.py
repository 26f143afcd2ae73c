"""The mixed Q_IHT / Q_GD (CloverMatrix4 x CloverVector8) for several signals with ONE matrix on the GPU: clm4_iht_v8_batch_one_matrix
(include/clover_hip_batch_t_v8.h) equals,
BYTE FOR BYTE, clm4_iht_v8_one_matrix per signal in order on the same stream, and clm4_iht_v8_batch with PhiT = clm4_transpose(Phi): x, t1 .. t3
and the generator state left behind.  Neither reference runs the new kernel (the second runs the row-major batched kernel on a stored
transpose, with CLV_MVM_BATCH=1).

(m, n): 128 x 256 and 256 x 128 (non-square both ways), 384 x 640 (ten output blocks of step 2: five workgroups).  nvec: 2, 3 and 5 (masked
slots), 8, 9 (a second group of one).  threshold none / FAST / REFERENCE, 3 iterations, both roundings, forced and by the rule."""
import numpy as np
import pytest

from mvm_v8_transposed_batch_data import KEYS
from oracle.binding import Oracle
from test_m8_mvm_batch import IHT_K, MU, get8, pairs8
from test_mvm_batch import assert_same_vectors, batch_kernel, pa
from test_mvm_batch_stochastic import keys_equal
from test_mvm_v8_transposed import matrix, vector

pytestmark = pytest.mark.gpu


def one_matrix_run(hip, mats, dy, m, n, x_len, thr, batch, rng=None, iters=3):
    """clm4_iht_v8_batch_one_matrix, or clm4_iht_v8_one_matrix per vector in order, with the parameters and the prefill of two_matrix_run"""
    L = hip.lib
    nvec = len(dy)
    lens = dict(x=n, t1=m, t2=m, t3=n)
    v = {k: pairs8(hip, nvec, ln, 0x55) for k, ln in lens.items()}
    if batch:
        arrs = {k: (pa([d[0] for d in v[k]]), pa([d[1] for d in v[k]])) for k in v}
        hip.check(L.clm4_iht_v8_batch_one_matrix(mats[0].ptr, mats[1].ptr, m, n, nvec, arrs["x"][0], arrs["x"][1], x_len, pa([d[0] for d in dy]),
                                              pa([d[1] for d in dy]), arrs["t1"][0], arrs["t1"][1], arrs["t2"][0], arrs["t2"][1], arrs["t3"][0],
                                              arrs["t3"][1], iters, IHT_K, MU, thr, rng.ptr if rng else None, None))
    else:
        for j in range(nvec):
            hip.check(L.clm4_iht_v8_one_matrix(mats[0].ptr, mats[1].ptr, m, n, v["x"][j][0].ptr, v["x"][j][1].ptr, x_len, dy[j][0].ptr, dy[j][1].ptr,
                                            v["t1"][j][0].ptr, v["t1"][j][1].ptr, v["t2"][j][0].ptr, v["t2"][j][1].ptr, v["t3"][j][0].ptr,
                                            v["t3"][j][1].ptr, iters, IHT_K, MU, thr, rng.ptr if rng else None, None))
    hip.sync()
    return {k: [get8(p, lens[k]) for p in v[k]] for k in v}


def two_matrix_run(hip, mats, dy, m, n, x_len, thr, rng=None, iters=3):
    """clm4_iht_v8_batch on (Phi, PhiT): the row-major batched kernel on a stored transpose"""
    L = hip.lib
    nvec = len(dy)
    lens = dict(x=n, t1=m, t2=m, t3=n)
    v = {k: pairs8(hip, nvec, ln, 0x55) for k, ln in lens.items()}
    arrs = {k: (pa([d[0] for d in v[k]]), pa([d[1] for d in v[k]])) for k in v}
    hip.check(L.clm4_iht_v8_batch(*[b.ptr for b in mats], m, n, nvec, arrs["x"][0], arrs["x"][1], x_len, pa([d[0] for d in dy]), pa([d[1] for d in dy]),
                                  arrs["t1"][0], arrs["t1"][1], arrs["t2"][0], arrs["t2"][1], arrs["t3"][0], arrs["t3"][1], iters, IHT_K, MU, thr,
                                  rng.ptr if rng else None, None))
    hip.sync()
    return {k: [get8(p, lens[k]) for p in v[k]] for k in v}


@pytest.mark.parametrize("generator", [False, True], ids=["deterministic", "generator"])
@pytest.mark.parametrize("nvec", [2, 3, 5, 8, 9])
@pytest.mark.parametrize("m,n", [(128, 256), (256, 128), (384, 640)], ids=lambda v: str(v))
def test_the_batched_one_matrix_loop_equals_the_single_loops_and_the_two_matrix_batch(hip, oracle, m, n, nvec, generator):
    rng = np.random.default_rng(m * 7 + n + 1)
    Phi = matrix(rng, m, n)
    PhiT = hip.m4_transpose(*Phi, m, n)
    mats = [hip.to_device(v) for v in (*Phi, *PhiT)]
    dy = [tuple(hip.to_device(a) for a in vector(rng, m)) for _ in range(nvec)]
    L = hip.lib
    x_len = n - 5

    def state():
        return hip.new_rng(*KEYS) if generator else None
    for thr in (0, 1, 2):
        st1 = state()
        one = one_matrix_run(hip, mats, dy, m, n, x_len, thr, batch=False, rng=st1)
        st2 = state()
        with batch_kernel("1"):
            two = two_matrix_run(hip, mats, dy, m, n, x_len, thr, rng=st2)
        assert_same_vectors(two, one, f"threshold={thr}: clm4_iht_v8_batch on the stored transpose against clm4_iht_v8_one_matrix:")
        for force in ("1", None):
            st3 = state()
            before = L.clv_mvm_batch_launches()
            with batch_kernel(force):
                got = one_matrix_run(hip, mats, dy, m, n, x_len, thr, batch=True, rng=st3)
            if force and nvec <= 8:
                assert L.clv_mvm_batch_launches() - before == 6, "one group, three iterations: two batched launches each"
            assert_same_vectors(got, one, f"threshold={thr} CLV_MVM_BATCH={force}:")
            if generator:
                assert keys_equal(hip.rng_get(st3), hip.rng_get(st1)), f"threshold={thr} CLV_MVM_BATCH={force}: the state against the single loops"
                assert keys_equal(hip.rng_get(st3), hip.rng_get(st2)), f"threshold={thr} CLV_MVM_BATCH={force}: the state against clm4_iht_v8_batch"
        assert any(np.any(x[0]) for x in one["x"]) and any(np.any(t[0]) for t in one["t3"]), "the loop left everything zero"
        if generator:
            assert not keys_equal(hip.rng_get(st1), Oracle.rng_keys(oracle.rng(*KEYS)))
    if generator:
        st = hip.new_rng(*KEYS)
        with batch_kernel("1"):
            one_matrix_run(hip, mats, dy, m, n, x_len, 1, batch=True, rng=st, iters=0)
        assert keys_equal(hip.rng_get(st), Oracle.rng_keys(oracle.rng(*KEYS))), "no iterations: nothing drawn, nothing committed"


def test_the_python_helper_reaches_the_one_matrix_loop_when_no_transpose_is_given(hip):
    """CloverHip.m4_iht_v8_batch(qPhiT=None) is clm4_iht_v8_batch_one_matrix: the bytes of the same helper on (Phi, clm4_transpose(Phi))"""
    m, n, nvec = 128, 256, 3
    rng = np.random.default_rng(m * 7 + n + 3)
    Phi = matrix(rng, m, n)
    PhiT = hip.m4_transpose(*Phi, m, n)
    ys = [vector(rng, m) for _ in range(nvec)]
    args = dict(iterations=2, K=IHT_K, mu=MU, threshold=1, x_len=n - 5)
    before = hip.lib.clv_mvm_batch_launches()
    with batch_kernel("1"):
        one = hip.m4_iht_v8_batch(*Phi, None, None, m, n, ys, **args)
        assert hip.lib.clv_mvm_batch_launches() - before == 4, "two iterations, two batched launches each"
        two = hip.m4_iht_v8_batch(*Phi, *PhiT, m, n, ys, **args)
    for j in range(nvec):
        for name in ("x", "t1", "t2", "t3"):
            assert np.array_equal(one[j][name][0], two[j][name][0]) and np.array_equal(one[j][name][1].view(np.uint32), two[j][name][1].view(np.uint32)), (j, name)
    assert any(np.any(o["t3"][0]) for o in one)
