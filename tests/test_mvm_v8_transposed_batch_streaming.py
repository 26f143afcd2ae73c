"""The nontemporal instantiations of the batched transposed mixed kernel: k_m4_mvm8_t_batch<NV, U, true, FUSE, ST> for NV = 2, 4 and 8, all
four (FUSE, ST).  The launcher has no switch that forces them at a small shape, so they run at 16384 x 32896 -- the shape of the single
call's test: one byte row more than the 256 MiB Infinity Cache holds, 257 workgroups (one beyond the whole groups of 16 that the XCD
pairing renumbers), four re-stagings of x -- with 2, 3 and 5 vectors.  Compared with the single device calls clm4_mvm_v8_transposed /
clm4_mvm_v8_transposed_scale_and_add in order only, state included: test_mvm_v8_transposed.py already holds those to the CPU at this
shape.  The matrix and the vectors are filled on the device (every byte a pair of nibbles in [-7, 7]: as int8 never -128), once for all
cases."""
import numpy as np
import pytest

from mvm_v8_transposed_batch_data import KEYS, eq
from test_m8_mvm_batch import copies_of, get8, pairs8
from test_mvm_v8_transposed_batch_capture import filled
from test_mvm_batch import batch_kernel, pa
from test_mvm_batch_stochastic import keys_equal

pytestmark = pytest.mark.gpu

ROWS, COLS = 16384, 32896
T = 256 << 20
assert ROWS * COLS // 2 > T and ROWS * (COLS - 128) // 2 <= T and COLS % 128 == 0
_arena = {}


def arena(hip):
    if not _arena:
        dA, dsA = hip.alloc(ROWS * COLS // 2), hip.alloc((ROWS // 64) * (COLS // 64) * 4)
        hip.check(hip.lib.clv_fill_random_nibbles(dA.ptr, dA.nbytes, 5, 0, None))
        hip.check(hip.lib.clv_fill_random_scales(dsA.ptr, dsA.nbytes // 4, 6, 0, None))
        _arena.update(A=(dA, dsA), x=filled(hip, 8, ROWS, 100), u=filled(hip, 8, COLS, 200))
    return _arena["A"], _arena["x"], _arena["u"]


@pytest.mark.parametrize("nvec", [2, 3, 5])
def test_the_nontemporal_instantiations_equal_the_single_calls(hip, nvec):
    L = hip.lib
    (dA, dsA), x, du = arena(hip)
    x = x[:nvec]
    xs = pa([d[0] for d in x]), pa([d[1] for d in x])
    det = None
    for generator in (False, True):
        # plain
        st1, st2 = (hip.new_rng(*KEYS), hip.new_rng(*KEYS)) if generator else (None, None)
        p1, p2 = (st1.ptr, st2.ptr) if generator else (None, None)
        one, many = pairs8(hip, nvec, COLS), pairs8(hip, nvec, COLS)
        for j in range(nvec):
            hip.check(L.clm4_mvm_v8_transposed(dA.ptr, dsA.ptr, ROWS, COLS, x[j][0].ptr, x[j][1].ptr, one[j][0].ptr, one[j][1].ptr, p1, None))
        before = L.clv_mvm_batch_launches()
        with batch_kernel("1"):
            hip.check(L.clm4_mvm_v8_transposed_batch(dA.ptr, dsA.ptr, ROWS, COLS, nvec, *xs, pa([o[0] for o in many]), pa([o[1] for o in many]), p2, None))
        hip.sync()
        assert L.clv_mvm_batch_launches() - before == 1
        t_single = [get8(o, COLS) for o in one]
        for j in range(nvec):
            assert eq(get8(many[j], COLS), t_single[j]), f"plain, generator={generator}, vector {j}"
        assert np.any(t_single[0][0]) and not eq(t_single[0], t_single[1])
        if generator:
            assert not eq(t_single[0], det[0]), "the noise changed nothing: the comparison shows less than it should"
        else:
            det = t_single
        # fused, continuing on the same states
        u1, u2 = copies_of(hip, du, nvec, COLS), copies_of(hip, du, nvec, COLS)
        t1, t2 = pairs8(hip, nvec, COLS), pairs8(hip, nvec, COLS)
        for j in range(nvec):
            hip.check(L.clm4_mvm_v8_transposed_scale_and_add(dA.ptr, dsA.ptr, ROWS, COLS, x[j][0].ptr, x[j][1].ptr, u1[j][0].ptr, u1[j][1].ptr, 0.37,
                                                          t1[j][0].ptr, t1[j][1].ptr, u1[j][0].ptr, u1[j][1].ptr, p1, None))
        before = L.clv_mvm_batch_launches()
        with batch_kernel("1"):
            hip.check(L.clm4_mvm_v8_transposed_scale_and_add_batch(dA.ptr, dsA.ptr, ROWS, COLS, nvec, *xs, pa([d[0] for d in u2]), pa([d[1] for d in u2]),
                                                                0.37, pa([d[0] for d in t2]), pa([d[1] for d in t2]), pa([d[0] for d in u2]),
                                                                pa([d[1] for d in u2]), p2, None))
        hip.sync()
        assert L.clv_mvm_batch_launches() - before == 1
        for j in range(nvec):
            assert eq(get8(t2[j], COLS), get8(t1[j], COLS)), f"fused, generator={generator}: t of vector {j}"
            assert eq(get8(u2[j], COLS), get8(u1[j], COLS)), f"fused in place, generator={generator}: r of vector {j}"
        assert not eq(get8(u1[0], COLS), get8(du[0], COLS))
        if generator:
            assert keys_equal(hip.rng_get(st1), hip.rng_get(st2)), "the state after the plain and the fused call"
