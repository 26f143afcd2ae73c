"""The four batched transposed mixed calls, CloverMatrix4 x CloverVector8, (include/clover_hip_batch_t_v8.h) under hipGraph capture: each is called once outside the capture,
captured once and replayed three times on CHANGED operands; every replay equals the eager single calls (clm4_mvm_v8_transposed,
clm4_mvm_v8_transposed_scale_and_add, clm4_iht_v8_one_matrix) on the same operands.  Deterministic: nothing is allocated during the call, no
pointer table lives on the device.  Stochastic: the state is in graph mode (clv_rng_graph_mode), the eager single calls continue the same
stream of draws on a second state, and after the replays both states are equal.  CLV_MVM_BATCH=1 throughout: the captured call is the
batched kernel (the launch counter says so).  The same coverage rule as test_capture_base.py, on the table of these calls."""
import numpy as np
import pytest

from capture_helpers import fresh_graph
from clover_amd.lib_binding import SIGNATURES_BATCH_T_V8
from mvm_v8_transposed_batch_data import KEYS, W, eq
from test_m8_mvm_batch import get8, pairs8
from test_mvm_batch import batch_kernel, pa
from test_mvm_batch_stochastic import keys_equal

ROWS, COLS, NVEC = 256, 64 * (W + 2), 5          # two workgroups, masked slots of the 8-vector instantiation
IM, IN, INV, ITERS = 128, 256, 3, 2
REPLAYS = 3


def filled(hip, count, n, seed):
    out = pairs8(hip, count, n)
    refill(hip, out, seed)
    return out


def refill(hip, bufs, seed):
    """every byte a pair of nibbles in [-7, 7]: as int8 never -128, what a quantiser leaves"""
    L = hip.lib
    for j, (q, s) in enumerate(bufs):
        hip.check(L.clv_fill_random_nibbles(q.ptr, q.nbytes, seed + 2 * j, 0, None))
        hip.check(L.clv_fill_random_scales(s.ptr, s.nbytes // 4, seed + 2 * j + 1, 0, None))
    hip.sync()


class Mvm:
    """clm4_mvm_v8_transposed_batch (at=None), clm4_mvm_v8_transposed_batch_at (at given: on the windows of the contiguous call) or the fused call"""

    def __init__(self, hip, fused=False, at=None):
        self.hip, self.fused, self.at = hip, fused, at
        self.A = filled(hip, 1, ROWS * COLS, 7)[0]                         # (more bytes and scales than the 4-bit image and its tile grid need)
        self.x, self.u = filled(hip, NVEC, ROWS, 100), filled(hip, NVEC, COLS, 200)
        self.t, self.r = pairs8(hip, NVEC, COLS), pairs8(hip, NVEC, COLS)
        self.changed = self.x
        self.launches = 1

    def enqueue(self, stream, rng):
        L, p = self.hip.lib, lambda v, i: pa([d[i] for d in v])  # noqa: E731
        head = (self.A[0].ptr, self.A[1].ptr, ROWS, COLS, NVEC, p(self.x, 0), p(self.x, 1))
        if self.fused:
            self.hip.check(L.clm4_mvm_v8_transposed_scale_and_add_batch(*head, p(self.u, 0), p(self.u, 1), 0.37, p(self.t, 0), p(self.t, 1), p(self.r, 0),
                                                                     p(self.r, 1), rng, stream))
        elif self.at is None:
            self.hip.check(L.clm4_mvm_v8_transposed_batch(*head, p(self.r, 0), p(self.r, 1), rng, stream))
        else:       # the windows of the contiguous call, so that the single calls are its reference
            G = COLS // 64
            self.hip.check(L.clm4_mvm_v8_transposed_batch_at(*head, p(self.r, 0), p(self.r, 1), rng, 0, 2 * G, NVEC * 2 * G, stream))

    def singles(self, rng):
        L = self.hip.lib
        wt, wr = pairs8(self.hip, NVEC, COLS), pairs8(self.hip, NVEC, COLS)
        for j in range(NVEC):
            if self.fused:
                self.hip.check(L.clm4_mvm_v8_transposed_scale_and_add(self.A[0].ptr, self.A[1].ptr, ROWS, COLS, self.x[j][0].ptr, self.x[j][1].ptr,
                                                                   self.u[j][0].ptr, self.u[j][1].ptr, 0.37, wt[j][0].ptr, wt[j][1].ptr, wr[j][0].ptr,
                                                                   wr[j][1].ptr, rng, None))
            else:
                self.hip.check(L.clm4_mvm_v8_transposed(self.A[0].ptr, self.A[1].ptr, ROWS, COLS, self.x[j][0].ptr, self.x[j][1].ptr, wr[j][0].ptr,
                                                     wr[j][1].ptr, rng, None))
        self.hip.sync()
        return [get8(p, COLS) for p in (wt if self.fused else []) + wr]

    def outputs(self):
        return [get8(p, COLS) for p in (self.t if self.fused else []) + self.r]


class Iht:
    """clm4_iht_v8_batch_one_matrix, FAST threshold"""

    def __init__(self, hip):
        self.hip = hip
        self.P = filled(hip, 1, IM * IN, 9)[0]
        self.y = filled(hip, INV, IM, 300)
        self.lens = dict(x=IN, t1=IM, t2=IM, t3=IN)
        self.v = {k: pairs8(hip, INV, n) for k, n in self.lens.items()}
        self.changed = self.y
        self.launches = 2 * ITERS

    def enqueue(self, stream, rng):
        p = lambda v, i: pa([d[i] for d in v])  # noqa: E731
        v = self.v
        self.hip.check(self.hip.lib.clm4_iht_v8_batch_one_matrix(self.P[0].ptr, self.P[1].ptr, IM, IN, INV, p(v["x"], 0), p(v["x"], 1), IN - 5, p(self.y, 0),
                                                              p(self.y, 1), p(v["t1"], 0), p(v["t1"], 1), p(v["t2"], 0), p(v["t2"], 1), p(v["t3"], 0),
                                                              p(v["t3"], 1), ITERS, IN // 4, 0.0002, 1, rng, stream))

    def singles(self, rng):
        w = {k: pairs8(self.hip, INV, n) for k, n in self.lens.items()}
        for j in range(INV):
            self.hip.check(self.hip.lib.clm4_iht_v8_one_matrix(self.P[0].ptr, self.P[1].ptr, IM, IN, w["x"][j][0].ptr, w["x"][j][1].ptr, IN - 5, self.y[j][0].ptr,
                                                            self.y[j][1].ptr, w["t1"][j][0].ptr, w["t1"][j][1].ptr, w["t2"][j][0].ptr, w["t2"][j][1].ptr,
                                                            w["t3"][j][0].ptr, w["t3"][j][1].ptr, ITERS, IN // 4, 0.0002, 1, rng, None))
        self.hip.sync()
        return [get8(p, self.lens[k]) for k in self.lens for p in w[k]]

    def outputs(self):
        return [get8(p, self.lens[k]) for k in self.lens for p in self.v[k]]


CALLS = {
    "clm4_mvm_v8_transposed_batch": lambda hip: Mvm(hip),
    "clm4_mvm_v8_transposed_batch_at": lambda hip: Mvm(hip, at=0),
    "clm4_mvm_v8_transposed_scale_and_add_batch": lambda hip: Mvm(hip, fused=True),
    "clm4_iht_v8_batch_one_matrix": lambda hip: Iht(hip),
}


def test_every_entry_point_of_the_table_is_captured():
    assert set(CALLS) == set(SIGNATURES_BATCH_T_V8)


@pytest.mark.gpu
@pytest.mark.parametrize("stochastic", [False, True], ids=["deterministic", "stochastic"])
@pytest.mark.parametrize("name", sorted(CALLS))
def test_the_call_is_captured_once_and_replayed_on_changed_operands(hip, name, stochastic):
    L = hip.lib
    with batch_kernel("1"):
        c = CALLS[name](hip)
        g = fresh_graph(L)
        captured, eager = (hip.new_rng(*KEYS), hip.new_rng(*KEYS)) if stochastic else (None, None)
        cp, ep = (captured.ptr, eager.ptr) if stochastic else (None, None)
        try:
            if stochastic:
                hip.check(L.clv_rng_graph_mode(cp, 1, g.stream))
            c.enqueue(g.stream, cp)                                         # one ordinary call first
            g.sync()
            want = c.singles(ep)
            assert all(eq(a, b) for a, b in zip(c.outputs(), want)), "the call outside the capture"
            before = L.clv_mvm_batch_launches()
            g.record(lambda s: c.enqueue(s, cp))
            assert L.clv_mvm_batch_launches() - before == c.launches, "the captured call did not take the batched kernel"
            seen = []
            for rep in range(REPLAYS):
                refill(hip, c.changed, 1000 + 100 * rep)
                g.replay()
                got, want = c.outputs(), c.singles(ep)
                for i, (a, b) in enumerate(zip(got, want)):
                    assert eq(a, b), f"replay {rep}: output {i}"
                seen.append(got)
            assert not eq(seen[0][-1], seen[1][-1]) and not eq(seen[1][-1], seen[2][-1]), "the replays saw the same operands"
            assert np.any(seen[1][-1][0])
            if stochastic:
                hip.check(L.clv_rng_graph_mode(cp, 0, g.stream))
                assert keys_equal(hip.rng_get(captured), hip.rng_get(eager)), "the state after the replays"
                assert not keys_equal(hip.rng_get(captured), hip.rng_get(hip.new_rng(*KEYS)))
        finally:
            g.close(L)
