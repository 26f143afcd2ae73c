"""The IHT / GD loops of the three operand pairs on a Phi built from the bands of edge_band_data.py (H and M's large scale scaled down so
that three iterations at mu = 2^-8 stay finite in the reference: test_edge_band_data_cpu.py asserts that, and that the iterates behind
the first hold a block of category Z and one of category T): clm4_iht and clm4_iht_v8 as one persistent launch and launch per step,
clm8_iht, the three *_iht_one_matrix, the three *_iht_batch and the three *_iht_batch_one_matrix.

x, t1, t2, t3 and their scales, every bit: persistent == launch-per-step == the reference's loop (the composition of
test_iht_persistent.py, with the lowest-index tie rule of the FAST threshold); one-matrix == two-matrix; batched == the single calls.
Threshold FAST with K = n / 4, K = 1, K = n and K = n - 64, and no threshold (GD).  Two tile columns of Phi are zero, one makes a block of x
come out with k = inf (elements 0, a subnormal scale) and one gives x non-zero subnormal magnitudes after the first iteration
(edge_band_data.loop_problem); at K = n - 64 fewer than K magnitudes are non-zero, so the threshold's tau is 0 and its tie group holds
more than 100 zeros -- test_edge_band_data_cpu.py asserts all of that on the reference."""
import pytest

import edge_band_data as D
from edge_band_gpu import eq, loops, m8, ref  # noqa: F401  (loops, m8, ref: fixtures)

pytestmark = pytest.mark.gpu

MODES = {"K=n/4": lambda n: (n // 4, 1), "K=1": lambda n: (1, 1), "K=n": lambda n: (n, 1), "K=n-64": lambda n: (n - 64, 1), "GD": lambda n: (0, 0)}


def same(a, b, what):
    for k in ("x", "t1", "t2", "t3"):
        assert eq(a[k], b[k]), f"{what}: {k}"


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("m,n", D.LOOP_SHAPES)
@pytest.mark.parametrize("pair", D.PAIRS)
def test_the_loops(loops, ref, pair, m, n, mode):  # noqa: F811
    P = loops(pair, m, n)
    K, thr = MODES[mode](n)
    Phi, PhiT, ys = P.host
    for iterations in (2, 3):                                                # after 2 the stored t1 still holds its block of category T
        steps = []
        for j in range(D.NVEC_MAX):
            got, count = P.single(j, K, thr, persistent=False, iterations=iterations)
            assert count == 0, "CLV_IHT_PERSISTENT=0: the launch-per-step loop"
            steps.append(got)
        for j in (0, 1):                                                     # y[1] has a zero block
            want, _ = D.loop_reference(ref, pair, Phi, PhiT, ys[j], m, n, K, thr, iterations=iterations)
            if iterations == 2:
                assert {"Z", "T"} <= set(D.block_categories(D.VECTOR_BITS[pair], want["t1"])), "the reference's t1 holds no block of category Z and T"
            same(steps[j], want, f"{iterations} iterations: launch per step against the reference's loop, measurement {j}")
            got, count = P.single(j, K, thr, persistent=True, iterations=iterations)
            assert count == (1 if P.abi.persistent else 0), "CLV_IHT_PERSISTENT=1: one persistent launch where the pair has the kernel"
            same(got, steps[j], f"{iterations} iterations: persistent against launch per step, measurement {j}")
            same(got, want, f"{iterations} iterations: persistent against the reference's loop, measurement {j}")
            got, count = P.single(j, K, thr, one_matrix=True, iterations=iterations)
            assert count == 0
            same(got, steps[j], f"{iterations} iterations: one matrix against two, measurement {j}")
        for nvec in (5, 9):                                                  # a group with masked slots; a full group and a remainder of one
            for one_matrix in (False, True):
                got, count = P.batched(nvec, K, thr, one_matrix=one_matrix, iterations=iterations)
                assert count == 2 * iterations, "forced: two batched launches per iteration for the group of two or more"
                for j in range(nvec):
                    same({k: got[k][j] for k in got}, steps[j],
                         f"{iterations} iterations: {'one-matrix ' if one_matrix else ''}batch of {nvec} against the single calls, measurement {j}")
