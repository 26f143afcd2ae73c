"""The three products of include/clover_hip_m8_f32.h on the GPU, bit for bit against references that are no device kernel of theirs:
m8.mvm_f32 (on m8.transpose for the transposed forms) of tests/matrix8_helpers.py, rf.scale_and_add of tests/fp32_helpers.py.

x is normal-distributed and the bytes cover the whole range, -128 included: against the right order a 16-chain summation changes most
outputs at these sizes (tests/test_m8_f32_cpu.py asserts at least a quarter on this very data), so a wrong order cannot pass.

Shapes (tests/m8_f32_helpers.py; M8FT_COLS and M8FT_U are read from clover_amd/csrc/matrix8_f32_t.hip, the chunk from the header):
- transposed: (128, 128); (128, 384): three strips; (384, 128); (256, 640); (CLM8_F32_T_CHUNK + 128, 384): the second staging chunk and a
  ragged last load group.  Strips are 128 columns: every strip is whole;
- the scale edges on A's grid (edge_problem): a tile scale near FLT_MAX, subnormal factors f32(s / 127) with subnormal products x f, in
  both chunks;
- fused, row-major (128, 128), (256, 640), (128, 1152: past the unroll of k_m8_mvm_f32, cols / 64 no multiple of 8), a 64-row shard
  (192, 256), and transposed on the shapes above: with t, without t, in place, a from {-1, 0.37}, and the "cancel" case u = -f32(a d),
  which leaves the rounding error of the product under a true single-rounding fma and +0 under anything else."""
import numpy as np
import pytest

from fp32_helpers import rf  # noqa: F401  (fixture)
from m8_f32_helpers import A_VALUES, CHUNK, HEADER, R_SHAPES, T_SHAPES, TINY, cancel_u, edge_problem, matrix, problem, same, vector
from matrix8_helpers import m8  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def test_the_two_chunk_shape_follows_the_exported_chunk(hip):
    assert f"#define CLM8_F32_T_CHUNK {CHUNK}" in HEADER and (CHUNK + 128, 384) in T_SHAPES


@pytest.fixture(scope="module")
def refs(m8):  # noqa: F811
    """per transposed shape: the problem and A' x from the restatement on the transpose, computed once"""
    out = {}
    for rows, cols in T_SHAPES:
        qA, sA, x, _, _, u = problem(rows, cols)
        qT, sT = m8.transpose(qA, sA, rows, cols)
        out[rows, cols] = (qA, sA, x, u, m8.mvm_f32(qT, sT, cols, rows, x))
    return out


@pytest.mark.parametrize("rows,cols", T_SHAPES, ids=lambda v: str(v))
def test_transposed_product_equals_the_restatement_on_the_transpose(hip, refs, rows, cols):
    qA, sA, x, _, want = refs[rows, cols]
    assert (qA == -128).any()
    got = hip.m8_mvm_f32_transposed(qA, sA, rows, cols, x)
    print(f"{rows} x {cols}: {np.count_nonzero(got.view(np.uint32) != want.view(np.uint32))} of {cols} outputs differ")
    assert same(got, want)


@pytest.mark.parametrize("rows,cols", T_SHAPES, ids=lambda v: str(v))
def test_transposed_product_equals_the_device_pair(hip, refs, rows, cols):
    """clm8_transpose + clm8_mvm_f32 on the device as well"""
    qA, sA, x, _, want = refs[rows, cols]
    qT, sT = hip.m8_transpose(qA, sA, rows, cols)
    assert same(hip.m8_mvm_f32(qT, sT, cols, rows, x), want)
    assert same(hip.m8_mvm_f32_transposed(qA, sA, rows, cols, x), want)


def test_transposed_product_on_the_scale_edges(hip, m8, rf):  # noqa: F811
    rows, cols, qA, sA, x, _, _ = edge_problem()
    qT, sT = m8.transpose(qA, sA, rows, cols)
    want = m8.mvm_f32(qT, sT, cols, rows, x)
    got = hip.m8_mvm_f32_transposed(qA, sA, rows, cols, x)
    assert np.isfinite(got).all()
    assert same(got, want)
    assert np.count_nonzero(got[128:192]) > 32 and (np.abs(got[128:192]) < TINY).all(), "the subnormals are kept"
    u = np.full(cols, 0.25, np.float32)
    t, r2 = hip.m8_mvm_f32_transposed_scale_and_add(qA, sA, rows, cols, x, u, 0.37)
    assert same(t, want) and same(r2, rf.scale_and_add(u, want, 0.37))
    qd, sd = hip.m8_transpose(qA, sA, rows, cols)
    assert same(hip.m8_mvm_f32(qd, sd, cols, rows, x), want), "the row-major kernel agrees: the result does not depend on which form ran"


def check_fused(call, rf, d, u, n):  # noqa: F811
    """call(u, a, in_place, want_t) -> (t, r2); d: the product from the restatement"""
    for a in A_VALUES:
        want = rf.scale_and_add(u, d, a)
        t, r2 = call(u, a, False, True)
        assert same(t, d) and same(r2, want), ("with t", a)
        t, r2 = call(u, a, False, False)
        assert t is None and same(r2, want), ("without t", a)
        t, r2 = call(u, a, True, True)
        assert same(t, d) and same(r2, want), ("in place", a)
        assert not same(want, u)
        uc = cancel_u(d, a)
        want_c = rf.scale_and_add(uc, d, a)
        t, r2 = call(uc, a, False, True)
        assert same(t, d) and same(r2, want_c), ("cancel", a)
        if a != -1.0:                                   # a = -1: the product is exact and the sum +0 either way
            assert np.count_nonzero(want_c) > n // 4, "the rounding error of the product is there to be seen"


@pytest.mark.parametrize("rows,cols", T_SHAPES, ids=lambda v: str(v))
def test_fused_transposed_step_equals_the_product_then_scale_and_add(hip, rf, refs, rows, cols):  # noqa: F811
    qA, sA, x, u, d = refs[rows, cols]
    dq, ds = hip.to_device(qA), hip.to_device(sA)
    check_fused(lambda uu, a, in_place, want_t: hip.m8_mvm_f32_transposed_scale_and_add(dq, ds, rows, cols, x, uu.copy(), a, in_place=in_place,
                                                                                         want_t=want_t), rf, d, u, cols)


@pytest.mark.parametrize("rows,cols", R_SHAPES, ids=lambda v: str(v))
def test_fused_row_major_step_equals_the_product_then_scale_and_add(hip, m8, rf, rows, cols):  # noqa: F811
    qA, sA, _, x, u, _ = problem(rows, cols)
    d = m8.mvm_f32(qA, sA, rows, cols, x)
    assert same(hip.m8_mvm_f32(qA, sA, rows, cols, x), d)
    dq, ds = hip.to_device(qA), hip.to_device(sA)
    check_fused(lambda uu, a, in_place, want_t: hip.m8_mvm_f32_scale_and_add(dq, ds, rows, cols, x, uu.copy(), a, in_place=in_place, want_t=want_t),
                rf, d, u, rows)


def test_fused_row_major_step_on_a_64_row_shard(hip, m8, rf):  # noqa: F811
    """rows a multiple of 64, as clm8_mvm_f32 takes them"""
    rows, cols = 192, 256
    rng = np.random.default_rng(5)
    qA, sA = matrix(rng, 256, cols)
    qA, sA = qA[:rows * cols], sA[:(rows // 64) * (cols // 64)]
    x, u = vector(rng, cols), vector(rng, rows)
    d = m8.mvm_f32(qA, sA, rows, cols, x)
    t, r2 = hip.m8_mvm_f32_scale_and_add(qA, sA, rows, cols, x, u, 0.37)
    assert same(t, d) and same(r2, rf.scale_and_add(u, d, 0.37))
