"""The transposed half-precision mvm on the GPU: clm_f16_mvm_transposed, clm_f16_mvm_f32_transposed and
clm_f16_mvm_transposed_scale_and_add give, BIT FOR BIT, what a stored transpose gives.  Bytes are compared twice: against the column-walk
restatement (tests/half16_t_restate.c, itself held to transpose + the row forms by test_f16_mvm_transposed_cpu.py) and against the device
pair clm_f16_transpose + clm_f16_mvm / clm_f16_mvm_f32 / clm_f16_mvm_scale_and_add.

Shapes (rows x cols; tests/f16_transposed_data.py reads F16T_COLS, F16T_U and F16T_CHUNK from clover_amd/csrc/half16_t.hip): the smallest at
which each thing can go wrong.
  128 x 128                                   the smallest
  256 x 128, 128 x 256                        non-square both ways: a product that forgets to transpose fails
  384 x 640
  32 U, 64 U, 32 (2 U + 1), 128 U rows x 128  (rounded up to multiples of 128) one register set, one round, a round plus a partial
                                              set, two rounds
  F16T_COLS - 128 (if positive), F16T_COLS, F16T_COLS + 128, 2 F16T_COLS + 128 columns at 128 and 256 rows
                                              the masked last workgroup (strips wider than 128 columns) and several workgroups
  C - 128, C, C + 128, 2 C + 128 rows x 128   the x re-staging barriers
  C + 64 U + 128 rows, three workgroups       a multiple of neither the chunk nor the round
Data: built to cancel across chains, so that a wrong summation order shows in the f16 bits (f16_transposed_data.py; the CPU test asserts
that it does on every shape here).  The nontemporal instantiations run at 8192 x 16512, one 128-column strip over 256 MiB: the launcher
has no switch that forces them at a small shape; they are compared against the device pair only."""
import numpy as np
import pytest

from f16_transposed_data import A_VALUES, NT_SHAPE, SHAPES, ZERO_COLUMN, big_matrix, vector_cols, vector_rows, vector_rows_f32
from f16_transposed_helpers import refs, rt, same  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rows,cols", SHAPES, ids=lambda v: str(v))
def test_transposed_mvm_equals_transpose_then_mvm(hip, rt, rows, cols):  # noqa: F811
    R = refs(hip, rt, rows, cols)
    got = hip.mf16_mvm_transposed(R.dA, rows, cols, R.S.x)
    assert same(got, R.cpu_t), "against the restatement's column walk"
    assert same(got, R.dev_t), "against clm_f16_transpose + clm_f16_mvm"
    assert got[ZERO_COLUMN] == 0 and np.count_nonzero(got) > cols // 2


@pytest.mark.parametrize("rows,cols", SHAPES, ids=lambda v: str(v))
def test_transposed_mvm_f32_equals_transpose_then_mvm_f32(hip, rt, rows, cols):  # noqa: F811
    R = refs(hip, rt, rows, cols)
    got = hip.mf16_mvm_f32_transposed(R.dA, rows, cols, R.S.xf)
    assert same(got, R.cpu_f32), "against the restatement's column walk"
    assert same(got, R.dev_f32), "against clm_f16_transpose + clm_f16_mvm_f32"
    assert got[ZERO_COLUMN] == 0 and np.count_nonzero(got) > cols // 2


@pytest.mark.parametrize("a", A_VALUES)
@pytest.mark.parametrize("form", ["t", "no_t", "in_place"])
@pytest.mark.parametrize("rows,cols", SHAPES, ids=lambda v: str(v))
def test_fused_transposed_mvm_equals_the_fused_call_on_a_stored_transpose(hip, rt, rows, cols, form, a):  # noqa: F811
    R = refs(hip, rt, rows, cols)
    t, r = hip.mf16_mvm_transposed_scale_and_add(R.dA, rows, cols, R.S.x, R.S.u, a, in_place=form == "in_place", want_t=form != "no_t")
    assert same(r, R.cpu_fused[a][1]), "r against the restatement"
    assert same(r, R.dev_fused[a][1]), "r against clm_f16_mvm_scale_and_add on the stored transpose"
    assert (t is None) == (form == "no_t")
    if t is not None:
        assert same(t, R.cpu_t) and same(t, R.dev_fused[a][0]), "t"
    assert not same(r, R.S.u)


def test_the_nontemporal_instantiations(hip):
    """k_f16_mvm_t<F16T_U, true, XF32, FUSE...>: f16, fp32 and fused.  The references are the device pair on the stored transpose"""
    L = hip.lib
    rows, cols = NT_SHAPE
    rng = np.random.default_rng(rows + cols)
    dA, dAt = hip.to_device(big_matrix(rng, rows, cols)), hip.alloc(2 * rows * cols)
    hip.check(L.clm_f16_transpose(dA.ptr, rows, cols, dAt.ptr, None))
    x, xf, u = vector_rows(rng, rows), vector_rows_f32(rng, rows), vector_cols(rng, cols)
    dx, dxf = hip.to_device(x), hip.to_device(xf)
    want, want32 = hip.alloc(2 * cols), hip.alloc(4 * cols)
    hip.check(L.clm_f16_mvm(dAt.ptr, cols, rows, dx.ptr, want.ptr, None))
    hip.check(L.clm_f16_mvm_f32(dAt.ptr, cols, rows, dxf.ptr, want32.ptr, None))
    want_t, want_r = hip.mf16_mvm_scale_and_add(dAt, cols, rows, x, u, A_VALUES[0])
    want, want32 = want.download(np.uint16, cols), want32.download(np.float32, cols)
    del dAt
    assert same(hip.mf16_mvm_transposed(dA, rows, cols, x), want), "f16 vectors"
    assert same(hip.mf16_mvm_f32_transposed(dA, rows, cols, xf), want32), "fp32 vectors"
    t, r = hip.mf16_mvm_transposed_scale_and_add(dA, rows, cols, x, u, A_VALUES[0])
    assert same(t, want_t) and same(r, want_r) and same(t, want), "fused"
    t, r = hip.mf16_mvm_transposed_scale_and_add(dA, rows, cols, x, u, A_VALUES[0], in_place=True, want_t=False)
    assert t is None and same(r, want_r), "fused, in place, t not stored"
    assert np.count_nonzero(want) > cols // 2 and want[ZERO_COLUMN] == 0
