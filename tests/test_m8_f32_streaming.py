"""The nontemporal (NT = true) instantiations of the CloverMatrix8 x fp32-vector kernels, each against a reference that is not a device
kernel: one whole-result case per kernel, on a shape just above the launchers' predicate (rows cols > T = 268 435 456 bytes), which
the cases assert, so a shape that stops selecting the streaming form fails instead of passing on the cached kernel.

The lines the map in tests/test_streaming_instantiations.py would carry:

matrix8.hip, clm8_mvm_f32_scale_and_add, rows cols > T:
- k_m8_mvm_f32<true, M4F32Fuse>: test_m8_mvm_f32_scale_and_add_streaming
matrix8_f32_t.hip, rows cols > T:
- k_m8_mvm_f32_t<M8FT_U, true>: test_m8_mvm_f32_transposed_streaming
- k_m8_mvm_f32_t<M8FT_U, true, M4F32Fuse>: test_m8_mvm_f32_transposed_scale_and_add_streaming

One matrix of 16384 x 16512 bytes (270 532 608: 129 strips of 128 columns and two staging chunks of rows for the transposed kernel, 512
row groups for the row-major one) is uploaded once and shared by the three cases; its references come once from the parallel build of
the restatement (m8p of tests/matrix8_helpers.py).  The bytes cover the whole range, -128 included."""
import numpy as np
import pytest

from fp32_helpers import rf  # noqa: F401  (fixture)
from m8_f32_helpers import same, vector
from matrix8_helpers import m8p  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

T = 256 << 20
ROWS, COLS = 16384, 16512
A = 0.37


@pytest.fixture(scope="module")
def big(hip, m8p):  # noqa: F811
    assert ROWS * COLS > T >= ROWS * (COLS - 128), "the launchers' predicate: the smallest width that streams at these rows"
    rng = np.random.default_rng(2028)
    q = np.frombuffer(rng.bytes(ROWS * COLS), np.int8).copy()
    assert (q == -128).any()
    s = rng.uniform(0.5, 2.0, size=(ROWS // 64) * (COLS // 64)).astype(np.float32)
    x_rows, x_cols, u_rows, u_cols = vector(rng, ROWS), vector(rng, COLS), vector(rng, ROWS), vector(rng, COLS)
    d_rm = m8p.mvm_f32(q, s, ROWS, COLS, x_cols)
    qT, sT = m8p.transpose(q, s, ROWS, COLS)
    d_t = m8p.mvm_f32(qT, sT, COLS, ROWS, x_rows)
    del qT, sT
    dq, ds = hip.to_device(q), hip.to_device(s)
    del q
    return dict(dq=dq, ds=ds, x_rows=x_rows, x_cols=x_cols, u_rows=u_rows, u_cols=u_cols, d_rm=d_rm, d_t=d_t)


def test_m8_mvm_f32_transposed_streaming(hip, big):
    got = hip.m8_mvm_f32_transposed(big["dq"], big["ds"], ROWS, COLS, big["x_rows"])
    assert same(got, big["d_t"]), np.count_nonzero(got != big["d_t"])


def test_m8_mvm_f32_transposed_scale_and_add_streaming(hip, rf, big):  # noqa: F811
    t, r2 = hip.m8_mvm_f32_transposed_scale_and_add(big["dq"], big["ds"], ROWS, COLS, big["x_rows"], big["u_cols"], A)
    assert same(t, big["d_t"]) and same(r2, rf.scale_and_add(big["u_cols"], big["d_t"], A))


def test_m8_mvm_f32_scale_and_add_streaming(hip, rf, big):  # noqa: F811
    t, r2 = hip.m8_mvm_f32_scale_and_add(big["dq"], big["ds"], ROWS, COLS, big["x_cols"], big["u_rows"], A)
    assert same(t, big["d_rm"]) and same(r2, rf.scale_and_add(big["u_rows"], big["d_rm"], A))
