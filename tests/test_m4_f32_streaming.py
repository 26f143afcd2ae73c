"""The nontemporal (NT = true) instantiations of the CloverMatrix4 x fp32-vector kernels, each against a reference that is not a device
kernel: one whole-result case per kernel, on a shape just above the launchers' predicate (rows cols / 2 > T = 268 435 456 bytes of
nibbles), which the cases assert, so a shape that stops selecting the streaming form fails instead of passing on the cached kernel.

The lines the map in tests/test_streaming_instantiations.py would carry:

mvm_f32.hip, clm4_mvm_f32_scale_and_add, rows cols / 2 > T:
- k_m4_mvm_f32<true, M4F32Fuse>: test_m4_mvm_f32_scale_and_add_streaming
mvm_f32_t.hip, rows cols / 2 > T:
- k_m4_mvm_f32_t<M4FT_U, true>: test_m4_mvm_f32_transposed_streaming
- k_m4_mvm_f32_t<M4FT_U, true, M4F32Fuse>: test_m4_mvm_f32_transposed_scale_and_add_streaming

One matrix of 16384 x 32896 (269 484 032 bytes of nibbles: 257 strips of 128 columns and two staging chunks of rows for the transposed
kernel, 256 row groups and three x chunks for the row-major one) is uploaded once and shared by the three cases; its references come from the
oracle once.  Peak host memory stays below 2 GiB."""
import numpy as np
import pytest

from fp32_helpers import rf  # noqa: F401  (fixture)
from m4_f32_helpers import same, vector

pytestmark = pytest.mark.gpu

T = 256 << 20
ROWS, COLS = 16384, 32896
A = 0.37


@pytest.fixture(scope="module")
def big(hip, oracle):
    assert ROWS * (COLS // 2) > T >= ROWS * ((COLS - 128) // 2), "the launchers' predicate: the smallest width that streams at these rows"
    rng = np.random.default_rng(2028)
    q = np.frombuffer(rng.bytes(ROWS * COLS // 2), np.uint8).copy()
    q[(q >> 4) == 8] ^= 0x80                                  # nibbles in [-7, 7], as a quantiser leaves them
    q[(q & 0xF) == 8] ^= 0x08
    s = rng.uniform(0.5, 2.0, size=(ROWS // 64) * (COLS // 64)).astype(np.float32)
    x_rows, x_cols, u_rows, u_cols = vector(rng, ROWS), vector(rng, COLS), vector(rng, ROWS), vector(rng, COLS)
    d_rm = oracle.m4_mvm_f32(q, s, ROWS, COLS, x_cols)
    qT, sT = oracle.m4_transpose(q, s, ROWS, COLS)
    d_t = oracle.m4_mvm_f32(qT, sT, COLS, ROWS, x_rows)
    del qT, sT
    dq, ds = hip.to_device(q), hip.to_device(s)
    del q
    return dict(dq=dq, ds=ds, x_rows=x_rows, x_cols=x_cols, u_rows=u_rows, u_cols=u_cols, d_rm=d_rm, d_t=d_t)


def test_m4_mvm_f32_transposed_streaming(hip, big):
    got = hip.m4_mvm_f32_transposed(big["dq"], big["ds"], ROWS, COLS, big["x_rows"])
    assert same(got, big["d_t"]), np.count_nonzero(got != big["d_t"])


def test_m4_mvm_f32_transposed_scale_and_add_streaming(hip, rf, big):  # noqa: F811
    t, r2 = hip.m4_mvm_f32_transposed_scale_and_add(big["dq"], big["ds"], ROWS, COLS, big["x_rows"], big["u_cols"], A)
    assert same(t, big["d_t"]) and same(r2, rf.scale_and_add(big["u_cols"], big["d_t"], A))


def test_m4_mvm_f32_scale_and_add_streaming(hip, rf, big):  # noqa: F811
    t, r2 = hip.m4_mvm_f32_scale_and_add(big["dq"], big["ds"], ROWS, COLS, big["x_cols"], big["u_rows"], A)
    assert same(t, big["d_rm"]) and same(r2, rf.scale_and_add(big["u_rows"], big["d_rm"], A))
