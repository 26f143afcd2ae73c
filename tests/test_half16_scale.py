"""The half-precision kernels at the sizes the benchmark times: the whole mvm result at 65536 x 65536 (an 8 GiB matrix, both vector
types) and the transpose of that matrix against the OpenMP build of the checker, and matrix quantize at 32768 x 32768."""
import numpy as np
import pytest

from half16_helpers import Dev, assert_chain_bound, random_f16_bits, rhp  # noqa: F401

pytestmark = pytest.mark.gpu

CHUNK = 1 << 28


def finite_f16_bits(rng, n):
    """n random f16 bit patterns with the top exponent bit cleared: |value| < 2, every subnormal and both zeros among them; made 512 MiB
    at a time"""
    h = np.empty(n, np.uint16)
    for o in range(0, n, CHUNK):
        c = h[o:o + CHUNK]
        c[:] = np.frombuffer(rng.bytes(2 * c.size), np.uint16)
        c &= 0xBFFF
    return h


@pytest.fixture(scope="module")
def big(hip):
    n = 65536
    rng = np.random.default_rng(2026)
    A = finite_f16_bits(rng, n * n)
    dA = hip.alloc(2 * n * n)
    for o in range(0, n * n, CHUNK):                                    # uploaded in pieces: no second host copy
        hip.check(hip.lib.clv_memcpy_h2d(dA.ptr + 2 * o, A[o:o + CHUNK].ctypes.data, 2 * min(CHUNK, n * n - o), None))
    hip.sync()
    return n, A, dA


def test_mvm_f16_at_65536_squared(hip, rhp, big):
    n, A, dA = big
    x = random_f16_bits(np.random.default_rng(1), n, -3, 1, 0.02)
    got = Dev(hip).mvm(dA, n, n, x)
    want = rhp.mvm(A, n, n, x)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert np.count_nonzero(np.isfinite(want.view(np.float16))) == n and np.unique(want).size > n // 8


def test_mvm_f32_at_65536_squared(hip, rhp, big):
    n, A, dA = big
    x = (np.random.default_rng(2).normal(size=n)).astype(np.float32)
    got = Dev(hip).mvm_f32(dA, n, n, x)
    want = rhp.mvm_f32(A, n, n, x)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.flatnonzero(got != want)[:8]
    rows = np.arange(0, n, 997)                                          # and a sample of rows against float64
    e, a = rhp.mvm_f32_64(np.ascontiguousarray(A.reshape(n, n)[rows]).ravel(), rows.size, n, x)
    assert_chain_bound(got[rows], e, a, n, "mvm_f32 65536^2")


def test_transpose_at_65536_squared(hip, rhp, big):
    n, A, dA = big
    dt = Dev(hip).transpose(dA, n, n)
    t = np.empty(n * n, np.uint16)
    for o in range(0, n * n, CHUNK):
        hip.check(hip.lib.clv_memcpy_d2h(t[o:o + CHUNK].ctypes.data, dt.ptr + 2 * o, 2 * min(CHUNK, n * n - o), None))
    del dt
    assert rhp.is_transpose(A, n, n, t)


def test_matrix_quantize_at_32768_squared(hip, rhp):
    n = 32768
    rng = np.random.default_rng(7)
    A = np.empty(n * n, np.float32)
    for o in range(0, n * n, CHUNK):                                     # values over the whole f16 range and beyond both ends of it
        c = A[o:o + CHUNK]
        c[:] = rng.standard_normal(c.size, dtype=np.float32)
        c *= np.exp2(rng.integers(-28, 18, size=c.size, dtype=np.int8).astype(np.float32))
    dA, dh = hip.alloc(4 * n * n), hip.alloc(2 * n * n)
    for o in range(0, n * n, CHUNK):
        hip.check(hip.lib.clv_memcpy_h2d(dA.ptr + 4 * o, A[o:o + CHUNK].ctypes.data, 4 * min(CHUNK, n * n - o), None))
    hip.check(hip.lib.clm_f16_quantize(dA.ptr, n, n, dh.ptr, None))
    got = dh.download(np.uint16, n * n)
    want = rhp.quantize(A)
    assert np.all(np.isfinite(A[::4097])) and np.array_equal(got, want)
    sub = np.count_nonzero((want & 0x7C00 == 0) & (want & 0x3FF != 0))
    assert sub > n and np.count_nonzero(want & 0x7FFF == 0x7C00) > n    # subnormal results and overflows are both in the data
