"""CloverMatrix8 at the sizes it is timed at, and on both sides of every dispatch threshold of clover_amd/csrc/matrix8.hip.

- 65536^2 (qA = 2^32 bytes: from row 32768 on every byte offset is past 2^31): mvm with an 8-bit vector in both rounding modes (1024
  row groups, each at its own place of the stream), mvm with an fp32 vector, transpose and transpose back.  32768^2: quantize whole
  (2^32 bytes of fp32 input) in both modes.
- the thresholds: restore above 256 MiB of output, transpose above 128 MiB, mvm / mvm_f32 above 256 MiB of matrix switch to streaming
  (nontemporal) loads and stores -- each call runs at the threshold and just past it.  A tall 2^20 x 128 and a wide 128 x 2^20
  stochastic quantize take each term of the tile order t = b_j v_blocks + b_i on its own.

Every result is compared bit for bit with the restatement (tests/matrix8_restate.c, its -fopenmp build), the generator state left
behind with the oracle's, and every mvm / quantize output also with float64 through the error bounds of tests/matrix8_helpers.py.
Data: full-range bytes, scales over 40 binades.  Peak host memory stays near 13 GiB (the 65536^2 transpose)."""
import numpy as np
import pytest

from matrix8_helpers import (Dev, assert_mvm8_bound, assert_mvm_f32_bound, assert_quantize_bound, binade_scales,  # noqa: F401
                             full_range_bytes, m8p, same, same_keys, x64)

pytestmark = pytest.mark.gpu

BAND = 1 << 28


def matrix(rows, cols, seed):
    rng = np.random.default_rng(seed)
    return full_range_bytes(rng, rows * cols), binade_scales(rng, (rows // 64) * (cols // 64))


def fp32_matrix(rows, cols, seed):
    """normal values times one power of two per 64 x 64 tile, 2^U(-20, 20), generated a band of tile rows at a time"""
    rng = np.random.default_rng(seed)
    A = np.empty((rows, cols), np.float32)
    mult = binade_scales(rng, (rows // 64) * (cols // 64)).reshape(rows // 64, cols // 64)
    band = max(64, (BAND // 4 // cols) // 64 * 64)
    for r0 in range(0, rows, band):
        r1 = min(rows, r0 + band)
        A[r0:r1] = rng.standard_normal((r1 - r0, cols), dtype=np.float32)
        A[r0:r1] *= np.repeat(np.repeat(mult[r0 // 64:r1 // 64], 64, 0), 64, 1)
    return A


def check_mvm(hip, dev, m8p, x64, oracle, qA, sA, dA, dsA, rows, cols, seed):
    """mvm with an 8-bit vector, deterministic then stochastic twice, and mvm_f32: bits, keys, float64 bounds"""
    rng = np.random.default_rng(seed)
    qx, sx = full_range_bytes(rng, cols), binade_scales(rng, cols // 64)
    exact, absum = x64.mvm8(qA, sA, rows, cols, qx, sx)
    r, sr = dev.mvm(dA, dsA, rows, cols, qx, sx)
    ro, sro = m8p.mvm(qA, sA, rows, cols, qx, sx)
    assert same(r, ro) and same(sr, sro), ("deterministic", rows, cols)
    assert_mvm8_bound(r, sr, exact, absum, cols, ("deterministic", rows, cols))
    st, o = hip.new_rng(seed, 77), oracle.rng(seed, 77)
    for rep in range(2):
        r, sr = dev.mvm(dA, dsA, rows, cols, qx, sx, rng=st)
        ro, sro = m8p.mvm(qA, sA, rows, cols, qx, sx, o)
        assert same(r, ro) and same(sr, sro), ("stochastic", rep, rows, cols)
        assert_mvm8_bound(r, sr, exact, absum, cols, ("stochastic", rep, rows, cols))
    assert same_keys(hip, st, oracle, o)
    x = (rng.standard_normal(cols, dtype=np.float32) * binade_scales(rng, cols, -10, 10)).astype(np.float32)
    f = dev.mvm_f32(dA, dsA, rows, cols, x)
    assert same(f, m8p.mvm_f32(qA, sA, rows, cols, x)), ("mvm_f32", rows, cols)
    assert_mvm_f32_bound(f, *x64.mvm_f32(qA, sA, rows, cols, x), cols, ("mvm_f32", rows, cols))


def check_transpose(dev, m8p, q, s, dq, ds, rows, cols):
    """transpose against the restatement, then transpose back and compare with the input a band at a time"""
    dt, dst = dev.transpose(dq, ds, rows, cols)
    qto, sto = m8p.transpose(q, s, rows, cols)
    for o in range(0, rows * cols, BAND):
        n = min(BAND, rows * cols - o)
        assert np.array_equal(dev.get(dt, np.int8, n, o), qto[o:o + n]), ("transpose", rows, cols, o)
    assert same(dev.get(dst, np.float32, s.size), sto)
    del qto, sto
    d2, ds2 = dev.transpose(dt, dst, cols, rows)
    del dt, dst
    for o in range(0, rows * cols, BAND):
        n = min(BAND, rows * cols - o)
        assert np.array_equal(dev.get(d2, np.int8, n, o), q[o:o + n]), ("transpose back", rows, cols, o)
    assert same(dev.get(ds2, np.float32, s.size), s)


# ---------------------------------------------------------------- 1. the timed size
@pytest.fixture(scope="module")
def big(hip):
    n = 65536
    qA, sA = matrix(n, n, n)
    yield n, qA, sA, hip.to_device(qA), hip.to_device(sA)


def test_gpu_mvm_65536(hip, m8p, x64, oracle, big):
    n, qA, sA, dA, dsA = big
    check_mvm(hip, Dev(hip), m8p, x64, oracle, qA, sA, dA, dsA, n, n, 1)


def test_gpu_transpose_65536_and_back(hip, m8p, big):
    n, qA, sA, dA, dsA = big
    check_transpose(Dev(hip), m8p, qA, sA, dA, dsA, n, n)


@pytest.mark.parametrize("stochastic", [False, True])
def test_gpu_quantize_32768(hip, m8p, oracle, stochastic):
    n = 32768
    A = fp32_matrix(n, n, 32768 + stochastic)
    st, o = (hip.new_rng(13, 17), oracle.rng(13, 17)) if stochastic else (None, None)
    q, s = Dev(hip).quantize(A, st)
    qo, so = m8p.quantize(A, o)
    assert same(q, qo) and same(s, so)
    del qo, so
    if stochastic:
        assert same_keys(hip, st, oracle, o)
    assert_quantize_bound(A, q, s)


# ---------------------------------------------------------------- 2. every dispatch branch, at its threshold and just past it
@pytest.mark.parametrize("shape", [(8192, 8192), (8192, 8320)])
def test_gpu_restore_threshold(hip, m8p, shape):
    """256 MiB of fp32 output exactly (cached stores), then 2 MiB more (nontemporal stores)"""
    rows, cols = shape
    q, s = matrix(rows, cols, rows + cols)
    assert same(hip.m8_restore(q, s, rows, cols), m8p.restore(q, s, rows, cols))


@pytest.mark.parametrize("shape", [(8192, 16384), (8192, 16512), (128, (1 << 20) + 128), ((1 << 20) + 128, 128)])
def test_gpu_transpose_threshold(hip, m8p, shape):
    """128 MiB of input exactly, then just past it: square-ish, one tile row, one tile column"""
    rows, cols = shape
    q, s = matrix(rows, cols, rows + 3 * cols)
    check_transpose(Dev(hip), m8p, q, s, hip.to_device(q), hip.to_device(s), rows, cols)


@pytest.mark.parametrize("shape", [(16384, 16384), (16384, 16512)])
def test_gpu_mvm_threshold(hip, m8p, x64, oracle, shape):
    """256 MiB of matrix exactly (cached loads), then just past it (streaming loads), both rounding modes and the fp32 vector"""
    rows, cols = shape
    qA, sA = matrix(rows, cols, rows + 5 * cols)
    check_mvm(hip, Dev(hip), m8p, x64, oracle, qA, sA, hip.to_device(qA), hip.to_device(sA), rows, cols, cols)


@pytest.mark.parametrize("shape", [(1 << 20, 128), (128, 1 << 20)])
def test_gpu_quantize_stochastic_tall_and_wide(hip, m8p, oracle, shape):
    """2^14 x 2 and 2 x 2^14 tiles: t = b_j v_blocks + b_i with each term spanning 2^14 on its own"""
    rows, cols = shape
    A = fp32_matrix(rows, cols, rows + 2 * cols)
    st, o = hip.new_rng(19, 23), oracle.rng(19, 23)
    for rep in range(2):
        q, s = Dev(hip).quantize(A, st)
        qo, so = m8p.quantize(A, o)
        assert same(q, qo) and same(s, so), rep
        assert_quantize_bound(A, q, s)
    assert same_keys(hip, st, oracle, o)
