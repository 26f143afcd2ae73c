"""CloverVector16 / CloverMatrix16 on the device against the checker (tests/half16_restate.c, pinned by tests/test_half16_cpu.py): every
entry point of the half-precision C ABI, bit for bit unless a test says otherwise (NaN payloads; dot FAST)."""
import numpy as np
import pytest

from clover_amd.lib_binding import DOT_EXACT, DOT_FAST, THRESHOLD_FAST, THRESHOLD_REFERENCE
from half16_helpers import (Dev, assert_chain_bound, make_f32, pad128, random_f16_bits, rh, rhp)  # noqa: F401

pytestmark = pytest.mark.gpu

KINDS = ["gaussian", "ties", "subnormal", "overflow", "zeros"]
LENGTHS = [1, 127, 128, 1000, 8192, 100003, (1 << 20) + 128]           # logical lengths: ragged ones are padded with zeros to 128


def padded(x, n_pad):
    out = np.zeros(n_pad, x.dtype)
    out[:x.size] = x
    return out


# ---------------------------------------------------------------- vectors
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", LENGTHS)
def test_vector_quantize_and_restore(hip, rh, kind, n):
    x = padded(make_f32(kind, n, n), pad128(n))
    h = hip.f16_quantize(x)
    want = rh.quantize(x)
    assert np.array_equal(h, want), (kind, n, np.flatnonzero(h != want)[:8])
    assert np.all(h[n:] == 0)                                          # the padding stays zero
    back = hip.f16_restore(h)
    assert np.array_equal(back.view(np.uint32), rh.restore(h).view(np.uint32))


def test_restore_every_bit_pattern_but_signalling_nans(hip, rh):
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    got, want = hip.f16_restore(h), rh.restore(h)
    nan = np.isnan(want)
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))      # all 2046 subnormals among them
    assert np.all(np.isnan(got[nan]))


def test_quantize_nan_stays_nan(hip, rh):
    """NaN inputs: required to stay NaN with their sign; the payload is not compared (the checker keeps the top payload bits and sets the
    quiet bit, which a conversion instruction need not do -- not measured here, so not asserted)"""
    x = padded(make_f32("nan", 4096, 3), 4096)
    h = hip.f16_quantize(x)
    want = rh.quantize(x)
    nan = np.isnan(x)
    assert np.array_equal(h[~nan], want[~nan])
    assert np.all(np.isnan(h[nan].view(np.float16)))


@pytest.mark.parametrize("kind", ["gaussian", "subnormal", "overflow", "zeros", "cancel"])
@pytest.mark.parametrize("n", [128, 1000, 8192, (1 << 20) + 128])
@pytest.mark.parametrize("in_place", [False, True])
def test_vector_scale_and_add(hip, rh, kind, n, in_place):
    n_pad = pad128(n)
    rng = np.random.default_rng(n)
    s = np.float32(-0.3721)
    if kind == "cancel":                                               # u = -s v to within rounding: the fused fma decides the result
        v = random_f16_bits(rng, n, 0, 1)
        u = (-(v.view(np.float16).astype(np.float32) * s)).astype(np.float16).view(np.uint16)
    else:
        if kind == "overflow":
            s = np.float32(1.0)
        u, v = rh.quantize(make_f32(kind, n, n + 1)), rh.quantize(make_f32(kind, n, n + 2))
        if kind == "overflow":                                         # finite operands whose sum passes 65520
            u, v = np.minimum(u & 0x7FFF, 0x7BFF).astype(np.uint16), np.minimum(v & 0x7FFF, 0x7BFF).astype(np.uint16)
    u, v = padded(u, n_pad), padded(v, n_pad)
    got = hip.f16_scale_and_add(u, v, float(s), in_place=in_place)
    want = rh.scale_and_add(u, v, s)
    assert np.array_equal(got, want), (kind, n, np.flatnonzero(got != want)[:8])
    if kind == "overflow":
        assert np.any(np.isinf(want.view(np.float16)))
    if kind == "subnormal":
        sub = want & 0x7C00 == 0
        assert np.any(sub & (want & 0x3FF != 0))


@pytest.mark.parametrize("n", [128, 1024, 8192, 8192 + 128, 65536 + 384, 1 << 20])
@pytest.mark.parametrize("sub", [0.0, 0.2])
def test_dot_exact_is_the_32_chain_order(hip, rh, n, sub):
    rng = np.random.default_rng(n)
    u, v = random_f16_bits(rng, n, -6, 6, sub), random_f16_bits(rng, n, -6, 6, sub)
    got, want = hip.f16_dot(u, v, DOT_EXACT), rh.dot(u, v)
    assert got.view(np.uint32) == want.view(np.uint32), (n, got, want)


def test_dot_of_subnormal_operands_only(hip, rh):
    """every operand an f16 subnormal: an instruction that flushed them would give 0"""
    rng = np.random.default_rng(1)
    n = 4096
    u = rng.integers(1, 0x400, size=n).astype(np.uint16)
    v = (rng.integers(1, 0x400, size=n) | 0x8000).astype(np.uint16)
    want = rh.dot(u, v)
    assert want != 0 and hip.f16_dot(u, v, DOT_EXACT).view(np.uint32) == want.view(np.uint32)
    e, a = rh.mvm64(u, 1, n, v)
    assert abs(float(hip.f16_dot(u, v, DOT_FAST)) - e[0]) <= 2e-6 * a[0]


@pytest.mark.parametrize("n", [128, 8192, 100096, 1 << 20, (1 << 24) + 128])
def test_dot_fast_meets_the_fast_bar(hip, rh, n):
    """|fast - float64| <= 2e-6 * sum |terms|; and a second call gives the same bits (one fixed tree)"""
    rng = np.random.default_rng(n)
    u, v = random_f16_bits(rng, n, -6, 6, 0.05), random_f16_bits(rng, n, -6, 6, 0.05)
    e, a = rh.mvm64(u, 1, n, v)
    got = hip.f16_dot(u, v, DOT_FAST)
    assert abs(float(got) - e[0]) <= 2e-6 * a[0], (n, got, e[0], a[0])
    assert hip.f16_dot(u, v, DOT_FAST).view(np.uint32) == got.view(np.uint32)


# ---------------------------------------------------------------- matrices
# (rows, cols): one row block; rows that are no multiple of a workgroup's 16 or 64; wide-short; tall-narrow; cols beyond one staged chunk of
# x (8192 f16 / 4096 fp32 elements) with a ragged last chunk; enough rows for the 64-row workgroups (>= 128 per CU pair)
SHAPES = [(16, 128), (1, 256), (100, 384), (128, 128), (7, 20480 + 128), (8, 65536), (40010, 128), (33000, 256), (1000, 8192 + 384)]


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_mvm_f16_vectors(hip, rh, rhp, rows, cols):
    rng = np.random.default_rng(rows + cols)
    A, x = random_f16_bits(rng, rows * cols, -4, 4, 0.02), random_f16_bits(rng, cols, -4, 4, 0.02)
    got = hip.mf16_mvm(A, rows, cols, x)
    want = (rhp if rows * cols > 1 << 20 else rh).mvm(A, rows, cols, x)
    assert np.array_equal(got, want), (rows, cols, np.flatnonzero(got != want)[:8])


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_mvm_f32_vectors(hip, rh, rhp, rows, cols):
    rng = np.random.default_rng(rows + cols + 1)
    A = random_f16_bits(rng, rows * cols, -4, 4, 0.02)
    x = (rng.normal(size=cols) * np.exp2(rng.integers(-10, 10, size=cols))).astype(np.float32)
    got = hip.mf16_mvm_f32(A, rows, cols, x)
    want = (rhp if rows * cols > 1 << 20 else rh).mvm_f32(A, rows, cols, x)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (rows, cols, np.flatnonzero(got != want)[:8])
    e, a = rhp.mvm_f32_64(A, rows, cols, x)
    assert_chain_bound(got, e, a, cols, "device mvm_f32 vs float64")


def test_mvm_with_subnormal_entries_and_an_overflowing_row(hip, rh):
    rng = np.random.default_rng(11)
    rows, cols = 192, 1024
    A, x = random_f16_bits(rng, rows * cols, -4, 4), random_f16_bits(rng, cols, -2, 2)
    A = A.reshape(rows, cols)
    A[0:64] = rng.integers(1, 0x400, size=(64, cols)).astype(np.uint16)            # rows of subnormals only
    x_sub = rng.integers(1, 0x400, size=cols).astype(np.uint16)                      # and a subnormal vector
    A[100] = np.float16(60000.0).view(np.uint16)                                     # fp32 row sum far beyond 65520
    A[101] = np.float16(-60000.0).view(np.uint16)
    xp = (np.abs(x.view(np.float16)) + np.float16(1)).astype(np.float16).view(np.uint16)
    for xv in (x, x_sub, xp):
        got, want = hip.mf16_mvm(A, rows, cols, xv), rh.mvm(A, rows, cols, xv)
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    r = rh.mvm(A, rows, cols, xp)
    assert r[100] == 0x7C00 and r[101] == 0xFC00                                     # +inf / -inf
    r = rh.mvm(A, rows, cols, x)
    assert np.any(r[0:64] & 0x7FFF != 0)                                             # the subnormal rows did not vanish
    xf = xp.view(np.float16).astype(np.float32)
    got, want = hip.mf16_mvm_f32(A, rows, cols, xf), rh.mvm_f32(A, rows, cols, xf)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.isfinite(got[100]) and got[100] > 65520


def test_mvm_on_row_shards_at_pointer_offsets(hip, rh):
    """a row shard of a matrix: the matrix pointer advanced by whole rows, the result written at an offset of the result vector"""
    rng = np.random.default_rng(12)
    rows, cols = 320, 512
    A, x = random_f16_bits(rng, rows * cols, -4, 4, 0.02), random_f16_bits(rng, cols, -4, 4)
    xf = (rng.normal(size=cols)).astype(np.float32)
    want, want32 = rh.mvm(A, rows, cols, x), rh.mvm_f32(A, rows, cols, xf)
    dA, dx, dxf = hip.to_device(A), hip.to_device(x), hip.to_device(xf)
    dr, dr32 = hip.alloc(2 * rows), hip.alloc(4 * rows)
    hip.check(hip.lib.clv_memset(dr.ptr, 0xFF, 2 * rows, None))
    hip.check(hip.lib.clv_memset(dr32.ptr, 0xFF, 4 * rows, None))
    for begin, count in [(0, 64), (64, 100), (164, 1), (165, 155)]:
        hip.check(hip.lib.clm_f16_mvm(dA.ptr + 2 * begin * cols, count, cols, dx.ptr, dr.ptr + 2 * begin, None))
        hip.check(hip.lib.clm_f16_mvm_f32(dA.ptr + 2 * begin * cols, count, cols, dxf.ptr, dr32.ptr + 4 * begin, None))
    assert np.array_equal(dr.download(np.uint16, rows), want)
    assert np.array_equal(dr32.download(np.uint32, rows), want32.view(np.uint32))


@pytest.mark.parametrize("kind", ["gaussian", "ties", "subnormal", "overflow"])
@pytest.mark.parametrize("rows,cols", [(128, 128), (256, 1152), (1280, 384)])
def test_matrix_quantize(hip, rh, kind, rows, cols):
    A = make_f32(kind, rows * cols, rows).reshape(rows, cols)
    got = hip.mf16_quantize(A)
    assert np.array_equal(got, rh.quantize(A).ravel())


@pytest.mark.parametrize("rows,cols", [(128, 128), (64, 64), (8, 8), (128, 384), (1152, 256), (72, 200), (200, 72), (8, 1000), (4096, 128)])
def test_transpose_and_back(hip, rh, rows, cols):
    rng = np.random.default_rng(rows * 7 + cols)
    h = rng.integers(0, 65536, size=rows * cols).astype(np.uint16)                   # any bit pattern: nothing is interpreted
    t = hip.mf16_transpose(h, rows, cols)
    assert np.array_equal(t, rh.transpose(h, rows, cols))
    assert np.array_equal(t.reshape(cols, rows), h.reshape(rows, cols).T)
    assert np.array_equal(hip.mf16_transpose(t, cols, rows), h)


# ---------------------------------------------------------------- threshold
def tied_vector(rng, n, n_pad):
    h = np.zeros(n_pad, np.uint16)
    h[:n] = random_f16_bits(rng, n, -3, 3, 0.05)
    levels = np.array([0.5, 1.5, 1.5, 2.25, 7.0], np.float16).view(np.uint16)
    idx = rng.choice(n, size=n // 2, replace=False)
    h[idx] = levels[rng.integers(0, levels.size, size=idx.size)] | (rng.integers(0, 2, size=idx.size).astype(np.uint16) << 15)   # ties of both signs
    h[n:] = 0x3C00                                                                   # what lies in the padding is not touched
    return h


def lowest_index_threshold(h, n, k):
    out = h.copy()
    if k >= n:
        return out
    mag = np.abs(h[:n].view(np.float16).astype(np.float32))
    out[:n] = 0
    if k == 0:
        return out
    tau = np.sort(mag)[n - k]
    above = np.flatnonzero(mag > tau)
    ties = np.flatnonzero(mag == tau)[:k - above.size]
    keep = np.concatenate([above, ties])
    out[keep] = h[keep]
    return out


THRESH_CASES = [(100, 10), (128, 64), (1000, 1), (8192, 1024), (8192, 0), (8192, 8191), (8192, 8192), (8192, 9000), (70001, 3000), (300000, 25000)]


@pytest.mark.parametrize("n,k", THRESH_CASES)
def test_threshold_reference_survivors_index_for_index(hip, rh, n, k):
    rng = np.random.default_rng(n + k)
    h = tied_vector(rng, n, pad128(n))
    got = hip.f16_threshold(h, n, k, THRESHOLD_REFERENCE)
    want = rh.threshold(h, n, k)
    assert np.array_equal(got, want), (n, k, np.flatnonzero(got != want)[:8])
    assert np.array_equal(got[n:], h[n:])


@pytest.mark.parametrize("n,k", [(100, 10), (1000, 1), (8192, 1024), (8192, 8191), (8192, 8192), (70001, 3000)])
def test_threshold_min_heap_contents(hip, rh, n, k):
    rng = np.random.default_rng(n + k + 1)
    h = tied_vector(rng, n, pad128(n))
    got, hv, hi = hip.f16_threshold_heap(h, n, k)
    want, wv, wi = rh.threshold_heap(h, n, k)
    assert np.array_equal(got, want)
    assert np.array_equal(hv.view(np.uint32), wv.view(np.uint32)) and np.array_equal(hi, wi)


@pytest.mark.parametrize("n,k", THRESH_CASES)
def test_threshold_fast_same_multiset_lowest_index_ties(hip, rh, n, k):
    rng = np.random.default_rng(n + k)
    h = tied_vector(rng, n, pad128(n))
    got = hip.f16_threshold(h, n, k, THRESHOLD_FAST)
    assert np.array_equal(got, lowest_index_threshold(h, n, k)), (n, k)
    ref = rh.threshold(h, n, k)
    mag = lambda v: np.sort(np.abs(v[:n].view(np.float16).astype(np.float32)))      # noqa: E731
    assert np.array_equal(mag(got), mag(ref))                                        # the reference's multiset of magnitudes
