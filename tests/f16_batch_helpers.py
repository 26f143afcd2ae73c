"""Shared data of the batched half-precision tests (tests/test_f16_mvm_batch.py, test_f16_threshold_batch.py, test_f16_iht_batch.py,
test_f16_mvm_batch_guarded.py, test_f16_mvm_batch_capture.py): the operand kinds, threshold vectors and IHT problems of
tests/test_half16_fused.py, stated here again because importing that module registers its guard-band and capture cases with the tables of
other test files as a side effect, which must not happen before those files are collected."""
import ctypes as C
import os

import numpy as np

from half16_helpers import random_f16_bits


def pa(bufs):
    """a host array of device pointers from DevBufs / addresses"""
    return (C.c_void_p * len(bufs))(*[b if isinstance(b, int) else b.ptr for b in bufs])


class forced:
    """CLV_MVM_BATCH for the calls inside; None = unset"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.saved = os.environ.pop("CLV_MVM_BATCH", None)
        if self.value is not None:
            os.environ["CLV_MVM_BATCH"] = self.value

    def __exit__(self, *exc):
        os.environ.pop("CLV_MVM_BATCH", None)
        if self.saved is not None:
            os.environ["CLV_MVM_BATCH"] = self.saved


def is_nan16(h):
    return (np.asarray(h, np.uint16) & 0x7FFF) > 0x7C00


def same16(got, want):
    """bit equality of two binary16 arrays; where `want` is a NaN, `got` has to be one (payload not compared)"""
    got, want = np.asarray(got, np.uint16), np.asarray(want, np.uint16)
    nan = is_nan16(want)
    return got.shape == want.shape and np.array_equal(got[~nan], want[~nan]) and bool(np.all(is_nan16(got[nan])))


KINDS = ["uniform", "subnormal", "overflow", "negzero"]
SCALES = (-1.0, 0.5, 0.0)


def _fast_bits(rng, n):
    """finite f16 patterns of magnitude 2^-4 .. 1, either sign (cheap enough for 2^27 elements)"""
    return rng.integers(0x2C00, 0x3C00, size=n, dtype=np.uint16) | (rng.integers(0, 2, size=n, dtype=np.uint16) << 15)


def _operands(kind, rows, cols):
    rng = np.random.default_rng(rows * 131 + cols + len(kind))
    if rows * cols > 1 << 22:
        return _fast_bits(rng, rows * cols), _fast_bits(rng, cols), random_f16_bits(rng, rows, -3, 3, 0.05)
    A, x, u = random_f16_bits(rng, rows * cols, -4, 4, 0.02), random_f16_bits(rng, cols, -2, 2), random_f16_bits(rng, rows, -3, 3, 0.05)
    if kind == "subnormal":                                          # subnormal entries times 2^-6: rows that are f16 subnormals, and u likewise
        A = (rng.integers(1, 0x400, size=rows * cols) | (rng.integers(0, 2, size=rows * cols) << 15)).astype(np.uint16)
        x = random_f16_bits(rng, cols, -7, -5)
        u = (rng.integers(1, 0x400, size=rows) | (rng.integers(0, 2, size=rows) << 15)).astype(np.uint16)
    elif kind == "overflow":                                         # rows 0 / 1: fp32 sums far beyond 65520 -> +inf / -inf
        A = A.reshape(rows, cols)
        A[0], A[1] = np.float16(60000.0).view(np.uint16), np.float16(-60000.0).view(np.uint16)
        A = A.ravel()
        x = (np.abs(x.view(np.float16)) + np.float16(1)).astype(np.float16).view(np.uint16)
    elif kind == "negzero":                                          # zero rows meet -0.0 in u: fma(+0, -1, -0) = -0
        A = A.reshape(rows, cols)
        A[::3] = 0
        A = A.ravel()
        u[::2] = 0x8000
    return A, x, u


def _check_kind(kind, t, r):
    if kind == "subnormal":
        assert np.any((t & 0x7C00 == 0) & (t & 0x3FF != 0)) and np.any((r[0.5] & 0x7C00 == 0) & (r[0.5] & 0x3FF != 0))
    if kind == "overflow":
        assert t[0] == 0x7C00 and t[1] == 0xFC00 and r[-1.0][0] == 0xFC00 and r[0.5][1] == 0xFC00 and is_nan16(r[0.0][:2]).all()
    if kind == "negzero":
        assert np.any(r[-1.0] == 0x8000) and np.any(t == 0)


THRESH_KINDS = ["random", "ties", "equal", "zeros", "inf"]


def _threshold_vector(kind, n, n_pad):
    rng = np.random.default_rng(n * 7 + len(kind))
    sign = (rng.integers(0, 2, size=n) << 15).astype(np.uint16)
    if kind == "random":
        h = random_f16_bits(rng, n, -3, 3, 0.05)
    elif kind == "ties":                                             # 8 distinct magnitudes, mixed signs
        levels = np.array([0.25, 0.5, 1.5, 1.5009765625, 2.25, 7.0, 6.1e-5, 3e-6], np.float16).view(np.uint16)
        h = levels[rng.integers(0, levels.size, size=n)] | sign
    elif kind == "equal":
        h = np.full(n, np.float16(1.5).view(np.uint16), np.uint16) | sign
    elif kind == "zeros":                                            # +-0 and subnormals
        h = np.where(rng.random(n) < 0.6, 0, rng.integers(1, 0x400, size=n)).astype(np.uint16) | sign
    else:                                                            # +-inf among finite values
        h = random_f16_bits(rng, n, -3, 3, 0.05)
        h[rng.integers(0, n, size=max(n // 50, 1))] = 0x7C00
        h[rng.integers(0, n, size=max(n // 50, 1))] = 0xFC00
    out = np.full(n_pad, 0x3C00, np.uint16)                          # what lies in the padding is not touched
    out[:n] = h
    return out


IHT_SHAPES = [(128, 256, 256), (256, 128, 100), (384, 640, 600)]          # (m, n, x_len)
MU = 0.5
_PROBLEMS = {}


def _iht_problem(R, m, n):
    """Phi ~ U(-1, 1) / sqrt(m): the eigenvalues of Phi' Phi stay below (1 + sqrt(n / m))^2 / 3 < 2 / MU for these shapes, so the iterates of
    x += MU Phi'(y - Phi x) stay bounded; y = Phi x_true for a sparse x_true of normal entries.  Quantized on the CPU once per shape."""
    if (m, n) not in _PROBLEMS:
        rng = np.random.default_rng(m * 3 + n)
        phi = (rng.uniform(-1, 1, size=(m, n)) / np.sqrt(m)).astype(np.float32)
        x_true = np.zeros(n, np.float32)
        x_true[rng.choice(n, n // 8, replace=False)] = rng.normal(size=n // 8).astype(np.float32)
        Phi = R.quantize(phi).ravel()
        _PROBLEMS[m, n] = (Phi, R.transpose(Phi, m, n), R.quantize((phi @ x_true).astype(np.float32)))
    return _PROBLEMS[m, n]


def _modes(x_len):
    """(name, threshold argument, K)"""
    return [("gd", 0, 0), ("fast", 1, x_len // 8), ("reference", 2, x_len // 8)]


def _scaled_matrix(seed, m, n):
    return (np.random.default_rng(seed).uniform(-1, 1, size=(m, n)) / np.sqrt(m)).astype(np.float32)
