"""Shared checkers of the half-precision tests (tests/test_half16_cpu.py, test_half16.py, test_half16_scale.py, test_half16_capture.py).

- Restate: tests/half16_restate.c, the plain-C restatement of the CloverVector16 / CloverMatrix16 semantics (software f16 conversion, the
  32 fma chains and their tree, the heap walk), built twice: `h16` as cc -O2 -ffp-contract=off -fno-fast-math, `h16p` the same with -mfma
  -fopenmp (at most 16 threads) for the large shapes.  test_half16_cpu.py checks that the two builds agree bit for bit.
- the float64 bound a dot / mvm must meet: assert_chain_bound (derivation in its docstring).
- data: make_f32 (the value kinds the conversion has to get right), Dev (the clv_f16_* / clm_f16_* calls on device buffers)."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

from clover_amd.build import repo_root

ROOT = repo_root()
RESTATE = Path(__file__).parent / "half16_restate.c"
U32 = 2.0 ** -24             # fp32 unit roundoff
U16 = 2.0 ** -11             # f16 unit roundoff
F16_TINY = 2.0 ** -25        # half the smallest f16 subnormal: the absolute rounding error below 2^-14

_u16 = C.POINTER(C.c_uint16)
_u32 = C.POINTER(C.c_uint32)
_fp = C.POINTER(C.c_float)
_dp = C.POINTER(C.c_double)
_u64 = C.c_uint64


def _p(a, t):
    return a.ctypes.data_as(t)


def h16(a):
    return np.ascontiguousarray(a, dtype=np.uint16)


class Restate:
    def __init__(self, so: Path):
        self.L = L = C.CDLL(str(so))
        L.rh_f16_to_f32.restype = C.c_float
        L.rh_f16_to_f32.argtypes = [C.c_uint16]
        L.rh_f32_to_f16.restype = C.c_uint16
        L.rh_f32_to_f16.argtypes = [C.c_float]
        L.rh_dot.restype = C.c_float
        L.rh_is_transpose.restype = C.c_int

    def widen_all(self):
        out = np.zeros(65536, np.float32)
        self.L.rh_widen_all(_p(out, _fp))
        return out

    def quantize(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        h = np.zeros(x.size, np.uint16)
        self.L.rh_quantize(_p(x, _fp), _u64(x.size), _p(h, _u16))
        return h.reshape(x.shape)

    def restore(self, h):
        h = h16(h)
        x = np.zeros(h.size, np.float32)
        self.L.rh_restore(_p(h, _u16), _u64(h.size), _p(x, _fp))
        return x.reshape(h.shape)

    def scale_and_add(self, u, v, s):
        u, v = h16(u), h16(v)
        r = np.zeros(u.size, np.uint16)
        self.L.rh_scale_and_add(_p(u, _u16), _p(v, _u16), C.c_float(s), _u64(u.size), _p(r, _u16))
        return r

    def dot(self, u, v):
        u, v = h16(u), h16(v)
        return np.float32(self.L.rh_dot(_p(u, _u16), _p(v, _u16), _u64(u.size)))

    def mvm(self, A, rows, cols, x):
        A, x = h16(A), h16(x)
        r = np.zeros(rows, np.uint16)
        self.L.rh_mvm(_p(A, _u16), _u64(rows), _u64(cols), _p(x, _u16), _p(r, _u16))
        return r

    def rowdots(self, A, rows, cols, x):
        A, x = h16(A), h16(x)
        d = np.zeros(rows, np.float32)
        self.L.rh_rowdots(_p(A, _u16), _u64(rows), _u64(cols), _p(x, _u16), _p(d, _fp))
        return d

    def mvm_f32(self, A, rows, cols, x):
        A, x = h16(A), np.ascontiguousarray(x, dtype=np.float32)
        r = np.zeros(rows, np.float32)
        self.L.rh_mvm_f32(_p(A, _u16), _u64(rows), _u64(cols), _p(x, _fp), _p(r, _fp))
        return r

    def transpose(self, h, rows, cols):
        h = h16(h)
        t = np.zeros(rows * cols, np.uint16)
        self.L.rh_transpose(_p(h, _u16), _u64(rows), _u64(cols), _p(t, _u16))
        return t

    def is_transpose(self, h, rows, cols, ht):
        return bool(self.L.rh_is_transpose(_p(h16(h), _u16), _u64(rows), _u64(cols), _p(h16(ht), _u16)))

    def mvm64(self, A, rows, cols, x):
        A, x = h16(A), h16(x)
        e, a = np.zeros(rows), np.zeros(rows)
        self.L.rh_mvm64(_p(A, _u16), _u64(rows), _u64(cols), _p(x, _u16), _p(e, _dp), _p(a, _dp))
        return e, a

    def mvm_f32_64(self, A, rows, cols, x):
        A, x = h16(A), np.ascontiguousarray(x, dtype=np.float32)
        e, a = np.zeros(rows), np.zeros(rows)
        self.L.rh_mvm_f32_64(_p(A, _u16), _u64(rows), _u64(cols), _p(x, _fp), _p(e, _dp), _p(a, _dp))
        return e, a

    def threshold_heap(self, h, n, k):
        """(thresholded copy, heap values, heap indices) of the reference's walk, 1 <= k <= n"""
        out = h16(h).copy()
        hv, hi = np.zeros(k, np.float32), np.zeros(k, np.uint32)
        self.L.rh_threshold_heap(_p(out, _u16), _u64(n), _u64(k), _p(hv, _fp), _p(hi, _u32))
        return out, hv, hi

    def threshold(self, h, n, k):
        """CloverVector16::threshold(k) as the ABI reads it: k >= n keeps everything, k = 0 keeps nothing"""
        if k >= n:
            return h16(h).copy()
        if k == 0:
            out = h16(h).copy()
            out[:n] = 0
            return out
        return self.threshold_heap(h, n, k)[0]

    def make_heap_of(self, values):
        values = np.ascontiguousarray(values, dtype=np.float32)
        hv, hi = np.zeros(values.size, np.float32), np.zeros(values.size, np.uint32)
        self.L.rh_make_heap_of(_p(values, _fp), _u64(values.size), _p(hv, _fp), _p(hi, _u32))
        return hv, hi


@functools.lru_cache(maxsize=None)
def _build(out: Path, flags: tuple) -> Path:
    subprocess.run(["cc", "-O2", "-ffp-contract=off", "-fno-fast-math", *flags, "-fPIC", "-shared", "-o", str(out), str(RESTATE), "-lm"], check=True)
    return out


def build_restate(base: Path, parallel: bool) -> Restate:
    return Restate(_build(base / ("librh16_omp.so" if parallel else "librh16.so"), ("-mfma", "-fopenmp") if parallel else ()))


@pytest.fixture(scope="module")
def rh(tmp_path_factory):
    return build_restate(tmp_path_factory.getbasetemp(), parallel=False)


@pytest.fixture(scope="module")
def rhp(tmp_path_factory):
    return build_restate(tmp_path_factory.getbasetemp(), parallel=True)


# ---------------------------------------------------------------- the float64 bound
def gamma(k):
    return k * U32 / (1.0 - k * U32)


def chain_bound(absum, n):
    """|d - exact| for the fp32 value d of the 32-chain order over n elements.

    The product of two f16 values has 22 significant bits and the product of an f16 and an fp32 value 35: either way fma(a, b, acc)
    rounds acc + a b ONCE.  An element passes through the n / 32 fmas of its chain (at most: the first of them adds to zero and is exact
    unless it underflows, which f16 x f16 >= 2^-48 and the data of these tests cannot) and then through the five additions of the tree
    (acc0 + acc1, sum0 + sum1, and the three levels of the horizontal add), each of relative error <= u = 2^-24.  With the usual
    gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability, lemma 3.1):  |d - exact| <= gamma_(n / 32 + 5) * sum |terms|."""
    return gamma(n // 32 + 5) * absum


def assert_chain_bound(d, exact, absum, n, what=""):
    lim = chain_bound(absum, n)
    err = np.abs(np.asarray(d, np.float64) - exact)
    bad = np.flatnonzero(~(err <= lim))
    assert bad.size == 0, (what, bad[:8], np.asarray(d)[bad[:8]], exact[bad[:8]], lim[bad[:8]])


def assert_f16_result_bound(r_bits, exact, absum, n, what=""):
    """the f16 result of mvm: the fp32 row value d (chain_bound) rounded to nearest, i.e. within u16 |d| + 2^-25 of d -- relative in the
    normal range, absolute half a subnormal step below it; rows whose |exact| + bound reaches 65520 may round to infinity and are checked
    for that only"""
    r = np.asarray(r_bits, np.uint16).view(np.float16).astype(np.float64)
    cb = chain_bound(absum, n)
    may_overflow = np.abs(exact) + cb >= 65520.0
    lim = cb + U16 * (np.abs(exact) + cb) + F16_TINY
    fin = ~may_overflow
    err = np.abs(r[fin] - exact[fin])
    bad = np.flatnonzero(~(err <= lim[fin]))
    assert bad.size == 0, (what, bad[:8], r[fin][bad[:8]], exact[fin][bad[:8]], lim[fin][bad[:8]])
    must = np.abs(exact) - cb >= 65520.0
    assert np.all(np.isinf(r[must])), what


# ---------------------------------------------------------------- data
def f16_midpoints():
    """every fp32 value that lies exactly between two neighbouring f16 values (normal and subnormal range, both signs), with its fp32
    neighbours either side: 3 x 2 x 63487 inputs.  Midpoints need 12 significant bits: exact in fp32."""
    h = np.arange(0, 0x7C00, dtype=np.uint16)                      # every finite non-negative f16; the midpoint above 65504 is 65520
    lo = h.view(np.float16).astype(np.float64)
    hi = np.concatenate([lo[1:], [65536.0]])
    mid = ((lo + hi) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (lo + hi) / 2)
    b = mid.view(np.uint32)
    pos = np.concatenate([b - 1, b, b + 1]).astype(np.uint32).view(np.float32)
    return np.concatenate([pos, -pos])


def make_f32(kind, n, seed):
    """fp32 inputs of the value kinds the conversion has to get right"""
    rng = np.random.default_rng(seed)
    if kind == "gaussian":
        return (rng.normal(size=n) * 3).astype(np.float32)
    if kind == "ties":
        m = f16_midpoints()
        return m[rng.integers(0, m.size, size=n)]
    if kind == "subnormal":                                         # results in the f16 subnormal range, and below it
        return (rng.uniform(-1, 1, size=n) * np.exp2(rng.integers(-27, -13, size=n))).astype(np.float32)
    if kind == "overflow":                                          # around the overflow boundary 65520 and far beyond it
        v = np.array([65504.0, 65519.996, 65520.0, 65520.004, 65536.0, 1e5, 3e38, np.inf], np.float32)
        x = v[rng.integers(0, v.size, size=n)] * rng.choice(np.array([-1, 1], np.float32), size=n)
        return x.astype(np.float32)
    if kind == "zeros":
        return rng.choice(np.array([0.0, -0.0, 1.0, -1.0, 2.0 ** -26, -2.0 ** -26], np.float32), size=n).astype(np.float32)
    if kind == "nan":
        x = (rng.normal(size=n)).astype(np.float32)
        x[rng.integers(0, n, size=max(n // 16, 1))] = np.nan
        return x
    raise ValueError(kind)


def random_f16_bits(rng, n, lo=-8, hi=8, subnormal_share=0.0):
    """n finite f16 bit patterns: normal magnitudes 2^U(lo, hi) of either sign, a share of them subnormal instead"""
    v = (rng.choice([-1.0, 1.0], size=n) * np.exp2(rng.uniform(lo, hi, size=n))).astype(np.float16).view(np.uint16)
    if subnormal_share:
        sub = rng.random(n) < subnormal_share
        v[sub] = (rng.integers(1, 0x400, size=int(sub.sum())) | (rng.integers(0, 2, size=int(sub.sum())) << 15)).astype(np.uint16)
    return v


def pad128(n):
    return (n + 127) // 128 * 128


# ---------------------------------------------------------------- device calls on buffers (so that an 8 GiB matrix is uploaded once)
def _ptr(b):
    return b if isinstance(b, int) else b.ptr


class Dev:
    def __init__(self, hip):
        self.hip, self.L = hip, hip.lib

    def get(self, buf, dtype, n, off=0):
        out = np.empty(n, dtype)
        self.hip.check(self.L.clv_memcpy_d2h(out.ctypes.data, _ptr(buf) + off, out.nbytes, None))
        return out

    def mvm(self, dA, rows, cols, hx):
        dx, dr = self.hip.to_device(h16(hx)), self.hip.alloc(max(2 * rows, 2))
        self.hip.check(self.L.clm_f16_mvm(_ptr(dA), rows, cols, dx.ptr, dr.ptr, None))
        return self.get(dr, np.uint16, rows)

    def mvm_f32(self, dA, rows, cols, x):
        dx, dr = self.hip.to_device(np.ascontiguousarray(x, np.float32)), self.hip.alloc(max(4 * rows, 4))
        self.hip.check(self.L.clm_f16_mvm_f32(_ptr(dA), rows, cols, dx.ptr, dr.ptr, None))
        return self.get(dr, np.float32, rows)

    def transpose(self, dh, rows, cols):
        dt = self.hip.alloc(2 * rows * cols)
        self.hip.check(self.L.clm_f16_transpose(_ptr(dh), rows, cols, dt.ptr, None))
        return dt
