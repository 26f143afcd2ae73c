"""Shared checkers of the CloverMatrix8 tests (tests/test_matrix8.py, tests/test_matrix8_scale.py, tests/test_graph_capture.py).

- Restate: tests/matrix8_restate.c, the plain-C restatement of the reference's SIMD order, built twice: `m8` as cc -O2
  -ffp-contract=off -fno-fast-math (the checker of the small shapes), `m8p` the same with -mfma -fopenmp (at most 16 threads) for the
  large ones.  test_matrix8.py checks that the two builds agree bit for bit.
- Exact64: tests/matrix8_exact64.c, float64 definitions of the two mvm forms, and the error bounds a device output must meet against
  them (not through the restatement).
- inputs: make_matrix / v8_inputs, full-range bytes and scales spread over many binades built in chunks."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

from clover_amd.build import repo_root
from conftest import bits

ROOT = repo_root()
RESTATE = Path(__file__).parent / "matrix8_restate.c"
EXACT64 = Path(__file__).parent / "matrix8_exact64.c"
U = 2.0 ** -24              # fp32 unit roundoff
STEP_SLACK = 2.0 ** -16     # one quantisation step is exceeded by at most 2^-18 (the rounded fma before the truncation) + 127 u (the
                            # rounded k = 127 / m): 1.15e-5 of a step

_i8 = C.POINTER(C.c_int8)
_fp = C.POINTER(C.c_float)
_dp = C.POINTER(C.c_double)
_u64 = C.c_uint64


class Restate:
    def __init__(self, so: Path):
        self.L = C.CDLL(str(so))

    @staticmethod
    def _p(a, t):
        return a.ctypes.data_as(t)

    def quantize(self, A, rng=None):
        A = np.ascontiguousarray(A, dtype=np.float32)
        rows, cols = A.shape
        q = np.zeros(rows * cols, np.int8)
        s = np.zeros((rows // 64) * (cols // 64), np.float32)
        self.L.rm8_quantize(self._p(A, _fp), _u64(rows), _u64(cols), self._p(q, _i8), self._p(s, _fp), C.byref(rng) if rng is not None else None)
        return q, s

    def restore(self, q, s, rows, cols):
        A = np.zeros(rows * cols, np.float32)
        self.L.rm8_restore(self._p(q, _i8), self._p(s, _fp), _u64(rows), _u64(cols), self._p(A, _fp))
        return A.reshape(rows, cols)

    def mvm(self, qA, sA, rows, cols, qx, sx, rng=None):
        r = np.zeros(rows, np.int8)
        sr = np.zeros(rows // 64, np.float32)
        self.L.rm8_mvm(self._p(qA, _i8), self._p(sA, _fp), _u64(rows), _u64(cols), self._p(qx, _i8), self._p(sx, _fp), self._p(r, _i8),
                       self._p(sr, _fp), C.byref(rng) if rng is not None else None)
        return r, sr

    def rowdots(self, qA, sA, rows, cols, qx, sx):
        d = np.zeros(rows, np.float32)
        self.L.rm8_rowdots(self._p(qA, _i8), self._p(sA, _fp), _u64(rows), _u64(cols), self._p(qx, _i8), self._p(sx, _fp), self._p(d, _fp))
        return d

    def mvm_f32(self, qA, sA, rows, cols, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        r = np.zeros(rows, np.float32)
        self.L.rm8_mvm_f32(self._p(qA, _i8), self._p(sA, _fp), _u64(rows), _u64(cols), self._p(x, _fp), self._p(r, _fp))
        return r

    def transpose(self, q, s, rows, cols):
        qt = np.zeros(rows * cols, np.int8)
        st = np.zeros((rows // 64) * (cols // 64), np.float32)
        self.L.rm8_transpose(self._p(q, _i8), self._p(s, _fp), _u64(rows), _u64(cols), self._p(qt, _i8), self._p(st, _fp))
        return qt, st


class Exact64:
    """(exact, absum) per row: the float64 value and the sum of its terms' magnitudes"""

    def __init__(self, so: Path):
        self.L = C.CDLL(str(so))

    def mvm8(self, qA, sA, rows, cols, qx, sx):
        e, a = np.zeros(rows), np.zeros(rows)
        self.L.x64_mvm8(qA.ctypes.data_as(_i8), sA.ctypes.data_as(_fp), _u64(rows), _u64(cols), qx.ctypes.data_as(_i8),
                        sx.ctypes.data_as(_fp), e.ctypes.data_as(_dp), a.ctypes.data_as(_dp))
        return e, a

    def mvm_f32(self, qA, sA, rows, cols, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        e, a = np.zeros(rows), np.zeros(rows)
        self.L.x64_mvm_f32(qA.ctypes.data_as(_i8), sA.ctypes.data_as(_fp), _u64(rows), _u64(cols), x.ctypes.data_as(_fp),
                           e.ctypes.data_as(_dp), a.ctypes.data_as(_dp))
        return e, a


@functools.lru_cache(maxsize=None)
def _build(out: Path, source: Path, flags: tuple, with_oracle: bool) -> Path:
    odir = ROOT / "oracle"            # liboracle.so exists: the oracle fixture builds it
    link = [f"-L{odir}", "-l:liboracle.so", f"-Wl,-rpath,{odir}"] if with_oracle else []
    subprocess.run(["cc", "-O2", "-ffp-contract=off", "-fno-fast-math", *flags, "-fPIC", "-shared", "-o", str(out), str(source), *link, "-lm"],
                   check=True)
    return out


def build_restate(base: Path, parallel: bool) -> Restate:
    flags = ("-mfma", "-fopenmp") if parallel else ()
    return Restate(_build(base / ("librm8_omp.so" if parallel else "librm8.so"), RESTATE, flags, True))


@pytest.fixture(scope="module")
def m8(oracle, tmp_path_factory):
    return build_restate(tmp_path_factory.getbasetemp(), parallel=False)


@pytest.fixture(scope="module")
def m8p(oracle, tmp_path_factory):
    return build_restate(tmp_path_factory.getbasetemp(), parallel=True)


@pytest.fixture(scope="module")
def x64(tmp_path_factory):
    return Exact64(_build(tmp_path_factory.getbasetemp() / "libx64.so", EXACT64, ("-fopenmp",), False))


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        return np.array_equal(bits(a), bits(b))
    return np.array_equal(a, b)


def make_matrix(kind, rows, cols, seed):
    rng = np.random.default_rng(seed)
    if kind == "normal":
        return (rng.normal(size=(rows, cols)) * 3).astype(np.float32)
    if kind == "zero_tiles":
        A = (rng.normal(size=(rows, cols))).astype(np.float32)
        for bi in range(rows // 64):
            for bj in range(cols // 64):
                if (bi + 2 * bj) % 3 == 0:
                    A[64 * bi:64 * bi + 64, 64 * bj:64 * bj + 64] = 0.0
        return A
    if kind == "extremes":
        vals = np.array([3.0e38, -3.0e38, 1e-38, -1e-38, 1e-45, 0.0, -0.0, 1.0, -1.0, 126.99, 65504.0], np.float32)
        A = rng.choice(vals, size=(rows, cols)).astype(np.float32)
        A[:64, :64] = rng.choice(vals[2:5], size=(64, 64))           # a tile whose maximum makes 127 / m overflow
        return A
    raise ValueError(kind)


def v8_inputs(oracle, cols, seed):
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=cols) * 3).astype(np.float32)
    return x, *oracle.v8_quantize(x)


CHUNK = 1 << 28


def full_range_bytes(rng, n):
    """n random int8 over the whole range, -128 mapped to -127 (a quantiser never writes it), generated 256 MiB at a time"""
    q = np.empty(n, np.int8)
    for o in range(0, n, CHUNK):
        c = q[o:o + CHUNK]
        c[:] = np.frombuffer(rng.bytes(c.size), np.int8)
        np.maximum(c, -127, out=c)
    return q


def binade_scales(rng, n, lo=-20, hi=20):
    """n positive fp32 scales 2^U(lo, hi): the chains of a product over many binades round at every step"""
    return np.exp2(rng.uniform(lo, hi, size=n)).astype(np.float32)


# ---------------------------------------------------------------- float64 bounds (u = 2^-24; L = the chain length of the kernel's order)
def assert_mvm8_bound(r, sr, exact, absum, cols, what=""):
    """8-bit mvm: L = cols / 64 fma per lane chain, the block factor f32(f32(su / 127) f32(sv / 127)) and the three-level tree:
    |d - exact| <= (L + 6) u sum|terms| for the fp32 row value d; the re-quantised value is within one step sr / 127 of d; sr is max |d|
    of its row group (1.0 if all are zero)"""
    L = cols // 64
    chain = (L + 6) * U * absum
    step = np.repeat(sr.astype(np.float64), 64) / 127.0
    back = r.astype(np.float64) * step
    err = np.abs(back - exact)
    lim = step * (1 + STEP_SLACK) + chain
    bad = np.flatnonzero(err > lim)
    assert bad.size == 0, (what, "restore(r) vs float64", bad[:8], err[bad[:8]], lim[bad[:8]])
    emax = np.abs(exact).reshape(-1, 64).max(axis=1)
    cmax = chain.reshape(-1, 64).max(axis=1)
    zero = absum.reshape(-1, 64).max(axis=1) == 0
    assert np.all(sr[zero] == 1.0), what
    dev = np.abs(sr.astype(np.float64) - emax)
    bad = np.flatnonzero(~zero & (dev > cmax))
    assert bad.size == 0, (what, "sr vs max |exact|", bad[:8], sr[bad[:8]], emax[bad[:8]], cmax[bad[:8]])


def assert_mvm_f32_bound(f, exact, absum, cols, what=""):
    """fp32-vector mvm: L = cols / 32 fma per accumulator, f32(x f32(s / 127)) and the five adds of the tree: (L + 8) u sum|terms|"""
    lim = (cols // 32 + 8) * U * absum
    err = np.abs(f.astype(np.float64) - exact)
    bad = np.flatnonzero(~(err <= lim))
    assert bad.size == 0, (what, bad[:8], f[bad[:8]], exact[bad[:8]], lim[bad[:8]])


def assert_quantize_bound(A, q, s, band_rows=2048, what=""):
    """every restored element within one step s / 127 of its input, and s bit-equal to the tile's largest |A| (1.0 for a zero tile);
    checked in bands of rows so that a 2^30-element matrix needs no float64 copy of itself"""
    rows, cols = A.shape
    hb = cols // 64
    q = q.reshape(rows, cols)
    s = s.reshape(rows // 64, hb)
    for r0 in range(0, rows, band_rows):
        r1 = min(rows, r0 + band_rows)
        Ab = A[r0:r1]
        tmax = np.abs(Ab).reshape((r1 - r0) // 64, 64, hb, 64).max(axis=(1, 3))
        tmax = np.where(tmax == 0, np.float32(1.0), tmax)
        assert same(s[r0 // 64:r1 // 64], tmax), (what, r0)
        step = np.repeat(np.repeat(s[r0 // 64:r1 // 64].astype(np.float64) / 127.0, 64, 0), 64, 1)
        err = np.abs(q[r0:r1].astype(np.float64) * step - Ab)
        assert np.all(err <= step * (1 + STEP_SLACK)), (what, r0, float((err / step).max()))


# ---------------------------------------------------------------- device calls
def _ptr(b):
    return b if isinstance(b, int) else b.ptr


class Dev:
    """the clm8_* calls on device buffers, so that a 4 GiB matrix is uploaded once"""

    def __init__(self, hip):
        self.hip, self.L = hip, hip.lib

    def get(self, buf, dtype, n, off=0):
        out = np.empty(n, dtype)
        self.hip.check(self.L.clv_memcpy_d2h(out.ctypes.data, buf.offset(off), out.nbytes, None))
        return out

    def mvm(self, dA, dsA, rows, cols, qx, sx, rng=None):
        dx, dsx = self.hip.to_device(qx), self.hip.to_device(sx)
        dr, dsr = self.hip.alloc(rows), self.hip.alloc(rows // 16)
        self.hip.check(self.L.clm8_mvm(_ptr(dA), _ptr(dsA), rows, cols, dx.ptr, dsx.ptr, dr.ptr, dsr.ptr, rng.ptr if rng else None, None))
        return self.get(dr, np.int8, rows), self.get(dsr, np.float32, rows // 64)

    def mvm_f32(self, dA, dsA, rows, cols, x):
        dx, dr = self.hip.to_device(np.ascontiguousarray(x, np.float32)), self.hip.alloc(4 * rows)
        self.hip.check(self.L.clm8_mvm_f32(_ptr(dA), _ptr(dsA), rows, cols, dx.ptr, dr.ptr, None))
        return self.get(dr, np.float32, rows)

    def transpose(self, dq, ds, rows, cols):
        dt, dst = self.hip.alloc(rows * cols), self.hip.alloc((rows // 64) * (cols // 64) * 4)
        self.hip.check(self.L.clm8_transpose(_ptr(dq), _ptr(ds), rows, cols, dt.ptr, dst.ptr, None))
        return dt, dst

    def quantize(self, A, rng=None):
        rows, cols = A.shape
        dA = self.hip.to_device(A)
        dq, ds = self.hip.alloc(rows * cols), self.hip.alloc((rows // 64) * (cols // 64) * 4)
        self.hip.check(self.L.clm8_quantize(dA.ptr, rows, cols, dq.ptr, ds.ptr, rng.ptr if rng else None, None))
        del dA
        return self.get(dq, np.int8, rows * cols), self.get(ds, np.float32, (rows // 64) * (cols // 64))


def same_keys(hip, st, oracle, o):
    k1, k2 = hip.rng_get(st)
    o1, o2 = oracle.rng_keys(o)
    return np.array_equal(k1, o1) and np.array_equal(k2, o2)


