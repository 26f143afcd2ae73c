"""Shared pieces of the fp32 device tests (tests/test_fp32_device_cpu.py, test_fp32_device.py, test_fp32_guard_bands.py,
test_fp32_capture.py).

- Restate: tests/fp32_restate.cpp, extern "C" wrappers around the functions of include/clover_fp32.h (pinned by test_fp32_baseline.py),
  built twice: `rf` as c++ -O2 -ffp-contract=off -fno-fast-math, `rfp` the same with -mfma -fopenmp (at most 16 threads).
  test_fp32_device_cpu.py checks that the two builds agree bit for bit.
- the float64 bound of dot FAST: fast_dot_bound (derivation in its docstring).
- data: make_ops (the value kinds the kernels have to get right), threshold_data, iht_problem."""
import ctypes as C
import functools
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from clover_amd.build import repo_root

ROOT = repo_root()
RESTATE = Path(__file__).parent / "fp32_restate.cpp"
U32 = 2.0 ** -24             # fp32 unit roundoff

_fp = C.POINTER(C.c_float)
_dp = C.POINTER(C.c_double)
_up = C.POINTER(C.c_uint64)
_u64 = C.c_uint64

KINDS = ("magnitudes", "subnormal", "cancel", "zeros")


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def bits(a):
    return f32(a).reshape(-1).view(np.uint32)


def _p(a, t=_fp):
    return a.ctypes.data_as(t)


class Restate:
    def __init__(self, so: Path):
        self.L = L = C.CDLL(str(so))
        L.rf_dot.restype = C.c_float
        L.rf_dot_sequential.restype = C.c_float

    def dot(self, u, v):
        u, v = f32(u), f32(v)
        return np.float32(self.L.rf_dot(_p(u), _p(v), _u64(u.size)))

    def dot_sequential(self, u, v):
        u, v = f32(u), f32(v)
        return np.float32(self.L.rf_dot_sequential(_p(u), _p(v), _u64(u.size)))

    def dot64(self, u, v):
        """(float64 sum of the exact products, float64 sum of their magnitudes)"""
        u, v = f32(u), f32(v)
        e, a = C.c_double(), C.c_double()
        self.L.rf_dot64(_p(u), _p(v), _u64(u.size), C.byref(e), C.byref(a))
        return e.value, a.value

    def scale_and_add(self, u, v, s):
        u, v = f32(u), f32(v)
        r = np.zeros(u.size, np.float32)
        self.L.rf_scale_and_add(_p(u), _p(v), C.c_float(s), _p(r), _u64(u.size))
        return r

    def mvm(self, A, rows, cols, x):
        A, x = f32(A), f32(x)
        y = np.zeros(rows, np.float32)
        self.L.rf_mvm(_p(A), _u64(rows), _u64(cols), _p(x), _p(y))
        return y

    def mvm_sequential(self, A, rows, cols, x):
        A, x = f32(A), f32(x)
        y = np.zeros(rows, np.float32)
        self.L.rf_mvm_sequential(_p(A), _u64(rows), _u64(cols), _p(x), _p(y))
        return y

    def transpose(self, A, rows, cols):
        A = f32(A)
        t = np.zeros(rows * cols, np.float32)
        self.L.rf_transpose(_p(A), _u64(rows), _u64(cols), _p(t))
        return t

    def threshold(self, x, n, k):
        """clover_fp32::keep_top_k over the first n elements of a copy (k >= n keeps everything, k = 0 nothing)"""
        out = f32(x).copy()
        self.L.rf_threshold(_p(out), _u64(n), _u64(k))
        return out

    def iht(self, Phi, PhiT, m, n, y, iterations, K, mu, threshold, x_len=None):
        """the loop of shim functions: ({"x", "t1", "t2", "t3"}, non-zero elements each iteration's threshold cleared)"""
        Phi, PhiT, y = f32(Phi), f32(PhiT), f32(y)
        v = {"x": np.full(n, 7.0, np.float32), "t1": np.zeros(m, np.float32), "t2": np.zeros(m, np.float32), "t3": np.zeros(n, np.float32)}
        zeroed = np.zeros(max(iterations, 1), np.uint64)
        self.L.rf_iht(_p(Phi), _p(PhiT), _u64(m), _u64(n), _p(v["x"]), _u64(n if x_len is None else x_len), _p(y), _p(v["t1"]), _p(v["t2"]),
                      _p(v["t3"]), _u64(iterations), _u64(K), C.c_float(mu), C.c_int(threshold), _p(zeroed, _up))
        return v, zeroed[:iterations]


@functools.lru_cache(maxsize=None)
def _build(out: Path, flags: tuple) -> Path:
    subprocess.run(["c++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", *flags, f"-I{ROOT / 'include'}", "-fPIC", "-shared", "-o",
                    str(out), str(RESTATE), "-lm"], check=True)
    return out


def build_restate(base: Path, parallel: bool) -> Restate:
    return Restate(_build(base / ("librf32_omp.so" if parallel else "librf32.so"), ("-mfma", "-fopenmp") if parallel else ()))


@pytest.fixture(scope="module")
def rf(tmp_path_factory):
    return build_restate(tmp_path_factory.getbasetemp(), parallel=False)


@pytest.fixture(scope="module")
def rfp(tmp_path_factory):
    return build_restate(tmp_path_factory.getbasetemp(), parallel=True)


# ---------------------------------------------------------------- the float64 bound of dot FAST
def gamma(k):
    return k * U32 / (1.0 - k * U32)


def fast_dot_grid(n_pad, compute_units):
    """workgroups of k_f32_dot_fast1 as clv_f32_dot sizes it: one per 256 groups of 4 elements, at most 4 per CU and 2048"""
    return min((n_pad // 4 + 255) // 256, 4 * compute_units, 256 * 8)


def fast_dot_bound(absum, n_pad, compute_units):
    """|d - exact| for clv_f32_dot FAST, from the order k_f32_dot_fast1 fixes (clover_amd/csrc/fp32.hip, dot_common.h).

    Every product enters through one fma, acc = round(acc + u v): one rounding, the product itself exact.  The longest path from a
    product to the result then passes
      L - 1 further fmas of the lane's chain, L = ceil(n / 4 / (grid * 256)) groups per lane (grid: fast_dot_grid),
      2 additions inside the lane, (acc0 + acc2) + (acc1 + acc3),
      6 shuffle additions and 2 of the four wave sums in block_sum_256,
      at most DOT_MAX_SLOTS_PER_THREAD = 8 additions of the collecting thread over its slots,
      6 + 2 in the collector's block_sum_256,
    each of relative error <= u = 2^-24: D = L + 26 roundings, and with gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of
    Numerical Algorithms, lemma 3.1)  |d - exact| <= gamma_D * sum |u_i v_i|.  Underflow adds an absolute 2^-150 per rounding, which the
    data of the FAST tests (magnitudes 2^-6 .. 2^6) never meets."""
    L = -(-(n_pad // 4) // (fast_dot_grid(n_pad, compute_units) * 256))
    return gamma(L + 26) * absum


# ---------------------------------------------------------------- data
def pad128(n):
    return (n + 127) // 128 * 128


def _mags(rng, n, lo, hi):
    return (rng.choice([-1.0, 1.0], size=n) * np.exp2(rng.uniform(lo, hi, size=n))).astype(np.float32)


def make_ops(kind, rows, cols, seed):
    """(A[rows * cols], x[cols], a): a matrix and a vector of one value kind -- rows = 1 gives the two operands of a dot or, as (u, v, a),
    of scale_and_add.
      magnitudes  2^U(-6, 6) of either sign
      subnormal   operands near 2^-70: every product and most sums are fp32 subnormals, which a flushing instruction turns into 0
                  (a = near 2^-70 too, u of scale_and_add is A itself scaled into the subnormal range by the caller)
      cancel      the second half of every row repeats the first against -x (1 + 2^-12): the row sums cancel to within rounding, so a
                  product rounded before it is added shows; for scale_and_add u = -a v to within rounding
      zeros       0, -0, 1, -1: the signs of zero sums"""
    rng = np.random.default_rng(seed)
    n = rows * cols
    if kind == "magnitudes":
        return _mags(rng, n, -6, 6), _mags(rng, cols, -6, 6), np.float32(0.37)
    if kind == "subnormal":
        return _mags(rng, n, -73, -64), _mags(rng, cols, -73, -64), np.float32(1.37 * 2.0 ** -70)
    if kind == "cancel":
        half = cols // 2
        A = _mags(rng, n, -3, 3).reshape(rows, cols)
        x = _mags(rng, cols, -3, 3)
        A[:, half:] = A[:, :half]
        x[half:] = -x[:half] * np.float32(1 + 2.0 ** -12)
        return A.reshape(-1).copy(), x, np.float32(-0.3721)
    if kind == "zeros":
        vals = np.array([0.0, -0.0, 1.0, -1.0], np.float32)
        return vals[rng.integers(0, 4, size=n)], vals[rng.integers(0, 4, size=cols)], np.float32(-1.0)
    raise ValueError(kind)


def make_axpy(kind, n, seed):
    """(u, v, a) of scale_and_add for one value kind"""
    v, u, a = make_ops(kind, 1, n, seed)
    if kind == "subnormal":
        u = (u * np.float32(2.0 ** -70)).astype(np.float32)                # u itself subnormal, like the product v a
    if kind == "cancel":
        u = (-(v * a)).astype(np.float32)                                   # the ROUNDED product: fma(v, a, u) is the rounding error
    return u, v, a


def threshold_data(kind, n_pad, seed):
    """distinct: all magnitudes different (a permutation of n_pad values, random signs); ties: five magnitudes (0 among them) of either
    sign, so that any cut but the extremes falls inside a run of equal values"""
    rng = np.random.default_rng(seed)
    sign = rng.choice(np.array([-1.0, 1.0], np.float32), size=n_pad)
    if kind == "distinct":
        return (sign * rng.permutation(n_pad).astype(np.float32) * np.float32(0.25) + sign * np.float32(0.125)).astype(np.float32)
    if kind == "ties":
        return (sign * np.array([0.0, 0.5, 1.5, 1.5, 3.0], np.float32)[rng.integers(0, 5, size=n_pad)]).astype(np.float32)
    raise ValueError(kind)


def iht_problem(m, n, seed, ties=False):
    """(Phi[m * n], PhiT[n * m], y[m], mu): a Gaussian sensing matrix scaled by 1 / sqrt(m) and the measurements of a signal with
    n / 16 non-zeros.  ties: small integers everywhere (Phi in {-1, 0, 1}, three quarters of it 0, a signal of +-1, mu a power of two),
    so that Phi' y takes few distinct magnitudes and the first cut falls among equal ones."""
    rng = np.random.default_rng(seed)
    if ties:
        Phi = (rng.integers(-1, 2, size=(m, n)) * (rng.random((m, n)) < 0.25)).astype(np.float32)
        mu = np.float32(1.0 / (1 << int(np.ceil(np.log2(m / 4)))))
    else:
        Phi = (rng.normal(size=(m, n)) / np.sqrt(m)).astype(np.float32)
        mu = np.float32(0.5)
    sig = np.zeros(n, np.float32)
    sup = rng.choice(n, size=n // 16, replace=False)
    sig[sup] = rng.choice([-1.0, 1.0], size=sup.size) * (1.0 if ties else rng.uniform(1, 2, size=sup.size))
    y = (Phi.astype(np.float64) @ sig).astype(np.float32)
    return Phi.reshape(-1).copy(), np.ascontiguousarray(Phi.T).reshape(-1), y, mu


def fast_threshold_model(x, n, k):
    """what CLV_THRESHOLD_FAST leaves: every element above the k-th largest magnitude of the first n, then the lowest-index ones equal
    to it until k survive; survivors keep their bits, the others of the first n become +0, the padding stays"""
    out = f32(x).copy()
    if k >= n:
        return out
    mag = np.abs(out[:n])
    if k == 0:
        out[:n] = 0
        return out
    tau = np.partition(mag, n - k)[n - k]
    keep = mag > tau
    ties = np.flatnonzero(mag == tau)
    keep[ties[:k - int(keep.sum())]] = True
    out[:n][~keep] = 0
    return out


def with_project_headers(src, name, seen=None):
    """the text of a source of clover_amd/csrc together with the headers of that directory it includes, directly or not -- common.h
    excepted, which the whole library shares (its clv_env is for the families that read the environment)"""
    seen = {"common.h"} if seen is None else seen
    if name in seen or not (src / name).exists():
        return ""
    seen.add(name)
    text = (src / name).read_text()
    return text + "".join(with_project_headers(src, inc, seen) for inc in re.findall(r'^#include "([^"]+)"', text, flags=re.M))
