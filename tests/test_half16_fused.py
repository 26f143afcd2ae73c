"""clm_f16_mvm_scale_and_add (the half-precision mvm with the CloverVector16::scaleAndAdd behind it in its epilogue), the one-workgroup FAST
threshold of CloverVector16 (k_f16_thresh_small) and clm_f16_iht (the whole half-precision Q_IHT / Q_GD loop in one call), through the C
ABI, the containers and CloverIHT.h.

Every comparison is on bits; the one exception is the project's standing one: where the reference is a NaN the result has to be a NaN,
its payload is not compared.  The reference side is never the new code: it is the CPU restatement (tests/half16_restate.c: mvm,
scale_and_add, threshold) and lowest_index_threshold of tests/test_half16.py composed in Python, and the device calls that existed before
-- clm_f16_mvm, clv_f16_scale_and_add, clv_f16_threshold_mode on its large-vector path -- issued one after another.

The guard-band cases of the new calls are registered with tests/test_guard_bands.py's own case table when this module is imported (its
coverage test counts every prototype of clover_amd.lib_binding.SIGNATURES) and run here; the capture cases likewise with the list of
tests/test_half16_capture.py, whose coverage test counts every f16 prototype."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_guard_bands as gb
import test_half16_capture as cap
from clover_amd.build import repo_root
from clover_amd.lib_binding import THRESHOLD_FAST, THRESHOLD_REFERENCE, load_library
from half16_helpers import pad128, random_f16_bits, rh, rhp  # noqa: F401
from matrix8_helpers import m8  # noqa: F401
from test_guard_bands import refs  # noqa: F401
from test_half16 import lowest_index_threshold

ROOT = repo_root()
INC = ROOT / "include"


def is_nan16(h):
    return (np.asarray(h, np.uint16) & 0x7FFF) > 0x7C00


def same16(got, want):
    """bit equality of two binary16 arrays; where `want` is a NaN, `got` has to be one (payload not compared)"""
    got, want = np.asarray(got, np.uint16), np.asarray(want, np.uint16)
    nan = is_nan16(want)
    return got.shape == want.shape and np.array_equal(got[~nan], want[~nan]) and bool(np.all(is_nan16(got[nan])))


# ---------------------------------------------------------------- CPU: the ABI from C, the headers' routing, the container methods, arguments
def _build_c_client(tmp_path):
    from clover_amd.build import build_hip_library
    lib = build_hip_library()
    exe = tmp_path / "half16_fused_from_c"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{INC}", str(ROOT / "tests" / "c" / "half16_fused_from_c.c"),
                    "-o", str(exe), f"-L{lib.parent}", "-lclover_hip", f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"],
                   check=True)
    return exe


def test_fused_calls_compile_and_link_from_c99(tmp_path):
    """the two declarations are plain C: a C99 client compiles with -pedantic, links, and runs (without a device it only reports that)"""
    p = subprocess.run([str(_build_c_client(tmp_path))], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and ("ok=1" in p.stdout or "no_device" in p.stdout), (p.returncode, p.stdout, p.stderr)


ROUTING_CLIENT = r'''
#include <CloverIHT.h>
void loops(CloverMatrix16 &Phi, CloverMatrix16 &PhiT, CloverVector16 &x, CloverVector16 &y, CloverVector16 &t1, CloverVector16 &t2, CloverVector16 &t3)
{
#ifdef DEDUCED
    Q_IHT(Phi, PhiT, x, y, t1, t2, t3, 3, 10, 0.5f);
    Q_GD(Phi, PhiT, x, y, t1, t2, t3, 3, 0.5f);
#else
    Q_IHT<CloverMatrix16, CloverVector16>(Phi, PhiT, x, y, t1, t2, t3, 3, 10, 0.5f);
    Q_GD<CloverMatrix16, CloverVector16>(Phi, PhiT, x, y, t1, t2, t3, 3, 0.5f);
#endif
}
'''


def _undefined_symbols(tmp_path, name, source, flags):
    src, obj = tmp_path / f"{name}.cpp", tmp_path / f"{name}.o"
    src.write_text(source)
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", *flags, f"-I{INC}", "-c", str(src), "-o", str(obj)], check=True)
    out = subprocess.run(["nm", "-u", str(obj)], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


@pytest.mark.parametrize("stochastic_build", [False, True])
@pytest.mark.parametrize("spelling", ["explicit", "deduced"])
def test_header_routes_the_half_precision_loops(tmp_path, spelling, stochastic_build):
    """Q_IHT / Q_GD for (CloverMatrix16, CloverVector16), template arguments spelled out or deduced, call clm_f16_iht and none of the
    separate steps -- whether or not the build disables stochastic rounding: the 16-bit classes have none"""
    flags = (["-DDEDUCED"] if spelling == "deduced" else []) + ([] if stochastic_build else ["-DCLOVER_STOCHASTIC_ROUNDING_DISABLED=1"])
    syms = _undefined_symbols(tmp_path, "route16", ROUTING_CLIENT, flags)
    ours = sorted(s for s in syms if s.startswith("cl"))
    assert "clm_f16_iht" in syms, ours
    assert "clm_f16_mvm" not in syms and "clv_f16_scale_and_add" not in syms and "clm_f16_mvm_scale_and_add" not in syms, ours


@pytest.mark.parametrize("explicit", [False, True])
def test_container_methods_compile(tmp_path, explicit):
    """CloverMatrix16::mvm_scaleAndAdd (both overloads) and iht_loop, in the tracked and the explicit-sync builds"""
    client = tmp_path / "f16_fused_client.cpp"
    client.write_text(r'''
#include <CloverMatrix16.h>
int main() {
    const uint64_t m = 128, n = 256;
    const CloverMatrix16 A(m, n), At(n, m);
    CloverVector16 x(n), y(m), u(m), t1(m), t2(m), t3(n);
    A.mvm_scaleAndAdd(x, u, -1.0f, t1, t2);
    A.mvm_scaleAndAdd(x, u, 0.5f, t1);
    A.iht_loop(At, x, y, t1, t2, t3, 3, 10, 0.5f, true);
    A.iht_loop(At, x, y, t1, t2, t3, 3, 0, 0.5f, false);
    return 0;
}
''')
    flags = ["-DCLOVER_HIP_EXPLICIT_SYNC"] if explicit else []
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", *flags, f"-I{INC}", "-c", str(client), "-o", str(tmp_path / "client.o")], check=True)


def test_fused_argument_checks_answer_without_a_device():
    """integer pointers: every violation is CLV_ERR_INVALID with a message before any pointer is used or any device work is done"""
    lib = load_library()
    err = lambda: lib.clv_last_error().decode()                                # noqa: E731
    A, x, u, t, r = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000

    def fused(A=A, rows=64, cols=128, x=x, u=u, t=t, r=r):
        return lib.clm_f16_mvm_scale_and_add(A, rows, cols, x, u, 0.5, t, r, None)
    for what, kw, word in (("A NULL", dict(A=None), "null"), ("x NULL", dict(x=None), "null"), ("u NULL", dict(u=None), "null"),
                           ("r NULL", dict(r=None), "null"), ("cols = 100", dict(cols=100), "multiple of 128"), ("t == x", dict(t=x), "alias"),
                           ("r == x", dict(r=x), "alias"), ("t == r", dict(t=r), "alias"), ("t == u", dict(t=u), "alias"),
                           ("A misaligned", dict(A=A + 8), "aligned"), ("x misaligned", dict(x=x + 2), "aligned"),
                           ("r at an odd address", dict(r=r + 1), "aligned")):
        rc = fused(**kw)
        assert rc == -1 and word in err(), (what, rc, err())
    assert fused(rows=0) == 0 and fused(rows=0, t=None) == 0                  # nothing to do: no device work either

    def iht(m=128, n=256, x_len=256, thr=1, Phi=A, y=u):
        return lib.clm_f16_iht(Phi, 0x9000, m, n, x, x_len, y, t, r, 0x6000, 2, 8, 0.5, thr, None)
    for what, kw, word in (("m = 64", dict(m=64), "m=64"), ("n = 192", dict(n=192), "n=192"), ("x_len > n", dict(x_len=257), "x_len=257"),
                           ("threshold = 3", dict(thr=3), "threshold 3"), ("threshold = -1", dict(thr=-1), "threshold -1"),
                           ("Phi NULL", dict(Phi=None), "null"), ("y NULL", dict(y=None), "null")):
        rc = iht(**kw)
        assert rc == -1 and word in err(), (what, rc, err())


# ---------------------------------------------------------------- GPU 1: the fused call = the two calls = the restatement
# x is staged 8192 f16 at a time, a full step of the row loop is 256 columns, a tail step 32
SHAPES = [(8, 128),          # one-wave workgroup, mostly tail rows; four tail steps
          (24, 256),         # exactly one full step
          (100, 384),        # full step + tail steps, ragged rows
          (128, 8192),       # exactly one x chunk
          (144, 8320),       # a second chunk of tail steps only
          (32808, 128)]      # the four-wave workgroup (rows / 64 >= 2 x 256 CUs) with a 40-row tail
STREAMING = [(16440, 8320), (32808, 4224)]      # one per workgroup form, both just past the 256 MiB nontemporal rule
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


def _reference(R, A, rows, cols, x, u):
    t = R.mvm(A, rows, cols, x)
    return t, {a: R.scale_and_add(u, t, np.float32(a)) for a in SCALES}


def _two_calls(hip, dA, rows, cols, x, u, a):
    """clm_f16_mvm then clv_f16_scale_and_add; the vector call takes whole CloverVector16 lengths, so t and u go in zero-padded to 128"""
    n_pad = pad128(rows)
    up = np.zeros(n_pad, np.uint16)
    up[:rows] = u
    dx, du, dt, dr = hip.to_device(x), hip.to_device(up), hip.to_device(np.zeros(n_pad, np.uint16)), hip.alloc(2 * n_pad)
    hip.check(hip.lib.clm_f16_mvm(dA.ptr, rows, cols, dx.ptr, dt.ptr, None))
    hip.check(hip.lib.clv_f16_scale_and_add(du.ptr, dt.ptr, a, n_pad, dr.ptr, None))
    return dt.download(np.uint16, rows), dr.download(np.uint16, rows)


def _check_kind(kind, t, r):
    if kind == "subnormal":
        assert np.any((t & 0x7C00 == 0) & (t & 0x3FF != 0)) and np.any((r[0.5] & 0x7C00 == 0) & (r[0.5] & 0x3FF != 0))
    if kind == "overflow":
        assert t[0] == 0x7C00 and t[1] == 0xFC00 and r[-1.0][0] == 0xFC00 and r[0.5][1] == 0xFC00 and is_nan16(r[0.0][:2]).all()
    if kind == "negzero":
        assert np.any(r[-1.0] == 0x8000) and np.any(t == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_gpu_fused_equals_the_two_calls_and_the_restatement(hip, rh, rhp, shape):  # noqa: F811
    rows, cols = shape
    for kind in (KINDS if rows * cols <= 1 << 22 else KINDS[:1]):
        A, x, u = _operands(kind, rows, cols)
        t_ref, r_ref = _reference(rhp if rows * cols > 1 << 20 else rh, A, rows, cols, x, u)
        _check_kind(kind, t_ref, r_ref)
        dA = hip.to_device(A)
        for a in SCALES:
            td, rd = _two_calls(hip, dA, rows, cols, x, u, a)
            assert same16(td, t_ref) and same16(rd, r_ref[a]), (kind, a, "the two calls")
            for want_t in (True, False):
                t, r = hip.mf16_mvm_scale_and_add(dA, rows, cols, x, u, a, want_t=want_t)
                assert same16(r, r_ref[a]), (kind, a, want_t, np.flatnonzero(r != r_ref[a])[:8])
                assert t is None or same16(t, t_ref), (kind, a, np.flatnonzero(t != t_ref)[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(100, 384), (144, 8320)])
def test_gpu_fused_in_place(hip, rh, shape):  # noqa: F811
    rows, cols = shape
    A, x, u = _operands("uniform", rows, cols)
    t_ref, r_ref = _reference(rh, A, rows, cols, x, u)
    for a in SCALES:
        for want_t in (True, False):
            t, r = hip.mf16_mvm_scale_and_add(A, rows, cols, x, u, a, in_place=True, want_t=want_t)
            assert same16(r, r_ref[a]) and (t is None or same16(t, t_ref)), (a, want_t)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", STREAMING)
def test_gpu_fused_streaming_loads(hip, rhp, shape):  # noqa: F811
    rows, cols = shape
    assert rows * cols * 2 > 256 << 20
    A, x, u = _operands("uniform", rows, cols)
    t_ref, r_ref = _reference(rhp, A, rows, cols, x, u)
    dA = hip.to_device(A)
    td, rd = _two_calls(hip, dA, rows, cols, x, u, -1.0)
    assert same16(td, t_ref) and same16(rd, r_ref[-1.0])
    for a, want_t in ((-1.0, True), (0.5, False)):
        t, r = hip.mf16_mvm_scale_and_add(dA, rows, cols, x, u, a, want_t=want_t)
        assert same16(r, r_ref[a]) and (t is None or same16(t, t_ref)), (a, np.flatnonzero(r != r_ref[a])[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("k", [16, 40])
def test_gpu_fused_on_row_shards_at_pointer_offsets(hip, rh, k):  # noqa: F811
    """A + k cols, u + k, t + k, r + k: the shard's rows equal the whole-matrix call's, the rows before it keep their prefill"""
    rows, cols, a = 100, 384, -1.0
    A, x, u = _operands("uniform", rows, cols)
    t_full, r_full = hip.mf16_mvm_scale_and_add(A, rows, cols, x, u, a)
    t_ref, r_ref = _reference(rh, A, rows, cols, x, u)
    assert same16(t_full, t_ref) and same16(r_full, r_ref[a])
    dA, dx, du, dt, dr = hip.to_device(A), hip.to_device(x), hip.to_device(u), hip.alloc(2 * rows), hip.alloc(2 * rows)
    for b in (dt, dr):
        hip.check(hip.lib.clv_memset(b.ptr, 0xEE, 2 * rows, None))
    hip.check(hip.lib.clm_f16_mvm_scale_and_add(dA.ptr + 2 * k * cols, rows - k, cols, dx.ptr, du.ptr + 2 * k, a, dt.ptr + 2 * k, dr.ptr + 2 * k, None))
    t, r = dt.download(np.uint16, rows), dr.download(np.uint16, rows)
    assert same16(t[k:], t_full[k:]) and same16(r[k:], r_full[k:])
    assert np.all(t[:k] == 0xEEEE) and np.all(r[:k] == 0xEEEE)


# ---------------------------------------------------------------- GPU 2: the one-workgroup threshold
# every W of the kernel (words per thread: n <= 2048 -> 1, 4096 -> 2, 8192 -> 4, 16384 -> 8, 32768 -> 16), odd n, n < n_pad, and the
# first n_pad beyond the dispatch limit
THRESH_N = [1, 2, 127, 128, 129, 2047, 2048, 2049, 4096, 8191, 8192, 16384, 32767, 32768, 32896 - 37]
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


def _threshold_switch(hip, h, n, k, small):
    if not small:
        os.environ["CLV_F16_THRESHOLD_SMALL"] = "0"
    try:
        return hip.f16_threshold(h, n, k, THRESHOLD_FAST)
    finally:
        os.environ.pop("CLV_F16_THRESHOLD_SMALL", None)


@pytest.mark.gpu
@pytest.mark.parametrize("n", THRESH_N)
def test_gpu_small_threshold_follows_the_lowest_index_rule_and_the_large_path(hip, n):
    n_pad = pad128(n)
    for kind in THRESH_KINDS:
        h = _threshold_vector(kind, n, n_pad)
        for k in sorted({0, 1, n // 4, n - 1}):
            want = lowest_index_threshold(h, n, k)
            got = _threshold_switch(hip, h, n, k, small=True)
            assert np.array_equal(got, want), (kind, n, k, np.flatnonzero(got != want)[:8])
            large = _threshold_switch(hip, h, n, k, small=False)
            assert np.array_equal(large, got), (kind, n, k, "CLV_F16_THRESHOLD_SMALL=0", np.flatnonzero(large != got)[:8])


# ---------------------------------------------------------------- GPU 3: clm_f16_iht
IHT_SHAPES = [(128, 256, 256), (256, 128, 100), (384, 640, 600)]          # (m, n, x_len)
MU = 0.5
ITERS = (0, 1, 2, 3, 5)
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


def _threshold_cpu(R, x, x_len, K, thr):
    return R.threshold(x, x_len, K) if thr == 2 else lowest_index_threshold(x, x_len, K)


_TRAJECTORIES = {}


def _cpu_loop(R, m, n, x_len, K, thr):
    """{iterations: dict(x, t1, t2, t3)} of the Python loop over the restatement, computed once per case"""
    key = (m, n, x_len, K, thr)
    if key not in _TRAJECTORIES:
        Phi, PhiT, y = _iht_problem(R, m, n)
        x, out = np.zeros(n, np.uint16), {0: dict(x=np.zeros(n, np.uint16))}
        for it in range(1, max(ITERS) + 1):
            t1 = R.mvm(Phi, m, n, x)
            t2 = R.scale_and_add(y, t1, np.float32(-1.0))
            t3 = R.mvm(PhiT, n, m, t2)
            x = R.scale_and_add(x, t3, np.float32(MU))
            if thr:
                x = _threshold_cpu(R, x, x_len, K, thr)
            out[it] = dict(x=x, t1=t1, t2=t2, t3=t3)
        _TRAJECTORIES[key] = out
    return _TRAJECTORIES[key]


def _device_loop(hip, Phi, PhiT, y, m, n, x_len, iters, K, thr):
    """the loop launch by launch with the calls that existed before the fused ones"""
    L = hip.lib
    d = [hip.to_device(v) for v in (Phi, PhiT, y)]
    x = hip.to_device(np.zeros(n, np.uint16))
    lens = dict(t1=m, t2=m, t3=n)
    v = {k: hip.alloc(2 * ln) for k, ln in lens.items()}
    for _ in range(iters):
        hip.check(L.clm_f16_mvm(d[0].ptr, m, n, x.ptr, v["t1"].ptr, None))
        hip.check(L.clv_f16_scale_and_add(d[2].ptr, v["t1"].ptr, -1.0, m, v["t2"].ptr, None))
        hip.check(L.clm_f16_mvm(d[1].ptr, n, m, v["t2"].ptr, v["t3"].ptr, None))
        hip.check(L.clv_f16_scale_and_add(x.ptr, v["t3"].ptr, MU, n, x.ptr, None))
        if thr:
            hip.check(L.clv_f16_threshold_mode(x.ptr, x_len, n, K, THRESHOLD_REFERENCE if thr == 2 else THRESHOLD_FAST, None, None))
    out = dict(x=x.download(np.uint16, n))
    out.update({k: v[k].download(np.uint16, ln) for k, ln in lens.items()})
    return out


@pytest.mark.parametrize("mode", range(3))
@pytest.mark.parametrize("shape", IHT_SHAPES)
def test_the_loop_problems_keep_the_threshold_busy(rh, shape, mode):  # noqa: F811
    """on the CPU reference alone: the iterates stay finite, and by the last iteration x has at least K non-zeros among its first x_len
    elements before the threshold cuts them (so the threshold does real work), exactly K after it"""
    m, n, x_len = shape
    name, thr, K = _modes(x_len)[mode]
    traj = _cpu_loop(rh, m, n, x_len, K, thr)
    for it in ITERS[1:]:
        for k, v in traj[it].items():
            assert np.all(v & 0x7C00 != 0x7C00), (name, it, k)
    last = traj[max(ITERS)]
    Phi, PhiT, y = _iht_problem(rh, m, n)
    before = rh.scale_and_add(traj[max(ITERS) - 1]["x"] if max(ITERS) > 1 else np.zeros(n, np.uint16), last["t3"], np.float32(MU))
    assert np.count_nonzero(before[:x_len] & 0x7FFF) >= max(K, 1), name
    if thr:
        assert np.count_nonzero(last["x"][:x_len] & 0x7FFF) == K, name
    else:
        assert np.array_equal(before, last["x"])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", range(3))
@pytest.mark.parametrize("shape", IHT_SHAPES)
def test_gpu_iht_call_equals_the_separate_calls_and_the_cpu_loop(hip, rh, shape, mode):  # noqa: F811
    m, n, x_len = shape
    name, thr, K = _modes(x_len)[mode]
    Phi, PhiT, y = _iht_problem(rh, m, n)
    traj = _cpu_loop(rh, m, n, x_len, K, thr)
    for iters in (0, 1, 5):
        got = hip.mf16_iht(Phi, PhiT, m, n, y, iters, K, MU, thr, x_len=x_len, prefill=0x55)
        dev = _device_loop(hip, Phi, PhiT, y, m, n, x_len, iters, K, thr)
        for k in ("x", "t1", "t2", "t3"):
            if iters == 0 and k != "x":
                assert np.all(got[k] == 0x5555), (name, k)           # untouched: the prefill
                continue
            for side, ref in (("cpu", traj[iters]), ("device", dev)):
                assert same16(got[k], ref[k]), (name, iters, k, side, np.flatnonzero(got[k] != ref[k])[:8])
        if iters == 0:
            assert not got["x"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", range(3))
def test_gpu_iht_call_clears_x_on_every_call(hip, rh, mode):  # noqa: F811
    """two iterations, then three, then five on the SAME buffers: every call starts from x = 0, so each equals the reference of its own
    iteration count (two then three is not five); a call of 0 iterations after them clears x and leaves t1..t3 as they were"""
    m, n, x_len = IHT_SHAPES[2]
    name, thr, K = _modes(x_len)[mode]
    Phi, PhiT, y = _iht_problem(rh, m, n)
    traj = _cpu_loop(rh, m, n, x_len, K, thr)
    d = [hip.to_device(v) for v in (Phi, PhiT, y)]
    lens = dict(x=n, t1=m, t2=m, t3=n)
    v = {k: hip.alloc(2 * ln) for k, ln in lens.items()}
    for iters in (2, 3, 5, 0):
        hip.check(hip.lib.clm_f16_iht(d[0].ptr, d[1].ptr, m, n, v["x"].ptr, x_len, d[2].ptr, v["t1"].ptr, v["t2"].ptr, v["t3"].ptr, iters, K, MU,
                                      thr, None))
        want = traj[iters] if iters else dict(traj[5], x=np.zeros(n, np.uint16))
        for k, ln in lens.items():
            assert same16(v[k].download(np.uint16, ln), want[k]), (name, iters, k)
    assert not same16(traj[3]["x"], traj[5]["x"])


# ---------------------------------------------------------------- GPU 4: the header loop
def _build_fused_client(tmp_path, explicit, fast):
    from clover_amd.build import build_hip_library
    lib = build_hip_library()
    exe = tmp_path / f"half16_fused_{'explicit' if explicit else 'tracked'}_{'fast' if fast else 'reference'}"
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", *(["-DCLOVER_HIP_EXPLICIT_SYNC"] if explicit else []),
                    *(["-DCLOVER_FAST"] if fast else []), f"-I{INC}", str(ROOT / "tests" / "cpp" / "half16_fused.cpp"), "-o", str(exe),
                    f"-L{lib.parent}", "-lclover_hip", f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("explicit", [False, True])
def test_gpu_header_specialised_loops_equal_the_method_calls(tmp_path, explicit, fast):
    """m = 256, n = 512: the specialised Q_IHT / Q_GD (CloverMatrix16::iht_loop -> clm_f16_iht) and mvm_scaleAndAdd give the digests of the
    method calls written out by hand, in both residency builds and under both exactness settings; a host pointer taken before the loop
    shows its result"""
    out = subprocess.run([str(_build_fused_client(tmp_path, explicit, fast)), "256", "512", "4", "64", "0.5"], check=True, capture_output=True,
                         text=True, timeout=300).stdout
    lines = {ln.split()[0]: dict(f.split("=") for f in ln.split()[1:]) for ln in out.splitlines() if "=" in ln and " " in ln}
    assert lines["pair"]["fused"] == lines["pair"]["separate"], out
    assert lines["iht"]["spec"] == lines["iht"]["hand"] and 0 < int(lines["iht"]["nonzero"]) <= 64, out
    assert lines["gd"]["spec"] == lines["gd"]["hand"] and lines["gd"]["spec"] != lines["iht"]["spec"], out
    assert "kept_pointer=1" in out and "done" in out, out


# ---------------------------------------------------------------- GPU 5: guard bands
def _scaled_matrix(seed, m, n):
    return (np.random.default_rng(seed).uniform(-1, 1, size=(m, n)) / np.sqrt(m)).astype(np.float32)


def _fused_case(rows, cols, with_t=True, in_place=False, shift=0):
    """shift: u, t and r start that many bytes behind a 256-byte boundary (they need only their element alignment)"""
    def build(R):
        A, x, u = gb.v16(rows * cols + 41, rows * cols), gb.v16(cols + 42, cols), gb.v16(rows + 43, rows)
        t = R.rh.mvm(A, rows, cols, x)
        r = R.rh.scale_and_add(u, t, np.float32(-0.5))
        regs, want = [("A", "input", A), ("x", "input", x)], {}
        if with_t:
            regs.append(("t", "output", 2 * rows, shift))
            want["t"] = t
        if in_place:
            regs.append(("u", "inout", u, shift))
            want["u"] = r
        else:
            regs += [("u", "input", u, shift), ("r", "output", 2 * rows, shift)]
            want["r"] = r
        return gb.Case(regs, lambda L, p: L.clm_f16_mvm_scale_and_add(p["A"], rows, cols, p["x"], p["u"], -0.5, p.get("t"),
                                                                      p["u" if in_place else "r"], None), want)
    return build


def _iht16_case(m, n, thr, iters=2):
    def build(R):
        x_len, K, mu = n - 5, n // 4, np.float32(0.5)
        Phi = R.rh.quantize(_scaled_matrix(m * n + 51, m, n)).ravel()
        PhiT = R.rh.transpose(Phi, m, n)
        y = gb.v16(m + 52, m)
        x = np.zeros(n, np.uint16)
        t1 = t2 = t3 = None
        for _ in range(iters):
            t1 = R.rh.mvm(Phi, m, n, x)
            t2 = R.rh.scale_and_add(y, t1, np.float32(-1.0))
            t3 = R.rh.mvm(PhiT, n, m, t2)
            x = R.rh.scale_and_add(x, t3, mu)
            if thr:
                x = gb.threshold_reference(R, 16, x, None, x_len, K, THRESHOLD_REFERENCE if thr == 2 else THRESHOLD_FAST)[0]
        want = dict(x=x, t1=t1, t2=t2, t3=t3)
        assert not any(np.any(v & 0x7C00 == 0x7C00) for v in want.values())
        regs = [("Phi", "input", Phi), ("PhiT", "input", PhiT), ("y", "input", y)] + [(k, "output", v.nbytes) for k, v in want.items()]
        return gb.Case(regs, lambda L, p: L.clm_f16_iht(p["Phi"], p["PhiT"], m, n, p["x"], x_len, p["y"], p["t1"], p["t2"], p["t3"], iters, K,
                                                        float(mu), thr, None), want)
    return build


FUSED_CASES = []
for _r, _c, _shift in [(64, 128, 0), (100, 256, 2)]:
    for _t in (True, False):
        FUSED_CASES.append((f"clm_f16_mvm_scale_and_add {_r}x{_c} t={_t}", _fused_case(_r, _c, with_t=_t, shift=_shift)))
    FUSED_CASES.append((f"clm_f16_mvm_scale_and_add {_r}x{_c} in place", _fused_case(_r, _c, in_place=True, shift=_shift)))
    FUSED_CASES.append((f"clm_f16_mvm_scale_and_add {_r}x{_c} in place t=False", _fused_case(_r, _c, with_t=False, in_place=True, shift=_shift)))
for _m, _n in [(128, 256), (256, 128)]:
    for _thr in (0, 1, 2):
        FUSED_CASES.append((f"clm_f16_iht {_m}x{_n} threshold={_thr}", _iht16_case(_m, _n, _thr)))
# the one-workgroup threshold with a caller workspace of exactly the size the query returns: exact outputs, the workspace left as it was
FUSED_CASES.append(("clv_f16_threshold_mode FAST n_pad=256 n=200 k=n/4 one workgroup, caller workspace",
                    gb._threshold(16, THRESHOLD_FAST, 256, gb.KS["n/4"], n=200, ws=lambda L, n_pad, k: L.clv_f16_threshold_workspace_bytes(n_pad),
                                  untouched=True)))
for _name, _build in FUSED_CASES:
    if _name not in gb.CASES:                 # the coverage test of test_guard_bands.py reads its table when it runs, after every module is imported
        gb.case(_name)(_build)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, _ in FUSED_CASES])
def test_gpu_fused_calls_write_their_outputs_and_nothing_else(hip, refs, name):  # noqa: F811
    case = dict(FUSED_CASES)[name](refs)
    gb.run_case(hip, case)
    if "caller workspace" in name:
        gb.run_case(hip, case, seed=11, scratch_fill=0xFF)


# ---------------------------------------------------------------- GPU 6: capture
def _capture_and_replay(hip, enqueue, outputs, set_inputs, wants):
    """capture `enqueue` on a non-default stream with the first inputs in place (after one ordinary warm call), then for every set of
    inputs: upload it into the same buffers, overwrite the outputs, replay the graph, and compare the outputs with that set's reference"""
    rt = C.CDLL("libamdhip64.so")
    stream, graph, gexec = C.c_void_p(), C.c_void_p(), C.c_void_p()

    def ok(rc):
        assert rc == 0, f"HIP runtime call failed: {rc}"
    ok(rt.hipStreamCreate(C.byref(stream)))
    set_inputs(0)
    enqueue(stream)
    ok(rt.hipStreamSynchronize(stream))
    ok(rt.hipStreamBeginCapture(stream, 0))
    enqueue(stream)
    ok(rt.hipStreamEndCapture(stream, C.byref(graph)))
    ok(rt.hipGraphInstantiate(C.byref(gexec), graph, None, None, 0))
    for i, want in enumerate(wants):
        set_inputs(i)
        for b in outputs:
            hip.check(hip.lib.clv_memset(b.ptr, 0xEE, b.nbytes, None))
        hip.sync()
        ok(rt.hipGraphLaunch(gexec, stream))
        ok(rt.hipStreamSynchronize(stream))
        for j, b in enumerate(outputs):
            assert same16(b.download(np.uint16), want[j]), (i, j)
    ok(rt.hipGraphExecDestroy(gexec))
    ok(rt.hipGraphDestroy(graph))
    ok(rt.hipStreamDestroy(stream))


# test_half16_capture.py's coverage test reads its list when it runs, after every module is imported; its own parametrisation was fixed
# when it was imported above, so these names only tell it that the two calls are captured here
CAPTURE_CASES = ["clm_f16_mvm_scale_and_add", "clm_f16_iht gd", "clm_f16_iht fast n=256"]
for _name in CAPTURE_CASES:
    if _name not in cap.CASES:
        cap.CASES.append(_name)


@pytest.mark.gpu
def test_gpu_captured_fused_call_replays_on_changed_inputs(hip, rh):  # noqa: F811
    rows, cols = 192, 640
    A, x0, u0 = _operands("uniform", rows, cols)
    _, x1, u1 = _operands("uniform", rows + 1, cols)
    u1 = u1[:rows].copy()
    dA, dx, du = hip.to_device(A), hip.alloc(2 * cols), hip.alloc(2 * rows)
    out = [hip.alloc(2 * rows), hip.alloc(2 * rows)]                                                # t, r
    sets = [(x0, u0), (x1, u1), (x0, u1)]
    wants = []
    for xs, us in sets:
        t = rh.mvm(A, rows, cols, xs)
        wants.append((t, rh.scale_and_add(us, t, np.float32(-1.0))))
    assert not np.array_equal(wants[0][0], wants[1][0])

    def set_inputs(i):
        dx.upload(sets[i][0])
        du.upload(sets[i][1])

    def enqueue(stream):
        hip.check(hip.lib.clm_f16_mvm_scale_and_add(dA.ptr, rows, cols, dx.ptr, du.ptr, -1.0, out[0].ptr, out[1].ptr, stream))
    _capture_and_replay(hip, enqueue, out, set_inputs, wants)


@pytest.mark.gpu
@pytest.mark.parametrize("thr", [0, 1])
def test_gpu_captured_loop_replays_on_changed_inputs(hip, rh, thr):  # noqa: F811
    """GD, and FAST at n = 256 (the one-workgroup threshold: no workspace, nothing to allocate under capture)"""
    m, n, iters, K = 128, 256, 2, 32
    Phi, PhiT, y0 = _iht_problem(rh, m, n)
    y1 = rh.scale_and_add(y0, y0[::-1].copy(), np.float32(0.5))
    d = [hip.to_device(v) for v in (Phi, PhiT)]
    dy = hip.alloc(2 * m)
    lens = (n, m, m, n)                                                                               # x, t1, t2, t3
    out = [hip.alloc(2 * ln) for ln in lens]
    wants = []
    for y in (y0, y1, y0):
        x = np.zeros(n, np.uint16)
        for _ in range(iters):
            t1 = rh.mvm(Phi, m, n, x)
            t2 = rh.scale_and_add(y, t1, np.float32(-1.0))
            t3 = rh.mvm(PhiT, n, m, t2)
            x = rh.scale_and_add(x, t3, np.float32(MU))
            if thr:
                x = lowest_index_threshold(x, n, K)
        wants.append((x, t1, t2, t3))
    assert not np.array_equal(wants[0][0], wants[1][0])

    def set_inputs(i):
        dy.upload((y0, y1, y0)[i])

    def enqueue(stream):
        hip.check(hip.lib.clm_f16_iht(d[0].ptr, d[1].ptr, m, n, out[0].ptr, n, dy.ptr, out[1].ptr, out[2].ptr, out[3].ptr, iters, K, MU, thr, stream))
    _capture_and_replay(hip, enqueue, out, set_inputs, wants)
