"""CloverMatrix8 (the reference's include/CloverMatrix8.h): quantize, restore, mvm with 8-bit and fp32 vectors, transpose.

The checker is tests/matrix8_restate.c, a plain-C restatement of the reference's SIMD order compiled here with
cc -O2 -ffp-contract=off -fno-fast-math and linked against the oracle for the XORShift stream (orc_rng_draw).  The CPU tests pin the
restatement against a float64 scalar definition; the GPU tests hold the device bit for bit to the restatement."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from clover_amd.build import repo_root
from conftest import bits

ROOT = repo_root()
RESTATE = Path(__file__).parent / "matrix8_restate.c"

_i8 = C.POINTER(C.c_int8)
_fp = C.POINTER(C.c_float)
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


@pytest.fixture(scope="module")
def m8(oracle, tmp_path_factory):
    out = tmp_path_factory.mktemp("m8") / "librm8.so"
    odir = ROOT / "oracle"            # liboracle.so exists: the oracle fixture builds it
    subprocess.run(["cc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-o", str(out), str(RESTATE),
                    f"-L{odir}", "-l:liboracle.so", f"-Wl,-rpath,{odir}", "-lm"], check=True)
    return Restate(out)


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


# ---------------------------------------------------------------- CPU: the restatement against float64 definitions
@pytest.mark.parametrize("seed", range(4))
def test_restatement_quantize_within_one_step(m8, seed):
    rng = np.random.default_rng(seed)
    rows, cols = 128 * int(rng.integers(1, 4)), 128 * int(rng.integers(1, 4))
    A = (rng.normal(size=(rows, cols)) * rng.uniform(0.1, 50)).astype(np.float32)
    q, s = m8.quantize(A)
    back = m8.restore(q, s, rows, cols).astype(np.float64)
    step = np.repeat(np.repeat(s.reshape(rows // 64, cols // 64).astype(np.float64) / 127.0, 64, 0), 64, 1)
    assert np.all(np.abs(back - A) <= step * (1 + 1e-4))
    assert np.all(np.abs(q) <= 127)
    tile_max = np.abs(A).reshape(rows // 64, 64, cols // 64, 64).max(axis=(1, 3)).astype(np.float32).ravel()
    assert same(s, tile_max)


def test_restatement_stochastic_quantize_within_one_step(m8, oracle):
    rng = np.random.default_rng(11)
    A = (rng.normal(size=(256, 384)) * 4).astype(np.float32)
    o = oracle.rng(3, 4)
    q, s = m8.quantize(A, o)
    back = m8.restore(q, s, 256, 384).astype(np.float64)
    step = np.repeat(np.repeat(s.reshape(4, 6).astype(np.float64) / 127.0, 64, 0), 64, 1)
    assert np.all(np.abs(back - A) <= step * (1 + 1e-4))
    qd, _ = m8.quantize(A)
    assert not np.array_equal(q, qd)           # the noise moved some values up a step


@pytest.mark.parametrize("seed", range(3))
def test_restatement_mvm_matches_float64(m8, oracle, seed):
    rng = np.random.default_rng(100 + seed)
    rows, cols = 128 * int(rng.integers(1, 4)), 128 * int(rng.integers(1, 6))
    qA, sA = m8.quantize((rng.normal(size=(rows, cols))).astype(np.float32))
    x, qx, sx = v8_inputs(oracle, cols, seed)
    A64 = m8.restore(qA, sA, rows, cols).astype(np.float64)
    x64 = oracle.v8_restore(qx, sx).astype(np.float64)
    exact = A64 @ x64
    d = m8.rowdots(qA, sA, rows, cols, qx, sx).astype(np.float64)
    scale = np.abs(A64) @ np.abs(x64) + 1e-30
    assert np.all(np.abs(d - exact) <= 1e-5 * scale)
    r, sr = m8.mvm(qA, sA, rows, cols, qx, sx)
    back = oracle.v8_restore(r, sr).astype(np.float64)
    assert np.all(np.abs(back - d) <= np.repeat(sr.astype(np.float64), 64) / 127.0 * (1 + 1e-4))
    # fp32 vector
    f = m8.mvm_f32(qA, sA, rows, cols, x).astype(np.float64)
    exact32 = A64 @ x.astype(np.float64)
    assert np.all(np.abs(f - exact32) <= 1e-5 * (np.abs(A64) @ np.abs(x.astype(np.float64)) + 1e-30))


def test_restatement_transpose_is_the_transpose(m8):
    rng = np.random.default_rng(5)
    rows, cols = 256, 384
    q = rng.integers(-127, 128, size=rows * cols).astype(np.int8)
    s = rng.uniform(0.1, 3, size=(rows // 64) * (cols // 64)).astype(np.float32)
    qt, st = m8.transpose(q, s, rows, cols)
    assert np.array_equal(qt.reshape(cols, rows), q.reshape(rows, cols).T)
    assert same(st.reshape(cols // 64, rows // 64), s.reshape(rows // 64, cols // 64).T)


def test_matrix8_header_compiles_standalone_and_dropin_client(tmp_path):
    inc = ROOT / "include"
    subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-x", "c++", f"-I{inc}", str(inc / "CloverMatrix8.h")], check=True)
    client = tmp_path / "m8_client.cpp"
    client.write_text(r'''
#include <CloverMatrix8.h>
#include <CloverIHT.h>
#include <iostream>
int main() {
    const uint64_t m = 128, n = 256;
    CloverMatrix32 A32(m, n);
    CloverMatrix8 A(m, n), At(n, m);
    A.quantize(A32);
    A.quantize_parallel(A32);
    A.quantize_scalar(A32);
    A.restore(A32);
    (void) A.get(1, 2);
    CloverVector8 x(n), r(m);
    CloverVector32 x32(n), r32(m);
    A.mvm(x, r);
    A.mvm_parallel(x, r);
    A.mvm_scalar(x, r);
    A.mvm(x32, r32);
    A.mvm_parallel(x32, r32);
    A.transpose(At);
    A.transpose_parallel(At);
    A.transpose_scalar(At);
    std::cout << A.getRows() << A.getCols() << A.getBytes() << A.getBitsLength() << A.toString().size() << std::endl;
    CloverVector8 y(m), xi(n), t1(m), t2(m), t3(n);
    Q_IHT<CloverMatrix8, CloverVector8>(A, At, xi, y, t1, t2, t3, 3, 10, 0.5f);
    Q_GD<CloverMatrix8, CloverVector8>(A, At, xi, y, t1, t2, t3, 3, 0.5f);
    return 0;
}
''')
    subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Wextra", f"-I{inc}", str(client)], check=True)


def _build_c_client(tmp_path):
    from clover_amd.build import build_hip_library
    lib = build_hip_library()
    exe = tmp_path / "matrix8_from_c"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "c" / "matrix8_from_c.c"),
                    "-o", str(exe), f"-L{lib.parent}", "-lclover_hip", f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lm"],
                   check=True)
    return exe


def test_clm8_calls_compile_and_link_from_c99(tmp_path):
    """the clm8_* declarations are plain C: a C99 client compiles with -pedantic, links, and runs (without a device it only reports that)"""
    p = subprocess.run([str(_build_c_client(tmp_path))], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and ("ok=1" in p.stdout or "no_device" in p.stdout), (p.returncode, p.stdout, p.stderr)


@pytest.mark.gpu
def test_gpu_c_client(tmp_path):
    p = subprocess.run([str(_build_c_client(tmp_path))], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "ok=1" in p.stdout and "bad_shape=-1" in p.stdout, (p.returncode, p.stdout, p.stderr)


# ---------------------------------------------------------------- GPU: bit for bit against the restatement
SMALL = [(128 * i, 128 * j) for i in range(1, 5) for j in range(1, 5)]
KINDS = ["normal", "zero_tiles", "extremes"]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_quantize_restore_small_shapes(hip, m8, kind):
    for rows, cols in SMALL:
        A = make_matrix(kind, rows, cols, rows * 31 + cols)
        q, s = hip.m8_quantize(A)
        qo, so = m8.quantize(A)
        assert same(q, qo) and same(s, so), (kind, rows, cols)
        assert same(hip.m8_restore(q, s, rows, cols), m8.restore(qo, so, rows, cols)), (kind, rows, cols)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_quantize_restore_ragged_and_8192(hip, m8, kind):
    # ragged: a 300 x 500 matrix padded with zeros to 384 x 512, as CloverMatrix pads (CloverMatrix.h:49-50)
    A = np.zeros((384, 512), np.float32)
    A[:300, :500] = make_matrix(kind, 384, 512, 7)[:300, :500]
    for M in (A, make_matrix(kind, 8192, 8192, 8)):
        rows, cols = M.shape
        q, s = hip.m8_quantize(M)
        qo, so = m8.quantize(M)
        assert same(q, qo) and same(s, so), (kind, rows, cols)
        assert same(hip.m8_restore(q, s, rows, cols), m8.restore(qo, so, rows, cols))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(384, 512), (2048, 4096)])
def test_gpu_quantize_stochastic_same_stream(hip, m8, oracle, shape):
    """(2048, 4096): 2048 tiles = 2048 workgroups, each jumping to its own place in the stream"""
    rows, cols = shape
    A = make_matrix("normal", rows, cols, rows + cols)
    st, o = hip.new_rng(21, 43), oracle.rng(21, 43)
    for _ in range(2):
        q, s = hip.m8_quantize(A, rng=st)
        qo, so = m8.quantize(A, o)
        assert same(q, qo) and same(s, so)
    k1, k2 = hip.rng_get(st)
    o1, o2 = oracle.rng_keys(o)
    assert np.array_equal(k2, o2) and np.array_equal(k1, o1)


@pytest.mark.gpu
def test_gpu_mvm_small_shapes(hip, m8, oracle):
    for rows, cols in SMALL + [(384, 512), (64, 128)]:
        qA, sA = m8.quantize(make_matrix("normal", rows, cols, rows + 7 * cols))
        x, qx, sx = v8_inputs(oracle, cols, rows)
        r, sr = hip.m8_mvm(qA, sA, rows, cols, qx, sx)
        ro, sro = m8.mvm(qA, sA, rows, cols, qx, sx)
        assert same(r, ro) and same(sr, sro), (rows, cols)
        assert same(hip.m8_mvm_f32(qA, sA, rows, cols, x), m8.mvm_f32(qA, sA, rows, cols, x)), (rows, cols)


@pytest.mark.gpu
def test_gpu_mvm_zero_and_extreme_tiles(hip, m8, oracle):
    rows, cols = 256, 384
    for kind in ("zero_tiles", "extremes"):
        qA, sA = m8.quantize(make_matrix(kind, rows, cols, 3))
        sA = np.where(sA > 1e30, np.float32(1e30), sA).astype(np.float32)       # keep the products finite
        x, qx, sx = v8_inputs(oracle, cols, 4)
        r, sr = hip.m8_mvm(qA, sA, rows, cols, qx, sx)
        ro, sro = m8.mvm(qA, sA, rows, cols, qx, sx)
        assert same(r, ro) and same(sr, sro), kind
        assert same(hip.m8_mvm_f32(qA, sA, rows, cols, x), m8.mvm_f32(qA, sA, rows, cols, x)), kind
    # an all-zero vector: every row value 0, every scale 1.0
    qz, sz = np.zeros(cols, np.int8), np.ones(cols // 64, np.float32)
    r, sr = hip.m8_mvm(qA, sA, rows, cols, qz, sz)
    assert not r.any() and np.all(sr == 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(384, 640), (8192, 1024)])
def test_gpu_mvm_stochastic_same_stream(hip, m8, oracle, shape):
    """(8192, 1024): 128 row groups, each workgroup at its own offset of the stream"""
    rows, cols = shape
    qA, sA = m8.quantize(make_matrix("normal", rows, cols, 9))
    x, qx, sx = v8_inputs(oracle, cols, 10)
    st, o = hip.new_rng(5, 9), oracle.rng(5, 9)
    for _ in range(2):
        r, sr = hip.m8_mvm(qA, sA, rows, cols, qx, sx, rng=st)
        ro, sro = m8.mvm(qA, sA, rows, cols, qx, sx, o)
        assert same(r, ro) and same(sr, sro)
    assert np.array_equal(hip.rng_get(st)[1], oracle.rng_keys(o)[1])
    assert np.array_equal(hip.rng_get(st)[0], oracle.rng_keys(o)[0])


@pytest.mark.gpu
def test_gpu_mvm_whole_32768(hip, m8, oracle):
    n = 32768
    rng = np.random.default_rng(32768)
    qA = rng.integers(-127, 128, size=n * n, dtype=np.int8)
    sA = rng.uniform(0.5, 2.0, size=(n // 64) ** 2).astype(np.float32)
    x, qx, sx = v8_inputs(oracle, n, 1)
    r, sr = hip.m8_mvm(qA, sA, n, n, qx, sx)
    ro, sro = m8.mvm(qA, sA, n, n, qx, sx)
    assert same(r, ro) and same(sr, sro)
    assert same(hip.m8_mvm_f32(qA, sA, n, n, x), m8.mvm_f32(qA, sA, n, n, x))


@pytest.mark.gpu
def test_gpu_transpose(hip, m8):
    for rows, cols in SMALL + [(384, 1152), (1280, 256)]:
        rng = np.random.default_rng(rows * 3 + cols)
        q = rng.integers(-127, 128, size=rows * cols, dtype=np.int8)
        s = rng.uniform(0.1, 3, size=(rows // 64) * (cols // 64)).astype(np.float32)
        qt, st = hip.m8_transpose(q, s, rows, cols)
        qto, sto = m8.transpose(q, s, rows, cols)
        assert same(qt, qto) and same(st, sto), (rows, cols)
        q2, s2 = hip.m8_transpose(qt, st, cols, rows)
        assert same(q2, q) and same(s2, s), (rows, cols)


@pytest.mark.gpu
def test_gpu_bad_arguments(hip):
    buf = hip.alloc(1 << 16)
    L = hip.lib
    assert L.clm8_quantize(buf.ptr, 100, 128, buf.ptr, buf.ptr, None, None) == -1
    assert b"multiples of 128" in L.clv_last_error()
    assert L.clm8_mvm(buf.ptr, buf.ptr, 96, 128, buf.ptr, buf.ptr, buf.ptr, buf.ptr, None, None) == -1
    assert L.clm8_mvm_f32(None, buf.ptr, 128, 128, buf.ptr, buf.ptr, None) == -1
    assert L.clm8_transpose(buf.ptr, buf.ptr, 128, 128, buf.ptr, buf.ptr, None) == -1
    assert L.clm8_restore(buf.ptr, buf.ptr, 128, 130, buf.ptr, None) == -1
    assert L.clm8_quantize(buf.ptr, 0, 0, buf.ptr, buf.ptr, None, None) == 0


# ---------------------------------------------------------------- GPU: the drop-in header, and Q_IHT / Q_GD through the generic templates
def _read8(path, n_values, n_scales):
    raw = np.fromfile(path, dtype=np.uint8)
    assert raw.size == n_values + 4 * n_scales
    return raw[:n_values].view(np.int8), raw[n_values:].view(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["iht", "gd"])
def test_gpu_header_mvm_agree_and_q_iht_loop(tmp_path, m8, oracle, mode):
    """mvm == mvm_parallel == mvm_scalar through CloverMatrix8.h (rounding disabled), then Q_IHT<CloverMatrix8, CloverVector8> at N = 1024
    (m = N / 2, K = N / 4) or Q_GD on its 1.5 N x N shape, 10 iterations: x, t1, t2, t3 equal a host loop of the restatement's mvm and
    the oracle's CloverVector8 scaleAndAdd / threshold (the default build's threshold is the reference's heap walk, as the oracle's)"""
    from clover_amd.build import build_hip_library
    lib = build_hip_library()
    exe = tmp_path / "matrix8_dropin"
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-DCLOVER_STOCHASTIC_ROUNDING_DISABLED=1", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "cpp" / "matrix8_dropin.cpp"), "-o", str(exe), f"-L{lib.parent}", "-lclover_hip",
                    f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    N = 1024
    m, n = (N // 2, N) if mode == "iht" else (3 * N // 2, N)
    K, iters, mu = N // 4, 10, 0.5
    rng = np.random.default_rng(1024)
    phi = (rng.normal(size=(m, n)) / np.sqrt(m)).astype(np.float32)
    x_true = np.zeros(n, np.float32)
    x_true[rng.choice(n, K, replace=False)] = rng.normal(size=K).astype(np.float32)
    y = (phi @ x_true).astype(np.float32)
    phi.tofile(tmp_path / "phi.f32")
    y.tofile(tmp_path / "y.f32")
    out = subprocess.run([str(exe), str(tmp_path), mode, str(m), str(n), str(iters), str(K), str(mu)], check=True, capture_output=True,
                         text=True, timeout=600).stdout
    assert "mvm_equal=1 mvm_f32_equal=1" in out and "done" in out, out

    qP, sP = _read8(tmp_path / "phi.bin", m * n, (m // 64) * (n // 64))
    qPo, sPo = m8.quantize(phi)
    assert same(qP, qPo) and same(sP, sPo)
    qT, sT = _read8(tmp_path / "phit.bin", m * n, (m // 64) * (n // 64))
    qTo, sTo = m8.transpose(qPo, sPo, m, n)
    assert same(qT, qTo) and same(sT, sTo)
    qy, sy = _read8(tmp_path / "y.bin", m, m // 64)
    qyo, syo = oracle.v8_quantize(y)
    assert same(qy, qyo) and same(sy, syo)
    xq = _read8(tmp_path / "xq.bin", n, n // 64)
    r1 = _read8(tmp_path / "r1.bin", m, m // 64)
    ro = m8.mvm(qPo, sPo, m, n, *xq)
    assert same(r1[0], ro[0]) and same(r1[1], ro[1])

    x = (np.zeros(n, np.int8), np.ones(n // 64, np.float32))
    for _ in range(iters):
        t1 = m8.mvm(qPo, sPo, m, n, *x)
        t2 = oracle.v8_scale_and_add(qyo, syo, t1[0], t1[1], -1.0)
        t3 = m8.mvm(qTo, sTo, n, m, *t2)
        x = oracle.v8_scale_and_add(x[0], x[1], t3[0], t3[1], mu)
        if mode == "iht":
            x = (oracle.v8_threshold(x[0], x[1], n, K), x[1])
    for name, ref, length in (("x", x, n), ("t1", t1, m), ("t2", t2, m), ("t3", t3, n)):
        got = _read8(tmp_path / f"{name}.bin", length, length // 64)
        assert same(got[0], ref[0]) and same(got[1], ref[1]), name
    assert np.count_nonzero(x[0]) > 0
