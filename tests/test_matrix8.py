"""CloverMatrix8 (the reference's include/CloverMatrix8.h): quantize, restore, mvm with 8-bit and fp32 vectors, transpose.

The checker is tests/matrix8_restate.c, a plain-C restatement of the reference's SIMD order compiled by tests/matrix8_helpers.py with
cc -O2 -ffp-contract=off -fno-fast-math and linked against the oracle for the XORShift stream (orc_rng_draw).  The CPU tests pin the
restatement against a float64 scalar definition; the GPU tests hold the device bit for bit to the restatement."""
import subprocess

import numpy as np
import pytest

from matrix8_helpers import (ROOT, Dev, assert_mvm8_bound, assert_mvm_f32_bound, binade_scales, full_range_bytes, m8, m8p,  # noqa: F401
                             make_matrix, same, same_keys, v8_inputs, x64)


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


@pytest.mark.parametrize("shape", [(128, 128), (384, 640), (1280, 2304), (64 * 65, 128)])
def test_restatement_parallel_build_is_the_serial_one(m8, m8p, oracle, shape):
    """the -mfma -fopenmp build (the checker of the large shapes) gives the serial build's bits, in both rounding modes, and leaves the
    generator where the serial build leaves it"""
    rows, cols = shape
    rows -= rows % 128
    rng = np.random.default_rng(rows + cols)
    A = (rng.normal(size=(rows, cols)) * np.exp2(rng.uniform(-20, 20, size=(rows, 1)))).astype(np.float32)
    x, qx, sx = v8_inputs(oracle, cols, rows)
    xr, qxr, sxr = v8_inputs(oracle, rows, cols)
    for keys in (None, (7, 11)):
        o1, o2 = (oracle.rng(*keys), oracle.rng(*keys)) if keys else (None, None)
        q1, s1 = m8.quantize(A, o1)
        q2, s2 = m8p.quantize(A, o2)
        assert same(q1, q2) and same(s1, s2), keys
        assert same(m8.rowdots(q1, s1, rows, cols, qx, sx), m8p.rowdots(q1, s1, rows, cols, qx, sx))
        r1, sr1 = m8.mvm(q1, s1, rows, cols, qx, sx, o1)
        r2, sr2 = m8p.mvm(q1, s1, rows, cols, qx, sx, o2)
        assert same(r1, r2) and same(sr1, sr2), keys
        assert same(m8.mvm_f32(q1, s1, rows, cols, x), m8p.mvm_f32(q1, s1, rows, cols, x))
        t1, st1 = m8.transpose(q1, s1, rows, cols)
        t2, st2 = m8p.transpose(q1, s1, rows, cols)
        assert same(t1, t2) and same(st1, st2)
        r1, sr1 = m8.mvm(t1, st1, cols, rows, qxr, sxr, o1)
        r2, sr2 = m8p.mvm(t1, st1, cols, rows, qxr, sxr, o2)
        assert same(r1, r2) and same(sr1, sr2), keys
        if keys:
            assert all(np.array_equal(a, b) for a, b in zip(oracle.rng_keys(o1), oracle.rng_keys(o2)))
    assert same(m8.restore(q1, s1, rows, cols), m8p.restore(q1, s1, rows, cols))


@pytest.mark.parametrize("cols", [128, 4096, 65536])
def test_restatement_within_float64_bounds_long_rows(m8p, x64, oracle, cols):
    """the restatement's mvm and mvm_f32 against float64 at up to 65536 columns, full-range bytes and scales over 40 binades: the
    bounds tests/matrix8_helpers.py also applies to the device outputs (the 1e-5 checks above stay)"""
    rows = 128
    rng = np.random.default_rng(cols)
    qA = full_range_bytes(rng, rows * cols)
    sA = binade_scales(rng, (rows // 64) * (cols // 64))
    qx = full_range_bytes(rng, cols)
    sx = binade_scales(rng, cols // 64)
    exact, absum = x64.mvm8(qA, sA, rows, cols, qx, sx)
    for keys in (None, (3, 5)):
        r, sr = m8p.mvm(qA, sA, rows, cols, qx, sx, oracle.rng(*keys) if keys else None)
        assert_mvm8_bound(r, sr, exact, absum, cols, keys)
    d = m8p.rowdots(qA, sA, rows, cols, qx, sx).astype(np.float64)
    assert np.all(np.abs(d - exact) <= (cols // 64 + 6) * 2.0 ** -24 * absum)
    x = (rng.normal(size=cols) * np.exp2(rng.uniform(-30, 30, size=cols))).astype(np.float32)
    assert_mvm_f32_bound(m8p.mvm_f32(qA, sA, rows, cols, x), *x64.mvm_f32(qA, sA, rows, cols, x), cols)


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


# ---------------------------------------------------------------- GPU: seeded shapes, row shards, numeric edges, two streams
@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(16))
def test_gpu_random_shapes_iht_chain(hip, m8p, oracle, seed):
    """the 8-bit counterpart of test_gpu_random_shapes.py: per seed a shape of 128 [1, 24] x 128 [1, 64], one of its four data kinds or
    "extremes", and the IHT loop's chain quantize -> transpose -> mvm (8-bit, A^T x) -> mvm_f32 (A times that result), each step fed
    the device's previous output, in both rounding modes; the generator state after the stochastic chain is the oracle's"""
    from test_gpu_random_shapes import _data
    rng = np.random.default_rng(8000 + seed)
    rows, cols = 128 * int(rng.integers(1, 25)), 128 * int(rng.integers(1, 65))
    kind = seed % 5
    A = make_matrix("extremes", rows, cols, seed) if kind == 4 else _data(rng, rows * cols, kind).reshape(rows, cols)
    x = _data(rng, rows, (seed + 1) % 4)
    qx, sx = oracle.v8_quantize(x)
    st, o = hip.new_rng(seed + 1, 1000 + seed), oracle.rng(seed + 1, 1000 + seed)
    for g, og in ((None, None), (st, o)):
        q, s = hip.m8_quantize(A, rng=g)
        qo, so = m8p.quantize(A, og)
        assert same(q, qo) and same(s, so), ("quantize", rows, cols, kind, g is None)
        if kind == 4:           # tiles of +-3e38: keep every later product finite (NaN and Inf are out of contract)
            s = so = np.minimum(s, np.float32(2.0 ** 40))
        qt, stt = hip.m8_transpose(q, s, rows, cols)
        qto, stto = m8p.transpose(qo, so, rows, cols)
        assert same(qt, qto) and same(stt, stto), ("transpose", rows, cols, kind)
        t, s_t = hip.m8_mvm(qt, stt, cols, rows, qx, sx, rng=g)
        to, s_to = m8p.mvm(qto, stto, cols, rows, qx, sx, og)
        assert same(t, to) and same(s_t, s_to), ("mvm", rows, cols, kind, g is None)
        xf = oracle.v8_restore(t, s_t)
        f = hip.m8_mvm_f32(q, s, rows, cols, xf)
        assert same(f, m8p.mvm_f32(qo, so, rows, cols, xf)), ("mvm_f32", rows, cols, kind)
        assert np.all(np.isfinite(f))
    assert same_keys(hip, st, oracle, o)


@pytest.mark.gpu
def test_gpu_mvm_row_shards(hip, m8p, oracle):
    """64 * odd rows of a 1024-row matrix, called at pointer offsets A + r0 cols, sA + (r0 / 64) (cols / 64): the rows of the whole call"""
    rows, cols = 1024, 1536
    rng = np.random.default_rng(1024)
    qA, sA = full_range_bytes(rng, rows * cols), binade_scales(rng, (rows // 64) * (cols // 64))
    qx, sx = full_range_bytes(rng, cols), binade_scales(rng, cols // 64)
    x = rng.standard_normal(cols, dtype=np.float32)
    dev, dA, dsA = Dev(hip), hip.to_device(qA), hip.to_device(sA)
    r, sr = dev.mvm(dA, dsA, rows, cols, qx, sx)
    f = dev.mvm_f32(dA, dsA, rows, cols, x)
    ro, sro = m8p.mvm(qA, sA, rows, cols, qx, sx)
    assert same(r, ro) and same(sr, sro) and same(f, m8p.mvm_f32(qA, sA, rows, cols, x))
    for r0, n in ((64, 64), (320, 192), (640, 320), (704, 320)):
        pA, psA = dA.offset(r0 * cols), dsA.offset(4 * (r0 // 64) * (cols // 64))
        rs, srs = dev.mvm(pA, psA, n, cols, qx, sx)
        assert same(rs, r[r0:r0 + n]) and same(srs, sr[r0 // 64:(r0 + n) // 64]), (r0, n)
        ros, sros = m8p.mvm(qA[r0 * cols:(r0 + n) * cols], sA[(r0 // 64) * (cols // 64):], n, cols, qx, sx)
        assert same(rs, ros) and same(srs, sros), (r0, n)
        fs = dev.mvm_f32(pA, psA, n, cols, x)
        assert same(fs, f[r0:r0 + n]), (r0, n)
        assert same(fs, m8p.mvm_f32(qA[r0 * cols:(r0 + n) * cols], sA[(r0 // 64) * (cols // 64):], n, cols, x)), (r0, n)


def _edge_operands():
    """A 384 x 256 matrix of six row groups and a vector whose block 1 has scale 0 and whose halves of every block are equal:
      rg 0: row l holds l - 32 in column 0 only, scale s_inf: the row values c (l - 32), c = f32(f32(s / 127) f32(1 / 127)), have a
            nonzero maximum m = 32 c below 127 / FLT_MAX, so 127 / m = inf;
      rg 1: the same with m just above that edge (ordinary bytes);
      rg 2: full-range bytes with a subnormal block factor c in every chain and normal row values;
      rg 3: even rows (v, -v) in the two halves of every block (each lane's integer dot is 0: the row value is exactly 0), odd rows
            full-range, scales over many binades;
      rg 4: full-range; rg 5: all zero (scale 1.0 after the re-quantisation)."""
    rows, cols = 384, 256
    rng = np.random.default_rng(384)
    qA = np.zeros((rows, cols), np.int8)
    qA[0:64, 0] = np.arange(64) - 32
    qA[64:128, 0] = np.arange(64) - 32
    qA[128:192] = full_range_bytes(rng, 64 * cols).reshape(64, cols)
    v = full_range_bytes(rng, 64 * cols).reshape(64, cols)
    qA[192:256] = v
    for b in range(cols // 64):
        qA[192:256:2, 64 * b + 32:64 * b + 64] = -v[0::2, 64 * b:64 * b + 32]
        qA[192:256:2, 64 * b:64 * b + 32] = v[0::2, 64 * b:64 * b + 32]
    qA[256:320] = full_range_bytes(rng, 64 * cols).reshape(64, cols)
    inv = np.float32(1 / 127)
    c_of = lambda s: np.float32(np.float32(np.float32(s) * inv) * np.float32(np.float32(1.0) * inv))     # noqa: E731
    s_inf, s_edge = np.float32(3.0e-37 / 32 * 127 * 127), np.float32(3.9e-37 / 32 * 127 * 127)
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(127) / (32 * c_of(s_inf))) and np.isfinite(np.float32(127) / (32 * c_of(s_edge)))
    sA = np.ones((rows // 64, cols // 64), np.float32)
    sA[0], sA[1], sA[2] = s_inf, s_edge, np.float32(1e-36)
    sA[3] = binade_scales(rng, cols // 64, -10, 10)         # x up to 2^100 in mvm_f32 stays finite: 2^100 2^10 127 cols < 2^128
    sA[4] = binade_scales(rng, cols // 64, -10, 10)
    qx = full_range_bytes(rng, cols)
    qx[0] = 1
    for b in range(cols // 64):
        qx[64 * b + 32:64 * b + 64] = qx[64 * b:64 * b + 32]
    sx = binade_scales(rng, cols // 64, -2, 2)
    sx[0], sx[1] = 1.0, 0.0
    assert c_of(1e-36) * sx.max() < np.finfo(np.float32).tiny
    return rows, cols, qA.ravel(), sA.ravel(), qx, sx


@pytest.mark.gpu
def test_gpu_mvm_numeric_edges(hip, m8, oracle):
    """bit for bit at the edges of the mvm epilogue and chains: 127 / m = inf for a nonzero m (all bytes 0, sr = m) and m just above
    it, subnormal block factors, a block with sx = 0, rows that cancel to exactly 0 next to nonzero rows; mvm_f32 with subnormal x and
    with x over 2^-120 .. 2^100.  Every input is finite: NaN and Inf are out of contract (the reference's _mm256_max_ps tree makes
    their result depend on operand order)."""
    rows, cols, qA, sA, qx, sx = _edge_operands()
    d = m8.rowdots(qA, sA, rows, cols, qx, sx)
    assert np.all(d[192:256:2] == 0) and np.all(d[193:256:2] != 0)
    st, o = hip.new_rng(3, 1), oracle.rng(3, 1)
    for g, og in ((None, None), (st, o)):
        r, sr = hip.m8_mvm(qA, sA, rows, cols, qx, sx, rng=g)
        ro, sro = m8.mvm(qA, sA, rows, cols, qx, sx, og)
        assert same(r, ro) and same(sr, sro), g is None
        with np.errstate(over="ignore"):
            assert not r[:64].any() and sr[0] == np.abs(d[:64]).max() and sr[0] > 0 and np.isinf(np.float32(127) / sr[0])
            assert r[64:128].any() and np.isfinite(np.float32(127) / sr[1])
        assert r[128:192].any() and sr[2] >= np.finfo(np.float32).tiny
        assert not r[320:].any() and sr[5] == 1.0
    assert same_keys(hip, st, oracle, o)
    rng = np.random.default_rng(7)
    for x in ((rng.standard_normal(cols) * 1e-40).astype(np.float32),
              (np.where(rng.random(cols) < 0.5, -1, 1) * np.exp2(rng.uniform(-120, 100, cols))).astype(np.float32)):
        assert np.all(np.isfinite(x))
        f = hip.m8_mvm_f32(qA, sA, rows, cols, x)
        assert same(f, m8.mvm_f32(qA, sA, rows, cols, x))
        assert np.all(np.isfinite(f)) and f[:256].any()


@pytest.mark.gpu
def test_gpu_two_streams_keep_their_own_generators(hip, m8p, oracle):
    """stochastic quantize and mvm interleaved on two streams, one generator state each, no host sync in between: each stream's
    results equal its own walk of the oracle"""
    import ctypes as C
    rt = C.CDLL("libamdhip64.so")
    L = hip.lib
    rows, cols = 2048, 2048
    A = make_matrix("normal", rows, cols, 2)
    qA, sA = m8p.quantize(A)
    x, qx, sx = v8_inputs(oracle, cols, 2)
    dAf, dqA, dsA, dqx, dsx = (hip.to_device(a) for a in (A, qA, sA, qx, sx))
    streams = [C.c_void_p(), C.c_void_p()]
    for s in streams:
        assert rt.hipStreamCreate(C.byref(s)) == 0
    keys = [(101, 202), (303, 404)]
    sts, ors = [hip.new_rng(*k) for k in keys], [oracle.rng(*k) for k in keys]
    steps = 3
    outs = [[(hip.alloc(rows * cols), hip.alloc(rows * cols // 1024), hip.alloc(rows), hip.alloc(rows // 16)) for _ in range(steps)]
            for _ in streams]
    for i in range(steps):
        for k, s in enumerate(streams):
            dq, ds, _, _ = outs[k][i]
            hip.check(L.clm8_quantize(dAf.ptr, rows, cols, dq.ptr, ds.ptr, sts[k].ptr, s))
        for k, s in enumerate(streams):
            _, _, dr, dsr = outs[k][i]
            hip.check(L.clm8_mvm(dqA.ptr, dsA.ptr, rows, cols, dqx.ptr, dsx.ptr, dr.ptr, dsr.ptr, sts[k].ptr, s))
    for s in streams:
        assert rt.hipStreamSynchronize(s) == 0
    for k in range(2):
        for i in range(steps):
            dq, ds, dr, dsr = outs[k][i]
            qo, so = m8p.quantize(A, ors[k])
            assert same(dq.download(np.int8), qo) and same(ds.download(np.float32), so), (k, i)
            ro, sro = m8p.mvm(qA, sA, rows, cols, qx, sx, ors[k])
            assert same(dr.download(np.int8), ro) and same(dsr.download(np.float32), sro), (k, i)
        assert same_keys(hip, sts[k], oracle, ors[k]), k
    for s in streams:
        assert rt.hipStreamDestroy(s) == 0


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


def _build_dropin(tmp_path):
    from clover_amd.build import build_hip_library
    lib = build_hip_library()
    exe = tmp_path / "matrix8_dropin"
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-DCLOVER_STOCHASTIC_ROUNDING_DISABLED=1", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "cpp" / "matrix8_dropin.cpp"), "-o", str(exe), f"-L{lib.parent}", "-lclover_hip",
                    f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["iht", "gd"])
def test_gpu_header_mvm_agree_and_q_iht_loop(tmp_path, m8, oracle, mode):
    """mvm == mvm_parallel == mvm_scalar through CloverMatrix8.h (rounding disabled), then Q_IHT<CloverMatrix8, CloverVector8> at N = 1024
    (m = N / 2, K = N / 4) or Q_GD on its 1.5 N x N shape, 10 iterations: x, t1, t2, t3 equal a host loop of the restatement's mvm and
    the oracle's CloverVector8 scaleAndAdd / threshold (the default build's threshold is the reference's heap walk, as the oracle's)"""
    N = 1024
    m, n = (N // 2, N) if mode == "iht" else (3 * N // 2, N)
    _header_loop(tmp_path, m8, oracle, mode, m, n, N // 4, 10)


@pytest.mark.gpu
def test_gpu_header_q_iht_at_the_readme_size(tmp_path, m8p, oracle):
    """the README's Q_IHT<CloverMatrix8, CloverVector8> configuration: N = 8192, m = 4096, K = 2048, 3 iterations, the default build"""
    _header_loop(tmp_path, m8p, oracle, "iht", 4096, 8192, 2048, 3)


@pytest.mark.gpu
def test_gpu_header_ragged_matrix(tmp_path, m8, oracle):
    """CloverMatrix8(300, 500) through the header: quantize, transpose, mvm and mvm_f32 equal the restatement on the zero-padded
    384 x 512 matrix"""
    m, n, rows, cols = 300, 500, 384, 512
    rng = np.random.default_rng(300)
    phi = (rng.normal(size=(m, n)) * np.exp2(rng.uniform(-8, 8, size=(m, 1)))).astype(np.float32)
    x = (rng.normal(size=n) * 3).astype(np.float32)
    phi.tofile(tmp_path / "phi.f32")
    x.tofile(tmp_path / "x.f32")
    out = subprocess.run([str(_build_dropin(tmp_path)), str(tmp_path), "ragged", str(m), str(n)], check=True, capture_output=True,
                         text=True, timeout=600).stdout
    assert f"rows={rows} cols={cols} done" in out, out
    P = np.zeros((rows, cols), np.float32)
    P[:m, :n] = phi
    xp = np.zeros(cols, np.float32)
    xp[:n] = x
    qPo, sPo = m8.quantize(P)
    qP, sP = _read8(tmp_path / "phi.bin", rows * cols, (rows // 64) * (cols // 64))
    assert same(qP, qPo) and same(sP, sPo)
    qT, sT = _read8(tmp_path / "phit.bin", rows * cols, (rows // 64) * (cols // 64))
    qTo, sTo = m8.transpose(qPo, sPo, rows, cols)
    assert same(qT, qTo) and same(sT, sTo)
    qx, sx = _read8(tmp_path / "xq.bin", cols, cols // 64)
    qxo, sxo = oracle.v8_quantize(xp)
    assert same(qx, qxo) and same(sx, sxo)
    r1 = _read8(tmp_path / "r1.bin", rows, rows // 64)
    ro = m8.mvm(qPo, sPo, rows, cols, qxo, sxo)
    assert same(r1[0], ro[0]) and same(r1[1], ro[1])
    f1 = np.fromfile(tmp_path / "f1.f32", dtype=np.float32)
    assert same(f1, m8.mvm_f32(qPo, sPo, rows, cols, xp))


def _header_loop(tmp_path, m8, oracle, mode, m, n, K, iters):
    exe = _build_dropin(tmp_path)
    mu = 0.5
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
