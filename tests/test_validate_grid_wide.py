"""CloverMatrix8, CloverVector16 and CloverMatrix16 through their C++ headers, the way a user of the reference would test them: three legs.

  device == `_scalar` twin   tests/cpp/validate_grid_wide.cpp: the reference's relations (test/validate/02_vector.cpp, 03_matrix.cpp at bit
                             counts 8 and 16) over its grid, both residency builds; tests/cpp/coherence_wide.cpp: kept pointers and views   (gpu)
  `_scalar` twin == restatement   tests/cpp/scalar_twins_wide.cpp against tests/matrix8_restate.c / tests/half16_restate.c, on the CPU
  device == restatement      the existing C ABI tests; here also through the headers with non-integer data at the grid's corner shapes     (gpu)
"""
import subprocess

import numpy as np
import pytest

from clover_amd.build import repo_root
from half16_helpers import F16_TINY, U16, U32, gamma, make_f32, pad128, rh, rhp  # noqa: F401
from matrix8_helpers import m8, m8p, make_matrix, same  # noqa: F401
from test_pointer_coherence import _link_flags

ROOT = repo_root()
CPP = ROOT / "tests" / "cpp"
BUILDS = {"tracked": (), "explicit": ("-DCLOVER_HIP_EXPLICIT_SYNC",)}
CXX = ["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-DCLOVER_STOCHASTIC_ROUNDING_DISABLED=1", f"-I{ROOT / 'include'}"]


def _build(tmp_path, name, build):
    exe = tmp_path / f"{name}_{build}"
    subprocess.run([*CXX, *BUILDS[build], str(CPP / f"{name}.cpp"), "-o", str(exe), *_link_flags()], check=True)
    return exe


def _build_with_fake_device(base, name, build):
    """host methods only: linked with the test double of the few calls clover_hip::Mirror makes, no HIP library and no device"""
    obj, exe = base / "fake_clv.o", base / f"{name}_{build}"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-c", f"-I{ROOT / 'include'}", str(CPP / "fake_clv.c"), "-o", str(obj)], check=True)
    subprocess.run([*CXX, *BUILDS[build], str(CPP / f"{name}.cpp"), str(obj), "-o", str(exe), "-lpthread"], check=True)
    return exe


# ================================================================ CPU
@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("name,ok", [("validate_grid_wide", "validate grid wide ok"), ("coherence_wide", "coherence wide ok")])
def test_wide_clients_build_in_both_residency_builds(tmp_path, name, ok, build):
    args = ["vector16"] if name == "validate_grid_wide" else []
    p = subprocess.run([str(_build(tmp_path, name, build)), *args], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and ("no_device" in p.stdout or ok in p.stdout), (p.returncode, p.stdout[-2000:], p.stderr[-1000:])


def test_size_mismatches_of_the_wide_classes_follow_the_reference_convention(tmp_path):
    """check_mvm / check_transpose / check_same_size of CloverMatrix8 and CloverMatrix16 and the length checks of CloverVector16: a message
    on stdout and exit(1) before any device work (tests/cpp/error_behaviour.cpp), as for the 4-bit classes"""
    exe = tmp_path / "errs"
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", f"-I{ROOT / 'include'}", str(CPP / "error_behaviour.cpp"), "-o", str(exe), *_link_flags()], check=True)
    mvm, tr, sz, vec = ("MVM can not be performed. Exiting ...", "Matrix can not be transposed. Exiting ...",
                        "Matrices do not have the same size. Exiting ...", "Vectors do not have the same size. Exiting ...")
    for case, msg in (("m8_mvm", mvm), ("m8_mvm32", mvm), ("m8_transpose", tr), ("m8_quantize", sz), ("m16_mvm", mvm), ("m16_mvm32", mvm),
                      ("m16_transpose", tr), ("m16_quantize", sz), ("v16_quantize", vec), ("v16_scaleAndAdd", vec)):
        p = subprocess.run([str(exe), case], capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and msg in p.stdout and "not reached" not in p.stdout, (case, p.returncode, p.stdout)


@pytest.fixture(scope="module", params=list(BUILDS))
def twins(request, tmp_path_factory):
    return _build_with_fake_device(tmp_path_factory.mktemp("twins"), "scalar_twins_wide", request.param)


def _run_twins(exe, *args):
    p = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "scalar twins wide done" in p.stdout, (p.returncode, p.stdout[-1000:], p.stderr[-1000:])
    return p.stdout


SHAPES = [(128, 128), (256, 1152), (1280, 384)]


@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("kind", ["normal", "zero_tiles", "extremes"])
def test_matrix8_scalar_twins_against_the_restatement(twins, m8, tmp_path, kind, rows, cols):
    """quantize_scalar, restore_scalar, transpose_scalar: the restatement's arithmetic, so bit for bit.  mvm_scalar with an fp32 vector is
    defined as a double accumulation of get(i, j) * x[j]; get(i, j) is restore_scalar's value R[i, j] (just compared), every product of
    two fp32 values is exact in double, the cols - 1 additions round to 2^-53 each and one rounding to fp32 follows.  The float64 value
    numpy computes from the same R and x carries the same summation error in its own order, hence twice cols 2^-53 sum |terms|.  Not
    for "extremes": its tile scales near 3e38 leave fp32 (tests/test_matrix8.py clamps them for the same reason)."""
    A = make_matrix(kind, rows, cols, rows + cols)
    x = (np.random.default_rng(cols).normal(size=cols) * 3).astype(np.float32)
    A.tofile(tmp_path / "A.f32")
    x.tofile(tmp_path / "x.f32")
    _run_twins(twins, "m8", tmp_path, rows, cols)
    tiles = (rows // 64) * (cols // 64)
    q, s = m8.quantize(A)
    got = np.fromfile(tmp_path / "q.bin", np.int8)
    assert got.size == rows * cols + 4 * tiles
    assert same(got[:rows * cols], q) and same(got[rows * cols:].view(np.float32), s), np.flatnonzero(got[:rows * cols] != q)[:8]
    R = m8.restore(q, s, rows, cols)
    assert same(np.fromfile(tmp_path / "r.f32", np.float32), R.ravel())
    qt, st = m8.transpose(q, s, rows, cols)
    got = np.fromfile(tmp_path / "t.bin", np.int8)
    assert same(got[:rows * cols], qt) and same(got[rows * cols:].view(np.float32), st)
    if kind != "extremes":
        f = np.fromfile(tmp_path / "f.f32", np.float32).astype(np.float64)
        R64, x64 = R.astype(np.float64), x.astype(np.float64)
        e, a = R64 @ x64, np.abs(R64) @ np.abs(x64)
        lim64 = 2 * cols * 2.0 ** -53 * a
        assert f.size == rows and np.all(np.abs(f - e) <= U32 * (np.abs(e) + lim64) + lim64)
        assert np.count_nonzero(f) > rows // 2


@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("kind", ["gaussian", "ties", "subnormal", "overflow"])
def test_matrix16_scalar_twins_against_the_restatement(twins, rh, tmp_path, kind, rows, cols):
    """quantize_scalar (matrix and vector) and transpose_scalar bit for bit, on the value kinds tests/test_half16.py quantizes.  The two
    mvm_scalar forms are defined in another order than the restatement's 32 chains -- one running fp32 sum of separately rounded products,
    and a double accumulation -- so they meet the float64 bounds tests/test_half16_dropin.py derives for them; on the finite kinds only
    ("ties" and "overflow" hold infinities, whose sums are NaN: the existing mvm tests use finite data too)."""
    A = make_f32(kind, rows * cols, rows).reshape(rows, cols)
    x = make_f32("gaussian" if kind == "subnormal" else kind, cols, cols + 1)      # subnormal entries times ordinary ones: sums that are not all 0
    A.tofile(tmp_path / "A.f32")
    x.tofile(tmp_path / "x.f32")
    _run_twins(twins, "m16", tmp_path, rows, cols)
    q, xq = rh.quantize(A).ravel(), rh.quantize(x)
    assert np.array_equal(np.fromfile(tmp_path / "q.bin", np.uint16), q)
    assert np.array_equal(np.fromfile(tmp_path / "t.bin", np.uint16), rh.transpose(q, rows, cols))
    assert np.array_equal(np.fromfile(tmp_path / "xq.bin", np.uint16), xq)
    if kind in ("gaussian", "subnormal"):
        n = cols
        e, a = rh.mvm64(q, rows, n, xq)
        r = np.fromfile(tmp_path / "r.bin", np.uint16).view(np.float16).astype(np.float64)
        lim = gamma(n + 1) * a                    # n roundings of the products and n - 1 of the sums, then the rounding to f16
        assert r.size == rows and np.all(np.abs(r - e) <= lim + U16 * (np.abs(e) + lim) + F16_TINY)
        e32, a32 = rh.mvm_f32_64(q, rows, n, x)
        f = np.fromfile(tmp_path / "f.f32", np.float32)
        assert f.size == rows and np.all(np.abs(f - e32) <= U32 * np.abs(e32) + n * 2.0 ** -53 * a32)     # double accumulation, one rounding
        assert np.count_nonzero(r) > rows // 2 and np.count_nonzero(f) > rows // 2            # subnormal: f16 results in the subnormal range


@pytest.mark.parametrize("n", [128, 1000, 2047])
@pytest.mark.parametrize("kind", ["gaussian", "ties", "subnormal", "overflow", "zeros"])
def test_vector16_scalar_twins_against_the_restatement(twins, rh, tmp_path, kind, n):
    """quantize_scalar, restore_scalar and both scaleAndAdd_scalar forms bit for bit (operands as in tests/test_half16.py: finite, and for
    "overflow" a = 1 so that sums pass 65520); dot_scalar, one running fp32 sum of separately rounded products, within gamma_(n + 1)
    sum |terms| of the float64 value"""
    n_pad = pad128(n)
    a = np.float32(1.0 if kind == "overflow" else -0.3721)
    x = make_f32(kind, n, n)
    u, v = np.zeros(n_pad, np.uint16), np.zeros(n_pad, np.uint16)
    u[:n], v[:n] = rh.quantize(make_f32(kind, n, n + 1)), rh.quantize(make_f32(kind, n, n + 2))
    if kind in ("overflow", "ties"):               # finite operands
        u, v = np.minimum(u & 0x7FFF, 0x7BFF).astype(np.uint16), np.minimum(v & 0x7FFF, 0x7BFF).astype(np.uint16)
    x.tofile(tmp_path / "x.f32")
    u.tofile(tmp_path / "u.bin")
    v.tofile(tmp_path / "v.bin")
    out = _run_twins(twins, "v16", tmp_path, n, repr(float(a)))
    xp = np.zeros(n_pad, np.float32)
    xp[:n] = x
    q = rh.quantize(xp)
    assert np.array_equal(np.fromfile(tmp_path / "q.bin", np.uint16), q)
    assert np.array_equal(np.fromfile(tmp_path / "r.f32", np.uint32), rh.restore(q).view(np.uint32))
    want = rh.scale_and_add(u, v, a)
    assert np.array_equal(np.fromfile(tmp_path / "s3.bin", np.uint16), want) and np.array_equal(np.fromfile(tmp_path / "s2.bin", np.uint16), want)
    if kind == "overflow":
        assert np.any(np.isinf(want.view(np.float16)))
    d = np.array([int(out.split("dot=")[1].split()[0], 16)], np.uint32).view(np.float32)[0]
    e, absum = rh.mvm64(u, 1, n_pad, v)
    assert abs(float(d) - e[0]) <= gamma(n_pad + 1) * absum[0], (d, e[0], absum[0])


# ================================================================ GPU
# seconds of one family in the page-tracked build on an MI355X host, as the client prints them, are noted at each entry; the time to beat is
# the existing validate_grid's matrices_s on the same machine.  A family above a third of it is split by grid row: same grid, more cases.
GRID_CASES = [("vector16",), ("matrix8", "1-5"), ("matrix8", "6-10"), ("matrix16",)]
GRID_TIMEOUT = 600


@pytest.mark.gpu
@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("case", GRID_CASES, ids="_".join)
def test_reference_relations_on_the_wide_classes(tmp_path, case, build):
    """every relation of the reference's harness for these classes, device method against `_scalar` twin, over its grid"""
    p = subprocess.run([str(_build(tmp_path, "validate_grid_wide", build)), *case], capture_output=True, text=True, timeout=GRID_TIMEOUT)
    print("\n".join(p.stdout.strip().splitlines()[-2:]))
    assert p.returncode == 0 and "validate grid wide ok" in p.stdout, (p.returncode, p.stdout[-3000:], p.stderr[-1000:])


CORNERS = [(128, 128), (128, 1280), (1280, 128), (1280, 1280)]


def _corner_run(tmp_path, family, build):
    p = subprocess.run([str(_build(tmp_path, "validate_grid_wide", build)), family, str(tmp_path), "corners"], capture_output=True, text=True, timeout=300)
    print("\n".join(p.stdout.strip().splitlines()[-2:]))
    assert p.returncode == 0 and "validate grid wide ok" in p.stdout, (p.returncode, p.stdout[-3000:], p.stderr[-1000:])


@pytest.mark.gpu
@pytest.mark.parametrize("build", list(BUILDS))
def test_matrix8_header_mvm_on_non_integer_data_equals_the_restatement(tmp_path, m8, oracle, build):
    """what the grid cannot see: with integer data every order of summation gives the same bits.  Uniform(-1, 1) data at the grid's four
    corner shapes: quantize, both mvm forms AND the 8-bit mvm_scalar (defined through the device's dot, so compared here and not on the
    CPU) equal tests/matrix8_restate.c byte for byte; the fp32-vector mvm_scalar meets its float64 bound"""
    _corner_run(tmp_path, "matrix8", build)
    for M, N in CORNERS:
        base, tiles = f"{M}x{N}_", (M // 64) * (N // 64)
        A, x = np.fromfile(tmp_path / (base + "A.f32"), np.float32).reshape(M, N), np.fromfile(tmp_path / (base + "x.f32"), np.float32)
        raw = np.fromfile(tmp_path / (base + "qA.bin"), np.int8)
        qA, sA = raw[:M * N].copy(), raw[M * N:].view(np.float32).copy()
        assert sA.size == tiles
        q, s = m8.quantize(A)
        assert same(qA, q) and same(sA, s), (M, N)
        raw = np.fromfile(tmp_path / (base + "qx.bin"), np.int8)
        qx, sx = raw[:N].copy(), raw[N:].view(np.float32).copy()
        oq, os_ = oracle.v8_quantize(x)
        assert same(qx, oq) and same(sx, os_[:N // 64]), (M, N)
        r, sr = m8.mvm(qA, sA, M, N, qx, sx)
        for name in ("r.bin", "rs.bin"):
            raw = np.fromfile(tmp_path / (base + name), np.int8)
            assert same(raw[:M], r) and same(raw[M:].view(np.float32), sr), (M, N, name, np.flatnonzero(raw[:M] != r)[:8])
        f = np.fromfile(tmp_path / (base + "f.f32"), np.float32)
        assert same(f, m8.mvm_f32(qA, sA, M, N, x)), (M, N)
        R64, x64 = m8.restore(qA, sA, M, N).astype(np.float64), x.astype(np.float64)
        e, a = R64 @ x64, np.abs(R64) @ np.abs(x64)
        lim64 = 2 * N * 2.0 ** -53 * a
        fs = np.fromfile(tmp_path / (base + "fs.f32"), np.float32).astype(np.float64)
        assert np.all(np.abs(fs - e) <= U32 * (np.abs(e) + lim64) + lim64), (M, N)


@pytest.mark.gpu
@pytest.mark.parametrize("build", list(BUILDS))
def test_matrix16_header_mvm_on_non_integer_data_equals_the_restatement(tmp_path, rh, build):
    """the same for CloverMatrix16: quantize and both mvm forms equal tests/half16_restate.c byte for byte; the two mvm_scalar forms, defined
    in other orders, meet their float64 bounds (an mvm_scalar that accumulated in double would pass here and in the grid: the byte
    comparison of mvm itself is what pins the kernel's order)"""
    _corner_run(tmp_path, "matrix16", build)
    for M, N in CORNERS:
        base = f"{M}x{N}_"
        A, x = np.fromfile(tmp_path / (base + "A.f32"), np.float32).reshape(M, N), np.fromfile(tmp_path / (base + "x.f32"), np.float32)
        qA, qx = np.fromfile(tmp_path / (base + "qA.bin"), np.uint16), np.fromfile(tmp_path / (base + "qx.bin"), np.uint16)
        assert np.array_equal(qA, rh.quantize(A).ravel()) and np.array_equal(qx, rh.quantize(x)), (M, N)
        r = np.fromfile(tmp_path / (base + "r.bin"), np.uint16)
        assert np.array_equal(r, rh.mvm(qA, M, N, qx)), (M, N, np.flatnonzero(r != rh.mvm(qA, M, N, qx))[:8])
        f = np.fromfile(tmp_path / (base + "f.f32"), np.float32)
        assert np.array_equal(f.view(np.uint32), rh.mvm_f32(qA, M, N, x).view(np.uint32)), (M, N)
        e, a = rh.mvm64(qA, M, N, qx)
        rs = np.fromfile(tmp_path / (base + "rs.bin"), np.uint16).view(np.float16).astype(np.float64)
        lim = gamma(N + 1) * a
        assert np.all(np.abs(rs - e) <= lim + U16 * (np.abs(e) + lim) + F16_TINY), (M, N)
        e32, a32 = rh.mvm_f32_64(qA, M, N, x)
        fs = np.fromfile(tmp_path / (base + "fs.f32"), np.float32)
        assert np.all(np.abs(fs - e32) <= U32 * np.abs(e32) + N * 2.0 ** -53 * a32), (M, N)


@pytest.mark.gpu
@pytest.mark.parametrize("build", list(BUILDS))
def test_kept_pointers_and_views_on_the_wide_classes(tmp_path, build):
    """tests/cpp/coherence_wide.cpp: pointers kept across quantize / scaleAndAdd / threshold / mvm / transpose, raw writes through them,
    copies, and CloverVector16(n, ptr) views; in the explicit-residency build with every pointer taken again after the device operation"""
    p = subprocess.run([str(_build(tmp_path, "coherence_wide", build)), ], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "coherence wide ok" in p.stdout and f"build={build}" in p.stdout, (p.returncode, p.stdout[-3000:], p.stderr[-1000:])
    assert build == "explicit" or "untracked_blocks=0" in p.stdout
