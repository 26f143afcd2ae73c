"""clm8_gemm, clm8_gemm_i32 and clm4_gemm_m8 on the device: every result equals the plain-C restatement (tests/gemm8_restate.c) bit for bit.

Inputs (gemm8_helpers.operands): bytes over the whole range, -128 and the nibble -8 included; scales over the binades 2^-40 .. 2^40,
different in every tile and every K-block, so that a wrong scale index cannot hide; all finite, no NaN can arise.  The `tiny` kind puts the
4-bit operand's scales near 2^-120: every c_b of the mixed form is then too small for its sixteenth to be exact and the kernel folds the
2^-4 of its nibble image into the integer instead (test_gemm8_cpu.py checks on the CPU that the case really lies there).

Shapes (M, N, K), the smallest at which each thing the kernel does can go wrong:
    (128, 128, 128)    one tile, one stage
    (128, 128, 384)    three stages: an odd stage count
    (256, 384, 256)    more tiles in N than in M
    (1280, 896, 256)   70 tiles (no multiple of 8), a last row group of 2 of the 8-wide grouping
    (384, 640, 128)    non-square tile counts
The references are computed once per process (gemm8_helpers.reference) and shared.

The guard-band cases of the three calls are registered with tests/test_guard_bands.py's table when this module is imported (its coverage
test counts every prototype of clover_amd.lib_binding.SIGNATURES) and run here."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import test_guard_bands as gb
from clover_amd.build import repo_root
from gemm8_helpers import bound, bytes8, nibbles4, operands, reference, rg, rgp, same_bits, scales  # noqa: F401

ROOT = repo_root()
SHAPES = [(128, 128, 128), (128, 128, 384), (256, 384, 256), (1280, 896, 256), (384, 640, 128)]
RANGES = [(0, 6), (1, 1), (5, 1), (1, 4), (2, 3)]          # K-block ranges on K = 384: odd and even begins, odd and even counts
CALLS = ["gemm", "gemm_m8", "i32"]


def _device(hip, call, M, N, K, kind="wide", kb=None):
    qA8, sA, qA4, sA4, qB8, sB = operands(M, N, K, kind)
    if call == "gemm":
        return hip.m8_gemm(qA8, sA, M, K, qB8, sB, N)
    if call == "gemm_m8":
        return hip.m4_gemm_m8(qA4, sA4, M, K, qB8, sB, N)
    return hip.m8_gemm_i32(qA8, M, K, qB8, N, *kb)


def _first_diff(got, want):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    return bad[:4].tolist(), [(got[tuple(i)], want[tuple(i)]) for i in bad[:4]]


@pytest.mark.gpu
@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("shape", SHAPES)
def test_gpu_result_equals_the_restatement(hip, rgp, shape, call):  # noqa: F811
    M, N, K = shape
    kb = (0, K // 64) if call == "i32" else None
    want = reference(rgp, call, M, N, K, kb=kb)
    got = _device(hip, call, M, N, K, kb=kb)
    assert got.dtype == want.dtype and same_bits(got, want), (call, shape, *_first_diff(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("call", ["gemm", "gemm_m8"])
@pytest.mark.parametrize("shape", [(128, 128, 384), (256, 384, 256)])
def test_gpu_scales_near_2_to_the_minus_120(hip, rgp, shape, call):  # noqa: F811
    """the mixed form's small-factor path (and, for the 8 x 8 form, factors and products in the denormals)"""
    M, N, K = shape
    want = reference(rgp, call, M, N, K, "tiny")
    assert np.count_nonzero(want) > want.size // 2
    got = _device(hip, call, M, N, K, "tiny")
    assert same_bits(got, want), (call, shape, *_first_diff(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("kb", RANGES)
def test_gpu_integer_sums_of_a_k_block_range(hip, rgp, kb):  # noqa: F811
    """any begin, any count: a range of odd length ends with a stage whose second K-block is staged as zeros, and a begin that is odd
    starts in the middle of what the fp32 forms stage together"""
    M, N, K = 128, 128, 384
    want = reference(rgp, "i32", M, N, K, kb=kb)
    got = _device(hip, "i32", M, N, K, kb=kb)
    assert np.array_equal(got, want), (kb, np.argwhere(got != want)[:4].tolist())


@pytest.mark.gpu
def test_gpu_integer_ranges_on_more_than_one_tile(hip, rgp):  # noqa: F811
    M, N, K = 256, 384, 256
    for kb in [(1, 3), (3, 1), (0, 3)]:
        assert np.array_equal(_device(hip, "i32", M, N, K, kb=kb), reference(rgp, "i32", M, N, K, kb=kb)), kb


@pytest.mark.gpu
def test_gpu_block_sums_folded_on_the_host_reproduce_the_fp32_call(hip, rg):  # noqa: F811
    """clm8_gemm_i32(kb, 1) for every K-block, folded with the restatement's chain step: the bits of clm8_gemm"""
    M, N, K = 256, 384, 256
    _, sA, _, _, _, sB = operands(M, N, K)
    c = np.zeros((M, N), np.float32)
    for b in range(K // 64):
        rg.fold_step(np.ascontiguousarray(_device(hip, "i32", M, N, K, kb=(b, 1))), sA, sB, M, N, K, b, c)
    got = _device(hip, "gemm", M, N, K)
    assert same_bits(c, got), _first_diff(c, got)


# ---------------------------------------------------------------- capture
@pytest.mark.gpu
@pytest.mark.parametrize("call", ["gemm", "gemm_m8"])
def test_gpu_captured_call_replays(hip, rgp, call):  # noqa: F811
    """no scratch, no workspace, no rng: the call is captured on a stream as it is (one kernel node, a linear graph), replayed twice into
    output buffers prefilled with 0xFF, and gives the bits of the direct call"""
    M, N, K = 256, 384, 256
    qA8, sA, qA4, sA4, qB8, sB = operands(M, N, K)
    fn = hip.lib.clm8_gemm if call == "gemm" else hip.lib.clm4_gemm_m8
    b = [hip.to_device(a) for a in ((qA8, sA, qB8, sB) if call == "gemm" else (qA4, sA4, qB8, sB))]
    direct = _device(hip, call, M, N, K)
    assert same_bits(direct, reference(rgp, call, M, N, K))
    out = hip.alloc(4 * M * N)
    rt = C.CDLL("libamdhip64.so")
    stream, graph, gexec = C.c_void_p(), C.c_void_p(), C.c_void_p()

    def ok(rc):
        assert rc == 0, f"HIP runtime call failed: {rc}"
    ok(rt.hipStreamCreate(C.byref(stream)))
    ok(rt.hipStreamBeginCapture(stream, 0))                                       # hipStreamCaptureModeGlobal
    rc = fn(b[0].ptr, b[1].ptr, M, K, b[2].ptr, b[3].ptr, N, out.ptr, stream)
    ok(rt.hipStreamEndCapture(stream, C.byref(graph)))
    hip.check(rc)
    n_nodes = C.c_size_t(0)
    ok(rt.hipGraphGetNodes(graph, None, C.byref(n_nodes)))
    assert n_nodes.value == 1
    ok(rt.hipGraphInstantiate(C.byref(gexec), graph, None, None, 0))
    for _ in range(2):
        hip.check(hip.lib.clv_memset(out.ptr, 0xFF, out.nbytes, None))
        hip.sync()
        ok(rt.hipGraphLaunch(gexec, stream))
        ok(rt.hipStreamSynchronize(stream))
        assert same_bits(out.download(np.float32, M * N).reshape(M, N), direct)
    ok(rt.hipGraphExecDestroy(gexec))
    ok(rt.hipGraphDestroy(graph))
    ok(rt.hipStreamDestroy(stream))


# ---------------------------------------------------------------- guard bands
def _guard_case(fn, M, N, K, kb=None):
    def build(R):
        rng = np.random.default_rng(M * 7 + N * 3 + K + len(fn))
        qB, sB = bytes8(rng, N, K), scales(rng, N, K, -6, 6)
        qA = nibbles4(rng, M, K) if fn == "clm4_gemm_m8" else bytes8(rng, M, K)
        sA = scales(rng, M, K, -6, 6)
        Rg = _RESTATE[0]
        if fn == "clm8_gemm_i32":
            return gb.Case([("A", "input", qA), ("B", "input", qB), ("S", "output", 4 * M * N)],
                           lambda L, p: L.clm8_gemm_i32(p["A"], M, K, p["B"], N, kb[0], kb[1], p["S"], None), {"S": Rg.gemm_i32(qA, M, K, qB, N, *kb)})
        want = Rg.gemm_m8(qA, sA, M, K, qB, sB, N) if fn == "clm4_gemm_m8" else Rg.gemm(qA, sA, M, K, qB, sB, N)
        return gb.Case([("A", "input", qA), ("sA", "input", sA), ("B", "input", qB), ("sB", "input", sB), ("C", "output", 4 * M * N)],
                       lambda L, p: getattr(L, fn)(p["A"], p["sA"], M, K, p["B"], p["sB"], N, p["C"], None), {"C": want})
    return build


_RESTATE = []                 # the restatement the builders use: the rgp fixture of the test that runs them
GUARD_CASES = []
for _M, _N, _K in [(128, 256, 128), (256, 128, 384)]:
    for _fn in ("clm8_gemm", "clm4_gemm_m8"):
        GUARD_CASES.append((f"{_fn} {_M}x{_N}x{_K}", _guard_case(_fn, _M, _N, _K)))
    GUARD_CASES.append((f"clm8_gemm_i32 {_M}x{_N}x{_K} all K-blocks", _guard_case("clm8_gemm_i32", _M, _N, _K, kb=(0, _K // 64))))
    GUARD_CASES.append((f"clm8_gemm_i32 {_M}x{_N}x{_K} K-block 1 alone (an odd range)", _guard_case("clm8_gemm_i32", _M, _N, _K, kb=(1, 1))))
for _name, _build in GUARD_CASES:
    if _name not in gb.CASES:                 # the coverage test of test_guard_bands.py reads its table when it runs, after every module is imported
        gb.case(_name)(_build)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, _ in GUARD_CASES])
def test_gpu_calls_write_their_outputs_and_nothing_else(hip, rgp, name):  # noqa: F811
    _RESTATE[:] = [rgp]
    gb.run_case(hip, dict(GUARD_CASES)[name](None))         # the builders take their references from the restatement above, not from gb.Refs


# ---------------------------------------------------------------- through the headers
@pytest.mark.gpu
def test_gpu_container_methods(hip, tmp_path):
    """CloverMatrix8::gemm and CloverMatrix4::gemm(const CloverMatrix8 &, ...) on matrices quantized through the headers (256 x 384 and
    128 x 384): C lies within (nb + 4) 2^-24 sum|terms| of the float64 product of the RESTORED matrices, and equals the ABI call on the
    images the client wrote, bit for bit"""
    from clover_amd.build import build_hip_library
    lib = build_hip_library()
    exe = tmp_path / "gemm8_dropin"
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "cpp" / "gemm8_dropin.cpp"), "-o", str(exe),
                    f"-L{lib.parent}", "-lclover_hip", f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    M, N, K = 256, 128, 384
    rng = np.random.default_rng(8)
    # tiles of different magnitude, so that the tile scales matter
    a = (rng.normal(size=(M, K)) * np.repeat(np.repeat(np.exp2(rng.uniform(-3, 3, size=(M // 64, K // 64))), 64, 0), 64, 1)).astype(np.float32)
    b = (rng.normal(size=(N, K)) * np.repeat(np.repeat(np.exp2(rng.uniform(-3, 3, size=(N // 64, K // 64))), 64, 0), 64, 1)).astype(np.float32)
    a.tofile(tmp_path / "a.f32")
    b.tofile(tmp_path / "b.f32")
    p = subprocess.run([str(exe), str(tmp_path), str(M), str(N), str(K)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "done" in p.stdout, (p.returncode, p.stdout, p.stderr)

    def image(name, rows, value_bytes, dtype):
        raw = np.fromfile(tmp_path / name, np.uint8)
        assert raw.size == value_bytes + (rows // 64) * (K // 64) * 4
        return np.ascontiguousarray(raw[:value_bytes].view(dtype)), np.ascontiguousarray(raw[value_bytes:].view(np.float32))
    qA8, sA8 = image("a8.bin", M, M * K, np.int8)
    qA4, sA4 = image("a4.bin", M, M * K // 2, np.uint8)
    qB8, sB8 = image("b8.bin", N, N * K, np.int8)
    assert sA8.size == (M // 64) * (K // 64) and len(set(sA8.tolist())) == sA8.size
    rb = np.fromfile(tmp_path / "rb8.f32", np.float32).reshape(N, K).astype(np.float64)
    for cname, rname, abi in (("c88.f32", "ra8.f32", lambda: hip.m8_gemm(qA8, sA8, M, K, qB8, sB8, N)),
                              ("c48.f32", "ra4.f32", lambda: hip.m4_gemm_m8(qA4, sA4, M, K, qB8, sB8, N))):
        c = np.fromfile(tmp_path / cname, np.float32).reshape(M, N)
        ra = np.fromfile(tmp_path / rname, np.float32).reshape(M, K).astype(np.float64)
        err, lim = np.abs(c.astype(np.float64) - ra @ rb.T), bound(np.abs(ra) @ np.abs(rb).T, K)
        print(f"{cname}: max err / bound = {float((err / lim).max()):.3f}")
        assert np.all(err <= lim), (cname, float((err / lim).max()))
        assert same_bits(c, abi()), cname
