"""CPU-side checks of the fp32 device path: the library exports what include/clover_hip_fp32.h declares and the binding's second table
covers it, the header is C99, every argument check answers without a device, the -DCLOVER_FP32_ON_DEVICE switch is the only thing that makes
a header client reference the new symbols, and the CPU reference of the GPU tests (tests/fp32_restate.cpp) and their data are what those
tests assume: two builds that agree, inputs that tell summation orders apart, loop problems that keep the threshold busy."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

from clover_amd.build import build_hip_library, repo_root
from clover_amd.lib_binding import SIGNATURES, SIGNATURES_FP32, load_library
from fp32_helpers import KINDS, bits, iht_problem, make_axpy, make_ops, rf, rfp, threshold_data  # noqa: F401

ROOT = repo_root()
# the shapes of tests/test_fp32_device.py
DOT_SIZES = (128, 8192, 4096 + 128, 8192 + 128, 1 << 20)
MVM_SHAPES = ((128, 128), (384, 4096), (128, 4096 + 128), (640, 1152), (256, 8576))
IHT_SHAPES = ((128, 256), (256, 512), (384, 1024))


def declared_symbols():
    text = (ROOT / "include" / "clover_hip_fp32.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cl[vm]_f32_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_what_the_header_declares_and_the_table_covers_it():
    syms = declared_symbols()
    assert len(syms) == 9 and sorted(SIGNATURES_FP32) == syms
    lib = ctypes.CDLL(str(build_hip_library()))                   # loads on a machine without a GPU
    assert not [s for s in syms if not hasattr(lib, s)]
    assert not set(SIGNATURES) & set(SIGNATURES_FP32)             # clover_hip.h's surface is what it was
    assert "_f32_scale_and_add" not in (ROOT / "include" / "clover_hip.h").read_text()
    bound = load_library()
    assert all(getattr(bound, s).argtypes == SIGNATURES_FP32[s][1] for s in syms)


def test_c99_client_of_the_header_compiles_and_links(tmp_path):
    lib = build_hip_library()
    exe = tmp_path / "fp32_from_c"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "c" / "fp32_from_c.c"),
                    "-o", str(exe), f"-L{lib.parent}", "-lclover_hip", f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"],
                   check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and ("dot=128.0" in p.stdout or "no_device" in p.stdout), (p.returncode, p.stdout, p.stderr)


def test_argument_checks_answer_without_a_device():
    lib = load_library()
    err = lambda: lib.clv_last_error().decode()                                # noqa: E731
    # scale_and_add
    assert lib.clv_f32_scale_and_add(16, None, 1.0, 128, 16, None) == -1 and "null" in err()
    assert lib.clv_f32_scale_and_add(16, 32, 1.0, 130, 16, None) == -1 and "multiple of 128" in err()
    assert lib.clv_f32_scale_and_add(16, 36, 1.0, 128, 16, None) == -1 and "aligned" in err()
    assert lib.clv_f32_scale_and_add(16, 32, 1.0, 128, 32, None) == -1 and "alias" in err()
    # dot
    assert lib.clv_f32_dot(None, 16, 128, 0, 16, None, None) == -1 and "null" in err()
    assert lib.clv_f32_dot(16, 16, 128, 0, None, None, None) == -1 and "null" in err()
    assert lib.clv_f32_dot(16, 16, 100, 0, 16, None, None) == -1 and "multiple of 128" in err()
    assert lib.clv_f32_dot(16, 16, 128, 7, 16, None, None) == -1 and "unknown mode" in err()
    assert lib.clv_f32_dot(16, 24, 128, 0, 16, None, None) == -1 and "aligned" in err()
    assert lib.clv_f32_dot(16, 16, 128, 1, 16, 8, None) == -1 and "workspace must be 16-byte aligned" in err()
    # threshold
    assert lib.clv_f32_threshold_mode(None, 100, 128, 10, 0, None, None) == -1 and "null" in err()
    assert lib.clv_f32_threshold_mode(16, 200, 128, 10, 0, None, None) == -1 and "n=200" in err()
    assert lib.clv_f32_threshold_mode(16, 100, 100, 10, 0, None, None) == -1 and "n_pad=100" in err()
    assert lib.clv_f32_threshold_mode(16, 100, 128, 10, 5, None, None) == -1 and "unknown mode" in err()
    assert lib.clv_f32_threshold_mode(20, 100, 128, 10, 0, None, None) == -1 and "aligned" in err()
    assert lib.clv_f32_threshold_mode(16, 100, 128, 10, 1, 24, None) == -1 and "workspace must be 16-byte aligned" in err()
    assert lib.clv_f32_threshold_mode(16, 1 << 32, 1 << 33, 10, 0, None, None) == -1 and "2^32" in err()
    # mvm and the fused form
    assert lib.clm_f32_mvm(None, 128, 128, 16, 32, None) == -1 and "null" in err()
    assert lib.clm_f32_mvm(16, 128, 128, 16, None, None) == -1 and "null" in err()
    assert lib.clm_f32_mvm(16, 128, 100, 16, 32, None) == -1 and "multiples of 128" in err()
    assert lib.clm_f32_mvm(16, 64, 128, 16, 32, None) == -1 and "multiples of 128" in err()
    assert lib.clm_f32_mvm(16, 128, 128, 24, 32, None) == -1 and "aligned" in err()
    assert lib.clm_f32_mvm(16, 128, 128, 32, 32, None) == -1 and "alias" in err()
    assert lib.clm_f32_mvm_scale_and_add(16, 128, 128, 32, None, 1.0, None, 48, None) == -1 and "null" in err()
    assert lib.clm_f32_mvm_scale_and_add(16, 128, 128, 32, 48, 1.0, None, None, None) == -1 and "null" in err()
    assert lib.clm_f32_mvm_scale_and_add(16, 128, 130, 32, 48, 1.0, None, 64, None) == -1 and "multiples of 128" in err()
    assert lib.clm_f32_mvm_scale_and_add(16, 100, 128, 32, 48, 1.0, None, 64, None) == -1 and "multiples of 128" in err()
    assert lib.clm_f32_mvm_scale_and_add(24, 128, 128, 32, 48, 1.0, None, 64, None) == -1 and "aligned" in err()
    assert lib.clm_f32_mvm_scale_and_add(16, 128, 128, 32, 50, 1.0, None, 64, None) == -1 and "aligned" in err()
    assert lib.clm_f32_mvm_scale_and_add(16, 128, 128, 32, 48, 1.0, None, 32, None) == -1 and "alias" in err()          # r2 == x
    assert lib.clm_f32_mvm_scale_and_add(16, 128, 128, 32, 48, 1.0, 32, 64, None) == -1 and "alias" in err()            # t == x
    assert lib.clm_f32_mvm_scale_and_add(16, 128, 128, 32, 48, 1.0, 48, 64, None) == -1 and "alias" in err()            # t == u
    assert lib.clm_f32_mvm_scale_and_add(16, 128, 128, 32, 48, 1.0, 64, 64, None) == -1 and "alias" in err()            # t == r2
    # transpose
    assert lib.clm_f32_transpose(None, 128, 128, 16, None) == -1 and "null" in err()
    assert lib.clm_f32_transpose(16, 128, 130, 32, None) == -1 and "multiples of 4" in err()
    assert lib.clm_f32_transpose(16, 128, 128, 16, None) == -1 and "in-place" in err()
    assert lib.clm_f32_transpose(16, 128, 128, 40, None) == -1 and "aligned" in err()
    # the loop
    ok = [16, 32, 128, 256, 48, 256, 64, 80, 96, 112, 1, 8, 0.5, 1, None]
    def iht(**kw):                                                             # noqa: E306
        names = ["Phi", "PhiT", "m", "n", "x", "x_len", "y", "t1", "t2", "t3", "iterations", "K", "mu", "threshold", "stream"]
        return lib.clm_f32_iht(*[kw.get(k, v) for k, v in zip(names, ok)])
    for p in ("Phi", "PhiT", "x", "y", "t1", "t2", "t3"):
        assert iht(**{p: None}) == -1 and "null" in err(), p
    assert iht(m=100) == -1 and "m=100" in err()
    assert iht(n=200, x_len=100) == -1 and "n=200" in err()
    assert iht(x_len=257) == -1 and "x_len=257" in err()
    assert iht(threshold=3) == -1 and "unknown threshold" in err()
    assert iht(Phi=24) == -1 and "aligned" in err()
    assert iht(x=52) == -1 and "aligned" in err()
    # nothing to do: no device work either
    assert lib.clv_f32_scale_and_add(16, 32, 1.0, 0, 16, None) == 0 and lib.clm_f32_mvm(16, 0, 128, 16, 32, None) == 0
    assert lib.clv_f32_threshold_mode(16, 100, 128, 100, 0, None, None) == 0             # k >= n: everything survives
    assert lib.clm_f32_transpose(16, 0, 128, 32, None) == 0
    assert lib.clv_f32_dot_workspace_bytes(1 << 20) == 0 and lib.clv_f32_threshold_workspace_bytes(1 << 20) > 4096 * 4


@pytest.mark.parametrize("explicit", [False, True])
def test_only_the_switch_makes_a_header_client_reference_the_fp32_symbols(tmp_path, explicit):
    """tests/cpp/fp32_device.cpp compiled to an object with and without -DCLOVER_FP32_ON_DEVICE, page-tracked and explicit-sync: nm -u"""
    def undefined(*flags):
        obj = tmp_path / ("with.o" if flags else "without.o")
        subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", *flags, *(["-DCLOVER_HIP_EXPLICIT_SYNC"] if explicit else []),
                        f"-I{ROOT / 'include'}", "-c", str(ROOT / "tests" / "cpp" / "fp32_device.cpp"), "-o", str(obj)], check=True)
        out = subprocess.run(["nm", "-u", str(obj)], check=True, capture_output=True, text=True).stdout
        return {line.split()[-1] for line in out.splitlines() if line.strip()}
    on, off = undefined("-DCLOVER_FP32_ON_DEVICE"), undefined()
    want = {"clv_f32_scale_and_add", "clv_f32_dot", "clv_f32_threshold_mode", "clm_f32_mvm", "clm_f32_mvm_scale_and_add", "clm_f32_transpose",
            "clm_f32_iht"}
    assert {s for s in on if "_f32_" in s} == want
    assert not {s for s in off if "_f32_" in s}


def test_the_two_restate_builds_agree(rf, rfp):
    for kind in KINDS:
        rows, cols = 200, 1152
        A, x, a = make_ops(kind, rows, cols, 3)
        assert np.array_equal(bits(rf.mvm(A, rows, cols, x)), bits(rfp.mvm(A, rows, cols, x))), kind
        assert bits(rf.dot(A[:cols], x))[0] == bits(rfp.dot(A[:cols], x))[0], kind
        u, v, a = make_axpy(kind, 4096, 4)
        assert np.array_equal(bits(rf.scale_and_add(u, v, a)), bits(rfp.scale_and_add(u, v, a))), kind
    A = make_ops("magnitudes", 136, 200, 5)[0]
    assert np.array_equal(bits(rf.transpose(A, 136, 200)), bits(rfp.transpose(A, 136, 200)))
    assert np.array_equal(rf.transpose(A, 136, 200).reshape(200, 136), A.reshape(136, 200).T)
    for kind in ("distinct", "ties"):
        x = threshold_data(kind, 1024, 6)
        assert np.array_equal(bits(rf.threshold(x, 1000, 250)), bits(rfp.threshold(x, 1000, 250))), kind
    Phi, PhiT, y, mu = iht_problem(128, 256, 7)
    a, za = rf.iht(Phi, PhiT, 128, 256, y, 4, 32, mu, 1)
    b, zb = rfp.iht(Phi, PhiT, 128, 256, y, 4, 32, mu, 1)
    assert all(np.array_equal(bits(a[k]), bits(b[k])) for k in a) and np.array_equal(za, zb)


def test_scale_and_add_data_tells_a_fused_fma_and_kept_subnormals(rf):
    """cancel: the fused result is the product's rounding error, which a rounded product turns into 0; subnormal: every result is a
    non-zero subnormal, which a flushing instruction would turn into 0"""
    u, v, a = make_axpy("cancel", 8192, 1)
    r = rf.scale_and_add(u, v, a)
    assert np.count_nonzero(r) > r.size // 2 and np.all((v * a + u).astype(np.float32) == 0)
    u, v, a = make_axpy("subnormal", 8192, 1)
    r = rf.scale_and_add(u, v, a)
    sub = (np.abs(r) < 2.0 ** -126) & (r != 0)
    assert sub.sum() > 0.9 * r.size


def test_dot_and_mvm_data_tell_summation_orders_apart(rfp):
    """the 32-chain value differs in its bits from the one-chain value (dot_sequential) in at least half of the dot cases (value kinds x
    sizes), and in at least half of the rows of every mvm shape for the magnitudes and for the cancelling data.  The other two kinds
    cannot tell orders apart by construction -- the sums of the zeros kind are small integers and sums of subnormals are fixed-point
    additions, both exact in any order: they are there for the signs of zero and for flushing, so the subnormal data must hold
    subnormal row values"""
    differ, cases = 0, 0
    for kind in KINDS:
        for n in DOT_SIZES:
            u, v, _ = make_ops(kind, 1, n, n)
            differ, cases = differ + int(bits(rfp.dot(u, v))[0] != bits(rfp.dot_sequential(u, v))[0]), cases + 1
    assert 2 * differ >= cases, (differ, cases)
    for rows, cols in MVM_SHAPES:
        for kind in KINDS:
            A, x, _ = make_ops(kind, rows, cols, rows + cols)
            chains, one = rfp.mvm(A, rows, cols, x), rfp.mvm_sequential(A, rows, cols, x)
            if kind in ("magnitudes", "cancel"):
                assert 2 * int((bits(chains) != bits(one)).sum()) >= rows, (kind, rows, cols)
            if kind == "subnormal":
                assert np.any((np.abs(chains) < 2.0 ** -126) & (chains != 0)), (rows, cols)


@pytest.mark.parametrize("m,n", IHT_SHAPES)
@pytest.mark.parametrize("ties", [False, True])
def test_loop_problems_keep_the_threshold_busy(rfp, m, n, ties):
    """every iteration's threshold zeroes at least one non-zero element; the tie-heavy problems have equal magnitudes on both sides of the
    cut (some kept, some cleared) in at least one iteration"""
    Phi, PhiT, y, mu = iht_problem(m, n, m + n, ties)
    K, iters = n // 8, 4
    v, zeroed = rfp.iht(Phi, PhiT, m, n, y, iters, K, mu, 1)
    assert np.all(zeroed >= 1), zeroed
    assert np.count_nonzero(v["x"]) == K
    if ties:
        cut, x = 0, np.zeros(n, np.float32)
        for _ in range(iters):
            t2 = rfp.scale_and_add(y, rfp.mvm(Phi, m, n, x), -1.0)
            x = rfp.scale_and_add(x, rfp.mvm(PhiT, n, m, t2), mu)
            after = rfp.threshold(x, n, K)
            tau = np.abs(after[after != 0]).min()
            cut += int(((np.abs(x) == tau) & (after == 0)).sum())
            x = after
        assert cut >= 1 and np.array_equal(bits(x), bits(v["x"]))
