"""The GEMM with 8-bit operands without a GPU: the restatement (tests/gemm8_restate.c) against numpy, the argument checks of the three
entry points, and the two container methods from C++.

- integer sums: the restatement's int32 sums (both forms) equal a numpy int64 matmul on the same bytes, for whole ranges and sub-ranges;
- fp32 results: within (nb + 4) 2^-24 sum_b |c_b S_b| of a float64 evaluation that uses the same fp32-rounded c_b (gemm8_helpers.bound:
  derived from one rounding per fma, not measured);
- the plain and the OpenMP build of the restatement agree bit for bit;
- every argument check answers CLV_ERR_INVALID with a message before a pointer is used (integer pointers, no device);
- a C++ client of CloverMatrix8::gemm and CloverMatrix4::gemm(const CloverMatrix8 &, ...) compiles and links, tracked and explicit-sync."""
import subprocess

import numpy as np
import pytest

from clover_amd.build import build_hip_library, repo_root
from clover_amd.lib_binding import load_library
from gemm8_helpers import (bound, block_sums, exact64, factors, operands, reference, rg, rgp, same_bits, sixteenth_is_exact,  # noqa: F401
                           unpack_nibbles)

ROOT = repo_root()
INC = ROOT / "include"
SHAPES = [(128, 128, 128), (128, 256, 384), (256, 384, 256)]          # (M, N, K)


@pytest.mark.parametrize("shape", SHAPES)
def test_integer_sums_equal_a_numpy_int64_matmul(rg, shape):  # noqa: F811
    M, N, K = shape
    qA8, _, qA4, _, qB8, _ = operands(M, N, K)
    a8, a4, b8 = qA8.reshape(M, K).astype(np.int64), unpack_nibbles(qA4, M, K).astype(np.int64), qB8.reshape(N, K).astype(np.int64)
    assert a8.min() == -128 and b8.min() == -128 and a4.min() == -8 and a4.max() == 7
    nb = K // 64
    for b, c in {(0, nb), (1, 1), (nb - 1, 1), (1, nb - 1)}:
        cols = slice(64 * b, 64 * (b + c))
        for what, got, a in (("8 x 8", rg.gemm_i32(qA8, M, K, qB8, N, b, c), a8), ("4 x 8", rg.gemm_m8_i32(qA4, M, K, qB8, N, b, c), a4)):
            want = a[:, cols] @ b8[:, cols].T
            assert np.abs(want).max() < 2 ** 31 and np.array_equal(got.astype(np.int64), want), (what, b, c)


@pytest.mark.parametrize("kind", ["wide", "tiny"])
@pytest.mark.parametrize("shape", SHAPES)
def test_fp32_results_lie_within_the_chain_bound_of_a_float64_evaluation(rg, shape, kind):  # noqa: F811
    M, N, K = shape
    qA8, sA, qA4, sA4, qB8, sB = operands(M, N, K, kind)
    b8 = qB8.reshape(N, K)
    for call, a, s, mixed in (("gemm", qA8.reshape(M, K), sA, False), ("gemm_m8", unpack_nibbles(qA4, M, K), sA4, True)):
        got = reference(rg, call, M, N, K, kind)
        assert np.all(np.isfinite(got))
        exact, absum = exact64(block_sums(a, b8, M, N, K), factors(s, sB, M, N, K, mixed), M, N, K)
        err, lim = np.abs(got.astype(np.float64) - exact), bound(absum, K)
        print(f"{call} {shape} {kind}: max err / bound = {float((err / np.maximum(lim, 1e-300)).max()):.3f}")
        bad = np.flatnonzero(~(err <= lim))
        assert bad.size == 0, (call, bad[:8], err.ravel()[bad[:8]], lim.ravel()[bad[:8]])
        assert np.count_nonzero(got) > got.size // 2, "the case must not degenerate to zeros"


def test_the_tiny_case_takes_the_small_factor_path_of_the_mixed_form():
    """at least one c_b of the mixed form fails the kernel's test (here: all of them), none is zero; the wide case passes it everywhere"""
    for M, N, K in SHAPES:
        _, _, _, sA4, _, sB = operands(M, N, K, "tiny")
        c = factors(sA4, sB, M, N, K, mixed=True)
        assert np.all(c > 0) and not np.any(sixteenth_is_exact(c))
        _, _, _, sA4, _, sB = operands(M, N, K, "wide")
        assert np.all(sixteenth_is_exact(factors(sA4, sB, M, N, K, mixed=True)))


def test_the_two_builds_of_the_restatement_agree(rg, rgp):  # noqa: F811
    M, N, K = 256, 384, 256
    for kind in ("wide", "tiny"):
        qA8, sA, qA4, sA4, qB8, sB = operands(M, N, K, kind)
        assert same_bits(rgp.gemm(qA8, sA, M, K, qB8, sB, N), reference(rg, "gemm", M, N, K, kind))
        assert same_bits(rgp.gemm_m8(qA4, sA4, M, K, qB8, sB, N), reference(rg, "gemm_m8", M, N, K, kind))
    assert np.array_equal(rgp.gemm_i32(qA8, M, K, qB8, N, 1, 2), rg.gemm_i32(qA8, M, K, qB8, N, 1, 2))


def test_the_chain_step_by_step_is_the_chain(rg):  # noqa: F811
    """folding per-block integer sums with rg8_fold_step reproduces rg8_gemm: what test_gemm8.py does with the device's sums"""
    M, N, K = 128, 256, 384
    qA8, sA, _, _, qB8, sB = operands(M, N, K)
    c = np.zeros((M, N), np.float32)
    for b in range(K // 64):
        rg.fold_step(rg.gemm_i32(qA8, M, K, qB8, N, b, 1), sA, sB, M, N, K, b, c)
    assert same_bits(c, reference(rg, "gemm", M, N, K))


# ---------------------------------------------------------------- argument checks
def test_argument_checks_answer_without_a_device():
    """integer pointers: every violation is CLV_ERR_INVALID with a message before any pointer is used or any device work is done"""
    lib = load_library()
    err = lambda: lib.clv_last_error().decode()                                # noqa: E731
    A, sA, B, sB, C_ = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000

    def fp32_form(fn):
        def call(A=A, sA=sA, M=128, K=256, B=B, sB=sB, N=128, C=C_):
            return getattr(lib, fn)(A, sA, M, K, B, sB, N, C, None)
        return call

    def i32_form(A=A, M=128, K=256, B=B, N=128, b=0, c=4, S=C_):
        return lib.clm8_gemm_i32(A, M, K, B, N, b, c, S, None)

    shape_cases = [("M = 64", dict(M=64), "M=64"), ("M = 0", dict(M=0), "M=0"), ("N = 192", dict(N=192), "N=192"), ("N = 0", dict(N=0), "N=0"),
                   ("K = 64", dict(K=64), "K=64"), ("K = 0", dict(K=0), "K=0")]
    for fn in ("clm8_gemm", "clm4_gemm_m8"):
        call = fp32_form(fn)
        for what, kw, word in [(f"{p} NULL", {p: None}, "null") for p in ("A", "sA", "B", "sB", "C")] + shape_cases + [
                ("A misaligned", dict(A=A + 8), "aligned"), ("B misaligned", dict(B=B + 4), "aligned"), ("C misaligned", dict(C=C_ + 4), "aligned"),
                ("sA at an odd address", dict(sA=sA + 1), "aligned"), ("sB at an odd address", dict(sB=sB + 2), "aligned")]:
            rc = call(**kw)
            assert rc == -1 and fn in err() and word in err(), (fn, what, rc, err())
    for what, kw, word in [(f"{p} NULL", {p: None}, "null") for p in ("A", "B", "S")] + shape_cases + [
            ("A misaligned", dict(A=A + 8), "aligned"), ("B misaligned", dict(B=B + 1), "aligned"), ("S misaligned", dict(S=C_ + 4), "aligned"),
            ("empty range", dict(c=0), "K-blocks"), ("begin past the end", dict(b=5, c=1), "K-blocks"), ("range past the end", dict(b=2, c=3), "K-blocks"),
            ("begin + count wraps", dict(b=2 ** 64 - 1, c=2), "K-blocks"),
            ("2048 K-blocks", dict(K=64 * 2048, c=2048), "overflow")]:
        rc = i32_form(**kw)
        assert rc == -1 and "clm8_gemm_i32" in err() and word in err(), (what, rc, err())


# ---------------------------------------------------------------- the container methods
CLIENT = r'''
#include <CloverMatrix4.h>
#include <CloverMatrix8.h>
int main(int argc, char **)
{
    const uint64_t M = 256, N = 128, K = 384;
    CloverMatrix8 A8(M, K), B8(N, K);
    CloverMatrix4 A4(M, K);
    CloverMatrix32 C(M, N);
    if (argc > 1000) {          /* compiled and linked, not run: there may be no device */
        A8.gemm(B8, C);
        A4.gemm(B8, C);
        const CloverMatrix4 &cA4 = A4;
        const CloverMatrix4 B4(N, K);
        cA4.gemm(B4, C);        /* the 4 x 4 overload is still found */
    }
    return 0;
}
'''


@pytest.mark.parametrize("explicit", [False, True])
@pytest.mark.parametrize("order", ["4 then 8", "8 then 4", "4 only"])
def test_container_methods_compile_and_link(tmp_path, explicit, order):
    """both gemm methods from a C++ client, in the tracked and the explicit-sync builds, whichever header comes first (CloverMatrix4.h alone
    brings CloverMatrix8 along: no cycle between the two)"""
    lib = build_hip_library()
    src = CLIENT
    if order == "8 then 4":
        src = src.replace("#include <CloverMatrix4.h>\n#include <CloverMatrix8.h>", "#include <CloverMatrix8.h>\n#include <CloverMatrix4.h>")
    elif order == "4 only":
        src = src.replace("#include <CloverMatrix8.h>\n", "")
    client = tmp_path / "gemm8_client.cpp"
    client.write_text(src)
    flags = ["-DCLOVER_HIP_EXPLICIT_SYNC"] if explicit else []
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", *flags, f"-I{INC}", str(client), "-o", str(tmp_path / "gemm8_client"),
                    f"-L{lib.parent}", "-lclover_hip", f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
