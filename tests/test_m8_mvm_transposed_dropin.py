"""The one-matrix methods of CloverMatrix8 (mvm_transposed, mvm_transposed_scaleAndAdd in both overloads, iht_loop_one_matrix,
Q_IHT_one_matrix / Q_GD_one_matrix of CloverIHT.h) through a C++11 client: with rounding disabled in the default (page-tracked) build and
with -DCLOVER_HIP_EXPLICIT_SYNC, and in the stochastic build (no -DCLOVER_STOCHASTIC_ROUNDING_DISABLED, the reference's default).  Each
result equals transpose() + its existing partner on the host-visible bytes -- stochastic: from the same keys, the loops against the same
steps composed from method calls -- and a host pointer kept across a call reads its result.  Phi 512 x 1024 and the parameters of
tests/test_mvm_batch_dropin.py.  The headers also compile on their own."""
import subprocess

import numpy as np
import pytest

from clover_amd.build import build_hip_library, repo_root
from test_mvm_batch_dropin import ITERS, MU, K, M, N

ROOT = repo_root()
BUILDS = {"default": ([], True), "CLOVER_HIP_EXPLICIT_SYNC": (["-DCLOVER_HIP_EXPLICIT_SYNC"], True), "stochastic": ([], False)}


def _build(tmp_path, flags, det=True):
    lib = build_hip_library()
    exe = tmp_path / f"m8_mvm_transposed_dropin_{len(flags)}{int(det)}"
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", *(["-DCLOVER_STOCHASTIC_ROUNDING_DISABLED=1"] if det else []), *flags,
                    f"-I{ROOT / 'include'}", str(ROOT / "tests" / "cpp" / "m8_mvm_transposed_dropin.cpp"), "-o", str(exe), f"-L{lib.parent}",
                    "-lclover_hip", f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


@pytest.mark.parametrize("build", list(BUILDS))
def test_one_matrix_m8_client_compiles_in_every_build(tmp_path, build):
    assert _build(tmp_path, *BUILDS[build]).exists()


@pytest.mark.parametrize("det", [True, False], ids=["rounding_disabled", "stochastic"])
@pytest.mark.parametrize("headers", [("CloverMatrix8.h",), ("CloverMatrix8.h", "CloverIHT.h"), ("CloverIHT.h",)], ids=lambda h: "+".join(h))
def test_the_headers_compile_on_their_own(tmp_path, headers, det):
    src = tmp_path / "only.cpp"
    src.write_text("".join(f"#include <{h}>\n" for h in headers) + "int main() { return 0; }\n")
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-fsyntax-only", *(["-DCLOVER_STOCHASTIC_ROUNDING_DISABLED=1"] if det else []),
                    f"-I{ROOT / 'include'}", str(src)], check=True)


@pytest.mark.gpu
@pytest.mark.parametrize("build", list(BUILDS))
def test_one_matrix_m8_methods_equal_their_stored_transpose_partners(tmp_path, build):
    rng = np.random.default_rng(7)
    Phi = rng.uniform(-1, 1, size=(M, N)).astype(np.float32)
    truth = np.zeros(N, np.float32)
    truth[np.random.default_rng(100).permutation(N)[:K]] = 1.0
    Phi.tofile(tmp_path / "phi.f32")
    (Phi @ truth).astype(np.float32).tofile(tmp_path / "y.f32")
    out = subprocess.run([str(_build(tmp_path, *BUILDS[build])), str(tmp_path), str(M), str(N), str(ITERS), str(K), repr(MU)], check=True,
                         capture_output=True, text=True, timeout=300).stdout
    for name in ("mvm_transposed", "mvm_transposed_scaleAndAdd", "mvm_transposed_scaleAndAdd_in_place", "Q_IHT_one_matrix", "Q_GD_one_matrix"):
        assert f"{name}_equal=1" in out, (name, out)
    assert "kept_pointer=1" in out and "done" in out, out
