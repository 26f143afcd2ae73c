"""The one-matrix methods of the containers on CloverVector8 vectors (CloverMatrix4::mvm_transposed, mvm_transposed_scaleAndAdd in both
overloads, iht_loop_one_matrix, Q_IHT_one_matrix / Q_GD_one_matrix of CloverIHT.h) through a C++ client, with rounding disabled in the
default (page-tracked) build, with -DCLOVER_FAST and with -DCLOVER_HIP_EXPLICIT_SYNC: each equals transpose() + its existing partner on the
host-visible bytes, and a host pointer kept across a call reads its result.  Phi 512 x 1024 and the parameters of
tests/test_mvm_batch_dropin.py."""
import subprocess

import numpy as np
import pytest

from clover_amd.build import build_hip_library, repo_root
from test_mvm_batch_dropin import ITERS, MU, K, M, N

ROOT = repo_root()
BUILDS = {"default": [], "CLOVER_FAST": ["-DCLOVER_FAST"], "CLOVER_HIP_EXPLICIT_SYNC": ["-DCLOVER_HIP_EXPLICIT_SYNC"]}


def _build(tmp_path, flags, det=True):
    lib = build_hip_library()
    exe = tmp_path / f"mvm_v8_transposed_dropin_{len(flags)}{int(det)}"
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", *(["-DCLOVER_STOCHASTIC_ROUNDING_DISABLED=1"] if det else []), *flags,
                    f"-I{ROOT / 'include'}", str(ROOT / "tests" / "cpp" / "mvm_v8_transposed_dropin.cpp"), "-o", str(exe), f"-L{lib.parent}",
                    "-lclover_hip", f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


@pytest.mark.parametrize("build", list(BUILDS))
def test_one_matrix_v8_client_compiles_in_every_build(tmp_path, build):
    assert _build(tmp_path, BUILDS[build]).exists()


def test_one_matrix_v8_client_compiles_with_stochastic_rounding_enabled(tmp_path):
    """without -DCLOVER_STOCHASTIC_ROUNDING_DISABLED the fused methods are the two calls: the same client builds"""
    assert _build(tmp_path, [], det=False).exists()


@pytest.mark.gpu
@pytest.mark.parametrize("build", list(BUILDS))
def test_one_matrix_v8_methods_equal_their_stored_transpose_partners(tmp_path, build):
    rng = np.random.default_rng(7)
    Phi = rng.uniform(-1, 1, size=(M, N)).astype(np.float32)
    truth = np.zeros(N, np.float32)
    truth[np.random.default_rng(100).permutation(N)[:K]] = 1.0
    Phi.tofile(tmp_path / "phi.f32")
    (Phi @ truth).astype(np.float32).tofile(tmp_path / "y.f32")
    out = subprocess.run([str(_build(tmp_path, BUILDS[build])), str(tmp_path), str(M), str(N), str(ITERS), str(K), repr(MU)], check=True,
                         capture_output=True, text=True, timeout=300).stdout
    for name in ("mvm_transposed", "mvm_transposed_scaleAndAdd", "mvm_transposed_scaleAndAdd_in_place", "Q_IHT_one_matrix", "Q_GD_one_matrix"):
        assert f"{name}_equal=1" in out, (name, out)
    assert "kept_pointer=1" in out and "done" in out, out
