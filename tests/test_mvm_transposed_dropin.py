"""The one-matrix methods of the containers (CloverMatrix4::mvm_transposed, mvm_transposed_scaleAndAdd in both overloads,
iht_loop_one_matrix, Q_IHT_one_matrix / Q_GD_one_matrix of CloverIHT.h) through a C++ client, in the page-tracked and the
-DCLOVER_HIP_EXPLICIT_SYNC build: each equals its partner on a stored transpose on the host-visible bytes, a host pointer kept across a
call reads its result, and one recovery run -- a K-sparse signal of ones, Phi 512 x 1024, K = 32, the generator of
tests/test_iht_recovery.py with the parameters of tests/test_mvm_batch_dropin.py -- brings the support back with ONE matrix."""
import subprocess

import numpy as np
import pytest

from clover_amd.build import build_hip_library, repo_root
from test_mvm_batch_dropin import ITERS, MU, K, M, N

ROOT = repo_root()


def _build(tmp_path, explicit, det=True):
    lib = build_hip_library()
    exe = tmp_path / f"mvm_transposed_dropin_{int(explicit)}{int(det)}"
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", *(["-DCLOVER_STOCHASTIC_ROUNDING_DISABLED=1"] if det else []),
                    *(["-DCLOVER_HIP_EXPLICIT_SYNC"] if explicit else []), f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "cpp" / "mvm_transposed_dropin.cpp"), "-o", str(exe), f"-L{lib.parent}", "-lclover_hip",
                    f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


@pytest.mark.parametrize("explicit", [False, True])
def test_one_matrix_client_compiles_in_both_builds(tmp_path, explicit):
    assert _build(tmp_path, explicit).exists()


def test_one_matrix_client_compiles_with_stochastic_rounding_enabled(tmp_path):
    """without -DCLOVER_STOCHASTIC_ROUNDING_DISABLED the fused methods are the two calls: the same client builds"""
    assert _build(tmp_path, False, det=False).exists()


@pytest.mark.gpu
@pytest.mark.parametrize("explicit", [False, True])
def test_one_matrix_methods_equal_their_stored_transpose_partners_and_recover_the_support(tmp_path, explicit):
    rng = np.random.default_rng(7)
    Phi = rng.uniform(-1, 1, size=(M, N)).astype(np.float32)
    truth = np.zeros(N, np.float32)
    truth[np.random.default_rng(100).permutation(N)[:K]] = 1.0
    Phi.tofile(tmp_path / "phi.f32")
    (Phi @ truth).astype(np.float32).tofile(tmp_path / "y.f32")
    out = subprocess.run([str(_build(tmp_path, explicit)), str(tmp_path), str(M), str(N), str(ITERS), str(K), repr(MU)], check=True,
                         capture_output=True, text=True, timeout=300).stdout
    for name in ("mvm_transposed", "mvm_transposed_scaleAndAdd", "mvm_transposed_scaleAndAdd_in_place", "Q_IHT_one_matrix", "Q_GD_one_matrix"):
        assert f"{name}_equal=1" in out, (name, out)
    assert "kept_pointer=1" in out and "done" in out, out
    x = np.fromfile(tmp_path / "x.f32", np.float32)
    assert x.size == N and np.count_nonzero(x) <= K
    hit = len(set(np.argsort(-np.abs(x))[:K].tolist()) & set(np.flatnonzero(truth).tolist()))
    print("support recovered:", hit)
    assert hit == K, hit
