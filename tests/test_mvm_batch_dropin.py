"""The batch methods of the containers (CloverMatrix4::mvm_batch, mvm_scaleAndAdd_batch, iht_loop_batch, CloverVector4::threshold_batch,
Q_IHT_batch / Q_GD_batch of CloverIHT.h) through a C++ client, in the page-tracked and the -DCLOVER_HIP_EXPLICIT_SYNC build: each equals its
single-call partner on the host-visible bytes, host pointers kept across a batch call read its results, and one recovery run -- 8 K-sparse
signals of ones with ONE Phi (512 x 1024, K = 32, the generator of tests/test_iht_recovery.py) -- brings all eight supports back."""
import subprocess

import numpy as np
import pytest

from clover_amd.build import build_hip_library, repo_root

ROOT = repo_root()
M, N, K, COUNT, ITERS = 512, 1024, 32, 8, 60
# the step of normalised IHT for columns of squared norm m / 3 (entries uniform in (-1, 1)) is 3 / m = 1 / 171; 1 / 200 stays below it
MU = 1.0 / 200


def _build(tmp_path, explicit):
    lib = build_hip_library()
    exe = tmp_path / ("mvm_batch_dropin_explicit" if explicit else "mvm_batch_dropin")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-DCLOVER_STOCHASTIC_ROUNDING_DISABLED=1",
                    *(["-DCLOVER_HIP_EXPLICIT_SYNC"] if explicit else []), f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "cpp" / "mvm_batch_dropin.cpp"), "-o", str(exe), f"-L{lib.parent}", "-lclover_hip",
                    f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


@pytest.mark.parametrize("explicit", [False, True])
def test_batch_client_compiles_in_both_builds(tmp_path, explicit):
    assert _build(tmp_path, explicit).exists()


def test_batch_client_compiles_with_stochastic_rounding_enabled(tmp_path):
    """without -DCLOVER_STOCHASTIC_ROUNDING_DISABLED the batch methods loop over the single methods: the same client builds"""
    lib = build_hip_library()
    exe = tmp_path / "mvm_batch_dropin_stochastic"
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "cpp" / "mvm_batch_dropin.cpp"), "-o",
                    str(exe), f"-L{lib.parent}", "-lclover_hip", f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert exe.exists()


@pytest.mark.gpu
@pytest.mark.parametrize("explicit", [False, True])
def test_batch_methods_equal_their_single_call_partners_and_recover_eight_supports(tmp_path, explicit):
    rng = np.random.default_rng(7)
    Phi = rng.uniform(-1, 1, size=(M, N)).astype(np.float32)
    truth = np.zeros((COUNT, N), np.float32)
    for j in range(COUNT):
        truth[j, np.random.default_rng(100 + j).permutation(N)[:K]] = 1.0
    Phi.tofile(tmp_path / "phi.f32")
    np.stack([Phi @ truth[j] for j in range(COUNT)]).astype(np.float32).tofile(tmp_path / "ys.f32")
    out = subprocess.run([str(_build(tmp_path, explicit)), str(tmp_path), str(M), str(N), str(COUNT), str(ITERS), str(K), repr(MU)], check=True,
                         capture_output=True, text=True, timeout=300).stdout
    for name in ("mvm_batch", "mvm_scaleAndAdd_batch", "mvm_scaleAndAdd_batch_in_place", "threshold_batch", "Q_IHT_batch", "Q_GD_batch"):
        assert f"{name}_equal=1" in out, (name, out)
    assert "kept_pointer=1" in out and "done" in out, out
    hits = []
    for j in range(COUNT):
        x = np.fromfile(tmp_path / f"x{j}.f32", np.float32)
        assert x.size == N and np.count_nonzero(x) <= K
        hits.append(len(set(np.argsort(-np.abs(x))[:K].tolist()) & set(np.flatnonzero(truth[j]).tolist())))
    print("supports recovered:", hits)
    assert hits == [K] * COUNT, hits
