"""The batch methods of CloverMatrix8 (mvm_batch, mvm_scaleAndAdd_batch, iht_loop_batch, Q_IHT_batch / Q_GD_batch of CloverIHT.h) through a
C++ client, in both rounding builds -- with -DCLOVER_STOCHASTIC_ROUNDING_DISABLED and as
one would compile against the reference, without it -- each page-tracked and with -DCLOVER_HIP_EXPLICIT_SYNC.  On the GPU, 512 x 1024 with
8 signals and the same keys on both sides (matrices and vectors): every batch method equals the loop of its single method on the
host-visible bytes, Q_IHT_batch / Q_GD_batch equal the loop of Q_IHT / Q_GD, the matrices' keys afterwards are equal, and the batched kernel
ran (clv_mvm_batch_launches rose over the batch calls and not over the single ones)."""
import subprocess

import numpy as np
import pytest

from clover_amd.build import build_hip_library, repo_root

ROOT = repo_root()
M, N, K, COUNT, ITERS = 512, 1024, 32, 8, 5
MU = 1.0 / 200
BUILDS = [(det, explicit) for det in (True, False) for explicit in (False, True)]
IDS = [("rounding_disabled" if det else "stochastic") + ("-explicit_sync" if explicit else "-tracked") for det, explicit in BUILDS]


def _build(tmp_path, det, explicit):
    lib = build_hip_library()
    exe = tmp_path / f"m8_mvm_batch_dropin_{int(det)}{int(explicit)}"
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", *(["-DCLOVER_STOCHASTIC_ROUNDING_DISABLED=1"] if det else []),
                    *(["-DCLOVER_HIP_EXPLICIT_SYNC"] if explicit else []), f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "cpp" / "m8_mvm_batch_dropin.cpp"), "-o", str(exe), f"-L{lib.parent}", "-lclover_hip",
                    f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


@pytest.mark.parametrize("det,explicit", BUILDS, ids=IDS)
def test_m8_batch_client_compiles_in_every_build(tmp_path, det, explicit):
    assert _build(tmp_path, det, explicit).exists()


@pytest.mark.gpu
@pytest.mark.parametrize("det,explicit", BUILDS, ids=IDS)
def test_m8_batch_methods_equal_the_loops_of_their_single_methods(tmp_path, det, explicit):
    rng = np.random.default_rng(7)
    Phi = rng.uniform(-1, 1, size=(M, N)).astype(np.float32)
    truth = np.zeros((COUNT, N), np.float32)
    for j in range(COUNT):
        truth[j, np.random.default_rng(100 + j).permutation(N)[:K]] = 1.0
    Phi.tofile(tmp_path / "phi.f32")
    np.stack([Phi @ truth[j] for j in range(COUNT)]).astype(np.float32).tofile(tmp_path / "ys.f32")
    out = subprocess.run([str(_build(tmp_path, det, explicit)), str(tmp_path), str(M), str(N), str(COUNT), str(ITERS), str(K), repr(MU)], check=True,
                         capture_output=True, text=True, timeout=300).stdout
    for name in ("mvm_batch", "mvm_scaleAndAdd_batch", "mvm_scaleAndAdd_batch_in_place", "Q_IHT_batch", "Q_GD_batch"):
        assert f"{name}_equal=1" in out, (name, out)
        assert f"{name}_keys_equal=1" in out, (name, out)
    assert "launches_rose=1" in out and "single_side_launches=0" in out and "done" in out, out
