"""The batched transposed methods of CloverMatrix8 (mvm_transposed_batch, mvm_transposed_scaleAndAdd_batch, iht_loop_batch_one_matrix) and
Q_IHT_batch_one_matrix / Q_GD_batch_one_matrix of CloverIHT.h through a C++ client, in both rounding builds -- with
-DCLOVER_STOCHASTIC_ROUNDING_DISABLED and as one would compile against the reference, without it -- each page-tracked and with
-DCLOVER_HIP_EXPLICIT_SYNC.  Without a GPU: the client compiles in every build, the rounding-disabled object references
clm8_iht_batch_one_matrix and the stochastic one the positioned call, and a client that uses none of the new methods references none of
the new symbols.  On the GPU, 256 x 384 (six output blocks: three workgroups) with 5 signals and the same keys on both sides: every
batch method equals the loop of its single method on the host-visible bytes, the loops equal Q_IHT_one_matrix / Q_GD_one_matrix per signal,
Phi's keys afterwards are equal, and the batched kernel ran (CLV_MVM_BATCH=1; the counter rose over the batch calls only)."""
import os
import subprocess

import numpy as np
import pytest

from clover_amd.build import build_hip_library, repo_root
from clover_amd.lib_binding import SIGNATURES_BATCH_T8

ROOT = repo_root()
M, N, K, COUNT, ITERS = 256, 384, 24, 5, 4
MU = 1.0 / 200
BUILDS = [(det, explicit) for det in (True, False) for explicit in (False, True)]
IDS = [("rounding_disabled" if det else "stochastic") + ("-explicit_sync" if explicit else "-tracked") for det, explicit in BUILDS]


def _flags(det, explicit):
    return ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", *(["-DCLOVER_STOCHASTIC_ROUNDING_DISABLED=1"] if det else []),
            *(["-DCLOVER_HIP_EXPLICIT_SYNC"] if explicit else []), f"-I{ROOT / 'include'}"]


# the client of the three transposed batch families is one source; the classes of this family:
CLIENT = ROOT / "tests" / "cpp" / "mvm_transposed_batch_dropin.cpp"
CLASSES = ["-DDROPIN_MATRIX=CloverMatrix8", "-DDROPIN_VECTOR=CloverVector8"]


def _build(tmp_path, det, explicit):
    lib = build_hip_library()
    exe = tmp_path / f"m8_mvm_transposed_batch_dropin_{int(det)}{int(explicit)}"
    subprocess.run([*_flags(det, explicit), *CLASSES, str(CLIENT), "-o", str(exe), f"-L{lib.parent}",
                    "-lclover_hip", f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def _undefined(tmp_path, source, det, explicit):
    obj = tmp_path / (source.stem + f"_{int(det)}{int(explicit)}.o")
    subprocess.run([*_flags(det, explicit), *CLASSES, "-c", str(source), "-o", str(obj)], check=True)
    out = subprocess.run(["nm", "-u", str(obj)], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


@pytest.mark.parametrize("det,explicit", BUILDS, ids=IDS)
def test_the_client_compiles_in_every_build_and_references_the_calls_of_its_rounding(tmp_path, det, explicit):
    assert _build(tmp_path, det, explicit).exists()
    und = _undefined(tmp_path, CLIENT, det, explicit)
    assert "clm8_mvm_transposed_batch" in und
    if det:
        assert {"clm8_iht_batch_one_matrix", "clm8_mvm_transposed_scale_and_add_batch"} <= und
    else:
        assert "clm8_mvm_transposed_batch_at" in und and "clm8_iht_batch_one_matrix" not in und


@pytest.mark.parametrize("det", [True, False], ids=["rounding_disabled", "stochastic"])
def test_a_client_that_uses_none_of_the_new_methods_references_none_of_the_new_symbols(tmp_path, det):
    und = _undefined(tmp_path, ROOT / "tests" / "cpp" / "m8_mvm_transposed_dropin.cpp", det, False)
    assert "clm8_mvm_transposed" in und, "the client of the single calls does use those"
    assert not und & set(SIGNATURES_BATCH_T8), und & set(SIGNATURES_BATCH_T8)


@pytest.mark.gpu
@pytest.mark.parametrize("det,explicit", BUILDS, ids=IDS)
def test_the_batch_methods_equal_the_loops_of_their_single_methods(tmp_path, det, explicit):
    rng = np.random.default_rng(11)
    Phi = rng.uniform(-1, 1, size=(M, N)).astype(np.float32)
    truth = np.zeros((COUNT, N), np.float32)
    for j in range(COUNT):
        truth[j, np.random.default_rng(100 + j).permutation(N)[:K]] = 1.0
    Phi.tofile(tmp_path / "phi.f32")
    np.stack([Phi @ truth[j] for j in range(COUNT)]).astype(np.float32).tofile(tmp_path / "ys.f32")
    out = subprocess.run([str(_build(tmp_path, det, explicit)), str(tmp_path), str(M), str(N), str(COUNT), str(ITERS), str(K), repr(MU)], check=True,
                         capture_output=True, text=True, timeout=300, env=dict(os.environ, CLV_MVM_BATCH="1")).stdout
    for name in ("mvm_transposed_batch", "mvm_transposed_scaleAndAdd_batch", "mvm_transposed_scaleAndAdd_batch_in_place", "Q_IHT_batch_one_matrix",
                 "Q_GD_batch_one_matrix"):
        assert f"{name}_equal=1" in out, (name, out)
        assert f"{name}_keys_equal=1" in out, (name, out)
    assert "launches_rose=1" in out and "single_side_launches=0" in out and "done" in out, out
