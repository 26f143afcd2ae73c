"""The batched transposed half-precision methods through the headers (tests/cpp/half16_transposed_batch.cpp):
CloverMatrix16::mvm_transposed_batch, mvm_transposed_scaleAndAdd_batch (both overloads), iht_loop_batch_one_matrix and the
Q_IHT_batch_one_matrix / Q_GD_batch_one_matrix overloads of CloverIHT.h, in both container modes (tracked, -DCLOVER_HIP_EXPLICIT_SYNC) and
both exactness builds (reference, -DCLOVER_FAST).  Every result is bit-identical to the single transposed methods called vector after
vector and to the loops written out method by method; the client runs under CLV_MVM_BATCH=1 and the batched kernel ran (the launch
counter of the client's own process)."""
import os
import subprocess

import pytest

from clover_amd.build import build_hip_library, repo_root

ROOT = repo_root()


def _build_client(tmp_path, explicit, fast):
    lib = build_hip_library()
    exe = tmp_path / f"half16_transposed_batch_{'explicit' if explicit else 'tracked'}_{'fast' if fast else 'reference'}"
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", *(["-DCLOVER_HIP_EXPLICIT_SYNC"] if explicit else []),
                    *(["-DCLOVER_FAST"] if fast else []), f"-I{ROOT / 'include'}", str(ROOT / "tests" / "cpp" / "half16_transposed_batch.cpp"), "-o",
                    str(exe), f"-L{lib.parent}", "-lclover_hip", f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("explicit", [False, True])
def test_gpu_header_batched_transposed_methods_equal_the_method_calls(tmp_path, explicit, fast):
    """m = 256, n = 640, 9 signals (a group of eight and a remainder group of one), 3 iterations, K = 64"""
    exe = _build_client(tmp_path, explicit, fast)
    und = subprocess.run(["nm", "-u", str(exe)], check=True, capture_output=True, text=True).stdout
    for name in ("clm_f16_mvm_transposed_batch", "clm_f16_mvm_transposed_scale_and_add_batch", "clm_f16_iht_batch_one_matrix"):
        assert name in und.split(), name
    assert "clm_f16_transpose" not in und.split(), "the client holds one matrix"
    out = subprocess.run([str(exe), "256", "640", "9", "3", "64", "0.5"], check=True, capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, CLV_MVM_BATCH="1")).stdout
    lines = {ln.split()[0]: dict(f.split("=") for f in ln.split()[1:]) for ln in out.splitlines() if "=" in ln and " " in ln}
    for name in ("mvm", "pair", "loop", "iht", "gd"):
        assert lines[name]["batch"] == lines[name]["single"], (name, out)
    assert "gd_differs_from_iht=1" in out and "done" in out, out
    nz = int(next(ln for ln in out.splitlines() if ln.startswith("nonzero=")).split("=")[1])
    assert 0 < nz <= 9 * 64, out
    # forced, two groups (8 + 1) each: mvm 2, pair 2 x 2, and 2 launches x 3 iterations x 2 groups for each of the three loops
    assert int(next(ln for ln in out.splitlines() if ln.startswith("launches=")).split("=")[1]) == 2 + 4 + 3 * 12, out
