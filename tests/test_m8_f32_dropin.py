"""CloverMatrix8 on CloverVector32 vectors through the headers (tests/cpp/m8_f32_loop.cpp, built with -DCLOVER_FP32_ON_DEVICE): the
Q_IHT / Q_GD overloads of CloverIHT.h equal the five method calls written out on the same containers, the _one_matrix forms equal the
two-matrix ones with PhiT = transpose_parallel(Phi), mvm_scaleAndAdd / mvm_transposed_scaleAndAdd (both overloads) equal their two
calls and mvm_transposed equals transpose_parallel + mvm -- under both exactness settings (the reference's threshold, -DCLOVER_FAST).
The client's object takes the five new calls."""
import subprocess

import pytest

from clover_amd.build import build_hip_library, repo_root
from clover_amd.lib_binding import SIGNATURES_M8_F32

ROOT = repo_root()


def _build_client(tmp_path, fast):
    lib = build_hip_library()
    exe = tmp_path / f"m8_f32_loop_{'fast' if fast else 'reference'}"
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-DCLOVER_FP32_ON_DEVICE", *(["-DCLOVER_FAST"] if fast else []), f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "cpp" / "m8_f32_loop.cpp"), "-o", str(exe), f"-L{lib.parent}", "-lclover_hip", f"-Wl,-rpath,{lib.parent}",
                    "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_the_client_builds_and_takes_the_five_calls(tmp_path):
    und = subprocess.run(["nm", "-u", str(_build_client(tmp_path, False))], check=True, capture_output=True, text=True).stdout.split()
    for name in SIGNATURES_M8_F32:
        assert name in und, name


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["reference", "fast"])
def test_gpu_header_loops_equal_the_method_calls_written_out(tmp_path, fast):
    """m = 256, n = 640 (a multiple of neither 256 nor 512 columns), 3 iterations, K = 64"""
    exe = _build_client(tmp_path, fast)
    out = subprocess.run([str(exe), "256", "640", "3", "64", "0.5"], check=True, capture_output=True, text=True, timeout=300).stdout
    lines = {ln.split()[0]: dict(f.split("=") for f in ln.split()[1:]) for ln in out.splitlines() if "=" in ln and " " in ln}
    for name in ("mvm", "pair", "iht", "iht1", "gd", "gd1"):
        assert lines[name]["fused"] == lines[name]["written_out"], (name, out)
    assert "gd_differs_from_iht=1" in out and "done" in out, out
    nz = int(next(ln for ln in out.splitlines() if ln.startswith("nonzero=")).split("=")[1])
    assert 0 < nz <= 64, out
