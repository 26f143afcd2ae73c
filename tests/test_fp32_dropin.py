"""CloverVector32.h / CloverMatrix32.h / CloverIHT.h under -DCLOVER_FP32_ON_DEVICE through tests/cpp/fp32_device.cpp, linked against the
real library: page-tracked and -DCLOVER_HIP_EXPLICIT_SYNC, default and -DCLOVER_FAST.  The client compares every routed method with the
clover_fp32:: function on the same data in its own process and prints one `name=0|1` line per check (see its header comment)."""
import subprocess

import pytest

from clover_amd.build import build_hip_library, repo_root

ROOT = repo_root()
CHECKS = ["transpose", "transpose_parallel", "mvm", "getData_stays_current", "mvm_parallel", "scaleAndAdd_out_of_place",
          "scaleAndAdd_parallel_out_of_place", "scaleAndAdd_in_place", "scaleAndAdd_parallel_in_place", "view_writes_through", "dot", "dot_parallel",
          "dot_scalar_stays_host", "threshold_distinct", "threshold_parallel_distinct", "threshold_ties", "threshold_parallel_ties", "mvm_scaleAndAdd",
          "mvm_scaleAndAdd_in_place", "q_iht_equals_method_calls", "q_gd_equals_method_calls", "q_iht_recovers_the_support"]


def _build(tmp_path, explicit, fast):
    lib = build_hip_library()
    exe = tmp_path / f"fp32_device_{int(explicit)}{int(fast)}"
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-DCLOVER_FP32_ON_DEVICE", *(["-DCLOVER_HIP_EXPLICIT_SYNC"] if explicit else []),
                    *(["-DCLOVER_FAST"] if fast else []), f"-I{ROOT / 'include'}", str(ROOT / "tests" / "cpp" / "fp32_device.cpp"), "-o", str(exe),
                    f"-L{lib.parent}", "-lclover_hip", f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("explicit", [False, True])
def test_header_client_builds_with_the_switch(tmp_path, explicit, fast):
    assert _build(tmp_path, explicit, fast).exists()


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("explicit", [False, True])
def test_routed_methods_equal_the_host_functions(tmp_path, explicit, fast):
    """N = 1024 (Phi 512 x 1024, a 32-sparse signal): every method, Q_IHT / Q_GD against the five method calls, and the recovery run"""
    p = subprocess.run([str(_build(tmp_path, explicit, fast)), "1024"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "done" in p.stdout, (p.returncode, p.stdout, p.stderr)
    for name in CHECKS:
        assert f"\n{name}=1\n" in "\n" + p.stdout, (name, p.stdout)
