"""tests/cpp/sharded_gather_root_timing.cpp: in the sharded GEMM loop, mode CLM4_GEMM_GATHER_ROOT with eight shards on one device, the events
of a timed step are ordered on EVERY shard -- clm4_sharded_step_timing gives a kernel time > 0 and an exchange time >= 0 -- also on the
shards that exchange nothing and with the compute streams 20 steps behind the host.  An exchange stream that does not wait for its
shard's kernel closes the step before the kernel has run and the exchange time comes out negative."""
import subprocess

import pytest

from clover_amd.build import build_hip_library, repo_root

ROOT = repo_root()


def _build(tmp_path):
    lib = build_hip_library()
    exe = tmp_path / "sharded_gather_root_timing"
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "cpp" / "sharded_gather_root_timing.cpp"),
                    "-o", str(exe), f"-L{lib.parent}", "-lclover_hip", f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_the_client_builds_and_reports_no_device_on_cpu(tmp_path):
    p = subprocess.run([str(_build(tmp_path))], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and ("no_device" in p.stdout or "timing ok" in p.stdout), (p.returncode, p.stdout, p.stderr)


@pytest.mark.gpu
def test_every_shard_of_a_gather_root_step_ends_its_exchange_after_its_kernel(tmp_path):
    p = subprocess.run([str(_build(tmp_path))], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "timing ok" in p.stdout, (p.returncode, p.stdout, p.stderr)
    assert sum("exchange_ms" in ln for ln in p.stdout.splitlines()) == 24
