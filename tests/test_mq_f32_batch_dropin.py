"""Several CloverVector32 signals with one CloverMatrix4 / CloverMatrix8 through the headers (tests/cpp/mq_f32_batch_dropin.cpp, built with
-DCLOVER_FP32_ON_DEVICE): Q_IHT_batch / Q_GD_batch on three signals equal three Q_IHT / Q_GD calls, mvm_batch equals three mvm calls and
mvm_scaleAndAdd_batch (both overloads) three mvm_scaleAndAdd calls, for both matrix widths, with the batched kernel forced
(CLV_MVM_BATCH=1).  The client's object takes the batched loop of both widths; a client built without the switch takes none of the six calls."""
import os
import subprocess

import pytest

from clover_amd.build import build_hip_library, repo_root
from clover_amd.lib_binding import SIGNATURES_BATCH_F32

ROOT = repo_root()


def _build_client(tmp_path, source, *defines):
    lib = build_hip_library()
    exe = tmp_path / (source.split(".")[0] + "".join(defines))
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", *defines, f"-I{ROOT / 'include'}", str(ROOT / "tests" / "cpp" / source), "-o", str(exe),
                    f"-L{lib.parent}", "-lclover_hip", f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def _undefined(exe):
    return subprocess.run(["nm", "-u", str(exe)], check=True, capture_output=True, text=True).stdout.split()


def test_the_client_takes_the_batched_calls_and_a_client_without_the_switch_takes_none(tmp_path):
    und = _undefined(_build_client(tmp_path, "mq_f32_batch_dropin.cpp", "-DCLOVER_FP32_ON_DEVICE"))
    for name in SIGNATURES_BATCH_F32:
        assert name in und, name
    und = _undefined(_build_client(tmp_path, "m8_mvm_batch_dropin.cpp"))   # the same headers (both matrix classes, CloverIHT.h) without the switch
    assert not [name for name in SIGNATURES_BATCH_F32 if name in und]


@pytest.mark.gpu
def test_gpu_header_batch_calls_equal_the_single_calls_signal_after_signal(tmp_path):
    """m = 256, n = 640, 3 iterations, K = 64, three signals, both widths"""
    exe = _build_client(tmp_path, "mq_f32_batch_dropin.cpp", "-DCLOVER_FP32_ON_DEVICE")
    out = subprocess.run([str(exe), "256", "640", "3", "64", "0.5"], check=True, capture_output=True, text=True, timeout=300,
                         env={**os.environ, "CLV_MVM_BATCH": "1"}).stdout
    lines = {ln.split()[0]: dict(f.split("=") for f in ln.split()[1:]) for ln in out.splitlines() if " " in ln}
    for width in ("m4", "m8"):
        for name in ("iht", "gd", "mvm", "pair"):
            assert lines[f"{width}_{name}"]["batch"] == lines[f"{width}_{name}"]["single"], (width, name, out)
        assert lines[f"{width}_iht"]["batch"] != lines[f"{width}_gd"]["batch"], out
        nz = int(next(ln for ln in out.splitlines() if ln.startswith(f"{width}_nonzero=")).split("=")[1])
        assert 0 < nz <= 64, out
    assert "done" in out, out
