"""clm_f16_iht_batch (include/clover_hip_batch_f16.h) on the GPU: the half-precision Q_IHT / Q_GD loop for several signals with one Phi,
every step batched.  x, t1, t2 and t3 of every signal equal clm_f16_iht on that signal and the CPU loop over the restatement
(tests/half16_restate.c), bit for bit; x is cleared on every call; a C++ client goes through the headers (iht_loop_batch, Q_IHT_batch,
Q_GD_batch and the batch mvm methods) in both container modes and both exactness builds and equals the method calls."""
import subprocess

import numpy as np
import pytest

from clover_amd.build import build_hip_library, repo_root
from f16_batch_helpers import IHT_SHAPES, MU, _iht_problem, _modes, forced, pa, same16
from half16_helpers import rh  # noqa: F401
from test_half16 import lowest_index_threshold

ROOT = repo_root()
ITERS = (0, 1, 3)
NVECS = (3, 9)
NAMES = ("x", "t1", "t2", "t3")
_LOOPS = {}


def _signals(R, m, n, count):
    """Phi, PhiT and `count` measurements that differ from one another: y_j = f16(y + 0.25 j roll(y, j))"""
    Phi, PhiT, y = _iht_problem(R, m, n)
    return Phi, PhiT, [y if j == 0 else R.scale_and_add(y, np.roll(y, j), np.float32(0.25 * j)) for j in range(count)]


def _cpu_loop(R, m, n, x_len, K, thr, j, iters):
    """the loop over the restatement for signal j, computed once per case"""
    key = (m, n, x_len, K, thr, j)
    if key not in _LOOPS:
        Phi, PhiT, ys = _signals(R, m, n, max(NVECS))
        x, out = np.zeros(n, np.uint16), {0: dict(x=np.zeros(n, np.uint16))}
        for it in range(1, max(ITERS) + 1):
            t1 = R.mvm(Phi, m, n, x)
            t2 = R.scale_and_add(ys[j], t1, np.float32(-1.0))
            t3 = R.mvm(PhiT, n, m, t2)
            x = R.scale_and_add(x, t3, np.float32(MU))
            if thr:
                x = R.threshold(x, x_len, K) if thr == 2 else lowest_index_threshold(x, x_len, K)
            out[it] = dict(x=x, t1=t1, t2=t2, t3=t3)
        _LOOPS[key] = out
    return _LOOPS[key][iters]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", range(3))
@pytest.mark.parametrize("shape", IHT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gpu_iht_batch_equals_the_single_call_per_signal_and_the_cpu_loop(hip, rh, shape, mode):  # noqa: F811
    m, n, x_len = shape
    name, thr, K = _modes(x_len)[mode]
    Phi, PhiT, ys = _signals(rh, m, n, max(NVECS))
    dPhi, dPhiT = hip.to_device(Phi), hip.to_device(PhiT)
    L = hip.lib
    for iters in ITERS:
        single = [hip.mf16_iht(Phi, PhiT, m, n, y, iters, K, MU, thr, x_len=x_len, prefill=0x55) for y in ys]
        for j in (0, max(NVECS) - 1):                                # the CPU loop for the first and the last signal
            for k in NAMES:
                if iters or k == "x":
                    assert same16(single[j][k], _cpu_loop(rh, m, n, x_len, K, thr, j, iters)[k]), (name, iters, j, k, "cpu")
        for nvec in NVECS:
            for env in ("1", "0", None):
                with forced(env):
                    before = L.clv_mvm_batch_launches()
                    got = hip.mf16_iht_batch(dPhi, dPhiT, m, n, ys[:nvec], iters, K, MU, thr, x_len=x_len, prefill=0x55)
                    launches = L.clv_mvm_batch_launches() - before
                # unset: the measured rule, groups of three or more over these cache-resident matrices
                groups = 0 if env == "0" else (nvec + 7) // 8 if env == "1" else nvec // 8 + (nvec % 8 >= 3)
                assert launches == 2 * iters * groups, (name, iters, nvec, env, launches)
                for j in range(nvec):
                    for k in NAMES:
                        if iters == 0 and k != "x":
                            assert np.all(got[j][k] == 0x5555), (name, nvec, env, j, k)      # untouched: the prefill
                        else:
                            assert same16(got[j][k], single[j][k]), (name, iters, nvec, env, j, k, np.flatnonzero(got[j][k] != single[j][k])[:8])
                    if iters == 0:
                        assert not got[j]["x"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", range(3))
def test_gpu_iht_batch_clears_x_on_every_call(hip, rh, mode):  # noqa: F811
    """two iterations, then three, then none on the SAME buffers: every call starts from x = 0, so each equals the single call of its own
    iteration count; a call of 0 iterations clears every x and leaves t1..t3 as they were"""
    m, n, x_len = IHT_SHAPES[2]
    name, thr, K = _modes(x_len)[mode]
    nvec = 3
    Phi, PhiT, ys = _signals(rh, m, n, nvec)
    d = [hip.to_device(v) for v in (Phi, PhiT)]
    dy = [hip.to_device(y) for y in ys]
    lens = dict(x=n, t1=m, t2=m, t3=n)
    v = {k: [hip.alloc(2 * ln) for _ in range(nvec)] for k, ln in lens.items()}
    last = None
    with forced("1"):
        for iters in (2, 3, 0):
            hip.check(hip.lib.clm_f16_iht_batch(d[0].ptr, d[1].ptr, m, n, nvec, pa(v["x"]), x_len, pa(dy), pa(v["t1"]), pa(v["t2"]), pa(v["t3"]),
                                                iters, K, MU, thr, None))
            for j in range(nvec):
                want = hip.mf16_iht(Phi, PhiT, m, n, ys[j], iters, K, MU, thr, x_len=x_len) if iters else dict(last[j], x=np.zeros(n, np.uint16))
                for k, ln in lens.items():
                    assert same16(v[k][j].download(np.uint16, ln), want[k]), (name, iters, j, k)
            if iters:
                last = [hip.mf16_iht(Phi, PhiT, m, n, y, iters, K, MU, thr, x_len=x_len) for y in ys]


# ---------------------------------------------------------------- the headers
def _build_client(tmp_path, explicit, fast):
    lib = build_hip_library()
    exe = tmp_path / f"half16_batch_{'explicit' if explicit else 'tracked'}_{'fast' if fast else 'reference'}"
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", *(["-DCLOVER_HIP_EXPLICIT_SYNC"] if explicit else []),
                    *(["-DCLOVER_FAST"] if fast else []), f"-I{ROOT / 'include'}", str(ROOT / "tests" / "cpp" / "half16_batch.cpp"), "-o", str(exe),
                    f"-L{lib.parent}", "-lclover_hip", f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("explicit", [False, True])
def test_gpu_header_batch_methods_equal_the_method_calls(tmp_path, explicit, fast):
    """m = 256, n = 512, 9 signals: mvm_batch, mvm_scaleAndAdd_batch (both overloads), iht_loop_batch, Q_IHT_batch and Q_GD_batch give the
    digests of the single methods called signal after signal, in both residency builds and under both exactness settings; the batched
    kernel ran (the launch counter of the client's own process)"""
    out = subprocess.run([str(_build_client(tmp_path, explicit, fast)), "256", "512", "9", "3", "64", "0.5"], check=True, capture_output=True,
                         text=True, timeout=300).stdout
    lines = {ln.split()[0]: dict(f.split("=") for f in ln.split()[1:]) for ln in out.splitlines() if "=" in ln and " " in ln}
    for name in ("mvm", "pair", "loop", "iht", "gd"):
        assert lines[name]["batch"] == lines[name]["single"], (name, out)
    assert "gd_differs_from_iht=1" in out and "done" in out, out
    nz = int(next(ln for ln in out.splitlines() if ln.startswith("nonzero=")).split("=")[1])
    assert 0 < nz <= 9 * 64, out
    # groups of 8 + 1: mvm 1, pair 2, and 2 x 3 iterations for each of the three loops -- the remainder group of one is a single call
    assert int(next(ln for ln in out.splitlines() if ln.startswith("launches=")).split("=")[1]) == 1 + 2 + 3 * 6, out
