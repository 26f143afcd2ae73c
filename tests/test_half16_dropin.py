"""CloverVector16.h / CloverMatrix16.h through a C++ client with the reference's method names, in the page-tracked and the
-DCLOVER_HIP_EXPLICIT_SYNC build; Q_IHT / Q_GD on <CloverMatrix16, CloverVector16> against a host loop built from the checker; and an IHT
recovery run at N = 8192."""
import subprocess

import numpy as np
import pytest

from clover_amd.build import build_hip_library, repo_root
from clover_amd.lib_binding import THRESHOLD_FAST
from half16_helpers import U32, gamma, rh, rhp  # noqa: F401

ROOT = repo_root()


def _build(tmp_path, explicit):
    lib = build_hip_library()
    exe = tmp_path / ("half16_dropin_explicit" if explicit else "half16_dropin")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-DCLOVER_STOCHASTIC_ROUNDING_DISABLED=1",
                    *(["-DCLOVER_HIP_EXPLICIT_SYNC"] if explicit else []), f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "cpp" / "half16_dropin.cpp"), "-o", str(exe), f"-L{lib.parent}", "-lclover_hip",
                    f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


@pytest.mark.parametrize("explicit", [False, True])
def test_header_client_compiles_without_f16c_in_both_builds(tmp_path, explicit):
    """g++ -std=c++11 with no -mf16c / -march: the host conversions are integer arithmetic; code that includes <CloverVector16.h>,
    <CloverMatrix16.h> and instantiates Q_IHT / Q_GD on them links against the library"""
    assert _build(tmp_path, explicit).exists()


def _u16(path, n):
    a = np.fromfile(path, np.uint16)
    assert a.size == n, (path, a.size, n)
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("explicit", [False, True])
@pytest.mark.parametrize("mode", ["iht", "gd"])
def test_header_methods_and_q_iht_loop(tmp_path, rh, mode, explicit):
    N, iters = 1024, 10
    m, n = (N // 2, N) if mode == "iht" else (3 * N // 2, N)
    K, mu = N // 4, (1.0 / m if mode == "iht" else 0.4)
    rng = np.random.default_rng(m)
    phi = rng.uniform(-1, 1, size=(m, n)).astype(np.float32)
    if mode == "gd":
        phi /= np.linalg.norm(phi, axis=1, keepdims=True)
    xt = np.zeros(n, np.float32)
    xt[rng.permutation(n)[:64]] = 1.0
    y = (phi @ (xt if mode == "iht" else np.sign(rng.uniform(-1, 1, n)).astype(np.float32))).astype(np.float32)
    phi.tofile(tmp_path / "phi.f32")
    y.tofile(tmp_path / "y.f32")
    out = subprocess.run([str(_build(tmp_path, explicit)), str(tmp_path), mode, str(m), str(n), str(iters), str(K), repr(mu)], check=True,
                         capture_output=True, text=True, timeout=600).stdout
    assert "mvm_equal=1 mvm_f32_equal=1" in out and "scalar_twins_equal=1" in out and "view_writes_through=1" in out and "done" in out, out

    Phi = rh.quantize(phi).ravel()
    PhiT = rh.transpose(Phi, m, n)
    yq = rh.quantize(y)
    x32 = phi[0] - phi[1]
    xq = rh.quantize(x32)
    assert np.array_equal(_u16(tmp_path / "phi.bin", m * n), Phi) and np.array_equal(_u16(tmp_path / "phit.bin", m * n), PhiT)
    assert np.array_equal(_u16(tmp_path / "y.bin", m), yq) and np.array_equal(_u16(tmp_path / "xq.bin", n), xq)
    # mvm through the header = the checker; mvm_scalar / dot_scalar within their bounds
    r1 = _u16(tmp_path / "r1.bin", m)
    assert np.array_equal(r1, rh.mvm(Phi, m, n, xq))
    f1 = np.fromfile(tmp_path / "f1.f32", np.float32)
    assert np.array_equal(f1.view(np.uint32), rh.mvm_f32(Phi, m, n, x32).view(np.uint32))
    # mvm_scalar: one running fp32 sum of n separately rounded products -- n roundings of the products (u each) and n - 1 of the sums:
    # |y - exact| <= gamma_(n + 1) sum |terms|, then the rounding to f16 (relative 2^-11, or half a subnormal step)
    e, a = rh.mvm64(Phi, m, n, xq)
    r3 = _u16(tmp_path / "r3_scalar.bin", m).view(np.float16).astype(np.float64)
    lim = gamma(n + 1) * a
    assert np.all(np.abs(r3 - e) <= lim + 2.0 ** -11 * (np.abs(e) + lim) + 2.0 ** -25)
    e32, a32 = rh.mvm_f32_64(Phi, m, n, x32)
    f3 = np.fromfile(tmp_path / "f3_scalar.f32", np.float32)
    assert np.all(np.abs(f3 - e32) <= U32 * np.abs(e32) + n * 2.0 ** -53 * a32)       # double accumulation, one rounding to fp32
    dots = dict(t.split("=") for t in out.split() if t.startswith("dot"))
    d_exact = np.array([int(dots["dot"], 16)], np.uint32).view(np.float32)[0]
    assert d_exact.view(np.uint32) == rh.dot(r1, yq).view(np.uint32)                  # the default build: the reference's order
    de, da = rh.mvm64(r1, 1, m, yq)
    d_fast = np.array([int(dots["dot_parallel"], 16)], np.uint32).view(np.float32)[0]
    d_scalar = np.array([int(dots["dot_scalar"], 16)], np.uint32).view(np.float32)[0]
    assert abs(float(d_fast) - de[0]) <= 2e-6 * da[0] and abs(float(d_scalar) - de[0]) <= gamma(m + 1) * da[0]
    # threshold_min_heap: the caller's heap holds the reference's entries, bits included
    k = max(K, 1)
    thr, hv, hi = rh.threshold_heap(xq, n, k)
    heap = np.fromfile(tmp_path / "heap.bin", np.uint32).reshape(k, 3)
    assert np.array_equal(_u16(tmp_path / "thr.bin", n), thr)
    assert np.array_equal(heap[:, 0], hv.view(np.uint32)) and np.array_equal(heap[:, 1], hi) and np.array_equal(heap[:, 2], xq[hi])
    # the loop: ten iterations equal a host loop of the checker's steps, bit for bit
    x = np.zeros(n, np.uint16)
    for _ in range(iters):
        t1 = rh.mvm(Phi, m, n, x)
        t2 = rh.scale_and_add(yq, t1, -1.0)
        t3 = rh.mvm(PhiT, n, m, t2)
        x = rh.scale_and_add(x, t3, np.float32(mu))
        if mode == "iht":
            x = rh.threshold(x, n, K)
    for name, want in (("x", x), ("t1", t1), ("t2", t2), ("t3", t3)):
        assert np.array_equal(_u16(tmp_path / f"{name}.bin", want.size), want), name
    assert np.count_nonzero(x) > 0


@pytest.mark.gpu
def test_f16_iht_recovers_the_sparse_support_at_n_8192(hip):
    """the reference's problem generator (Phi uniform(-1, 1), a K-sparse x of ones, y = Phi x in fp32) at N = 8192, m = N / 2: the
    half-precision loop x <- H_K(x + mu Phi'(y - Phi x)) on the device brings the support back"""
    m, n, K, iters, mu = 4096, 8192, 64, 60, 1.0 / 4096
    rng = np.random.default_rng(7)
    Phi = rng.uniform(-1, 1, size=(m, n)).astype(np.float32)
    x_true = np.zeros(n, np.float32)
    x_true[rng.permutation(n)[:K]] = 1.0
    y = Phi @ x_true
    L = hip.lib
    dPhi32, dy32 = hip.to_device(Phi), hip.to_device(y)
    dPhi, dPhiT, dy = hip.alloc(2 * m * n), hip.alloc(2 * m * n), hip.alloc(2 * m)
    hip.check(L.clm_f16_quantize(dPhi32.ptr, m, n, dPhi.ptr, None))
    hip.check(L.clm_f16_transpose(dPhi.ptr, m, n, dPhiT.ptr, None))
    hip.check(L.clv_f16_quantize(dy32.ptr, m, dy.ptr, None))
    x, t1, t2, t3, xr = hip.alloc(2 * n), hip.alloc(2 * m), hip.alloc(2 * m), hip.alloc(2 * n), hip.alloc(4 * n)
    hip.check(L.clv_memset(x.ptr, 0, 2 * n, None))
    for _ in range(iters):
        hip.check(L.clm_f16_mvm(dPhi.ptr, m, n, x.ptr, t1.ptr, None))
        hip.check(L.clv_f16_scale_and_add(dy.ptr, t1.ptr, -1.0, m, t2.ptr, None))
        hip.check(L.clm_f16_mvm(dPhiT.ptr, n, m, t2.ptr, t3.ptr, None))
        hip.check(L.clv_f16_scale_and_add(x.ptr, t3.ptr, mu, n, x.ptr, None))
        hip.check(L.clv_f16_threshold_mode(x.ptr, n, n, K, THRESHOLD_FAST, None, None))
    hip.check(L.clv_f16_restore(x.ptr, n, xr.ptr, None))
    xs = xr.download(np.float32, n)
    assert np.count_nonzero(xs) <= K
    hit = len(set(np.argsort(-np.abs(xs))[:K].tolist()) & set(np.flatnonzero(x_true).tolist()))
    err = float(np.linalg.norm(xs - x_true) / np.linalg.norm(x_true))
    print(f"f16: support {hit}/{K}, relative error {err:.3f}")
    assert hit == K and err < 0.05        # 11 significant bits per element: finer than the 8-bit vectors' bar (K - 1, 0.25)
