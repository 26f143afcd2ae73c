"""Every entry point of include/clover_hip_fp32.h that writes device memory, on the guarded arena of tests/guarded.py: outputs exact over
their declared range (against tests/fp32_restate.cpp), inputs and everything outside unchanged.  Every `workspace` argument is given
exactly the bytes its size query returns, prefilled with 0x00 and with 0xFF, and the results are equal.  The cases live here, not in
tests/test_guard_bands.py, whose table is pinned to the surface of clover_hip.h."""
import numpy as np
import pytest

from clover_amd.lib_binding import DOT_EXACT, DOT_FAST, SIGNATURES_FP32, THRESHOLD_FAST, THRESHOLD_REFERENCE
from fp32_helpers import fast_threshold_model, iht_problem, make_axpy, make_ops, rfp, threshold_data  # noqa: F401
from guarded import Arena

pytestmark = pytest.mark.gpu

# no device memory is written by the size queries
EXCLUDED = {"clv_f32_dot_workspace_bytes", "clv_f32_threshold_workspace_bytes"}
CASES = {}


def case(name):
    def deco(fn):
        CASES[name] = fn
        return fn
    return deco


def run(hip, regions, call, expected, seed=1):
    """regions: (name, kind, data-or-nbytes[, fill]); returns what the arena held in its output / inout / scratch regions"""
    arena = Arena(hip, seed)
    for name, kind, what, *fill in regions:
        if kind in ("input", "inout"):
            arena.add(name, kind, data=what)
        else:
            arena.add(name, kind, nbytes=what, fill=fill[0] if fill else None)
    arena.upload()
    try:
        p = {name: arena.ptr(name) for name in arena.regions}
        hip.check(call(hip.lib, p))
        hip.check(hip.lib.clv_stream_sync(None))
        return arena.check(expected(hip) if callable(expected) else expected)
    finally:
        arena.close()


# ---------------------------------------------------------------- vectors
N = 1024 + 128


@case("clv_f32_scale_and_add out of place")
def _(hip, R, fill):
    u, v, a = make_axpy("magnitudes", N, 1)
    return run(hip, [("u", "input", u), ("v", "input", v), ("r", "output", 4 * N)],
               lambda L, p: L.clv_f32_scale_and_add(p["u"], p["v"], float(a), N, p["r"], None), {"r": R.scale_and_add(u, v, a)})


@case("clv_f32_scale_and_add in place")
def _(hip, R, fill):
    u, v, a = make_axpy("cancel", N, 2)
    return run(hip, [("u", "inout", u), ("v", "input", v)], lambda L, p: L.clv_f32_scale_and_add(p["u"], p["v"], float(a), N, p["u"], None),
               {"u": R.scale_and_add(u, v, a)})


def _dot(mode):
    def go(hip, R, fill):
        n = 8192 + 128
        u, v, _ = make_ops("magnitudes", 1, n, 3)
        ws = int(hip.lib.clv_f32_dot_workspace_bytes(n))
        assert ws == 0                                                        # a pointer with nothing behind it but guard
        want = {"out": np.array([R.dot(u, v)], np.float32)} if mode == DOT_EXACT else (lambda h: {"out": np.array([h.f32_dot(u, v, DOT_FAST)], np.float32)})
        return run(hip, [("u", "input", u), ("v", "input", v), ("out", "output", 4), ("ws", "scratch", ws, fill)],
                   lambda L, p: L.clv_f32_dot(p["u"], p["v"], n, mode, p["out"], p["ws"], None), want)
    return go


case("clv_f32_dot exact")(_dot(DOT_EXACT))
case("clv_f32_dot fast")(_dot(DOT_FAST))


def _threshold(mode, n_pad, kind):
    def go(hip, R, fill):
        n = n_pad - 37
        k = n // 4
        x = threshold_data(kind, n_pad, 4)
        x[n:] = np.float32(-5.5)
        L = hip.lib
        ws = int(L.clv_f32_threshold_workspace_bytes(n_pad) if mode == THRESHOLD_FAST else L.clv_threshold_reference_workspace_bytes_k(n_pad, k))
        want = fast_threshold_model(x, n, k) if mode == THRESHOLD_FAST else R.threshold(x, n, k)
        return run(hip, [("x", "inout", x), ("ws", "scratch", ws, fill)],
                   lambda L, p: L.clv_f32_threshold_mode(p["x"], n, n_pad, k, mode, p["ws"], None), {"x": want})
    return go


case("clv_f32_threshold_mode fast, one workgroup")(_threshold(THRESHOLD_FAST, 1024, "ties"))
case("clv_f32_threshold_mode fast, large path")(_threshold(THRESHOLD_FAST, 16384 + 128, "ties"))
case("clv_f32_threshold_mode reference")(_threshold(THRESHOLD_REFERENCE, 16384 + 128, "distinct"))


# ---------------------------------------------------------------- matrices
ROWS, COLS = 256, 384


@case("clm_f32_mvm")
def _(hip, R, fill):
    A, x, _ = make_ops("magnitudes", ROWS, COLS, 5)
    return run(hip, [("A", "input", A), ("x", "input", x), ("r", "output", 4 * ROWS)],
               lambda L, p: L.clm_f32_mvm(p["A"], ROWS, COLS, p["x"], p["r"], None), {"r": R.mvm(A, ROWS, COLS, x)})


def _fused(with_t, in_place):
    def go(hip, R, fill):
        A, x, a = make_ops("magnitudes", ROWS, COLS, 6)
        u = make_ops("magnitudes", 1, ROWS, 7)[0]
        d = R.mvm(A, ROWS, COLS, x)
        r = R.scale_and_add(u, d, a)
        regions = [("A", "input", A), ("x", "input", x), ("u", "inout" if in_place else "input", u)]
        want = {"u": r} if in_place else {"r2": r}
        if with_t:
            regions.append(("t", "output", 4 * ROWS))
            want["t"] = d
        if not in_place:
            regions.append(("r2", "output", 4 * ROWS))
        return run(hip, regions, lambda L, p: L.clm_f32_mvm_scale_and_add(p["A"], ROWS, COLS, p["x"], p["u"], float(a), p.get("t"),
                                                                         p["u"] if in_place else p["r2"], None), want)
    return go


case("clm_f32_mvm_scale_and_add")(_fused(True, False))
case("clm_f32_mvm_scale_and_add without t")(_fused(False, False))
case("clm_f32_mvm_scale_and_add in place")(_fused(True, True))


@case("clm_f32_transpose with edge tiles")
def _(hip, R, fill):
    rows, cols = 132, 200
    A = make_ops("magnitudes", rows, cols, 8)[0]
    return run(hip, [("A", "input", A), ("At", "output", 4 * rows * cols)], lambda L, p: L.clm_f32_transpose(p["A"], rows, cols, p["At"], None),
               {"At": R.transpose(A, rows, cols)})


def _iht(threshold):
    def go(hip, R, fill):
        m, n, iters, K = 128, 256, 3, 32
        Phi, PhiT, y, mu = iht_problem(m, n, 9, ties=True)
        if threshold == 1:
            hx = np.zeros(n, np.float32)
            for _ in range(iters):
                h1 = R.mvm(Phi, m, n, hx)
                h2 = R.scale_and_add(y, h1, -1.0)
                h3 = R.mvm(PhiT, n, m, h2)
                hx = fast_threshold_model(R.scale_and_add(hx, h3, mu), n - 20, K)
            want = {"x": hx, "t1": h1, "t2": h2, "t3": h3}
        else:
            want = R.iht(Phi, PhiT, m, n, y, iters, K, mu, threshold, x_len=n - 20)[0]
        return run(hip, [("Phi", "input", Phi), ("PhiT", "input", PhiT), ("y", "input", y), ("x", "output", 4 * n), ("t1", "output", 4 * m),
                         ("t2", "output", 4 * m), ("t3", "output", 4 * n)],
                   lambda L, p: L.clm_f32_iht(p["Phi"], p["PhiT"], m, n, p["x"], n - 20, p["y"], p["t1"], p["t2"], p["t3"], iters, K, float(mu),
                                              threshold, None), want)
    return go


for _thr, _name in ((0, "gd"), (1, "fast"), (2, "reference")):
    case(f"clm_f32_iht {_name}")(_iht(_thr))


@pytest.mark.parametrize("name", list(CASES))
def test_call_writes_its_outputs_and_nothing_else(hip, rfp, name):
    """with a workspace region: once prefilled with 0x00 and once with 0xFF, and the outputs agree (the arena has checked both against
    the reference already)"""
    a = CASES[name](hip, rfp, 0x00)
    if "ws" in a:
        b = CASES[name](hip, rfp, 0xFF)
        assert all(np.array_equal(a[k], b[k]) for k in a if k != "ws"), name


def test_the_cases_cover_every_fp32_entry_point():
    assert {name.split()[0] for name in CASES} | EXCLUDED == set(SIGNATURES_FP32)
    assert EXCLUDED <= set(SIGNATURES_FP32) and not EXCLUDED & {name.split()[0] for name in CASES}
    with_workspace = {"clv_f32_dot", "clv_f32_threshold_mode"}                # the entry points with a `workspace` argument
    assert with_workspace <= {name.split()[0] for name in CASES}
