"""CloverVector32 / CloverMatrix32 on the device (clover_amd/csrc/fp32.hip, the BITS = 32 threshold of threshold4.hip) against the functions
of include/clover_fp32.h through tests/fp32_restate.cpp: bit for bit, except dot FAST, which is held to the bound its order gives.

Shapes follow the kernels' constants: F32_X_BYTES = 16 KiB (4096 elements of x per LDS chunk), F32_MVM_U = 8 chain steps (256 columns) per
unrolled round, 8 rows per wave and 8 or 32 per workgroup, F32_DOT_CH = 4096 elements per LDS round of dot EXACT, 64 x 64 transpose
tiles, 16384 elements in the one-workgroup threshold."""
import ctypes as C
import os

import numpy as np
import pytest

from clover_amd.lib_binding import DOT_EXACT, DOT_FAST, THRESHOLD_FAST, THRESHOLD_REFERENCE
from fp32_helpers import (KINDS, bits, fast_dot_bound, fast_threshold_model, iht_problem, make_axpy, make_ops, rfp, threshold_data)  # noqa: F401

pytestmark = pytest.mark.gpu


def same(a, b):
    return np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------- scale_and_add
@pytest.mark.parametrize("n", [128, 1000, 8192, (1 << 20) + 128])
def test_scale_and_add_every_value_kind_out_of_place_and_in_place(hip, rfp, n):
    """1000 is padded to 1024 (the ABI sees n_pad); 2^20 + 128 leaves the last workgroup 32 of its 1024 groups"""
    n_pad = (n + 127) // 128 * 128
    for kind in KINDS:
        u, v, a = make_axpy(kind, n_pad, n)
        want = rfp.scale_and_add(u, v, a)
        assert same(hip.f32_scale_and_add(u, v, float(a)), want), kind
        assert same(hip.f32_scale_and_add(u, v, float(a), in_place=True), want), kind
    if n == 8192:                                                             # the data is what the CPU tests say it is
        assert np.count_nonzero(want) > 0


# ---------------------------------------------------------------- dot
@pytest.mark.parametrize("n", [128, 8192, 4096 + 128, 8192 + 128, 1 << 20])
def test_dot_exact_is_the_32_chain_order(hip, rfp, n):
    """4096 + 128 and 8192 + 128: one and two full LDS rounds of k_f32_dot_exact and a short one"""
    for kind in KINDS:
        u, v, _ = make_ops(kind, 1, n, n)
        got = hip.f32_dot(u, v, DOT_EXACT)
        assert bits(got)[0] == bits(rfp.dot(u, v))[0], (kind, got, rfp.dot(u, v))


@pytest.mark.parametrize("n", [128, 8192 + 128, (1 << 20) + 128, 1 << 22, (1 << 22) + (1 << 20) + 128])
def test_dot_fast_is_reproducible_and_within_its_bound(hip, rfp, n):
    """|d - exact| <= gamma_D sum |u_i v_i| with D = L + 26 (fast_dot_bound derives it from the kernel).  On 256 CUs the grid is capped at
    1024 workgroups = 2^20 elements per round: 2^20 + 128 gives some lanes a second group, 2^22 exactly the 4 of one unrolled round,
    2^22 + 2^20 + 128 a second, partial round"""
    cus = hip.device_info()["compute_units"]
    u, v, _ = make_ops("magnitudes", 1, n, n)
    du, dv = hip.to_device(u), hip.to_device(v)
    d1, d2 = hip.f32_dot(du, dv, DOT_FAST), hip.f32_dot(du, dv, DOT_FAST)
    assert bits(d1)[0] == bits(d2)[0]
    exact, absum = rfp.dot64(u, v)
    lim = fast_dot_bound(absum, n, cus)
    print(f"n={n}: |d - exact| = {abs(float(d1) - exact):.3e}, bound {lim:.3e}")
    assert abs(float(d1) - exact) <= lim


# ---------------------------------------------------------------- mvm
MVM_SHAPES = [(128, 128), (384, 4096), (128, 4096 + 128), (640, 1152), (256, 8576), (16384, 128)]


@pytest.mark.parametrize("rows,cols", MVM_SHAPES)
def test_mvm_and_the_fused_form_equal_the_host_rows(hip, rfp, rows, cols):
    """(128, 128): 4 chain steps, fewer than the unroll of 8.  (384, 4096) / (128, 4096 + 128): one x chunk of 16 KiB, and a short second
    one.  (640, 1152): 36 steps = 4 unrolled rounds + 4 single ones (rows is a multiple of 128, so no workgroup of 8 or 32 rows has a
    tail).  (256, 8576): three chunks.  (16384, 128): the first row count that takes the four-wave workgroup on 256 CUs
    (rows / 32 >= 2 x CUs); the shapes above take the one-wave one."""
    L = hip.lib
    for kind in KINDS:
        A, x, a = make_ops(kind, rows, cols, rows + cols)
        u = make_ops(kind, 1, rows, 7)[0] if kind != "subnormal" else (make_ops(kind, 1, rows, 7)[0] * np.float32(2.0 ** -70)).astype(np.float32)
        a = float(a) if kind != "subnormal" else 1.0
        d = rfp.mvm(A, rows, cols, x)
        r = rfp.scale_and_add(u, d, a)
        dA = hip.to_device(A)
        assert same(hip.f32_mvm(dA, rows, cols, x), d), kind
        t, r2 = hip.f32_mvm_scale_and_add(dA, rows, cols, x, u, a)
        assert same(t, d) and same(r2, r), kind
        t, r2 = hip.f32_mvm_scale_and_add(dA, rows, cols, x, u, a, want_t=False)
        assert t is None and same(r2, r), kind
        t, r2 = hip.f32_mvm_scale_and_add(dA, rows, cols, x, u, a, in_place=True)
        assert same(t, d) and same(r2, r), kind
        if rows >= 256:                                                       # two row shards at pointer offsets, the second one in place
            dx, du, dt, dr = hip.to_device(x), hip.to_device(u), hip.alloc(4 * rows), hip.alloc(4 * rows)
            cut = 128
            hip.check(L.clm_f32_mvm_scale_and_add(dA.ptr, cut, cols, dx.ptr, du.ptr, a, dt.ptr, dr.ptr, None))
            hip.check(L.clm_f32_mvm_scale_and_add(dA.ptr + 4 * cut * cols, rows - cut, cols, dx.ptr, du.ptr + 4 * cut, a, dt.ptr + 4 * cut,
                                                  du.ptr + 4 * cut, None))
            assert same(dt.download(np.float32, rows), d), kind
            assert same(dr.download(np.float32, rows)[:cut], r[:cut]) and same(du.download(np.float32, rows)[cut:], r[cut:]), kind
            assert same(du.download(np.float32, rows)[:cut], u[:cut]), kind


def test_mvm_streams_a_matrix_beyond_the_infinity_cache_with_one_wave_workgroups(hip, rfp):
    """128 x (2^19 + 128): 256 MiB + 64 KiB, the nontemporal loads of the one-wave kernel (the 64-bit test below takes them in the
    four-wave one).  One random row block repeated: the test is about the load path, every row still has its own sum"""
    rows, cols = 128, (1 << 19) + 128
    rng = np.random.default_rng(1)
    A = np.tile((rng.choice([-1.0, 1.0], size=1 << 20) * np.exp2(rng.uniform(-3, 3, size=1 << 20))).astype(np.float32), rows * cols // (1 << 20) + 1)[:rows * cols]
    x = make_ops("magnitudes", 1, cols, 2)[0]
    assert same(hip.f32_mvm(A, rows, cols, x), rfp.mvm(A, rows, cols, x))


def test_mvm_addresses_rows_beyond_4_gib(hip, rfp):
    """a (32768 + 128) x 32768 matrix of small integers filled on the device; the last 128 rows start 4 GiB into it.  Their sums are
    exact integers: the test is about addresses"""
    rows, cols = 32768 + 128, 32768
    L = hip.lib
    dA, dx = hip.alloc(4 * rows * cols), hip.alloc(4 * cols)
    hip.check(L.clv_fill_random_ints_f32(dA.ptr, rows * cols, 3, 11, 0, None))
    hip.check(L.clv_fill_random_ints_f32(dx.ptr, cols, 3, 12, 0, None))
    dr = hip.alloc(4 * rows)
    hip.check(L.clv_memset(dr.ptr, 0xFF, 4 * rows, None))
    hip.check(L.clm_f32_mvm(dA.ptr, rows, cols, dx.ptr, dr.ptr, None))
    tail = np.empty(128 * cols, np.float32)
    hip.check(L.clv_memcpy_d2h(tail.ctypes.data, dA.ptr + 4 * (rows - 128) * cols, tail.nbytes, None))
    x = dx.download(np.float32, cols)
    hip.sync()
    got = dr.download(np.float32, rows)
    want = rfp.mvm(tail, 128, cols, x)
    assert np.array_equal(want, (tail.reshape(128, cols).astype(np.float64) @ x.astype(np.float64)).astype(np.float32))     # exact integers
    assert np.count_nonzero(want) > 100 and same(got[rows - 128:], want)
    assert not np.any(np.isnan(got))                                          # every row was stored


# ---------------------------------------------------------------- transpose
@pytest.mark.parametrize("rows,cols", [(128, 128), (128, 384), (640, 256), (128, 1024), (132, 200), (4, 68)])
def test_transpose_moves_every_element(hip, rows, cols):
    """(132, 200) and (4, 68): the ABI takes multiples of 4, and these leave edge tiles of the 64 x 64 grid partly masked either way"""
    A = np.arange(rows * cols, dtype=np.uint32).view(np.float32)              # every element its own bit pattern (NaN patterns included)
    got = hip.f32_transpose(A, rows, cols)
    assert np.array_equal(got.view(np.uint32).reshape(cols, rows), A.view(np.uint32).reshape(rows, cols).T)


# ---------------------------------------------------------------- threshold
def _threshold_case(n_pad, kind):
    n = n_pad - 37 if n_pad > 128 else 100
    x = threshold_data(kind, n_pad, n_pad)
    x[n:] = np.float32(-5.5)                                                  # padding: not ours to touch
    return n, x


@pytest.mark.parametrize("kind", ["distinct", "ties"])
@pytest.mark.parametrize("n_pad", [128, 1024, 16384, 16384 + 128, 1 << 20])
def test_threshold_fast_and_reference(hip, rfp, n_pad, kind):
    """16384 is the last size of the one-workgroup kernel (16 words per thread), 16384 + 128 the first of the large path; below that the
    large path is taken once more with CLV_F32_THRESHOLD_SMALL=0 and must give the small kernel's bits"""
    n, x = _threshold_case(n_pad, kind)
    for k in (1, n // 4, n - 1):
        ref = hip.f32_threshold(x, n, k, THRESHOLD_REFERENCE)
        assert same(ref, rfp.threshold(x, n, k)), (k, "reference")
        fast = hip.f32_threshold(x, n, k, THRESHOLD_FAST)
        assert same(fast, fast_threshold_model(x, n, k)), (k, "fast")
        assert np.array_equal(np.sort(np.abs(fast[:n])), np.sort(np.abs(ref[:n]))), (k, "multiset")
        assert same(fast[n:], x[n:]) and same(ref[n:], x[n:])
        if n_pad <= 16384:
            os.environ["CLV_F32_THRESHOLD_SMALL"] = "0"
            try:
                large = hip.f32_threshold(x, n, k, THRESHOLD_FAST)
            finally:
                del os.environ["CLV_F32_THRESHOLD_SMALL"]
            assert same(large, fast), (k, "large path")


def test_threshold_k_zero_and_k_at_least_n(hip):
    n, x = _threshold_case(1024, "distinct")
    for mode in (THRESHOLD_FAST, THRESHOLD_REFERENCE):
        got = hip.f32_threshold(x, n, 0, mode)
        assert not np.any(got[:n]) and same(got[n:], x[n:])
        assert same(hip.f32_threshold(x, n, n, mode), x) and same(hip.f32_threshold(x, n, n + 5, mode), x)


# ---------------------------------------------------------------- the loop
@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("m,n", [(128, 256), (256, 512), (384, 1024)])
def test_iht_loop_equals_the_separate_calls_and_the_host_loop(hip, rfp, m, n, ties):
    L = hip.lib
    Phi, PhiT, y, mu = iht_problem(m, n, m + n, ties)
    K, iters = n // 8, 4
    dPhi, dPhiT = hip.to_device(Phi), hip.to_device(PhiT)
    for threshold in (0, 1, 2):
        for x_len in (n, n - 50):
            one = hip.f32_iht(dPhi, dPhiT, m, n, y, iters, K, float(mu), threshold, x_len=x_len)           # buffers prefilled with 0x55
            # the separate calls on the device
            dy, x, t1, t2, t3 = hip.to_device(y), hip.alloc(4 * n), hip.alloc(4 * m), hip.alloc(4 * m), hip.alloc(4 * n)
            hip.check(L.clv_memset(x.ptr, 0, 4 * n, None))
            for _ in range(iters):
                hip.check(L.clm_f32_mvm(dPhi.ptr, m, n, x.ptr, t1.ptr, None))
                hip.check(L.clv_f32_scale_and_add(dy.ptr, t1.ptr, -1.0, m, t2.ptr, None))
                hip.check(L.clm_f32_mvm(dPhiT.ptr, n, m, t2.ptr, t3.ptr, None))
                hip.check(L.clv_f32_scale_and_add(x.ptr, t3.ptr, float(mu), n, x.ptr, None))
                if threshold:
                    hip.check(L.clv_f32_threshold_mode(x.ptr, x_len, n, K, THRESHOLD_FAST if threshold == 1 else THRESHOLD_REFERENCE, None, None))
            sep = {"x": x.download(np.float32, n), "t1": t1.download(np.float32, m), "t2": t2.download(np.float32, m), "t3": t3.download(np.float32, n)}
            for name in sep:
                assert same(one[name], sep[name]), (threshold, x_len, name)
            # the host loop of shim functions (FAST: the same loop with the lowest-index rule in place of the heap walk)
            if threshold == 1:
                hx = np.zeros(n, np.float32)
                for _ in range(iters):
                    h1 = rfp.mvm(Phi, m, n, hx)
                    h2 = rfp.scale_and_add(y, h1, -1.0)
                    h3 = rfp.mvm(PhiT, n, m, h2)
                    hx = fast_threshold_model(rfp.scale_and_add(hx, h3, mu), x_len, K)
                host = {"x": hx, "t1": h1, "t2": h2, "t3": h3}
            else:
                host = rfp.iht(Phi, PhiT, m, n, y, iters, K, mu, threshold, x_len=x_len)[0]
            for name in host:
                assert same(one[name], host[name]), (threshold, x_len, name, "host")
            if threshold:
                assert np.count_nonzero(one["x"][:x_len]) == K


def test_iht_zero_iterations_clears_x_and_nothing_else(hip):
    Phi, PhiT, y, mu = iht_problem(128, 256, 1)
    got = hip.f32_iht(Phi, PhiT, 128, 256, y, 0, 32, float(mu), 1)
    assert not np.any(got["x"].view(np.uint32))
    for name in ("t1", "t2", "t3"):
        assert np.all(got[name].view(np.uint32) == 0x55555555), name
