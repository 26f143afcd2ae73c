"""CPU-side checks of the half-precision path: the checker (tests/half16_restate.c) is pinned against numpy's float16 and against float64,
its two builds agree, and the new C ABI entry points validate their arguments and link from C99 without a GPU."""
import subprocess

import numpy as np
import pytest

from clover_amd.build import build_hip_library, repo_root
from clover_amd.lib_binding import load_library
from half16_helpers import (assert_chain_bound, assert_f16_result_bound, f16_midpoints, make_f32, random_f16_bits, rh, rhp)  # noqa: F401


def test_widening_equals_numpy_on_every_bit_pattern(rh):
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    want = h.view(np.float16).astype(np.float32)
    got = rh.widen_all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))          # NaN payloads included
    assert np.array_equal(rh.restore(h).view(np.uint32), want.view(np.uint32))


def _narrow_inputs():
    parts = [f16_midpoints()]                                                   # every tie and its fp32 neighbours, both signs
    parts.append(np.array([65504.0, 65519.996, 65520.0, 65520.004, 65536.0, 1e5, 3.4e38, np.inf, 0.0, 2.0 ** -24, 2.0 ** -25,
                           np.float32(2.0 ** -25) * np.float32(1 + 2.0 ** -23), 2.0 ** -26, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 1e-45, 1e-38],
                          np.float32))
    parts.append(-parts[-1])
    parts.append(np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float32)[np.r_[0:0x7C01, 0x8000:0xFC01]])   # exact f16 values
    rng = np.random.default_rng(5)
    parts.append((rng.uniform(-1, 1, size=200000) * np.exp2(rng.integers(-30, 18, size=200000))).astype(np.float32))
    parts.append(rng.integers(0, 2 ** 32, size=200000, dtype=np.uint64).astype(np.uint32).view(np.float32))      # any bit pattern
    x = np.concatenate(parts)
    return x[~np.isnan(x)]


def test_narrowing_equals_numpy_round_to_nearest_even(rh):
    x = _narrow_inputs()
    with np.errstate(over="ignore"):
        want = x.astype(np.float16).view(np.uint16)
    got = rh.quantize(x)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (x[bad[:8]], got[bad[:8]], want[bad[:8]])
    # the cases by name
    one = lambda v: int(rh.quantize(np.array([v], np.float32))[0])          # noqa: E731
    assert one(65519.996) == 0x7BFF and one(65520.0) == 0x7C00 and one(-65520.0) == 0xFC00
    assert one(2.0 ** -24) == 0x0001 and one(2.0 ** -25) == 0x0000 and one(np.float32(2.0 ** -25) * np.float32(1 + 2.0 ** -23)) == 0x0001
    assert one(3 * 2.0 ** -25) == 0x0002                                       # tie between subnormals 1 and 2: to even
    assert one(-0.0) == 0x8000 and one(0.0) == 0 and one(np.inf) == 0x7C00 and one(-np.inf) == 0xFC00
    assert one(1.0 + 2.0 ** -11) == 0x3C00 and one(1.0 + 3 * 2.0 ** -11) == 0x3C02      # ties to even, both directions


def test_narrowing_keeps_nan_a_nan(rh):
    x = np.array([np.nan, -np.nan], np.float32)
    x = np.concatenate([x, np.array([0x7F800001, 0xFFC12345], np.uint32).view(np.float32)])
    got = rh.quantize(x)
    assert np.all(np.isnan(got.view(np.float16))) and np.array_equal(got >> 15, x.view(np.uint32) >> 31)


def _round_to_f32(q):
    """the fp32 value nearest to the rational q, ties to even (q well inside the fp32 range)"""
    from fractions import Fraction
    c = np.float32(float(q))
    cands = [c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))]
    best = min(cands, key=lambda f: (abs(Fraction(float(f)) - q), int(np.float32(f).view(np.uint32)) & 1))
    return np.float32(best)


def test_scale_and_add_is_one_fused_fma_then_rne(rh):
    """against exact rational arithmetic: r = f16(round_f32(v * s + u)), the product never rounded on its own"""
    from fractions import Fraction
    rng = np.random.default_rng(2)
    n = 2048
    u, v = random_f16_bits(rng, n, subnormal_share=0.1), random_f16_bits(rng, n, subnormal_share=0.1)
    v[:256] = random_f16_bits(rng, 256, 0, 1)                                  # cancellation: u = -v * s to within rounding
    s = np.float32(-0.3721)
    u[:256] = (-(v[:256].view(np.float16).astype(np.float32) * s)).astype(np.float16).view(np.uint16)
    uf, vf = u.view(np.float16).astype(np.float64), v.view(np.float16).astype(np.float64)
    f = np.array([_round_to_f32(Fraction(float(vf[i])) * Fraction(float(s)) + Fraction(float(uf[i]))) for i in range(n)], np.float32)
    want = f.astype(np.float16).view(np.uint16)
    got = rh.scale_and_add(u, v, s)
    assert np.array_equal(got, want)
    unfused = (vf.astype(np.float32) * s + uf.astype(np.float32)).astype(np.float16).view(np.uint16)
    assert not np.array_equal(unfused, want)                                   # the data tells a fused fma from a rounded product


@pytest.mark.parametrize("n", [128, 4096, 65536])
def test_dot_within_the_derived_bound_of_float64(rh, n):
    rng = np.random.default_rng(n)
    u, v = random_f16_bits(rng, n, -6, 6, 0.05), random_f16_bits(rng, n, -6, 6, 0.05)
    e, a = rh.mvm64(u, 1, n, v)
    assert_chain_bound(np.array([rh.dot(u, v)]), e, a, n, f"dot n={n}")
    assert a[0] > 0 and abs(e[0]) < a[0]


@pytest.mark.parametrize("rows,cols", [(64, 128), (48, 4096), (16, 16384)])
def test_mvm_within_the_derived_bound_of_float64(rh, rows, cols):
    rng = np.random.default_rng(rows * cols)
    A, x = random_f16_bits(rng, rows * cols, -4, 4, 0.05), random_f16_bits(rng, cols, -4, 4, 0.05)
    e, a = rh.mvm64(A, rows, cols, x)
    assert_chain_bound(rh.rowdots(A, rows, cols, x), e, a, cols, "rowdots")
    assert_f16_result_bound(rh.mvm(A, rows, cols, x), e, a, cols, "mvm f16")
    xf = (rng.normal(size=cols) * 3).astype(np.float32)
    e, a = rh.mvm_f32_64(A, rows, cols, xf)
    assert_chain_bound(rh.mvm_f32(A, rows, cols, xf), e, a, cols, "mvm f32")
    # the mvm rows are the dot, and the f16 result is the rounded row value
    assert rh.dot(A[:cols], x).view(np.uint32) == rh.rowdots(A, rows, cols, x)[0].view(np.uint32)
    assert np.array_equal(rh.mvm(A, rows, cols, x), rh.quantize(rh.rowdots(A, rows, cols, x)))


def test_chain_order_is_what_the_bits_say(rh):
    """a permutation that keeps every element in its chain and its position keeps the bits; the 32-chain order differs from a plain
    running sum on ordinary data (so a checker that summed in another order would be caught by the device comparison)"""
    rng = np.random.default_rng(9)
    n = 4096
    u, v = random_f16_bits(rng, n, -6, 6), random_f16_bits(rng, n, -6, 6)
    d = rh.dot(u, v)
    uf, vf = u.view(np.float16).astype(np.float32), v.view(np.float16).astype(np.float32)
    acc = np.zeros(32, np.float32)
    for j in range(0, n, 32):
        acc = (vf[j:j + 32].astype(np.float64) * uf[j:j + 32].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)     # 22 + 24 bits fit float64
    s = (acc[0:8] + acc[8:16]) + (acc[16:24] + acc[24:32])
    t = s[4:8] + s[0:4]
    assert np.float32((t[0] + t[2]) + (t[1] + t[3])).view(np.uint32) == d.view(np.uint32)
    plain = np.float32(0)
    for j in range(n):
        plain = np.float32(plain + vf[j] * uf[j])
    assert plain.view(np.uint32) != d.view(np.uint32)


def test_openmp_build_equals_the_serial_build(rh, rhp):
    rng = np.random.default_rng(4)
    rows, cols = 200, 1024
    A, x = random_f16_bits(rng, rows * cols, -4, 4, 0.05), random_f16_bits(rng, cols, -4, 4, 0.05)
    xf = (rng.normal(size=cols)).astype(np.float32)
    f = make_f32("ties", 1 << 16, 1)
    assert np.array_equal(rh.quantize(f), rhp.quantize(f))
    assert np.array_equal(rh.restore(A).view(np.uint32), rhp.restore(A).view(np.uint32))
    assert np.array_equal(rh.scale_and_add(A, A[::-1].copy(), 0.37), rhp.scale_and_add(A, A[::-1].copy(), 0.37))
    assert np.array_equal(rh.mvm(A, rows, cols, x), rhp.mvm(A, rows, cols, x))
    assert np.array_equal(rh.mvm_f32(A, rows, cols, xf).view(np.uint32), rhp.mvm_f32(A, rows, cols, xf).view(np.uint32))
    assert rh.dot(A[:cols], x).view(np.uint32) == rhp.dot(A[:cols], x).view(np.uint32)
    assert np.array_equal(rh.transpose(A, rows, cols), rhp.transpose(A, rows, cols))
    assert np.array_equal(rh.transpose(A, rows, cols).reshape(cols, rows), A.reshape(rows, cols).T)
    assert rhp.is_transpose(A, rows, cols, rh.transpose(A, rows, cols)) and not rhp.is_transpose(A, rows, cols, A)


@pytest.mark.parametrize("k", [1, 2, 3, 8, 9, 64, 65, 1000])
def test_restated_make_heap_equals_std_make_heap(rh, tmp_path_factory, k):
    exe = tmp_path_factory.getbasetemp() / "half16_stdheap"
    if not exe.exists():
        subprocess.run(["c++", "-O1", "-std=c++17", "-o", str(exe), str(repo_root() / "tests" / "cpp" / "half16_stdheap.cpp")], check=True)
    rng = np.random.default_rng(k)
    vals = rng.integers(0, 6, size=k).astype(np.float32)                       # many ties
    if k >= 8:
        vals[rng.integers(0, k, size=2)] = np.nan
    out = subprocess.run([str(exe)], input=" ".join(f"{b:08x}" for b in vals.view(np.uint32)), capture_output=True, text=True, check=True).stdout.split()
    want_bits, want_idx = [int(t, 16) for t in out[0::2]], [int(t) for t in out[1::2]]
    hv, hi = rh.make_heap_of(vals)
    assert list(hv.view(np.uint32)) == want_bits and list(hi) == want_idx


def test_threshold_walk_keeps_the_k_largest(rh):
    rng = np.random.default_rng(3)
    n, k = 1000, 100
    h = random_f16_bits(rng, 1024, -3, 3)
    h[rng.integers(0, n, size=300)] = np.float16(1.5).view(np.uint16)           # ties
    out, hv, hi = rh.threshold_heap(h, n, k)
    kept = np.flatnonzero(out[:n])
    assert kept.size == k and np.array_equal(out[kept], h[kept]) and np.array_equal(out[n:], h[n:])
    mag = np.abs(h[:n].view(np.float16).astype(np.float32))
    assert np.array_equal(np.sort(mag[kept]), np.sort(mag)[n - k:]) and sorted(hi) == sorted(kept)
    assert np.array_equal(rh.threshold(h, n, 0)[:n], np.zeros(n, np.uint16)) and np.array_equal(rh.threshold(h, n, n), h)


# ---------------------------------------------------------------- the C ABI without a GPU
def test_f16_argument_checks_answer_without_a_device():
    lib = load_library()
    err = lambda: lib.clv_last_error().decode()                                # noqa: E731
    assert lib.clv_f16_quantize(None, 128, None, None) == -1 and "null" in err()
    assert lib.clv_f16_quantize(16, 100, 16, None) == -1 and "multiple of 128" in err()
    assert lib.clv_f16_quantize(16, 128, 18, None) == -1 and "aligned" in err()
    assert lib.clv_f16_restore(None, 128, None, None) == -1 and "null" in err()
    assert lib.clv_f16_restore(16, 64, 16, None) == -1 and "multiple of 128" in err()
    assert lib.clv_f16_scale_and_add(16, None, 1.0, 128, 16, None) == -1 and "null" in err()
    assert lib.clv_f16_scale_and_add(16, 16, 1.0, 130, 16, None) == -1 and "multiple of 128" in err()
    assert lib.clv_f16_dot(16, 16, 128, 7, 16, None, None) == -1 and "unknown mode" in err()
    assert lib.clv_f16_dot(16, 16, 100, 0, 16, None, None) == -1 and "multiple of 128" in err()
    assert lib.clv_f16_dot(None, 16, 128, 0, 16, None, None) == -1 and "null" in err()
    assert lib.clv_f16_threshold_mode(None, 100, 128, 10, 0, None, None) == -1 and "null" in err()
    assert lib.clv_f16_threshold_mode(16, 200, 128, 10, 0, None, None) == -1 and "n=200" in err()
    assert lib.clv_f16_threshold_mode(16, 100, 128, 10, 5, None, None) == -1 and "unknown mode" in err()
    assert lib.clv_f16_threshold_heap(16, 100, 128, 0, 16, None, None) == -1 and "k=0" in err()
    assert lib.clv_f16_threshold_heap(16, 100, 128, 101, 16, None, None) == -1 and "k=101" in err()
    assert lib.clv_f16_threshold_heap(16, 100, 128, 10, None, None, None) == -1 and "null" in err()
    assert lib.clm_f16_quantize(16, 100, 128, 16, None) == -1 and "multiples of 128" in err()
    assert lib.clm_f16_mvm(16, 64, 100, 16, 32, None) == -1 and "multiple of 128" in err()
    assert lib.clm_f16_mvm(16, 64, 128, 32, 32, None) == -1 and "alias" in err()
    assert lib.clm_f16_mvm(None, 64, 128, 16, 32, None) == -1 and "null" in err()
    assert lib.clm_f16_mvm_f32(16, 64, 128, 24, 32, None) == -1 and "aligned" in err()
    assert lib.clm_f16_mvm_f32(16, 64, 64, 16, 32, None) == -1 and "multiple of 128" in err()
    assert lib.clm_f16_transpose(16, 128, 100, 32, None) == -1 and "multiples of 8" in err()
    assert lib.clm_f16_transpose(16, 128, 128, 16, None) == -1 and "in-place" in err()
    assert lib.clm_f16_transpose(None, 128, 128, 16, None) == -1 and "null" in err()
    # nothing to do: no device work either
    assert lib.clv_f16_quantize(16, 0, 16, None) == 0 and lib.clm_f16_mvm(16, 0, 128, 16, 32, None) == 0
    assert lib.clv_f16_threshold_mode(16, 100, 128, 100, 0, None, None) == 0             # k >= n: everything survives
    assert lib.clv_f16_dot_workspace_bytes(1 << 20) == 0 and lib.clv_f16_threshold_workspace_bytes(1 << 20) > 4096 * 4


def _build_c_client(tmp_path):
    lib = build_hip_library()
    exe = tmp_path / "half16_from_c"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{repo_root() / 'include'}",
                    str(repo_root() / "tests" / "c" / "half16_from_c.c"), "-o", str(exe), f"-L{lib.parent}", "-lclover_hip",
                    f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_c99_client_of_the_f16_declarations_compiles_and_links(tmp_path):
    p = subprocess.run([str(_build_c_client(tmp_path))], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and ("dot=128.0" in p.stdout or "no_device" in p.stdout), (p.returncode, p.stdout, p.stderr)


@pytest.mark.gpu
def test_c99_client_gets_its_answer_on_the_gpu(tmp_path):
    p = subprocess.run([str(_build_c_client(tmp_path))], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "dot=128.0" in p.stdout, (p.returncode, p.stdout, p.stderr)
