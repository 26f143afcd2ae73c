"""clm8_mvm_scale_and_add (the 8-bit mvm with the CloverVector8::scaleAndAdd behind it in its epilogue) and clm8_iht (the whole 8-bit
Q_IHT / Q_GD loop in one call), through the C ABI, the containers and CloverIHT.h.

Every comparison is bit for bit.  The reference side is never the new code: it is the CPU restatement m8.mvm (tests/matrix8_restate.c)
followed by oracle.v8_scale_and_add and the threshold checkers of tests/test_mixed8.py, and the existing device calls clm8_mvm,
clv8_scale_and_add and clv8_threshold_mode issued one after another.

The guard-band cases of the two calls are registered with tests/test_guard_bands.py's own case table when this module is imported (its
coverage test counts every prototype of clover_amd.lib_binding.SIGNATURES) and run here."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import test_guard_bands as gb
from clover_amd.build import repo_root
from clover_amd.lib_binding import THRESHOLD_FAST, THRESHOLD_REFERENCE
from half16_helpers import rh  # noqa: F401
from matrix8_helpers import binade_scales, full_range_bytes, m8, make_matrix, same, same_keys, v8_inputs  # noqa: F401
from test_guard_bands import refs  # noqa: F401
from test_mixed8 import _threshold8_lowest_index

ROOT = repo_root()
INC = ROOT / "include"


# ---------------------------------------------------------------- CPU: the ABI from C, the headers' routing, the container methods
def _build_c_client(tmp_path):
    from clover_amd.build import build_hip_library
    lib = build_hip_library()
    exe = tmp_path / "matrix8_fused_from_c"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", f"-I{INC}", str(ROOT / "tests" / "c" / "matrix8_fused_from_c.c"),
                    "-o", str(exe), f"-L{lib.parent}", "-lclover_hip", f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lm"],
                   check=True)
    return exe


def test_fused_calls_compile_and_link_from_c99(tmp_path):
    """the two declarations are plain C: a C99 client compiles with -pedantic, links, and runs (without a device it only reports that)"""
    p = subprocess.run([str(_build_c_client(tmp_path))], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and ("ok=1" in p.stdout or "no_device" in p.stdout), (p.returncode, p.stdout, p.stderr)


ROUTING_CLIENT = r'''
#include <CloverIHT.h>
void loops(CloverMatrix8 &Phi, CloverMatrix8 &PhiT, CloverVector8 &x, CloverVector8 &y, CloverVector8 &t1, CloverVector8 &t2, CloverVector8 &t3)
{
#ifdef DEDUCED
    Q_IHT(Phi, PhiT, x, y, t1, t2, t3, 3, 10, 0.5f);
    Q_GD(Phi, PhiT, x, y, t1, t2, t3, 3, 0.5f);
#else
    Q_IHT<CloverMatrix8, CloverVector8>(Phi, PhiT, x, y, t1, t2, t3, 3, 10, 0.5f);
    Q_GD<CloverMatrix8, CloverVector8>(Phi, PhiT, x, y, t1, t2, t3, 3, 0.5f);
#endif
}
'''


def _undefined_symbols(tmp_path, name, source, flags):
    src, obj = tmp_path / f"{name}.cpp", tmp_path / f"{name}.o"
    src.write_text(source)
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", *flags, f"-I{INC}", "-c", str(src), "-o", str(obj)], check=True)
    out = subprocess.run(["nm", "-u", str(obj)], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


@pytest.mark.parametrize("spelling", ["explicit", "deduced"])
def test_header_routes_the_8_bit_loops(tmp_path, spelling):
    """Q_IHT / Q_GD for (CloverMatrix8, CloverVector8), template arguments spelled out or deduced: with rounding disabled the object calls
    clm8_iht; with stochastic rounding it calls the separate steps (each object draws from its own generator) and not clm8_iht"""
    d = ["-DDEDUCED"] if spelling == "deduced" else []
    det = _undefined_symbols(tmp_path, "det", ROUTING_CLIENT, ["-DCLOVER_STOCHASTIC_ROUNDING_DISABLED=1", *d])
    assert "clm8_iht" in det, sorted(s for s in det if s.startswith("cl"))
    sto = _undefined_symbols(tmp_path, "sto", ROUTING_CLIENT, d)
    assert ("clm8_mvm_scale_and_add" in sto or "clm8_mvm" in sto) and "clm8_iht" not in sto, sorted(s for s in sto if s.startswith("cl"))


@pytest.mark.parametrize("explicit", [False, True])
@pytest.mark.parametrize("deterministic", [False, True])
def test_container_methods_compile(tmp_path, explicit, deterministic):
    """CloverMatrix8::mvm_scaleAndAdd (both overloads) and iht_loop, in the tracked and the explicit-sync builds, either rounding"""
    client = tmp_path / "m8_fused_client.cpp"
    client.write_text(r'''
#include <CloverMatrix8.h>
int main() {
    const uint64_t m = 128, n = 256;
    CloverMatrix8 A(m, n), At(n, m);
    CloverVector8 x(n), y(m), u(m), t1(m), t2(m), t3(n);
    A.mvm_scaleAndAdd(x, u, -1.0f, t1, t2);
    A.mvm_scaleAndAdd(x, u, 0.5f, t1);
    A.iht_loop(At, x, y, t1, t2, t3, 3, 10, 0.5f, true);
    A.iht_loop(At, x, y, t1, t2, t3, 3, 0, 0.5f, false);
    return 0;
}
''')
    flags = (["-DCLOVER_HIP_EXPLICIT_SYNC"] if explicit else []) + (["-DCLOVER_STOCHASTIC_ROUNDING_DISABLED=1"] if deterministic else [])
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", *flags, f"-I{INC}", "-c", str(client), "-o", str(tmp_path / "client.o")], check=True)


# ---------------------------------------------------------------- GPU 1: the fused call = the two calls = the CPU restatement
SHAPES = [(64, 128),        # one row group; tail-only loop: 2 blocks < M8_MVM_U
          (128, 128),
          (192, 512),       # exactly one full step of the loop
          (128, 640),       # full step + tail
          (320, 1152),      # two full steps + tail; odd number of row groups
          (1024, 2048)]
KINDS = ["normal", "zero_tiles", "extremes"]


def _operands(oracle, m8, kind, rows, cols, variant):  # noqa: F811
    qA, sA = m8.quantize(make_matrix(kind, rows, cols, 5 * rows + cols))
    sA = np.where(sA > 1e30, np.float32(1e30), sA).astype(np.float32)            # extremes: keep the products finite
    if variant == "quantized":
        _, qx, sx = v8_inputs(oracle, cols, rows + 1)
        _, qu, su = v8_inputs(oracle, rows, cols + 2)
    else:
        rng = np.random.default_rng(rows * 7 + cols)
        qx, sx = full_range_bytes(rng, cols), binade_scales(rng, cols // 64)
        qu, su = full_range_bytes(rng, rows), binade_scales(rng, rows // 64)
    if kind == "zero_tiles":                                                      # row group 0 of A and block 0 of u: both maxima are 0 -> 1.0
        qA = qA.copy()
        qA[:64 * cols] = 0
        qu = qu.copy()
        qu[:64] = 0
    return qA, sA, qx, sx, qu, su


def _device_scale_and_add(hip, qu, su, qv, sv, a, rng=None):
    """clv8_scale_and_add takes whole CloverVector8 lengths (multiples of 128) and the mvm family a row shard (a multiple of 64): a shard's
    vectors go in with one zero block behind them.  Blocks are independent and block b takes draws 2 b, 2 b + 1 of the call's stream, so
    the first len(qu) elements are those of the unpadded operation; a padded stochastic call leaves the generator two draws further."""
    n = qu.size
    if n % 128:
        qu, qv = np.concatenate([qu, np.zeros(64, np.int8)]), np.concatenate([qv, np.zeros(64, np.int8)])
        su, sv = np.concatenate([su, np.ones(1, np.float32)]), np.concatenate([sv, np.ones(1, np.float32)])
    r, sr = hip.v8_scale_and_add(qu, su, qv, sv, a, rng=rng)
    return r[:n].copy(), sr[:n // 64].copy()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_gpu_fused_equals_the_two_calls_and_the_restatement(hip, m8, oracle, shape, kind):  # noqa: F811
    rows, cols = shape
    for variant in (("quantized", "full_range") if kind == "normal" else ("quantized",)):
        qA, sA, qx, sx, qu, su = _operands(oracle, m8, kind, rows, cols, variant)
        to, sto = m8.mvm(qA, sA, rows, cols, qx, sx)
        td, std = hip.m8_mvm(qA, sA, rows, cols, qx, sx)
        assert same(td, to) and same(std, sto)
        for a in (-1.0, 0.5, 0.0):
            ro, sro = oracle.v8_scale_and_add(qu, su, to, sto, a)
            rd, srd = _device_scale_and_add(hip, qu, su, td, std, a)
            assert same(rd, ro) and same(srd, sro)
            if kind == "zero_tiles":
                assert sto[0] == 1.0 and sro[0] == 1.0 and not ro[:64].any()
            for want_t in (True, False):
                for in_place in (False, True):
                    t, st, r, sr = hip.m8_mvm_scale_and_add(qA, sA, rows, cols, qx, sx, qu, su, a, in_place=in_place, want_t=want_t)
                    what = (variant, a, want_t, in_place)
                    assert same(r, ro) and same(sr, sro), what
                    if want_t:
                        assert same(t, to) and same(st, sto), what


# ---------------------------------------------------------------- GPU 2: stochastic rounding
@pytest.mark.gpu
@pytest.mark.parametrize("segments", [1, 4])
@pytest.mark.parametrize("shape", [(128, 640), (320, 1152)])
def test_gpu_fused_stochastic_same_stream(hip, m8, oracle, shape, segments):  # noqa: F811
    """t, r and the generator afterwards are those of m8.mvm(rng) then oracle.v8_scale_and_add(rng) on ONE generator, and those of the two
    device calls on a generator seeded alike; `segments` shapes the separate clv8_scale_and_add's walk of the stream.  Three launches
    per generator: each continues where its predecessor left the state.  rows = 320 is a row shard: the separate scaleAndAdd runs on
    the vectors padded to 384 (_device_scale_and_add), which costs its generator two more draws, so that generator is put back on the
    oracle's keys after each round and only the fused call's state is compared there."""
    rows, cols = shape
    qA, sA, qx, sx, qu, su = _operands(oracle, m8, "normal", rows, cols, "quantized")
    fused, apart, o = hip.new_rng(11, 13), hip.new_rng(11, 13), oracle.rng(11, 13)
    assert hip.lib.clv_rng_set_segments(segments) == 0
    try:
        for want_t, in_place, a in ((True, False, -1.0), (False, True, 0.5), (True, True, 0.25)):
            to, sto = m8.mvm(qA, sA, rows, cols, qx, sx, o)
            ro, sro = oracle.v8_scale_and_add(qu, su, to, sto, a, o)
            td, std = hip.m8_mvm(qA, sA, rows, cols, qx, sx, rng=apart)
            rd, srd = _device_scale_and_add(hip, qu, su, td, std, a, rng=apart)
            assert same(td, to) and same(std, sto) and same(rd, ro) and same(srd, sro)
            if rows % 128:
                k1, k2 = (np.ascontiguousarray(k, np.uint64) for k in oracle.rng_keys(o))
                hip.check(hip.lib.clv_rng_set(apart.ptr, k1.ctypes.data_as(C.POINTER(C.c_uint64)), k2.ctypes.data_as(C.POINTER(C.c_uint64)), None))
                hip.sync()
            t, st, r, sr = hip.m8_mvm_scale_and_add(qA, sA, rows, cols, qx, sx, qu, su, a, rng=fused, in_place=in_place, want_t=want_t)
            assert same(r, ro) and same(sr, sro), (want_t, in_place)
            if want_t:
                assert same(t, to) and same(st, sto)
            assert same_keys(hip, fused, oracle, o) and same_keys(hip, apart, oracle, o)
    finally:
        hip.lib.clv_rng_set_segments(0)


# ---------------------------------------------------------------- GPU 3: clm8_iht
IHT_SHAPES = [(128, 256, 256), (384, 128, 128), (512, 1024, 1000)]          # (m, n, x_len); (384, 128): the GD shape, m > n
MU = 0.5


def _iht_modes(n, x_len):
    """(name, threshold argument, K, stochastic)"""
    return [("gd", 0, 0, False), ("fast K=1", 1, 1, False), ("fast K=n/4", 1, n // 4, False), ("fast K=x_len", 1, x_len, False),
            ("reference K=n/4", 2, n // 4, False), ("fast K=n/4 stochastic", 1, n // 4, True)]


_PROBLEMS = {}


def _iht_problem(m8, oracle, m, n):  # noqa: F811
    """Phi, PhiT and y of a recovery problem, quantized on the CPU once per shape and shared by the tests below"""
    if (m, n) not in _PROBLEMS:
        rng = np.random.default_rng(m * 3 + n)
        phi = (rng.normal(size=(m, n)) / np.sqrt(m)).astype(np.float32)
        x_true = np.zeros(n, np.float32)
        x_true[rng.choice(n, n // 8, replace=False)] = rng.normal(size=n // 8).astype(np.float32)
        Phi = m8.quantize(phi)
        _PROBLEMS[m, n] = (Phi, m8.transpose(*Phi, m, n), oracle.v8_quantize((phi @ x_true).astype(np.float32)))
    return _PROBLEMS[m, n]


def _threshold_cpu(oracle, q, s, x_len, K, thr):
    return oracle.v8_threshold(q, s, x_len, K) if thr == 2 else _threshold8_lowest_index(q, s, x_len, K)


def _cpu_loop(m8, oracle, Phi, PhiT, y, m, n, x_len, iters, K, thr, o):  # noqa: F811
    x = (np.zeros(n, np.int8), np.ones(n // 64, np.float32))
    t1 = t2 = t3 = None
    for _ in range(iters):
        t1 = m8.mvm(*Phi, m, n, *x, o)
        t2 = oracle.v8_scale_and_add(*y, *t1, -1.0, o)
        t3 = m8.mvm(*PhiT, n, m, *t2, o)
        x = oracle.v8_scale_and_add(*x, *t3, MU, o)
        if thr:
            x = (_threshold_cpu(oracle, x[0], x[1], x_len, K, thr), x[1])
    return dict(x=x, t1=t1, t2=t2, t3=t3)


def _device_loop(hip, Phi, PhiT, y, m, n, x_len, iters, K, thr, st):
    """the loop launch by launch with the calls that existed before the fused ones"""
    L = hip.lib
    d = [hip.to_device(v) for v in (*Phi, *PhiT, *y)]
    x = (hip.to_device(np.zeros(n, np.int8)), hip.to_device(np.ones(n // 64, np.float32)))
    lens = dict(t1=m, t2=m, t3=n)
    v = {k: (hip.alloc(ln), hip.alloc(ln // 16)) for k, ln in lens.items()}
    g = st.ptr if st else None
    for _ in range(iters):
        hip.check(L.clm8_mvm(d[0].ptr, d[1].ptr, m, n, x[0].ptr, x[1].ptr, v["t1"][0].ptr, v["t1"][1].ptr, g, None))
        hip.check(L.clv8_scale_and_add(d[4].ptr, d[5].ptr, v["t1"][0].ptr, v["t1"][1].ptr, -1.0, m, v["t2"][0].ptr, v["t2"][1].ptr, g, None))
        hip.check(L.clm8_mvm(d[2].ptr, d[3].ptr, n, m, v["t2"][0].ptr, v["t2"][1].ptr, v["t3"][0].ptr, v["t3"][1].ptr, g, None))
        hip.check(L.clv8_scale_and_add(x[0].ptr, x[1].ptr, v["t3"][0].ptr, v["t3"][1].ptr, MU, n, x[0].ptr, x[1].ptr, g, None))
        if thr:
            hip.check(L.clv8_threshold_mode(x[0].ptr, x[1].ptr, x_len, n, K, THRESHOLD_REFERENCE if thr == 2 else THRESHOLD_FAST, None, None))
    out = dict(x=(x[0].download(np.int8, n), x[1].download(np.float32, n // 64)))
    out.update({k: (v[k][0].download(np.int8, ln), v[k][1].download(np.float32, ln // 64)) for k, ln in lens.items()})
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("mode", range(6))
@pytest.mark.parametrize("shape", IHT_SHAPES)
def test_gpu_iht_call_equals_the_separate_calls_and_the_cpu_loop(hip, m8, oracle, shape, mode):  # noqa: F811
    m, n, x_len = shape
    name, thr, K, stochastic = _iht_modes(n, x_len)[mode]
    Phi, PhiT, y = _iht_problem(m8, oracle, m, n)
    for iters in (0, 1, 3):
        st, st2, o = (hip.new_rng(3, 5), hip.new_rng(3, 5), oracle.rng(3, 5)) if stochastic else (None, None, None)
        got = hip.m8_iht(*Phi, *PhiT, m, n, *y, iters, K, MU, thr, x_len=x_len, rng=st, prefill=0x55)
        cpu = _cpu_loop(m8, oracle, Phi, PhiT, y, m, n, x_len, iters, K, thr, o)
        dev = _device_loop(hip, Phi, PhiT, y, m, n, x_len, iters, K, thr, st2)
        for k in ("x", "t1", "t2", "t3"):
            if iters == 0 and k != "x":                       # untouched: the prefill, values and scales
                assert all(np.all(a.view(np.uint8) == 0x55) for a in got[k]), (name, k)
                continue
            for side, ref in (("cpu", cpu), ("device", dev)):
                assert same(got[k][0], ref[k][0]) and same(got[k][1], ref[k][1]), (name, iters, k, side)
        if iters == 0:
            assert not got["x"][0].any() and np.all(got["x"][1] == 1.0)
        if iters == 3 and thr and K > 1:
            assert 0 < np.count_nonzero(got["x"][0][:x_len]) <= K, name          # the elements from x_len on are outside the threshold
        if stochastic:
            assert same_keys(hip, st, oracle, o) and same_keys(hip, st2, oracle, o), (name, iters)


# ---------------------------------------------------------------- GPU 4: the header loop
def _build_fused_client(tmp_path, explicit):
    from clover_amd.build import build_hip_library
    lib = build_hip_library()
    exe = tmp_path / ("matrix8_fused_explicit" if explicit else "matrix8_fused_tracked")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-DCLOVER_STOCHASTIC_ROUNDING_DISABLED=1",
                    *(["-DCLOVER_HIP_EXPLICIT_SYNC"] if explicit else []), f"-I{INC}", str(ROOT / "tests" / "cpp" / "matrix8_fused.cpp"), "-o", str(exe),
                    f"-L{lib.parent}", "-lclover_hip", f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


@pytest.mark.gpu
@pytest.mark.parametrize("explicit", [False, True])
def test_gpu_header_specialised_loops_equal_the_method_calls(tmp_path, explicit):
    """m = 256, n = 512: the specialised Q_IHT / Q_GD (CloverMatrix8::iht_loop -> clm8_iht) and mvm_scaleAndAdd give the digests of the
    method calls written out by hand; a host pointer taken before the loop shows its result"""
    out = subprocess.run([str(_build_fused_client(tmp_path, explicit)), "256", "512", "4", "128", "0.5"], check=True, capture_output=True, text=True,
                         timeout=300).stdout
    lines = {ln.split()[0]: dict(f.split("=") for f in ln.split()[1:]) for ln in out.splitlines() if "=" in ln and " " in ln}
    assert lines["pair"]["fused"] == lines["pair"]["separate"], out
    assert lines["iht"]["spec"] == lines["iht"]["hand"] and 0 < int(lines["iht"]["nonzero"]) <= 128, out
    assert lines["gd"]["spec"] == lines["gd"]["hand"] and lines["gd"]["spec"] != lines["iht"]["spec"], out
    assert "kept_pointer=1" in out and "done" in out, out


# ---------------------------------------------------------------- GPU 5: guard bands and arguments
def _fused_case(rows, cols, st=False, with_t=True, in_place=False):
    def build(R):
        qA, sA = gb.m8data(rows * cols + 21, rows, cols)
        qx, sx = gb.v8(cols + 22, cols)
        qu, su = gb.v8(rows + 23, rows)
        o = R.oracle.rng(*gb.KEYS) if st else None
        t, st_ = R.m8.mvm(qA, sA, rows, cols, qx, sx, o)
        r, sr = R.oracle.v8_scale_and_add(qu, su, t, st_, -0.5, o)
        regs = [("A", "input", qA), ("sA", "input", sA), ("x", "input", qx), ("sx", "input", sx)] + ([("rng", "state", None)] if st else [])
        want = {}
        if with_t:
            regs += [("t", "output", rows), ("st", "output", rows // 16)]
            want.update(t=t, st=st_)
        if in_place:
            regs += [("u", "inout", qu), ("su", "inout", su)]
            want.update(u=r, su=sr)
        else:
            regs += [("u", "input", qu), ("su", "input", su), ("r", "output", rows), ("sr", "output", rows // 16)]
            want.update(r=r, sr=sr)
        return gb.Case(regs, lambda L, p: L.clm8_mvm_scale_and_add(p["A"], p["sA"], rows, cols, p["x"], p["sx"], p["u"], p["su"], -0.5, p.get("t"),
                                                                   p.get("st"), p["u" if in_place else "r"], p["su" if in_place else "sr"],
                                                                   p.get("rng"), None), want, orng=o)
    return build


def _iht8_case(m, n, thr, iters=2, st=False):
    def build(R):
        x_len, K, mu = n - 5, n // 4, np.float32(0.25)
        qP, sP = gb.m8data(m * n + 31, m, n)
        qT, sT = R.m8.transpose(qP, sP, m, n)
        y = gb.v8(m + 32, m)
        o = R.oracle.rng(*gb.KEYS) if st else None
        x = (np.zeros(n, np.int8), np.ones(n // 64, np.float32))
        t1 = t2 = t3 = None
        for _ in range(iters):
            t1 = R.m8.mvm(qP, sP, m, n, *x, o)
            t2 = R.oracle.v8_scale_and_add(*y, *t1, -1.0, o)
            t3 = R.m8.mvm(qT, sT, n, m, *t2, o)
            x = R.oracle.v8_scale_and_add(*x, *t3, float(mu), o)
            if thr:
                x = (gb.threshold_reference(R, 8, x[0], x[1], x_len, K, THRESHOLD_REFERENCE if thr == 2 else THRESHOLD_FAST)[0], x[1])
        want = dict(x=x[0], sx=x[1], t1=t1[0], st1=t1[1], t2=t2[0], st2=t2[1], t3=t3[0], st3=t3[1])
        regs = [("Phi", "input", qP), ("sPhi", "input", sP), ("PhiT", "input", qT), ("sPhiT", "input", sT), ("y", "input", y[0]), ("sy", "input", y[1])]
        regs += [(k, "output", v.nbytes) for k, v in want.items()] + ([("rng", "state", None)] if st else [])
        return gb.Case(regs, lambda L, p: L.clm8_iht(p["Phi"], p["sPhi"], p["PhiT"], p["sPhiT"], m, n, p["x"], p["sx"], x_len, p["y"], p["sy"], p["t1"],
                                                     p["st1"], p["t2"], p["st2"], p["t3"], p["st3"], iters, K, float(mu), thr, p.get("rng"), None),
                       want, orng=o)
    return build


FUSED_CASES = []
for _r, _c in [(64, 128), (128, 256)]:
    for _st in (False, True):
        for _t in (True, False):
            FUSED_CASES.append((f"clm8_mvm_scale_and_add {_r}x{_c} stochastic={_st} t={_t}", _fused_case(_r, _c, st=_st, with_t=_t)))
    FUSED_CASES.append((f"clm8_mvm_scale_and_add {_r}x{_c} in place", _fused_case(_r, _c, in_place=True)))
    FUSED_CASES.append((f"clm8_mvm_scale_and_add {_r}x{_c} in place t=False", _fused_case(_r, _c, with_t=False, in_place=True)))
for _m, _n in [(128, 256), (256, 128)]:
    for _thr in (0, 1, 2):
        FUSED_CASES.append((f"clm8_iht {_m}x{_n} threshold={_thr}", _iht8_case(_m, _n, _thr)))
FUSED_CASES.append(("clm8_iht 128x256 threshold=1 stochastic", _iht8_case(128, 256, 1, st=True)))
for _name, _build in FUSED_CASES:
    if _name not in gb.CASES:                 # the coverage test of test_guard_bands.py reads its table when it runs, after every module is imported
        gb.case(_name)(_build)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, _ in FUSED_CASES])
def test_gpu_fused_calls_write_their_outputs_and_nothing_else(hip, refs, name):  # noqa: F811
    gb.run_case(hip, dict(FUSED_CASES)[name](refs))


@pytest.mark.gpu
def test_gpu_fused_bad_arguments(hip):
    """every bad call returns CLV_ERR_INVALID with a message and launches nothing: the outputs keep their prefill"""
    L = hip.lib
    bufs = {k: hip.alloc(1 << 16) for k in ("A", "x", "u", "t", "r", "sx", "su", "st", "sr", "y")}
    for b in bufs.values():
        hip.check(L.clv_memset(b.ptr, 0x5A, b.nbytes, None))
    p = {k: b.ptr for k, b in bufs.items()}

    def fused(rows=128, cols=128, x=p["x"], sx=p["sx"], t=p["t"], st=p["st"], r=p["r"], sr=p["sr"]):
        return L.clm8_mvm_scale_and_add(p["A"], p["A"], rows, cols, x, sx, p["u"], p["su"], 0.5, t, st, r, sr, None, None)

    for what, rc in (("r == x", fused(r=p["x"])), ("t == x", fused(t=p["x"])), ("t without st", fused(st=None)), ("st without t", fused(t=None)),
                     ("r == t", fused(r=p["t"])), ("rows = 96", fused(rows=96)), ("cols = 64", fused(cols=64)), ("r NULL", fused(r=None))):
        assert rc == -1 and L.clv_last_error(), what
    assert fused(rows=0) == 0
    iht = lambda m, n, x_len: L.clm8_iht(p["A"], p["A"], p["A"], p["A"], m, n, p["x"], p["sx"], x_len, p["y"], p["su"], p["t"], p["st"], p["r"],  # noqa: E731
                                         p["sr"], p["u"], p["su"], 2, 8, 0.5, 1, None, None)
    assert iht(128, 128, 129) == -1 and b"x_len" in L.clv_last_error()
    assert iht(128, 192, 128) == -1 and iht(64, 128, 128) == -1
    hip.sync()
    for k in ("x", "u", "t", "r", "sx", "su", "st", "sr"):
        assert np.all(bufs[k].download(np.uint8) == 0x5A), k


# ---------------------------------------------------------------- GPU 6: capture
def _capture_and_replay(hip, enqueue, outputs, clear):
    """one ordinary warm call, capture on a non-default stream, two replays: the outputs after each replay equal the warm call's bits"""
    rt = C.CDLL("libamdhip64.so")
    stream, graph, gexec = C.c_void_p(), C.c_void_p(), C.c_void_p()

    def ok(rc):
        assert rc == 0, f"HIP runtime call failed: {rc}"
    ok(rt.hipStreamCreate(C.byref(stream)))
    enqueue(stream)
    ok(rt.hipStreamSynchronize(stream))
    want = [b.download(np.uint8) for b in outputs]
    ok(rt.hipStreamBeginCapture(stream, 0))
    enqueue(stream)
    ok(rt.hipStreamEndCapture(stream, C.byref(graph)))
    ok(rt.hipGraphInstantiate(C.byref(gexec), graph, None, None, 0))
    for rep in range(2):
        clear()
        ok(rt.hipGraphLaunch(gexec, stream))
        ok(rt.hipStreamSynchronize(stream))
        for i, b in enumerate(outputs):
            assert same(b.download(np.uint8), want[i]), (rep, i)
    ok(rt.hipGraphExecDestroy(gexec))
    ok(rt.hipGraphDestroy(graph))
    ok(rt.hipStreamDestroy(stream))
    return want


@pytest.mark.gpu
def test_gpu_captured_fused_call_replays(hip, m8, oracle):  # noqa: F811
    rows, cols = 192, 640
    qA, sA, qx, sx, qu, su = _operands(oracle, m8, "normal", rows, cols, "quantized")
    d = [hip.to_device(v) for v in (qA, sA, qx, sx, qu, su)]
    out = [hip.alloc(rows), hip.alloc(rows // 16), hip.alloc(rows), hip.alloc(rows // 16)]           # t, st, r, sr

    def clear():
        for b in out:
            hip.check(hip.lib.clv_memset(b.ptr, 0xEE, b.nbytes, None))
        hip.sync()

    def enqueue(stream):
        hip.check(hip.lib.clm8_mvm_scale_and_add(d[0].ptr, d[1].ptr, rows, cols, d[2].ptr, d[3].ptr, d[4].ptr, d[5].ptr, -1.0, out[0].ptr, out[1].ptr,
                                                 out[2].ptr, out[3].ptr, None, stream))
    got = _capture_and_replay(hip, enqueue, out, clear)
    to, sto = m8.mvm(qA, sA, rows, cols, qx, sx)
    ro, sro = oracle.v8_scale_and_add(qu, su, to, sto, -1.0)
    for g, w in zip(got, (to, sto, ro, sro)):
        assert same(g, np.ascontiguousarray(w).view(np.uint8))


@pytest.mark.gpu
def test_gpu_captured_gd_loop_replays(hip, m8, oracle):  # noqa: F811
    m, n, iters = 128, 256, 2
    Phi, PhiT, y = _iht_problem(m8, oracle, m, n)
    d = [hip.to_device(v) for v in (*Phi, *PhiT, *y)]
    lens = (n, m, m, n)                                                                               # x, t1, t2, t3
    out = [b for ln in lens for b in (hip.alloc(ln), hip.alloc(ln // 16))]

    def clear():
        for b in out:
            hip.check(hip.lib.clv_memset(b.ptr, 0xEE, b.nbytes, None))
        hip.sync()

    def enqueue(stream):
        hip.check(hip.lib.clm8_iht(d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, m, n, out[0].ptr, out[1].ptr, n, d[4].ptr, d[5].ptr, out[2].ptr, out[3].ptr,
                                   out[4].ptr, out[5].ptr, out[6].ptr, out[7].ptr, iters, 0, MU, 0, None, stream))
    got = _capture_and_replay(hip, enqueue, out, clear)
    cpu = _cpu_loop(m8, oracle, Phi, PhiT, y, m, n, n, iters, 0, 0, None)
    for i, k in enumerate(("x", "t1", "t2", "t3")):
        assert same(got[2 * i], cpu[k][0].view(np.uint8)) and same(got[2 * i + 1], cpu[k][1].view(np.uint8)), k
