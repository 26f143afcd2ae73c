"""CloverMatrix4 on fp32 vectors (include/clover_hip_m4_f32.h: clm4_mvm_f32_scale_and_add, clm4_mvm_f32_transposed,
clm4_mvm_f32_transposed_scale_and_add, clm4_iht_f32, clm4_iht_f32_one_matrix) without a GPU:

- the header of their own declares exactly the five calls, the library exports them, the table of their own (SIGNATURES_M4_F32) binds them
  and CloverHip has a method for each; the header is plain C99 and a client links;
- every argument rule answers CLV_ERR_INVALID before any device work, with a message that names the call and the argument, on a machine
  that has no device;
- the column-walk restatement (tests/m4_f32_t_restate.c) equals oracle.m4_transpose + oracle.m4_mvm_f32 bit for bit on every shape the
  GPU tests use (the scale edges included), and on that data a 16-chain walk changes most outputs, so that a comparison of bits on the GPU
  can tell a wrong summation order;
- the Python composition of the loop gives the same bits with Phi' stored and with Phi' t2 taken through the restatement: the GPU tests
  have one reference for both loops;
- the container methods compile in both exactness builds under -DCLOVER_FP32_ON_DEVICE; a program without the switch compiles as before
  and references none of the five names.

The addresses below are never dereferenced: a call that passes validation has rows == 0 or cols == 0, so nothing runs."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import clover_amd.lib_binding as lb
from clover_amd.build import HIP_SOURCES, build_hip_library, repo_root
from clover_amd.lib_binding import load_library
from fp32_helpers import rf, with_project_headers  # noqa: F401  (fixture)
from m4_f32_helpers import (CHUNK, COLS, LOOP_SHAPES, R_SHAPES, T_SHAPES, U, edge_problem, loop_problem, loop_reference, m4rt, problem, same,  # noqa: F401
                            tie_K)
from test_mvm_batch_cpu import addr, failed

INC = repo_root() / "include"
FUSED, MVT, FUSED_T, IHT, IHT1 = ("clm4_mvm_f32_scale_and_add", "clm4_mvm_f32_transposed", "clm4_mvm_f32_transposed_scale_and_add", "clm4_iht_f32",
                                  "clm4_iht_f32_one_matrix")
NAMES = {FUSED: 10, MVT: 7, FUSED_T: 10, IHT: 17, IHT1: 15}
METHODS = ("m4_mvm_f32_scale_and_add", "m4_mvm_f32_transposed", "m4_mvm_f32_transposed_scale_and_add", "m4_iht_f32", "m4_iht_f32_one_matrix")


@pytest.fixture(scope="module")
def lib():
    return load_library()


# ---------------------------------------------------------------- header, library, table
def declared(header):
    text = re.sub(r"/\*.*?\*/", "", (INC / header).read_text(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(cl[mv]\w*)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)}


def test_the_five_calls_are_declared_exported_and_bound():
    assert (INC / "clover_hip_m4_f32.h").exists(), "the header of the fp32-vector calls of CloverMatrix4"
    decl = declared("clover_hip_m4_f32.h")
    table = getattr(lb, "SIGNATURES_M4_F32", None)
    assert table is not None, "lib_binding has no SIGNATURES_M4_F32"
    assert sorted(decl) == sorted(NAMES) == sorted(table)
    raw = C.CDLL(str(build_hip_library()))
    bound = load_library()
    for name, arity in NAMES.items():
        assert len(decl[name].split(",")) == arity, name
        assert hasattr(raw, name), f"{name} is not exported"
        assert len(table[name][1]) == arity and table[name][0] is C.c_int, name
        assert getattr(bound, name).argtypes is not None, f"{name} is not bound by load_library"
    for other in (getattr(lb, n) for n in dir(lb) if n.startswith("SIGNATURES") and n != "SIGNATURES_M4_F32"):
        assert not set(table) & set(other)
    for method in METHODS:
        assert callable(getattr(lb.CloverHip, method, None)), method
    for header in INC.glob("clover_hip*.h"):
        if header.name != "clover_hip_m4_f32.h":
            for name in NAMES:
                assert not re.search(r"\b" + name + r"\b", header.read_text()), f"{name} occurs in {header.name}"


def test_the_signatures_follow_their_neighbours():
    """the fused calls take what clm4_mvm_f32 takes plus (u, a, t, r2) as clm_f32_mvm_scale_and_add; the loops what clm_f32_iht takes with a
    scale grid behind each matrix; the one-matrix loop drops the PhiT pair"""
    main, fp32, ours = declared("clover_hip.h"), declared("clover_hip_fp32.h"), declared("clover_hip_m4_f32.h")

    def types(params):
        return [re.sub(r"\s+", " ", re.sub(r"\w+$", "", p.strip())).strip() for p in params.split(",")]
    plain, fused32, iht32 = types(main["clm4_mvm_f32"]), types(fp32["clm_f32_mvm_scale_and_add"]), types(fp32["clm_f32_iht"])
    assert types(ours[MVT]) == plain
    assert types(ours[FUSED]) == types(ours[FUSED_T]) == plain[:5] + fused32[4:]
    assert types(ours[IHT]) == [plain[0], plain[1]] * 2 + iht32[2:]
    assert types(ours[IHT1]) == [plain[0], plain[1]] + iht32[2:]
    assert lb.SIGNATURES_M4_F32[MVT] == lb.SIGNATURES["clm4_mvm_f32"]


def test_the_kernel_is_a_source_of_the_library_and_the_header_a_dependency():
    assert "mvm_f32_t.hip" in HIP_SOURCES
    src = repo_root() / "clover_amd" / "csrc"
    own = (src / "mvm_f32_t.hip").read_text()
    text = with_project_headers(src, "mvm_f32_t.hip")            # the walk and the host driver are headers both widths include
    for header in ("mvm_f32_t_device.h", "mvm_f32_host.h", "mvm_f32_device.h"):
        assert (src / header).read_text() in text, header
    for shared in ("M4F32Fuse", "m4f32_store", "m4f32_streaming", "unpack8_16th", "times16_is_finite", '#include "mvm_f32_device.h"'):
        assert shared in text, shared
    for width in ("m4f32_streaming", "unpack8_16th", "times16_is_finite"):      # what the 4-bit width puts into the shared code: its traits
        assert width in own, width
    assert "M4F32Fuse" in (src / "mvm_f32.hip").read_text(), "the fused instantiation sits next to k_m4_mvm_f32"
    assert not re.search(r"\bgetenv\b|clv_env", text), "no environment hooks"
    assert "clover_hip_m4_f32.h" in (repo_root() / "clover_amd" / "build.py").read_text(), "the header is a dependency of the library"
    assert COLS in (64, 128, 256) and CHUNK % (64 * U) == 0


C99_CLIENT = r'''
#include <stdio.h>
#include "clover_hip_m4_f32.h"
int main(void)
{
    /* rows == 0 or cols == 0: the arguments are checked, nothing runs */
    const int8_t *A = (const int8_t *)0x100000;
    const float *sA = (const float *)0x200000, *x = (const float *)0x300000, *u = (const float *)0x400000;
    float *r = (float *)0x500000, *t = (float *)0x600000, *t2 = (float *)0x700000, *t3 = (float *)0x800000;
    int ok = clm4_mvm_f32_transposed(A, sA, 0, 256, x, r, NULL) == CLV_OK;
    ok = ok && clm4_mvm_f32_transposed_scale_and_add(A, sA, 128, 0, x, u, 0.5f, NULL, r, NULL) == CLV_OK;
    ok = ok && clm4_mvm_f32_scale_and_add(A, sA, 0, 256, x, r, 0.5f, t, r, NULL) == CLV_OK;
    ok = ok && clm4_mvm_f32_transposed(A, sA, 128, 100, x, r, NULL) == CLV_ERR_INVALID;
    ok = ok && clm4_iht_f32(A, sA, A + 0x10000, sA + 0x1000, 128, 256, r, 257, x, t, t2, t3, 3, 8, 0.5f, 1, NULL) == CLV_ERR_INVALID;
    ok = ok && clm4_iht_f32_one_matrix(A, sA, 128, 256, r, 256, x, t, t, t3, 3, 8, 0.5f, 1, NULL) == CLV_ERR_INVALID;
    ok = ok && CLM4_F32_T_CHUNK % 128 == 0;
    printf("ok=%d\n", ok);
    return !ok;
}
'''


def test_the_header_is_plain_c99_and_a_client_links(tmp_path):
    lib = build_hip_library()
    src, exe = tmp_path / "m4_f32_from_c.c", tmp_path / "m4_f32_from_c"
    src.write_text(C99_CLIENT)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{INC}", str(src), "-o", str(exe), f"-L{lib.parent}",
                    "-lclover_hip", f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "ok=1" in p.stdout, (p.returncode, p.stdout, p.stderr)


CONTAINER_CLIENT = r'''
#include <CloverIHT.h>
int main() {
    const uint64_t m = 128, n = 256;
    CloverMatrix4 A(m, n), At(n, m);
    CloverVector32 x(n), y(m), t1(m), t2(m), t3(n), r(n);
    A.mvm(x, t1);
#ifdef USE_NEW
    A.mvm_transposed(y, t3);
    A.mvm_transposed_parallel(y, t3);
#endif
#ifdef CLOVER_FP32_ON_DEVICE
    A.mvm_scaleAndAdd(x, y, -1.0f, t1, t2);                        /* out of place */
    A.mvm_scaleAndAdd(x, y, -1.0f, t1);                            /* in place */
    A.mvm_transposed_scaleAndAdd(y, x, 0.5f, t3, r);
    A.mvm_transposed_scaleAndAdd(y, x, 0.5f, t3);
    A.iht_loop(At, x, y, t1, t2, t3, 3, 10, 0.5f, true);
    A.iht_loop_one_matrix(x, y, t1, t2, t3, 3, 10, 0.5f, true);
    Q_IHT(A, At, x, y, t1, t2, t3, 3, 10, 0.5f);
    Q_GD(A, At, x, y, t1, t2, t3, 3, 0.5f);
    Q_IHT_one_matrix(A, x, y, t1, t2, t3, 3, 10, 0.5f);
    Q_GD_one_matrix(A, x, y, t1, t2, t3, 3, 0.5f);
#else
    Q_IHT(A, At, x, y, t1, t2, t3, 3, 10, 0.5f);                   /* the generic template: one device product, host vector steps */
    Q_GD(A, At, x, y, t1, t2, t3, 3, 0.5f);
#endif
    return 0;
}
'''


def _undefined(tmp_path, flags):
    src, obj = tmp_path / "m4_f32_client.cpp", tmp_path / ("m4_f32_client" + "".join(flags).replace("-D", "_") + ".o")
    src.write_text(CONTAINER_CLIENT)
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", *flags, f"-I{INC}", "-c", str(src), "-o", str(obj)], check=True)
    out = subprocess.run(["nm", "-u", str(obj)], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


@pytest.mark.parametrize("fast", [False, True])
def test_the_container_methods_and_the_loops_compile_and_reach_the_new_calls(tmp_path, fast):
    syms = _undefined(tmp_path, ["-DCLOVER_FP32_ON_DEVICE", "-DUSE_NEW"] + (["-DCLOVER_FAST"] if fast else []))
    assert set(NAMES) <= syms, sorted(s for s in syms if s.startswith("cl"))


def test_without_the_switch_a_program_compiles_as_before_and_links_none_of_the_new_names(tmp_path):
    syms = _undefined(tmp_path, [])
    assert not syms & set(NAMES), sorted(syms & set(NAMES))
    assert "clm4_mvm_f32" in syms
    # mvm_transposed for fp32 vectors is unconditional, as mvm: it needs only device_ro / device_wo
    assert _undefined(tmp_path, ["-DUSE_NEW"]) & set(NAMES) == {MVT}


# ---------------------------------------------------------------- the argument checks
# 128 x 256: the nibbles have 16384 bytes, the grid 2 x 4 scales.  Row-major: x 1024 bytes, u / t / r2 512; transposed: x 512, the others 1024
A_, S_, X_, R_, U_, T_ = addr(0), addr(2), addr(4), addr(6), addr(8), addr(10)


def mvt(lib, rows=128, cols=256, A=A_, sA=S_, x=X_, r=R_):
    return lib.clm4_mvm_f32_transposed(A, sA, rows, cols, x, r, None)


def fused(lib, fn, rows=128, cols=256, A=A_, sA=S_, x=X_, u=U_, t=T_, r2=R_):
    return getattr(lib, fn)(A, sA, rows, cols, x, u, 0.5, t, r2, None)


LOOP_PTRS = ("Phi", "sPhi", "PhiT", "sPhiT", "x", "y", "t1", "t2", "t3")


def iht(lib, fn, m=128, n=256, x_len=256, thr=1, **kw):
    p = {k: addr(20 + 2 * i) for i, k in enumerate(LOOP_PTRS)}
    p.update(kw)
    mats = (p["Phi"], p["sPhi"]) + ((p["PhiT"], p["sPhiT"]) if fn == IHT else ())
    return getattr(lib, fn)(*mats, m, n, p["x"], x_len, p["y"], p["t1"], p["t2"], p["t3"], 3, 8, 0.5, thr, None)


def loop_ptrs(fn):
    return [k for k in LOOP_PTRS if fn == IHT or "PhiT" not in k]


def test_an_empty_matrix_returns_ok_with_nothing_done(lib):
    for kw in (dict(rows=0), dict(cols=0), dict(rows=0, cols=0)):
        assert mvt(lib, **kw) == 0, kw
        for fn in (FUSED, FUSED_T):
            assert fused(lib, fn, **kw) == 0 and fused(lib, fn, t=None, **kw) == 0, (fn, kw)


def test_null_pointers_are_named(lib):
    for k, word in (("A", "A is NULL"), ("sA", "sA is NULL"), ("x", "x is NULL"), ("r", "r is NULL")):
        failed(lib, mvt(lib, **{k: None}), MVT, word)
        failed(lib, mvt(lib, rows=0, **{k: None}), MVT, word)                      # checked even where nothing would run
    for fn in (FUSED, FUSED_T):
        for k, word in (("A", "A is NULL"), ("sA", "sA is NULL"), ("x", "x is NULL"), ("u", "u is NULL"), ("r2", "r2 is NULL")):
            failed(lib, fused(lib, fn, **{k: None}), fn, word)
        assert fused(lib, fn, rows=0, t=None) == 0                                  # t alone may be NULL
    for fn in (IHT, IHT1):
        for k in loop_ptrs(fn):
            failed(lib, iht(lib, fn, **{k: None}), fn, f"{k} is NULL")


def test_size_rules(lib):
    failed(lib, mvt(lib, cols=100), MVT, "cols=100", "multiples of 128")
    failed(lib, mvt(lib, rows=64), MVT, "rows=64", "multiples of 128")
    failed(lib, mvt(lib, rows=200, cols=0), MVT, "rows=200")                        # an empty matrix still has a valid shape
    failed(lib, fused(lib, FUSED_T, rows=192), FUSED_T, "rows=192", "multiples of 128")
    failed(lib, fused(lib, FUSED_T, cols=64), FUSED_T, "cols=64", "multiples of 128")
    # row-major: the shapes of clm4_mvm_f32 -- rows a multiple of 64 (a row shard), cols of 128
    assert fused(lib, FUSED, rows=64, cols=0) == 0
    failed(lib, fused(lib, FUSED, rows=96), FUSED, "rows=96", "multiple of 64")
    failed(lib, fused(lib, FUSED, cols=192), FUSED, "cols=192", "of 128")
    for fn in (IHT, IHT1):
        failed(lib, iht(lib, fn, m=64), fn, "m=64", "multiples of 128")
        failed(lib, iht(lib, fn, n=192), fn, "n=192", "multiples of 128")
        failed(lib, iht(lib, fn, x_len=257), fn, "x_len=257", "n=256")
        failed(lib, iht(lib, fn, thr=3), fn, "threshold 3")
        failed(lib, iht(lib, fn, thr=-1), fn, "threshold -1")


def test_alignment_rules(lib):
    failed(lib, mvt(lib, A=A_ + 8), MVT, "A must be 16-byte aligned")
    failed(lib, mvt(lib, x=X_ + 4), MVT, "x must be 16-byte aligned")
    failed(lib, mvt(lib, r=R_ + 2), MVT, "r must be 4-byte aligned")
    failed(lib, mvt(lib, sA=S_ + 1), MVT, "sA", "4-byte aligned")
    assert mvt(lib, rows=0, r=R_ + 4) == 0                                          # results need only their element alignment
    for fn in (FUSED, FUSED_T):
        failed(lib, fused(lib, fn, A=A_ + 4), fn, "A must be 16-byte aligned")
        failed(lib, fused(lib, fn, x=X_ + 8), fn, "x must be 16-byte aligned")
        for k in ("u", "t", "r2"):
            failed(lib, fused(lib, fn, **{k: addr(12) + 2}), fn, "u, t and r2 must be 4-byte aligned")
        assert fused(lib, fn, rows=0, u=U_ + 4, t=T_ + 8, r2=R_ + 12) == 0
    for fn in (IHT, IHT1):
        failed(lib, iht(lib, fn, Phi=addr(20) + 8), fn, "matrices must be 16-byte aligned")
        failed(lib, iht(lib, fn, x=addr(28) + 4), fn, "x must be 16-byte aligned")
        failed(lib, iht(lib, fn, t2=addr(34) + 8), fn, "t2 must be 16-byte aligned")
        failed(lib, iht(lib, fn, t1=addr(32) + 2), fn, "4-byte aligned")
        failed(lib, iht(lib, fn, y=addr(30) + 1), fn, "4-byte aligned")
    failed(lib, iht(lib, IHT, PhiT=addr(24) + 8), IHT, "matrices must be 16-byte aligned")


def test_outputs_may_not_overlap_the_matrix_its_scales_x_or_each_other(lib):
    failed(lib, mvt(lib, r=X_), MVT, "overlaps", "`r`", "`x`")                       # r == x
    failed(lib, mvt(lib, r=X_ + 512 - 16), MVT, "overlaps")                         # x is sized by the ROWS
    failed(lib, mvt(lib, r=X_ - 1024 + 16), MVT, "overlaps")                        # r is sized by the COLUMNS
    assert mvt(lib, rows=0, r=X_) == 0                                              # no rows: x is empty
    failed(lib, mvt(lib, r=A_), MVT, "overlaps", "`A`")                             # an output inside the nibbles
    failed(lib, mvt(lib, r=A_ + 128 * 128 - 4), MVT, "overlaps", "`A`")
    failed(lib, mvt(lib, r=S_ + 28), MVT, "overlaps", "`sA`")                       # the last of the 8 scales
    for fn, xb, ob in ((FUSED, 1024, 512), (FUSED_T, 512, 1024)):
        failed(lib, fused(lib, fn, r2=X_), fn, "overlaps", "`r2`", "`x`")
        failed(lib, fused(lib, fn, r2=X_ + xb - 4), fn, "overlaps")
        failed(lib, fused(lib, fn, t=X_), fn, "overlaps", "`t`", "`x`")
        failed(lib, fused(lib, fn, t=R_), fn, "overlaps", "`t`", "`r2`")            # t == r2
        failed(lib, fused(lib, fn, t=R_ + ob - 4), fn, "overlaps")
        failed(lib, fused(lib, fn, t=U_), fn, "overlaps", "`t`", "`u`")             # t == u
        failed(lib, fused(lib, fn, r2=U_ + 4), fn, "overlaps", "`u`")               # r2 inside u, but not the in-place form
        failed(lib, fused(lib, fn, r2=A_ + 4096), fn, "overlaps", "`A`")
        failed(lib, fused(lib, fn, t=A_ + 4096), fn, "overlaps", "`A`")
        failed(lib, fused(lib, fn, t=S_), fn, "overlaps", "`sA`")
        failed(lib, fused(lib, fn, r2=S_ + 16), fn, "overlaps", "`sA`")
        failed(lib, fused(lib, fn, u=U_, r2=U_, t=U_), fn, "overlaps")              # in place, but t on top of it


def test_the_in_place_form_passes_validation(lib):
    for fn in (FUSED, FUSED_T):
        assert fused(lib, fn, cols=0, u=U_, r2=U_) == 0                             # cols == 0: everything is checked, nothing runs
        # with columns r2 == u passes the overlap check: the same call with t on x is refused for t, not for r2
        failed(lib, fused(lib, fn, u=U_, r2=U_, t=X_), fn, "overlaps", "`t`")


def test_the_loop_buffers_are_distinct(lib):
    p = {k: addr(20 + 2 * i) for i, k in enumerate(LOOP_PTRS)}
    for fn in (IHT, IHT1):
        for a, b in (("t3", "x"), ("t1", "y"), ("t2", "t1"), ("t3", "t2"), ("x", "y"), ("t1", "x")):
            failed(lib, iht(lib, fn, **{a: p[b]}), fn, "overlaps", f"`{a}`", f"`{b}`")
        failed(lib, iht(lib, fn, t2=p["t1"] + 256), fn, "overlaps")                 # t2 inside t1
        failed(lib, iht(lib, fn, t2=p["Phi"]), fn, "overlaps", "`Phi`")
        failed(lib, iht(lib, fn, x=p["Phi"] + 4096), fn, "overlaps", "`Phi`")
        failed(lib, iht(lib, fn, t3=p["sPhi"]), fn, "overlaps", "`sPhi`")
    failed(lib, iht(lib, IHT, t1=p["PhiT"] + 1024), IHT, "overlaps", "`PhiT`")
    failed(lib, iht(lib, IHT, x=p["sPhiT"]), IHT, "overlaps", "`sPhiT`")


# ---------------------------------------------------------------- the restatement and the references of the GPU tests
@pytest.mark.parametrize("rows,cols", T_SHAPES, ids=lambda v: str(v))
def test_the_column_walk_equals_transpose_then_the_row_product(oracle, m4rt, rows, cols):  # noqa: F811
    qA, sA, x = problem(rows, cols)[:3]
    qT, sT = oracle.m4_transpose(qA, sA, rows, cols)
    want = oracle.m4_mvm_f32(qT, sT, cols, rows, x)
    assert same(m4rt.mvm_f32_transposed(qA, sA, rows, cols, x), want)
    wrong = m4rt.mvm_f32_transposed(qA, sA, rows, cols, x, chains=16)
    changed = np.count_nonzero(wrong.view(np.uint32) != want.view(np.uint32))
    print(f"{rows} x {cols}: a 16-chain walk changes {changed} of {cols} outputs")
    assert changed >= cols // 4, "the data does not tell a wrong summation order apart"


def test_the_column_walk_on_the_scale_edges(oracle, m4rt):  # noqa: F811
    rows, cols, qA, sA, x, huge, tiny = edge_problem()
    qT, sT = oracle.m4_transpose(qA, sA, rows, cols)
    want = oracle.m4_mvm_f32(qT, sT, cols, rows, x)
    assert same(m4rt.mvm_f32_transposed(qA, sA, rows, cols, x), want)
    assert np.isfinite(want).all()
    for _, _, s in huge:
        assert float(np.float32(s) / np.float32(7)) * 16 > float(np.finfo(np.float32).max)
    assert {rt < CHUNK // 64 for rt, _, _ in huge} == {rt < CHUNK // 64 for rt, _, _ in tiny} == {True, False}, "tiles in both chunks"
    assert any(0 < np.float32(s) / np.float32(7) < np.float32(2.0 ** -126) for _, _, s in tiny), "a subnormal factor"
    for ct in {ct for _, ct, _ in tiny}:                             # these columns hold the tiny tiles' products and nothing else
        assert np.count_nonzero(want[64 * ct:64 * ct + 64]) > 32, ct


@pytest.mark.parametrize("m,n", LOOP_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("ties", [False, True])
def test_the_composed_loop_is_the_same_with_a_stored_transpose_and_through_the_column_walk(oracle, rf, m4rt, m, n, ties):  # noqa: F811
    qPhi, sPhi, y, mu = loop_problem(oracle, m, n, ties)
    qT, sT = oracle.m4_transpose(qPhi, sPhi, m, n)
    x_len = n - 64
    K = tie_K(oracle, rf, qPhi, sPhi, qT, sT, m, n, y, mu, x_len) if ties else n // 8
    for thr in (0, 1, 2):
        two = loop_reference(oracle, rf, qPhi, sPhi, m, n, y, 3, K, mu, thr, x_len, lambda t2: oracle.m4_mvm_f32(qT, sT, n, m, t2))
        one = loop_reference(oracle, rf, qPhi, sPhi, m, n, y, 3, K, mu, thr, x_len, lambda t2: m4rt.mvm_f32_transposed(qPhi, sPhi, m, n, t2))
        for k in two:
            assert same(one[k], two[k]), (thr, k)
            assert np.isfinite(two[k]).all(), (thr, k)
        if thr:
            assert 0 < np.count_nonzero(two["x"][:x_len]) <= K and np.count_nonzero(two["x"]), thr
    none = loop_reference(oracle, rf, qPhi, sPhi, m, n, y, 0, K, mu, 1, x_len, None)
    assert not none["x"].any() and np.all(none["t3"].view(np.uint8) == 0x55)


def test_the_shapes_cover_the_paths_of_the_kernels():
    assert (CHUNK + 128, 384) in T_SHAPES and CHUNK == 8192, "the two-chunk shape follows the chunk the header exports"
    assert any(c % 256 == 128 for _, c in T_SHAPES), "a last strip that is half outside at 256 columns per workgroup"
    assert any((r // 32) % (2 * U) not in (0,) for r, _ in T_SHAPES), "a ragged last pair of load groups"
    assert any(c > 16384 for _, c in R_SHAPES), "the second x chunk of the row-major kernel"
