"""The transposed half-precision calls (include/clover_hip_f16_t.h: clm_f16_mvm_transposed, clm_f16_mvm_f32_transposed,
clm_f16_mvm_transposed_scale_and_add, clm_f16_iht_one_matrix) without a GPU:

- the column-walk restatement (tests/half16_t_restate.c) equals rh_transpose + rh_mvm / rh_mvm_f32 / rh_scale_and_add of
  tests/half16_restate.c bit for bit on every shape the GPU tests use, and on each of those shapes' data every wrong-order variant of the
  walk differs from the right one -- in at least one f16 result and in at least one fp32 value of the _f32 form -- so that a comparison
  of bits on the GPU can tell a wrong summation order;
- the header of their own declares exactly the four calls, the library exports them, the table of their own (SIGNATURES_F16_T) binds
  them and is disjoint from the other six tables; the header is plain C99; the container methods and the Q_IHT_one_matrix /
  Q_GD_one_matrix overloads compile in both container modes and both exactness builds;
- every argument rule answers CLV_ERR_INVALID before any device work, on a machine that has no device.

The addresses below are never dereferenced: a call that passes validation has rows == 0 or cols == 0, so nothing runs.  A is rows x cols
binary16: x has 2 rows bytes (4 rows in the _f32 form), r, u and t 2 cols (r 4 cols in the _f32 form)."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from clover_amd.build import HIP_SOURCES, build_hip_library, repo_root
from clover_amd.lib_binding import (SIGNATURES, SIGNATURES_BATCH_F16, SIGNATURES_BATCH_T, SIGNATURES_BATCH_T8, SIGNATURES_BATCH_T_V8, SIGNATURES_F16_T,
                                    SIGNATURES_FP32, load_library)
from f16_transposed_data import A_VALUES, IHT_SHAPES, SHAPES, ZERO_COLUMN, case
from f16_transposed_helpers import RIGHT, WRONG, rt, same  # noqa: F401  (fixture)
from test_mvm_batch_cpu import addr, failed

INC = repo_root() / "include"
MVT, MVT32, FUSED, IHT1 = "clm_f16_mvm_transposed", "clm_f16_mvm_f32_transposed", "clm_f16_mvm_transposed_scale_and_add", "clm_f16_iht_one_matrix"
NAMES = {MVT: 6, MVT32: 6, FUSED: 9, IHT1: 14}
OTHERS = (SIGNATURES, SIGNATURES_FP32, SIGNATURES_BATCH_T, SIGNATURES_BATCH_T8, SIGNATURES_BATCH_T_V8, SIGNATURES_BATCH_F16)


@pytest.fixture(scope="module")
def lib():
    return load_library()


# ---------------------------------------------------------------- the restatement and the data
@pytest.mark.parametrize("rows,cols", SHAPES, ids=lambda v: str(v))
def test_the_column_walk_equals_transpose_then_the_row_forms(rt, rows, cols):  # noqa: F811
    S = case(rows, cols)
    At = rt.transpose(S.A, rows, cols)
    assert rt.is_transpose(S.A, rows, cols, At)
    t = rt.mvm_transposed(S.A, rows, cols, S.x)
    assert same(t, rt.mvm(At, cols, rows, S.x))
    assert same(rt.columns(S.A, rows, cols, S.x), rt.rowdots(At, cols, rows, S.x))
    assert same(rt.mvm_f32_transposed(S.A, rows, cols, S.xf), rt.mvm_f32(At, cols, rows, S.xf))
    for a in A_VALUES:
        t2, r = rt.mvm_transposed_scale_and_add(S.A, rows, cols, S.x, S.u, a)
        assert same(t2, t) and same(r, rt.scale_and_add(S.u, t, a)), a
        assert not same(r, S.u)
    assert t[ZERO_COLUMN] == 0 and np.count_nonzero(t) > cols // 2, "the zero column gives +0; the cancellation leaves results"
    assert np.all(np.isfinite(t.view(np.float16)))


@pytest.mark.parametrize("rows,cols", SHAPES, ids=lambda v: str(v))
def test_the_data_tells_every_wrong_order_apart(rt, rows, cols):  # noqa: F811
    """the condition the GPU comparisons rest on: each wrong summation order changes at least one f16 result and at least one fp32 value
    of the _f32 form, on this very data"""
    S = case(rows, cols)
    t, f = rt.mvm_transposed(S.A, rows, cols, S.x), rt.mvm_f32_transposed(S.A, rows, cols, S.xf)
    for name, order in WRONG.items():
        n16 = np.count_nonzero(rt.mvm_transposed(S.A, rows, cols, S.x, order) != t)
        n32 = np.count_nonzero(rt.mvm_f32_transposed(S.A, rows, cols, S.xf, order).view(np.uint32) != f.view(np.uint32))
        print(f"{rows} x {cols}, {name}: {n16} of {cols} f16 results and {n32} of {cols} fp32 values differ")
        assert n16 >= 1, (name, "the f16 results do not show this order")
        assert n32 >= 1, (name, "the fp32 values do not show this order")


def test_the_loop_shapes_are_shapes_of_the_product():
    assert set(IHT_SHAPES) <= set(SHAPES)


# ---------------------------------------------------------------- header, library, table
def declared(header):
    text = re.sub(r"/\*.*?\*/", "", (INC / header).read_text(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(cl[mv]\w*)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)}


def test_the_header_declares_exactly_the_four_calls_and_the_table_binds_them():
    decl = declared("clover_hip_f16_t.h")
    assert sorted(decl) == sorted(NAMES) == sorted(SIGNATURES_F16_T)
    raw = C.CDLL(str(build_hip_library()))
    for name, arity in NAMES.items():
        assert len(decl[name].split(",")) == arity, name
        assert hasattr(raw, name), f"{name} is not exported"
        assert len(SIGNATURES_F16_T[name][1]) == arity and SIGNATURES_F16_T[name][0] is C.c_int, name
        assert getattr(load_library(), name).argtypes is not None, f"{name} is not bound by load_library"
    for other in OTHERS:
        assert not set(SIGNATURES_F16_T) & set(other)
    for header in ("clover_hip.h", "clover_hip_fp32.h", "clover_hip_batch_t.h", "clover_hip_batch_t8.h", "clover_hip_batch_t_v8.h", "clover_hip_batch_f16.h"):
        text = (INC / header).read_text()
        for name in NAMES:
            assert not re.search(r"\b" + name + r"\b", text), f"{name} occurs in {header}"


def test_the_signatures_follow_the_calls_on_a_stored_transpose():
    """each call takes what its counterpart of clover_hip.h takes; the loop drops PhiT"""
    main, ours = declared("clover_hip.h"), declared("clover_hip_f16_t.h")

    def types(params):
        return [re.sub(r"\s+", " ", re.sub(r"\w+$", "", p.strip())).strip() for p in params.split(",")]
    assert types(ours[MVT]) == types(main["clm_f16_mvm"]) and SIGNATURES_F16_T[MVT] == SIGNATURES["clm_f16_mvm"]
    assert types(ours[MVT32]) == types(main["clm_f16_mvm_f32"]) and SIGNATURES_F16_T[MVT32] == SIGNATURES["clm_f16_mvm_f32"]
    assert types(ours[FUSED]) == types(main["clm_f16_mvm_scale_and_add"]) and SIGNATURES_F16_T[FUSED] == SIGNATURES["clm_f16_mvm_scale_and_add"]
    one = types(main["clm_f16_iht"])
    assert types(ours[IHT1]) == one[:1] + one[2:]
    res, args = SIGNATURES["clm_f16_iht"]
    assert SIGNATURES_F16_T[IHT1] == (res, args[:1] + args[2:])


def test_the_kernel_is_a_source_of_the_library_and_the_header_a_dependency():
    assert "half16_t.hip" in HIP_SOURCES
    text = (repo_root() / "clover_amd" / "csrc" / "half16_t.hip").read_text()
    for macro in ("F16T_COLS", "F16T_U"):                  # the constants the GPU tests take their shapes from
        assert re.search(r"#define\s+" + macro + r"\s+\d+\b", text), macro
    assert re.search(r"#define\s+F16T_CHUNK\s+\d+u", text)
    for shared in ("F16Fuse", "f16_fuse_store", "f16_bits", "ld_stream", "F16_STREAMING", '#include "half16_device.h"'):
        assert shared in text, shared
    assert not re.search(r"\basm\b", text), "no inline assembly of its own"
    build = (repo_root() / "clover_amd" / "build.py").read_text()
    assert "clover_hip_f16_t.h" in build, "the header is a dependency of the library"


C99_CLIENT = r'''
#include <stdio.h>
#include "clover_hip_f16_t.h"
int main(void)
{
    /* rows == 0 or cols == 0: the arguments are checked, nothing runs */
    const uint16_t *A = (const uint16_t *)0x10000, *x = (const uint16_t *)0x20000, *u = (const uint16_t *)0x30000;
    uint16_t *r = (uint16_t *)0x40000, *t = (uint16_t *)0x50000;
    int ok = clm_f16_mvm_transposed(A, 0, 256, x, r, NULL) == CLV_OK;
    ok = ok && clm_f16_mvm_f32_transposed(A, 128, 0, (const float *)x, (float *)r, NULL) == CLV_OK;
    ok = ok && clm_f16_mvm_transposed_scale_and_add(A, 0, 256, x, u, 0.5f, NULL, r, NULL) == CLV_OK;
    ok = ok && clm_f16_mvm_transposed_scale_and_add(A, 0, 256, x, r, 0.5f, t, r, NULL) == CLV_OK;
    ok = ok && clm_f16_mvm_transposed(A, 128, 100, x, r, NULL) == CLV_ERR_INVALID;
    ok = ok && clm_f16_iht_one_matrix(A, 128, 256, r, 257, x, t, t, t, 3, 8, 0.5f, 1, NULL) == CLV_ERR_INVALID;
    printf("ok=%d\n", ok);
    return !ok;
}
'''


def test_the_header_is_plain_c99_and_a_client_links(tmp_path):
    lib = build_hip_library()
    src, exe = tmp_path / "f16_t_from_c.c", tmp_path / "f16_t_from_c"
    src.write_text(C99_CLIENT)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{INC}", str(src), "-o", str(exe), f"-L{lib.parent}",
                    "-lclover_hip", f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "ok=1" in p.stdout, (p.returncode, p.stdout, p.stderr)


CONTAINER_CLIENT = r'''
#include <CloverIHT.h>
int main() {
    const uint64_t m = 128, n = 256;
    CloverMatrix16 A(m, n);
    CloverVector16 x(n), y(m), t1(m), t2(m), t3(n), r(n);
    CloverVector32 xf(m), rf(n);
    A.mvm_transposed(y, t3);
    A.mvm_transposed(xf, rf);
    A.mvm_transposed_scaleAndAdd(y, x, 0.5f, t3, r);               /* out of place */
    A.mvm_transposed_scaleAndAdd(y, x, 0.5f, t3);                  /* in place */
    A.iht_loop_one_matrix(x, y, t1, t2, t3, 3, 10, 0.5f, true);
    Q_IHT_one_matrix(A, x, y, t1, t2, t3, 3, 10, 0.5f);
    Q_GD_one_matrix(A, x, y, t1, t2, t3, 3, 0.5f);
    return 0;
}
'''


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("explicit", [False, True])
def test_the_container_methods_and_the_loops_compile_and_reach_the_new_calls(tmp_path, explicit, fast):
    """tracked and -DCLOVER_HIP_EXPLICIT_SYNC, reference and -DCLOVER_FAST: the object references the four new calls, no transposition and
    none of the calls on a stored transpose"""
    src, obj = tmp_path / "f16_t_client.cpp", tmp_path / "f16_t_client.o"
    src.write_text(CONTAINER_CLIENT)
    flags = (["-DCLOVER_HIP_EXPLICIT_SYNC"] if explicit else []) + (["-DCLOVER_FAST"] if fast else [])
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", *flags, f"-I{INC}", "-c", str(src), "-o", str(obj)], check=True)
    out = subprocess.run(["nm", "-u", str(obj)], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NAMES) <= syms, sorted(s for s in syms if s.startswith("cl"))
    assert not syms & {"clm_f16_transpose", "clm_f16_mvm", "clm_f16_mvm_f32", "clm_f16_mvm_scale_and_add", "clm_f16_iht"}, \
        sorted(s for s in syms if s.startswith("cl"))


# ---------------------------------------------------------------- the argument checks
# 128 x 256: the matrix has 65536 bytes, x 256 (512 as fp32), r / u / t 512 (r 1024 as fp32).  addr(i) are 1 MiB apart
A_, X_, R_, U_, T_ = addr(0), addr(2), addr(4), addr(6), addr(8)


def mvt(lib, rows=128, cols=256, A=A_, x=X_, r=R_, f32=False):
    return (lib.clm_f16_mvm_f32_transposed if f32 else lib.clm_f16_mvm_transposed)(A, rows, cols, x, r, None)


def fused(lib, rows=128, cols=256, A=A_, x=X_, u=U_, t=T_, r=R_):
    return lib.clm_f16_mvm_transposed_scale_and_add(A, rows, cols, x, u, 0.5, t, r, None)


def iht(lib, m=128, n=256, x_len=256, thr=1, Phi=A_, **kw):
    p = {k: addr(20 + 2 * i) for i, k in enumerate(("x", "y", "t1", "t2", "t3"))}
    p.update(kw)
    return lib.clm_f16_iht_one_matrix(Phi, m, n, p["x"], x_len, p["y"], p["t1"], p["t2"], p["t3"], 3, 8, 0.5, thr, None)


def test_an_empty_matrix_returns_ok_with_nothing_done(lib):
    for kw in (dict(rows=0), dict(cols=0), dict(rows=0, cols=0)):
        assert mvt(lib, **kw) == 0 and mvt(lib, f32=True, **kw) == 0 and fused(lib, **kw) == 0 and fused(lib, t=None, **kw) == 0, kw


def test_null_pointers(lib):
    for f32, name in ((False, MVT), (True, MVT32)):
        failed(lib, mvt(lib, A=None, f32=f32), name, "null pointer")
        failed(lib, mvt(lib, x=None, f32=f32), name, "null pointer")
        failed(lib, mvt(lib, r=None, f32=f32), name, "null pointer")
        failed(lib, mvt(lib, rows=0, r=None, f32=f32), name, "null pointer")      # checked even where nothing would run
    for kw in (dict(A=None), dict(x=None), dict(u=None), dict(r=None)):
        failed(lib, fused(lib, **kw), FUSED, "null pointer")
    assert fused(lib, rows=0, t=None) == 0                                          # t alone may be NULL
    for k in ("Phi", "x", "y", "t1", "t2", "t3"):
        failed(lib, iht(lib, **{k: None}), IHT1, "null pointer")


def test_size_and_alignment_rules(lib):
    for f32, name in ((False, MVT), (True, MVT32)):
        failed(lib, mvt(lib, cols=100, f32=f32), name, "cols=100", "multiples of 128")
        failed(lib, mvt(lib, rows=64, f32=f32), name, "rows=64", "multiples of 128")
        failed(lib, mvt(lib, rows=200, cols=0, f32=f32), name, "rows=200")          # an empty matrix still has a valid shape
        failed(lib, mvt(lib, A=A_ + 8, f32=f32), name, "16-byte aligned")
        failed(lib, mvt(lib, x=X_ + 4, f32=f32), name, "16-byte aligned")
    failed(lib, mvt(lib, r=R_ + 1), MVT, "2-byte aligned")
    failed(lib, mvt(lib, r=R_ + 2, f32=True), MVT32, "4-byte aligned")
    assert mvt(lib, rows=0, r=R_ + 2) == 0 and mvt(lib, rows=0, r=R_ + 4, f32=True) == 0      # results need only their element alignment
    failed(lib, fused(lib, cols=100), FUSED, "cols=100")
    failed(lib, fused(lib, rows=192), FUSED, "rows=192")
    failed(lib, fused(lib, A=A_ + 2), FUSED, "16-byte aligned")
    failed(lib, fused(lib, x=X_ + 8), FUSED, "16-byte aligned")
    for k in ("u", "t", "r"):
        failed(lib, fused(lib, **{k: addr(12) + 1}), FUSED, "2-byte aligned")
    assert fused(lib, rows=0, u=U_ + 2, t=T_ + 6, r=R_ + 10) == 0
    failed(lib, iht(lib, m=64), IHT1, "m=64")
    failed(lib, iht(lib, n=192), IHT1, "n=192")
    failed(lib, iht(lib, x_len=257), IHT1, "x_len=257")
    failed(lib, iht(lib, thr=3), IHT1, "threshold 3")
    failed(lib, iht(lib, thr=-1), IHT1, "threshold -1")
    failed(lib, iht(lib, Phi=A_ + 8), IHT1, "16-byte aligned")
    failed(lib, iht(lib, x=addr(20) + 2), IHT1, "16-byte aligned")
    failed(lib, iht(lib, t2=addr(26) + 8), IHT1, "16-byte aligned")
    failed(lib, iht(lib, t1=addr(24) + 1), IHT1, "2-byte aligned")
    failed(lib, iht(lib, y=addr(22) + 1), IHT1, "2-byte aligned")


def test_outputs_may_not_overlap_the_matrix_x_or_each_other(lib):
    for f32, name, xb, rb in ((False, MVT, 256, 512), (True, MVT32, 512, 1024)):
        failed(lib, mvt(lib, r=X_, f32=f32), name, "overlaps")                      # r == x
        failed(lib, mvt(lib, r=X_ + xb - 16, f32=f32), name, "overlaps")            # x is sized by the ROWS
        failed(lib, mvt(lib, r=X_ - rb + 16, f32=f32), name, "overlaps")            # r is sized by the COLUMNS
        failed(lib, mvt(lib, r=A_, f32=f32), name, "overlaps")                      # an output inside the matrix
        failed(lib, mvt(lib, r=A_ + 2 * 128 * 256 - 4, f32=f32), name, "overlaps")
        assert mvt(lib, rows=0, r=X_, f32=f32) == 0                                 # no rows: x is empty
    failed(lib, fused(lib, r=X_), FUSED, "overlaps")
    failed(lib, fused(lib, t=X_), FUSED, "overlaps")
    failed(lib, fused(lib, t=R_), FUSED, "overlaps")                                # t == r
    failed(lib, fused(lib, t=R_ + 510), FUSED, "overlaps")
    failed(lib, fused(lib, t=U_), FUSED, "overlaps")                                # t == u
    failed(lib, fused(lib, r=U_ + 2), FUSED, "overlaps")                            # r inside u, but not the in-place form
    failed(lib, fused(lib, r=A_ + 4096), FUSED, "overlaps")
    failed(lib, fused(lib, t=A_ + 4096), FUSED, "overlaps")
    failed(lib, fused(lib, u=U_, r=U_, t=U_), FUSED, "overlaps")                    # in place, but t on top of it
    failed(lib, iht(lib, t3=addr(20)), IHT1, "overlaps")                            # t3 == x
    failed(lib, iht(lib, t1=addr(22)), IHT1, "overlaps")                            # t1 == y
    failed(lib, iht(lib, t2=addr(24) + 128), IHT1, "overlaps")                      # t2 inside t1
    failed(lib, iht(lib, t2=A_), IHT1, "overlaps")
    failed(lib, iht(lib, x=A_ + 4096), IHT1, "overlaps")


def test_the_in_place_form_passes_validation(lib):
    # cols == 0: everything is checked, nothing runs
    assert fused(lib, cols=0, u=U_, r=U_) == 0
    # with columns r == u passes the overlap check: the same call with t on x is refused for t, not for r
    failed(lib, fused(lib, u=U_, r=U_, t=X_), FUSED, "overlaps", "`t`")
