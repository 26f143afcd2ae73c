"""The batched transposed half-precision calls (include/clover_hip_batch_f16_t.h: clm_f16_mvm_transposed_batch,
clm_f16_mvm_transposed_scale_and_add_batch, clm_f16_iht_batch_one_matrix) without a GPU: the header of their own declares exactly them,
the library exports them, the table of their own (SIGNATURES_BATCH_F16_T) binds them and touches none of the other seven tables nor any
other header; the header is plain C99; the container methods and the Q_IHT_batch_one_matrix / Q_GD_batch_one_matrix overloads compile in
both container modes and both exactness builds; every argument check answers before any device work, on a machine that has no device;
and the data of the GPU tests tells every wrong summation order apart, for every shape and every vector they use.

The pointer arrays are HOST arrays of device pointers; the addresses below are never dereferenced (a call that passes validation has
rows == 0, cols == 0 or nvec == 0, so nothing runs).  A is rows x cols binary16 (2 rows cols bytes): x has 2 rows bytes, r, u and t
2 cols."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from clover_amd.build import HIP_SOURCES, build_hip_library, repo_root
from clover_amd.lib_binding import (SIGNATURES, SIGNATURES_BATCH_F16, SIGNATURES_BATCH_F16_T, SIGNATURES_BATCH_T, SIGNATURES_BATCH_T8,
                                    SIGNATURES_BATCH_T_V8, SIGNATURES_F16_T, SIGNATURES_FP32, load_library)
from f16_transposed_batch_data import CHUNK_RE, COLS_RE, SHAPES, U_RE, count_for, x_of
from f16_transposed_data import ZERO_COLUMN, case
from f16_transposed_helpers import WRONG, rt  # noqa: F401  (fixture)
from test_mvm_batch_cpu import addr, arr, failed

INC = repo_root() / "include"
MVM, FUSED, IHT = "clm_f16_mvm_transposed_batch", "clm_f16_mvm_transposed_scale_and_add_batch", "clm_f16_iht_batch_one_matrix"
NAMES = {MVM: 7, FUSED: 10, IHT: 15}
OTHERS = (SIGNATURES, SIGNATURES_FP32, SIGNATURES_BATCH_T, SIGNATURES_BATCH_T8, SIGNATURES_BATCH_T_V8, SIGNATURES_BATCH_F16, SIGNATURES_F16_T)


@pytest.fixture(scope="module")
def lib():
    return load_library()


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", (INC / header).read_text(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(cl[mv]\w*)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)}


# ---------------------------------------------------------------- header, library, table
def test_the_header_declares_exactly_the_three_calls_and_the_table_binds_them():
    decl = declared("clover_hip_batch_f16_t.h")
    assert sorted(decl) == sorted(NAMES) == sorted(SIGNATURES_BATCH_F16_T)
    raw = C.CDLL(str(build_hip_library()))
    for name, arity in NAMES.items():
        assert len(decl[name].split(",")) == arity, name
        assert hasattr(raw, name), f"{name} is not exported"
        assert len(SIGNATURES_BATCH_F16_T[name][1]) == arity and SIGNATURES_BATCH_F16_T[name][0] is C.c_int, name
        assert getattr(load_library(), name).argtypes is not None, f"{name} is not bound by load_library"
    for other in OTHERS:
        assert not set(SIGNATURES_BATCH_F16_T) & set(other)
    for header in sorted(INC.glob("clover_hip*.h")):
        if header.name != "clover_hip_batch_f16_t.h":
            for name in NAMES:
                assert not re.search(r"\b" + name + r"\b", header.read_text()), f"{name} occurs in {header.name}"


def test_the_signatures_follow_the_single_transposed_calls():
    """each product call takes the single transposed call's scalars, with nvec behind the shape and an array where the single call has a
    vector; the loop is clm_f16_iht_batch without PhiT"""
    single, batch, ours = declared("clover_hip_f16_t.h"), declared("clover_hip_batch_f16.h"), declared("clover_hip_batch_f16_t.h")

    def types(params):
        return [re.sub(r"\s+", " ", re.sub(r"\w+$", "", p.strip())).strip() for p in params.split(",")]

    def as_array(t):
        return {"const uint16_t *": "const uint16_t *const *", "uint16_t *": "uint16_t *const *"}.get(t, t)
    one = types(single["clm_f16_mvm_transposed"])
    assert types(ours[MVM]) == one[:3] + ["uint64_t"] + [as_array(t) for t in one[3:5]] + one[5:]
    one = types(single["clm_f16_mvm_transposed_scale_and_add"])
    assert types(ours[FUSED]) == one[:3] + ["uint64_t"] + [as_array(t) for t in one[3:5]] + ["float"] + [as_array(t) for t in one[6:8]] + one[8:]
    held = types(batch["clm_f16_iht_batch"])
    assert types(ours[IHT]) == held[:1] + held[2:]
    one = types(single["clm_f16_iht_one_matrix"])
    assert types(ours[IHT]) == one[:3] + ["uint64_t", as_array(one[3]), one[4]] + [as_array(t) for t in one[5:9]] + one[9:]
    # the tables: those of the row-major batch, whose C types these calls share; the loop without PhiT
    assert SIGNATURES_BATCH_F16_T[MVM] == SIGNATURES_BATCH_F16["clm_f16_mvm_batch"]
    assert SIGNATURES_BATCH_F16_T[FUSED] == SIGNATURES_BATCH_F16["clm_f16_mvm_scale_and_add_batch"]
    res, args = SIGNATURES_BATCH_F16["clm_f16_iht_batch"]
    assert SIGNATURES_BATCH_F16_T[IHT] == (res, args[:1] + args[2:])


def test_the_kernel_is_a_source_of_the_library_and_the_header_a_dependency():
    assert "half16_t_batch.hip" in HIP_SOURCES
    csrc = repo_root() / "clover_amd" / "csrc"
    text = (csrc / "half16_t_batch.hip").read_text()
    for regex in (COLS_RE, U_RE, CHUNK_RE):              # the constants the GPU tests take their shapes from
        assert re.search(regex, text), regex
    for shared in ("F16Fuse", "f16_fuse_store", "f16_bits", "ld_stream", "F16_STREAMING"):       # the device side: beside the kernel
        assert shared in text, shared
    assert not re.search(r"\basm\b", text), "no inline assembly"
    # the host side: one driver for both half-precision families, no group loop in either source
    host = (csrc / "half16_batch_host.h").read_text()
    for shared in ("mvm_batch_forced", "clv_internal_mvm_batch_count"):
        assert shared in host, shared
    for name in ("half16_batch.hip", "half16_t_batch.hip"):
        source = (csrc / name).read_text()
        assert re.search(r'^#include "half16_batch_host\.h"', source, flags=re.M), name
        assert not re.search(r"\bfor\s*\([^{\n]*CLM4_MVM_BATCH_MAX", source), f"{name} has a group loop of its own"
    assert not (csrc / "half16_batch.h").exists()
    build = (repo_root() / "clover_amd" / "build.py").read_text()
    assert "clover_hip_batch_f16_t.h" in build, "the header is a dependency of the library"


C99_CLIENT = r'''
#include <stdio.h>
#include "clover_hip_batch_f16_t.h"
int main(void)
{
    /* nvec == 0: the matrix arguments are checked, nothing else is looked at, nothing runs */
    const uint16_t *A = (const uint16_t *)0x10000;
    int ok = clm_f16_mvm_transposed_batch(A, 128, 256, 0, NULL, NULL, NULL) == CLV_OK;
    ok = ok && clm_f16_mvm_transposed_scale_and_add_batch(A, 128, 256, 0, NULL, NULL, 0.5f, NULL, NULL, NULL) == CLV_OK;
    ok = ok && clm_f16_iht_batch_one_matrix(A, 128, 256, 0, NULL, 256, NULL, NULL, NULL, NULL, 3, 8, 0.5f, 1, NULL) == CLV_OK;
    ok = ok && clm_f16_mvm_transposed_batch(A, 128, 100, 0, NULL, NULL, NULL) == CLV_ERR_INVALID;
    ok = ok && clm_f16_mvm_transposed_batch(A, 64, 128, 0, NULL, NULL, NULL) == CLV_ERR_INVALID;
    ok = ok && clm_f16_iht_batch_one_matrix(A, 128, 256, 0, NULL, 257, NULL, NULL, NULL, NULL, 3, 8, 0.5f, 1, NULL) == CLV_ERR_INVALID;
    printf("ok=%d\n", ok);
    return !ok;
}
'''


def test_the_header_is_plain_c99_and_a_client_links(tmp_path):
    lib = build_hip_library()
    src, exe = tmp_path / "batch_f16_t_from_c.c", tmp_path / "batch_f16_t_from_c"
    src.write_text(C99_CLIENT)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{INC}", str(src), "-o", str(exe), f"-L{lib.parent}",
                    "-lclover_hip", f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "ok=1" in p.stdout, (p.returncode, p.stdout, p.stderr)


CONTAINER_CLIENT = r'''
#include <CloverIHT.h>
int main() {
    const uint64_t m = 128, n = 256, count = 3;
    CloverMatrix16 A(m, n);
    CloverVector16 *x[count], *y[count], *u[count], *t1[count], *t2[count], *t3[count];
    for (uint64_t j = 0; j < count; j++) {
        x[j] = new CloverVector16(n); y[j] = new CloverVector16(m); u[j] = new CloverVector16(n);
        t1[j] = new CloverVector16(m); t2[j] = new CloverVector16(m); t3[j] = new CloverVector16(n);
    }
    A.mvm_transposed_batch(y, t3, count);
    A.mvm_transposed_scaleAndAdd_batch(y, u, 0.5f, t3, x, count);          /* out of place */
    A.mvm_transposed_scaleAndAdd_batch(y, u, 0.5f, t3, count);             /* in place */
    A.iht_loop_batch_one_matrix(x, y, t1, t2, t3, count, 3, 10, 0.5f, true);
    Q_IHT_batch_one_matrix(A, x, y, t1, t2, t3, count, 3, 10, 0.5f);
    Q_GD_batch_one_matrix(A, x, y, t1, t2, t3, count, 3, 0.5f);
    return 0;
}
'''


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("explicit", [False, True])
def test_the_container_methods_and_the_loops_compile_and_reach_the_new_calls(tmp_path, explicit, fast):
    """tracked and -DCLOVER_HIP_EXPLICIT_SYNC, reference and -DCLOVER_FAST: the object references the three new calls, no transposition,
    no other half-precision mvm and no other half-precision loop"""
    src, obj = tmp_path / "f16_t_batch_client.cpp", tmp_path / "f16_t_batch_client.o"
    src.write_text(CONTAINER_CLIENT)
    flags = (["-DCLOVER_HIP_EXPLICIT_SYNC"] if explicit else []) + (["-DCLOVER_FAST"] if fast else [])
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", *flags, f"-I{INC}", "-c", str(src), "-o", str(obj)], check=True)
    out = subprocess.run(["nm", "-u", str(obj)], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    ours = sorted(s for s in syms if s.startswith("cl"))
    assert set(NAMES) <= syms, ours
    assert not [s for s in syms if s.startswith("clm_f16_mvm") and s not in NAMES], ours
    assert not syms & {"clm_f16_transpose", "clm_f16_iht", "clm_f16_iht_batch", "clm_f16_iht_one_matrix"}, ours


# ---------------------------------------------------------------- the argument checks
# 128 x 256: the matrix has 65536 bytes, x 256, r / u / t 512.  addr(i) are 1 MiB apart
A_ = addr(0)


def mvm(lib, rows=128, cols=256, nvec=2, A=A_, x="default", r="default"):
    x = arr(addr(2), addr(3)) if x == "default" else x
    r = arr(addr(6), addr(7)) if r == "default" else r
    return lib.clm_f16_mvm_transposed_batch(A, rows, cols, nvec, x, r, None)


def fused(lib, rows=128, cols=256, nvec=2, A=A_, **kw):
    p = dict(x=arr(addr(2), addr(3)), u=arr(addr(10), addr(11)), t=arr(addr(14), addr(15)), r=arr(addr(6), addr(7)))
    p.update(kw)
    return lib.clm_f16_mvm_transposed_scale_and_add_batch(A, rows, cols, nvec, p["x"], p["u"], 0.5, p["t"], p["r"], None)


def iht(lib, m=128, n=256, nvec=2, x_len=256, thr=1, Phi=A_, **kw):
    p = {k: arr(addr(20 + 2 * i), addr(21 + 2 * i)) for i, k in enumerate(("x", "y", "t1", "t2", "t3"))}
    p.update(kw)
    return lib.clm_f16_iht_batch_one_matrix(Phi, m, n, nvec, p["x"], x_len, p["y"], p["t1"], p["t2"], p["t3"], 3, 8, 0.5, thr, None)


def test_empty_calls_return_ok_and_launch_nothing(lib):
    before = lib.clv_mvm_batch_launches()
    assert lib.clm_f16_mvm_transposed_batch(A_, 128, 256, 0, None, None, None) == 0
    assert lib.clm_f16_mvm_transposed_scale_and_add_batch(A_, 128, 256, 0, None, None, 0.5, None, None, None) == 0
    assert iht(lib, nvec=0, x=None, y=None, t1=None, t2=None, t3=None) == 0
    for kw in (dict(rows=0), dict(cols=0), dict(rows=0, cols=0)):
        assert mvm(lib, **kw) == 0 and fused(lib, **kw) == 0 and fused(lib, t=None, **kw) == 0, kw
    assert mvm(lib, rows=0, nvec=1) == 0 and fused(lib, cols=0, nvec=1) == 0
    assert lib.clv_mvm_batch_launches() == before


def test_null_arrays_and_null_entries(lib):
    failed(lib, mvm(lib, A=None), MVM, "null")
    failed(lib, mvm(lib, x=None), MVM, "null pointer array")
    failed(lib, mvm(lib, r=None), MVM, "null pointer array")
    failed(lib, mvm(lib, x=arr(None, addr(3))), MVM, "vector 0")
    failed(lib, mvm(lib, r=arr(addr(6), None)), MVM, "vector 1")
    failed(lib, mvm(lib, rows=0, r=arr(addr(6), None)), MVM, "vector 1")            # checked even where nothing would run
    failed(lib, fused(lib, A=None), FUSED, "null")
    failed(lib, fused(lib, x=None), FUSED, "null pointer array")
    failed(lib, fused(lib, u=None), FUSED, "null pointer array")
    failed(lib, fused(lib, r=None), FUSED, "null pointer array")
    failed(lib, fused(lib, u=arr(addr(10), None)), FUSED, "vector 1")
    failed(lib, fused(lib, t=arr(None, addr(15))), FUSED, "vector 0")
    assert fused(lib, rows=0, t=None) == 0                                          # the whole t array may be NULL
    failed(lib, iht(lib, Phi=None), IHT, "null pointer")
    for k in ("x", "y", "t1", "t2", "t3"):
        failed(lib, iht(lib, **{k: None}), IHT, "null pointer array")
    failed(lib, iht(lib, y=arr(addr(22), None)), IHT, "vector 1")
    failed(lib, iht(lib, t3=arr(None, addr(29))), IHT, "vector 0")


def test_size_and_alignment_rules(lib):
    failed(lib, mvm(lib, cols=100), MVM, "cols=100", "multiples of 128")
    failed(lib, mvm(lib, rows=64), MVM, "rows=64", "multiples of 128")
    failed(lib, mvm(lib, rows=200, cols=0), MVM, "rows=200")                        # an empty matrix still has a valid shape
    failed(lib, fused(lib, cols=100), FUSED, "cols=100", "multiples of 128")
    failed(lib, fused(lib, rows=192), FUSED, "rows=192")
    failed(lib, mvm(lib, A=A_ + 8), MVM, "16-byte aligned")
    failed(lib, fused(lib, A=A_ + 2), FUSED, "16-byte aligned")
    failed(lib, mvm(lib, x=arr(addr(2), addr(3) + 2)), MVM, "16-byte aligned", "vector 1")
    failed(lib, fused(lib, x=arr(addr(2) + 8, addr(3))), FUSED, "16-byte aligned", "vector 0")
    failed(lib, mvm(lib, r=arr(addr(6), addr(7) + 1)), MVM, "2-byte aligned", "vector 1")
    failed(lib, fused(lib, r=arr(addr(6) + 1, addr(7))), FUSED, "2-byte aligned", "vector 0")
    failed(lib, fused(lib, u=arr(addr(10), addr(11) + 3)), FUSED, "2-byte aligned", "vector 1")
    failed(lib, fused(lib, t=arr(addr(14), addr(15) + 1)), FUSED, "2-byte aligned", "vector 1")
    assert mvm(lib, rows=0, r=arr(addr(6) + 2, addr(7) + 6)) == 0                   # results need only their element alignment
    # the limits of the single transposed call
    failed(lib, mvm(lib, rows=1 << 40, cols=1 << 40, nvec=0, x=None, r=None), MVM, "matrix too large")
    failed(lib, fused(lib, rows=1 << 40, cols=1 << 40, nvec=0), FUSED, "matrix too large")
    failed(lib, mvm(lib, rows=1 << 37, cols=128, nvec=0, x=None, r=None), MVM, "matrix too large")
    failed(lib, iht(lib, m=1 << 40, n=1 << 40, x_len=0, nvec=0), IHT, "matrix too large")
    failed(lib, iht(lib, m=64), IHT, "m=64")
    failed(lib, iht(lib, n=192), IHT, "n=192")
    failed(lib, iht(lib, x_len=257), IHT, "x_len=257")
    failed(lib, iht(lib, thr=3), IHT, "threshold 3")
    failed(lib, iht(lib, thr=-1), IHT, "threshold -1")
    failed(lib, iht(lib, Phi=A_ + 8), IHT, "16-byte aligned")
    failed(lib, iht(lib, x=arr(addr(20), addr(21) + 2)), IHT, "16-byte aligned", "vector 1")
    failed(lib, iht(lib, t2=arr(addr(26) + 8, addr(27))), IHT, "16-byte aligned", "vector 0")
    failed(lib, iht(lib, t1=arr(addr(24), addr(25) + 1)), IHT, "2-byte aligned", "vector 1")
    failed(lib, iht(lib, y=arr(addr(22) + 1, addr(23))), IHT, "2-byte aligned", "vector 0")


def test_the_aliases_the_single_calls_refuse_are_refused_by_name(lib):
    failed(lib, mvm(lib, r=arr(addr(6), addr(3))), MVM, "alias", "vector 1")                     # r[1] == x[1]
    failed(lib, fused(lib, r=arr(addr(2), addr(7))), FUSED, "alias", "vector 0")                 # r[0] == x[0]
    failed(lib, fused(lib, t=arr(addr(14), addr(3))), FUSED, "alias", "vector 1")                # t[1] == x[1]
    failed(lib, fused(lib, t=arr(addr(14), addr(7))), FUSED, "t of vector 1", "alias")           # t[1] == r[1]
    failed(lib, fused(lib, t=arr(addr(10), addr(15))), FUSED, "t of vector 0", "alias")          # t[0] == u[0]


def test_outputs_may_not_overlap_inputs_of_any_vector_nor_the_matrix_nor_each_other(lib):
    before = lib.clv_mvm_batch_launches()
    # r of vector 0 is x of vector 1: another workgroup may still be reading it
    failed(lib, mvm(lib, r=arr(addr(3), addr(7))), MVM, "overlaps", "vector 0", "vector 1")
    failed(lib, mvm(lib, r=arr(addr(3) + 254, addr(7))), MVM, "overlaps")                        # x is sized by the ROWS: 256 bytes
    assert mvm(lib, cols=0, r=arr(addr(3) + 256, addr(7))) == 0
    failed(lib, mvm(lib, r=arr(addr(3) - 510, addr(7))), MVM, "overlaps")                        # r is sized by the COLUMNS: 512 bytes
    assert mvm(lib, rows=0, r=arr(addr(3) - 512, addr(7))) == 0
    failed(lib, mvm(lib, r=arr(addr(6), addr(6))), MVM, "overlaps", "vector 0", "vector 1")      # two equal outputs
    failed(lib, mvm(lib, r=arr(addr(6), addr(6) + 510)), MVM, "overlaps")
    failed(lib, mvm(lib, r=arr(addr(6), A_)), MVM, "overlaps", "matrix")                         # an output inside the matrix
    failed(lib, mvm(lib, r=arr(addr(6), A_ + 2 * 128 * 256 - 2)), MVM, "overlaps", "matrix")
    failed(lib, fused(lib, r=arr(addr(3), addr(7))), FUSED, "overlaps", "vector 0", "vector 1")  # r[0] == x[1]
    failed(lib, fused(lib, r=arr(addr(6), addr(10))), FUSED, "overlaps")                         # r[1] == u[0]: not the in-place form
    failed(lib, fused(lib, r=arr(addr(6), addr(10) + 510)), FUSED, "overlaps")                   # u is sized by the COLUMNS
    failed(lib, fused(lib, t=arr(addr(14), addr(6))), FUSED, "overlaps")                         # t[1] == r[0]
    failed(lib, fused(lib, t=arr(addr(14), addr(14))), FUSED, "overlaps")
    failed(lib, fused(lib, t=arr(addr(14), addr(2))), FUSED, "overlaps")                         # t[1] == x[0]
    failed(lib, fused(lib, r=arr(addr(6), A_ + 4096)), FUSED, "overlaps", "matrix")
    failed(lib, fused(lib, t=arr(A_ + 4096, addr(15))), FUSED, "overlaps", "matrix")
    failed(lib, iht(lib, t3=arr(addr(28), addr(20))), IHT, "overlaps")                           # t3[1] == x[0]
    failed(lib, iht(lib, t1=arr(addr(24), addr(22))), IHT, "overlaps")                           # t1[1] == y[0]
    failed(lib, iht(lib, x=arr(addr(20), addr(20))), IHT, "overlaps")
    failed(lib, iht(lib, t2=arr(addr(26), addr(24) + 128)), IHT, "overlaps")                     # t2[1] inside t1[0]
    failed(lib, iht(lib, t2=arr(addr(26), A_)), IHT, "overlaps", "matrix")
    failed(lib, iht(lib, x=arr(addr(20), A_ + 4096)), IHT, "overlaps", "matrix")
    assert lib.clv_mvm_batch_launches() == before


def test_repeated_inputs_and_the_in_place_form_pass_validation(lib):
    # cols == 0: everything is checked, nothing runs (x keeps its 256 bytes, the results are empty)
    assert mvm(lib, cols=0, x=arr(addr(2), addr(2))) == 0
    assert fused(lib, cols=0, u=arr(addr(10), addr(10))) == 0
    assert fused(lib, cols=0, r=arr(addr(10), addr(11))) == 0                                    # r[j] == u[j]
    assert fused(lib, rows=0, r=arr(addr(10), addr(11)), t=None) == 0
    # with columns the in-place form passes the overlap check and is refused only for a reason of its own: vector 1's u is vector 0's result
    failed(lib, fused(lib, r=arr(addr(10), addr(7)), u=arr(addr(10), addr(10))), FUSED, "overlaps")


# ---------------------------------------------------------------- the data of the GPU tests
@pytest.mark.parametrize("rows,cols", SHAPES, ids=lambda v: str(v))
def test_the_data_tells_every_wrong_order_apart_for_every_vector(rt, rows, cols):  # noqa: F811
    """the condition the GPU comparisons rest on: on this very data each wrong summation order changes at least one f16 result of every
    vector of the shape; all results are finite and the zero column gives +0"""
    S = case(rows, cols)
    for j in range(count_for((rows, cols))):
        x = x_of(rows, cols, j)
        assert x.size == rows and (j == 0 or not np.array_equal(x, S.x))
        t = rt.mvm_transposed(S.A, rows, cols, x)
        assert np.all(np.isfinite(t.view(np.float16))) and t[ZERO_COLUMN] == 0
        for name, order in WRONG.items():
            n16 = np.count_nonzero(rt.mvm_transposed(S.A, rows, cols, x, order) != t)
            assert n16 >= 1, (name, "vector", j, "the f16 results do not show this order")
