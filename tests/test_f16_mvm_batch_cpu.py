"""The batched half-precision calls, CloverMatrix16 x CloverVector16 (include/clover_hip_batch_f16.h: clm_f16_mvm_batch,
clm_f16_mvm_scale_and_add_batch, clv_f16_threshold_batch, clm_f16_iht_batch) without a GPU: the header of their own declares exactly them,
the library exports them, the table of their own (SIGNATURES_BATCH_F16) binds them and touches none of the other five tables nor
clover_hip.h; the header is plain C99; the container methods and the Q_IHT_batch / Q_GD_batch overloads compile in both container modes
and both exactness builds; and every argument check answers before any device work, on a machine that has no device.

The pointer arrays are HOST arrays of device pointers; the addresses below are never dereferenced (a call that passes validation has
rows == 0 or nvec == 0, so nothing runs).  A is rows x cols binary16 (2 rows cols bytes): x has 2 cols bytes, r, u and t 2 rows."""
import ctypes as C
import re
import subprocess

import pytest

from clover_amd.build import HIP_SOURCES, build_hip_library, repo_root
from clover_amd.lib_binding import (SIGNATURES, SIGNATURES_BATCH_F16, SIGNATURES_BATCH_T, SIGNATURES_BATCH_T8, SIGNATURES_BATCH_T_V8, SIGNATURES_FP32,
                                    load_library)
from test_mvm_batch_cpu import addr, arr, failed

INC = repo_root() / "include"
NAMES = {"clm_f16_mvm_batch": 7, "clm_f16_mvm_scale_and_add_batch": 10, "clv_f16_threshold_batch": 7, "clm_f16_iht_batch": 16}
OTHERS = (SIGNATURES, SIGNATURES_FP32, SIGNATURES_BATCH_T, SIGNATURES_BATCH_T8, SIGNATURES_BATCH_T_V8)
MVM, FUSED, THRESH, IHT = "clm_f16_mvm_batch", "clm_f16_mvm_scale_and_add_batch", "clv_f16_threshold_batch", "clm_f16_iht_batch"


@pytest.fixture(scope="module")
def lib():
    return load_library()


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", (INC / header).read_text(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(cl[mv]\w*)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)}


# ---------------------------------------------------------------- header, library, table
def test_the_header_declares_exactly_the_four_calls_and_the_table_binds_them():
    decl = declared("clover_hip_batch_f16.h")
    assert sorted(decl) == sorted(NAMES) == sorted(SIGNATURES_BATCH_F16)
    raw = C.CDLL(str(build_hip_library()))
    for name, arity in NAMES.items():
        assert len(decl[name].split(",")) == arity, name
        assert hasattr(raw, name), f"{name} is not exported"
        assert len(SIGNATURES_BATCH_F16[name][1]) == arity and SIGNATURES_BATCH_F16[name][0] is C.c_int, name
        assert getattr(load_library(), name).argtypes is not None, f"{name} is not bound by load_library"
    for other in OTHERS:
        assert not set(SIGNATURES_BATCH_F16) & set(other)
    for header in ("clover_hip.h", "clover_hip_fp32.h", "clover_hip_batch_t.h", "clover_hip_batch_t8.h", "clover_hip_batch_t_v8.h"):
        text = (INC / header).read_text()
        for name in NAMES:
            assert not re.search(r"\b" + name + r"\b", text), f"{name} occurs in {header}"
    assert sorted(declared("clover_hip_batch_t.h")) == sorted(SIGNATURES_BATCH_T)
    assert sorted(declared("clover_hip_batch_t8.h")) == sorted(SIGNATURES_BATCH_T8)
    assert sorted(declared("clover_hip_batch_t_v8.h")) == sorted(SIGNATURES_BATCH_T_V8)


def test_the_signatures_follow_the_single_calls():
    """each batch call takes the single call's scalars, with nvec behind the shape and an array where the single call has a vector"""
    main, ours = declared("clover_hip.h"), declared("clover_hip_batch_f16.h")

    def types(params):
        return [re.sub(r"\s+", " ", re.sub(r"\w+$", "", p.strip())).strip() for p in params.split(",")]

    def as_array(t):
        return {"const uint16_t *": "const uint16_t *const *", "uint16_t *": "uint16_t *const *"}.get(t, t)
    one = types(main["clm_f16_mvm"])
    assert types(ours[MVM]) == one[:3] + ["uint64_t"] + [as_array(t) for t in one[3:5]] + one[5:]
    one = types(main["clm_f16_mvm_scale_and_add"])
    assert types(ours[FUSED]) == one[:3] + ["uint64_t"] + [as_array(t) for t in one[3:5]] + ["float"] + [as_array(t) for t in one[6:8]] + one[8:]
    one = types(main["clm_f16_iht"])
    assert types(ours[IHT]) == one[:4] + ["uint64_t", as_array(one[4]), one[5]] + [as_array(t) for t in one[6:10]] + one[10:]
    one = types(main["clv_f16_threshold_mode"])                     # the batch call has no workspace argument, as clv8_threshold_batch
    assert types(ours[THRESH]) == [as_array(one[0]), "uint64_t"] + one[1:5] + one[6:]
    assert SIGNATURES_BATCH_F16[THRESH] == (SIGNATURES["clv8_threshold_batch"][0], SIGNATURES["clv8_threshold_batch"][1][1:])


def test_the_kernel_is_a_source_of_the_library():
    assert "half16_batch.hip" in HIP_SOURCES
    csrc = repo_root() / "clover_amd" / "csrc"
    text = (csrc / "half16_batch.hip").read_text()
    # the chunk of x the GPU tests take their shapes from: 512 columns per wave of the workgroup
    assert re.search(r"#define\s+F16B_CHUNK\(WAVES\)\s+\(512u \* \(WAVES\)\)", text)
    for shared in ("f16_fuse_store", "f16_bits", "ld_stream", "F16_STREAMING", "f16_chain_tree"):      # the device side: beside the kernel
        assert shared in text, shared
    assert not re.search(r"\basm\b", text), "no inline assembly"
    # the host side: the driver it shares with the transposed family, no group loop of its own
    host = (csrc / "half16_batch_host.h").read_text()
    for shared in ("mvm_batch_forced", "clv_internal_mvm_batch_count"):
        assert shared in host, shared
    assert re.search(r'^#include "half16_batch_host\.h"', text, flags=re.M)
    assert not re.search(r"\bfor\s*\([^{\n]*CLM4_MVM_BATCH_MAX", text), "half16_batch.hip has a group loop of its own"
    build = (repo_root() / "clover_amd" / "build.py").read_text()
    assert "clover_hip_batch_f16.h" in build, "the header is a dependency of the library"


C99_CLIENT = r'''
#include <stdio.h>
#include "clover_hip_batch_f16.h"
int main(void)
{
    /* nvec == 0: the matrix arguments are checked, nothing else is looked at, nothing runs */
    const uint16_t *A = (const uint16_t *)0x10000;
    int ok = clm_f16_mvm_batch(A, 128, 256, 0, NULL, NULL, NULL) == CLV_OK;
    ok = ok && clm_f16_mvm_scale_and_add_batch(A, 128, 256, 0, NULL, NULL, 0.5f, NULL, NULL, NULL) == CLV_OK;
    ok = ok && clv_f16_threshold_batch(NULL, 0, 100, 128, 4, CLV_THRESHOLD_FAST, NULL) == CLV_OK;
    ok = ok && clm_f16_iht_batch(A, A + 128 * 256, 128, 256, 0, NULL, 256, NULL, NULL, NULL, NULL, 3, 8, 0.5f, 1, NULL) == CLV_OK;
    ok = ok && clm_f16_mvm_batch(A, 128, 100, 0, NULL, NULL, NULL) == CLV_ERR_INVALID;
    printf("ok=%d\n", ok);
    return !ok;
}
'''


def test_the_header_is_plain_c99_and_a_client_links(tmp_path):
    lib = build_hip_library()
    src, exe = tmp_path / "batch_f16_from_c.c", tmp_path / "batch_f16_from_c"
    src.write_text(C99_CLIENT)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{INC}", str(src), "-o", str(exe), f"-L{lib.parent}",
                    "-lclover_hip", f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "ok=1" in p.stdout, (p.returncode, p.stdout, p.stderr)


CONTAINER_CLIENT = r'''
#include <CloverIHT.h>
int main() {
    const uint64_t m = 128, n = 256, count = 3;
    CloverMatrix16 A(m, n), At(n, m);
    CloverVector16 *x[count], *y[count], *u[count], *t1[count], *t2[count], *t3[count];
    for (uint64_t j = 0; j < count; j++) {
        x[j] = new CloverVector16(n); y[j] = new CloverVector16(m); u[j] = new CloverVector16(m);
        t1[j] = new CloverVector16(m); t2[j] = new CloverVector16(m); t3[j] = new CloverVector16(n);
    }
    A.mvm_batch(x, t1, count);
    A.mvm_scaleAndAdd_batch(x, y, -1.0f, t1, t2, count);            /* out of place */
    A.mvm_scaleAndAdd_batch(x, u, 0.5f, t1, count);                 /* in place */
    A.iht_loop_batch(At, x, y, t1, t2, t3, count, 3, 10, 0.5f, true);
    Q_IHT_batch(A, At, x, y, t1, t2, t3, count, 3, 10, 0.5f);
    Q_GD_batch(A, At, x, y, t1, t2, t3, count, 3, 0.5f);
    return 0;
}
'''


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("explicit", [False, True])
def test_the_container_methods_and_the_loops_compile_and_reach_the_batch_calls(tmp_path, explicit, fast):
    """tracked and -DCLOVER_HIP_EXPLICIT_SYNC, reference and -DCLOVER_FAST: the object references the three batch calls and none of the
    single half-precision mvm calls"""
    src, obj = tmp_path / "f16_batch_client.cpp", tmp_path / "f16_batch_client.o"
    src.write_text(CONTAINER_CLIENT)
    flags = (["-DCLOVER_HIP_EXPLICIT_SYNC"] if explicit else []) + (["-DCLOVER_FAST"] if fast else [])
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", *flags, f"-I{INC}", "-c", str(src), "-o", str(obj)], check=True)
    out = subprocess.run(["nm", "-u", str(obj)], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {MVM, FUSED, IHT} <= syms, sorted(s for s in syms if s.startswith("cl"))
    assert not syms & {"clm_f16_mvm", "clm_f16_mvm_scale_and_add", "clm_f16_iht"}, sorted(s for s in syms if s.startswith("cl"))


# ---------------------------------------------------------------- the argument checks
# 128 x 256: the matrix has 65536 bytes, x 512, r / u / t 256.  addr(i) are 1 MiB apart
A_ = addr(0)


def mvm(lib, rows=128, cols=256, nvec=2, A=A_, x="default", r="default"):
    x = arr(addr(2), addr(3)) if x == "default" else x
    r = arr(addr(6), addr(7)) if r == "default" else r
    return lib.clm_f16_mvm_batch(A, rows, cols, nvec, x, r, None)


def fused(lib, rows=128, cols=256, nvec=2, A=A_, **kw):
    p = dict(x=arr(addr(2), addr(3)), u=arr(addr(10), addr(11)), t=arr(addr(14), addr(15)), r=arr(addr(6), addr(7)))
    p.update(kw)
    return lib.clm_f16_mvm_scale_and_add_batch(A, rows, cols, nvec, p["x"], p["u"], 0.5, p["t"], p["r"], None)


def thresh(lib, h="default", nvec=2, n=200, n_pad=256, k=8, mode=0):
    h = arr(addr(2), addr(3)) if h == "default" else h
    return lib.clv_f16_threshold_batch(h, nvec, n, n_pad, k, mode, None)


def iht(lib, m=128, n=256, nvec=2, x_len=256, thr=1, Phi=A_, PhiT=addr(1), **kw):
    p = {k: arr(addr(20 + 2 * i), addr(21 + 2 * i)) for i, k in enumerate(("x", "y", "t1", "t2", "t3"))}
    p.update(kw)
    return lib.clm_f16_iht_batch(Phi, PhiT, m, n, nvec, p["x"], x_len, p["y"], p["t1"], p["t2"], p["t3"], 3, 8, 0.5, thr, None)


def test_nvec_zero_and_rows_zero_return_ok(lib):
    before = lib.clv_mvm_batch_launches()
    assert lib.clm_f16_mvm_batch(A_, 128, 256, 0, None, None, None) == 0
    assert lib.clm_f16_mvm_scale_and_add_batch(A_, 128, 256, 0, None, None, 0.5, None, None, None) == 0
    assert lib.clv_f16_threshold_batch(None, 0, 100, 128, 4, 0, None) == 0
    assert iht(lib, nvec=0, x=None, y=None, t1=None, t2=None, t3=None) == 0
    assert mvm(lib, rows=0) == 0 and fused(lib, rows=0) == 0 and fused(lib, rows=0, t=None) == 0
    assert lib.clv_mvm_batch_launches() == before


def test_null_arrays_and_null_entries(lib):
    failed(lib, mvm(lib, A=None), MVM, "null")
    failed(lib, mvm(lib, x=None), MVM, "null pointer array")
    failed(lib, mvm(lib, r=None), MVM, "null pointer array")
    failed(lib, mvm(lib, x=arr(None, addr(3))), MVM, "vector 0")
    failed(lib, mvm(lib, r=arr(addr(6), None)), MVM, "vector 1")
    failed(lib, fused(lib, u=None), FUSED, "null pointer array")
    failed(lib, fused(lib, r=None), FUSED, "null pointer array")
    failed(lib, fused(lib, u=arr(addr(10), None)), FUSED, "vector 1")
    failed(lib, fused(lib, t=arr(None, addr(15))), FUSED, "vector 0")
    assert fused(lib, rows=0, t=None) == 0                                          # the whole t array may be NULL
    failed(lib, thresh(lib, h=None), THRESH, "null pointer array")
    failed(lib, thresh(lib, h=arr(addr(2), None)), THRESH, "vector 1")
    failed(lib, iht(lib, Phi=None), IHT, "null pointer")
    failed(lib, iht(lib, PhiT=None), IHT, "null pointer")
    failed(lib, iht(lib, t2=None), IHT, "null pointer array")
    failed(lib, iht(lib, y=arr(addr(22), None)), IHT, "vector 1")


def test_size_and_alignment_rules(lib):
    failed(lib, mvm(lib, cols=100), MVM, "cols=100", "multiple of 128")
    failed(lib, fused(lib, cols=100), FUSED, "cols=100", "multiple of 128")
    failed(lib, mvm(lib, A=A_ + 8), MVM, "16-byte aligned")
    failed(lib, fused(lib, A=A_ + 2), FUSED, "16-byte aligned")
    failed(lib, mvm(lib, x=arr(addr(2), addr(3) + 2)), MVM, "16-byte aligned", "vector 1")
    failed(lib, fused(lib, x=arr(addr(2) + 8, addr(3))), FUSED, "16-byte aligned", "vector 0")
    failed(lib, mvm(lib, r=arr(addr(6), addr(7) + 1)), MVM, "2-byte aligned", "vector 1")
    failed(lib, fused(lib, r=arr(addr(6) + 1, addr(7))), FUSED, "2-byte aligned", "vector 0")
    failed(lib, fused(lib, u=arr(addr(10), addr(11) + 3)), FUSED, "2-byte aligned", "vector 1")
    failed(lib, fused(lib, t=arr(addr(14), addr(15) + 1)), FUSED, "2-byte aligned", "vector 1")
    assert mvm(lib, rows=0, r=arr(addr(6) + 2, addr(7) + 6)) == 0                   # results need only their element alignment
    failed(lib, iht(lib, m=64), IHT, "m=64")
    failed(lib, iht(lib, n=192), IHT, "n=192")
    failed(lib, iht(lib, x_len=257), IHT, "x_len=257")
    failed(lib, iht(lib, thr=3), IHT, "threshold 3")
    failed(lib, iht(lib, thr=-1), IHT, "threshold -1")
    failed(lib, iht(lib, Phi=A_ + 8), IHT, "16-byte aligned")
    failed(lib, iht(lib, x=arr(addr(20), addr(21) + 2)), IHT, "16-byte aligned", "vector 1")
    failed(lib, iht(lib, t2=arr(addr(26) + 8, addr(27))), IHT, "16-byte aligned", "vector 0")
    failed(lib, iht(lib, t1=arr(addr(24), addr(25) + 1)), IHT, "2-byte aligned", "vector 1")
    failed(lib, thresh(lib, mode=7), THRESH, "unknown mode 7")
    failed(lib, thresh(lib, n_pad=200), THRESH, "n_pad=200")
    failed(lib, thresh(lib, n=257), THRESH, "n=257")


def test_the_aliases_the_single_calls_refuse_are_refused_by_name(lib):
    failed(lib, mvm(lib, r=arr(addr(6), addr(3))), MVM, "alias", "vector 1")                     # r[1] == x[1]
    failed(lib, fused(lib, r=arr(addr(2), addr(7))), FUSED, "alias", "vector 0")                 # r[0] == x[0]
    failed(lib, fused(lib, t=arr(addr(14), addr(3))), FUSED, "alias", "vector 1")                # t[1] == x[1]
    failed(lib, fused(lib, t=arr(addr(14), addr(7))), FUSED, "t of vector 1", "alias")           # t[1] == r[1]
    failed(lib, fused(lib, t=arr(addr(10), addr(15))), FUSED, "t of vector 0", "alias")          # t[0] == u[0]


def test_outputs_may_not_overlap_inputs_of_any_vector_nor_each_other(lib):
    before = lib.clv_mvm_batch_launches()
    # r of vector 0 is x of vector 1: another workgroup may still be reading it
    failed(lib, mvm(lib, r=arr(addr(3), addr(7))), MVM, "overlaps", "vector 0", "vector 1")
    failed(lib, mvm(lib, r=arr(addr(3) + 510, addr(7))), MVM, "overlaps")                        # x is sized by the COLUMNS: 512 bytes
    assert mvm(lib, rows=0, r=arr(addr(3) + 512, addr(7))) == 0
    failed(lib, mvm(lib, r=arr(addr(3) - 254, addr(7))), MVM, "overlaps")                        # r is sized by the ROWS: 256 bytes
    failed(lib, mvm(lib, r=arr(addr(6), addr(6))), MVM, "overlaps", "vector 0", "vector 1")      # two equal outputs
    failed(lib, mvm(lib, r=arr(addr(6), addr(6) + 254)), MVM, "overlaps")
    failed(lib, mvm(lib, r=arr(addr(6), A_)), MVM, "overlaps", "matrix")                         # an output inside the matrix
    failed(lib, mvm(lib, r=arr(addr(6), A_ + 2 * 128 * 256 - 2)), MVM, "overlaps", "matrix")
    failed(lib, fused(lib, r=arr(addr(3), addr(7))), FUSED, "overlaps", "vector 0", "vector 1")  # r[0] == x[1]
    failed(lib, fused(lib, r=arr(addr(6), addr(10))), FUSED, "overlaps")                         # r[1] == u[0]: not the in-place form
    failed(lib, fused(lib, t=arr(addr(14), addr(6))), FUSED, "overlaps")                         # t[1] == r[0]
    failed(lib, fused(lib, t=arr(addr(14), addr(14))), FUSED, "overlaps")
    failed(lib, fused(lib, r=arr(addr(6), A_ + 4096)), FUSED, "overlaps", "matrix")
    failed(lib, thresh(lib, h=arr(addr(2), addr(2))), THRESH, "overlaps", "vector 0", "vector 1")
    failed(lib, thresh(lib, h=arr(addr(2), addr(2) + 510)), THRESH, "overlaps")                  # a vector is 2 n_pad bytes
    failed(lib, iht(lib, t3=arr(addr(28), addr(20))), IHT, "overlaps")                           # t3[1] == x[0]
    failed(lib, iht(lib, t1=arr(addr(24), addr(22))), IHT, "overlaps")                           # t1[1] == y[0]
    failed(lib, iht(lib, x=arr(addr(20), addr(20))), IHT, "overlaps")
    failed(lib, iht(lib, t2=arr(addr(26), A_)), IHT, "overlaps", "matrix")
    failed(lib, iht(lib, t2=arr(addr(26), addr(1) + 4096)), IHT, "overlaps", "matrix")           # inside PhiT
    assert lib.clv_mvm_batch_launches() == before


def test_repeated_inputs_and_the_in_place_form_pass_validation(lib):
    # rows == 0: everything is checked, nothing runs (x keeps its 512 bytes, the results are empty)
    assert mvm(lib, rows=0, x=arr(addr(2), addr(2))) == 0
    assert fused(lib, rows=0, u=arr(addr(10), addr(10))) == 0
    assert fused(lib, rows=0, r=arr(addr(10), addr(11))) == 0                                    # r[j] == u[j]
    # with rows the in-place form passes the overlap check and is refused only for a reason of its own: vector 1's u is vector 0's result
    failed(lib, fused(lib, r=arr(addr(10), addr(7)), u=arr(addr(10), addr(10))), FUSED, "overlaps")
