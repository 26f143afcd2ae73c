"""The batched transposed mixed calls, CloverMatrix4 x CloverVector8 (include/clover_hip_batch_t_v8.h: clm4_mvm_v8_transposed_batch, clm4_mvm_v8_transposed_batch_at,
clm4_mvm_v8_transposed_scale_and_add_batch, clm4_iht_v8_batch_one_matrix) without a GPU: the header of their own declares exactly them, the
library exports them, the table of their own (SIGNATURES_BATCH_T_V8) binds them and touches none of the other four tables nor clover_hip.h,
clover_hip_batch_t.h or clover_hip_batch_t8.h; a C99 client compiles with -pedantic and links; every argument check answers before any device work, on a
machine that has no device; and the CPU reference that the GPU tests compare against tells the failure modes apart.

The pointer arrays are HOST arrays of device pointers; the addresses below are never dereferenced (a call that passes validation has
rows == 0 or nvec == 0, so nothing runs).  A is rows x cols nibbles (rows * cols / 2 bytes): x has rows bytes, r cols."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from clover_amd.build import HIP_SOURCES, build_hip_library, repo_root
from clover_amd.lib_binding import SIGNATURES, SIGNATURES_BATCH_T, SIGNATURES_BATCH_T8, SIGNATURES_BATCH_T_V8, SIGNATURES_FP32, load_library
from mvm_v8_transposed_batch_data import A_FUSED, C_, KEYS, NVMAX, S_, U_OF, W, data, eq, same
from oracle.binding import Oracle
from test_mvm_batch_cpu import DEFAULT, addr, arr, failed
from test_mvm_batch_stochastic import keys_equal

NAMES = {"clm4_mvm_v8_transposed_batch": 11, "clm4_mvm_v8_transposed_batch_at": 14, "clm4_mvm_v8_transposed_scale_and_add_batch": 16,
         "clm4_iht_v8_batch_one_matrix": 22}
TWO_MATRIX = {"clm4_mvm_v8_transposed_batch": "clm4_mvm_v8_batch", "clm4_mvm_v8_transposed_batch_at": "clm4_mvm_v8_batch_at",
              "clm4_mvm_v8_transposed_scale_and_add_batch": "clm4_mvm_v8_scale_and_add_batch"}
RNG = addr(60)


@pytest.fixture(scope="module")
def lib():
    return load_library()


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", (repo_root() / "include" / header).read_text(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(cl[mv]\w*)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)}


# ---------------------------------------------------------------- header, library, table
def test_the_header_declares_exactly_the_four_calls_and_the_table_binds_them():
    decl = declared("clover_hip_batch_t_v8.h")
    assert sorted(decl) == sorted(NAMES) == sorted(SIGNATURES_BATCH_T_V8)
    raw = C.CDLL(str(build_hip_library()))
    for name, arity in NAMES.items():
        assert len(decl[name].split(",")) == arity, name
        assert hasattr(raw, name), f"{name} is not exported"
        assert len(SIGNATURES_BATCH_T_V8[name][1]) == arity, name
    for other in (SIGNATURES, SIGNATURES_FP32, SIGNATURES_BATCH_T, SIGNATURES_BATCH_T8):
        assert not set(SIGNATURES_BATCH_T_V8) & set(other)
    for header in ("clover_hip.h", "clover_hip_batch_t.h", "clover_hip_batch_t8.h"):
        text = (repo_root() / "include" / header).read_text()
        for name in NAMES:
            assert not re.search(r"\b" + name + r"\b", text), f"{name} occurs in {header}"
    assert sorted(declared("clover_hip_batch_t.h")) == sorted(SIGNATURES_BATCH_T), "the 4-bit header keeps its four names"
    assert sorted(declared("clover_hip_batch_t8.h")) == sorted(SIGNATURES_BATCH_T8), "the 8-bit header keeps its four names"
    assert hasattr(load_library(), "clm4_iht_v8_batch_one_matrix") and load_library().clm4_iht_v8_batch_one_matrix.argtypes is not None


def test_the_signatures_are_those_of_the_two_matrix_family():
    """the three mvm calls take what clm4_mvm_v8_batch / _at / clm4_mvm_v8_scale_and_add_batch take; the loop is clm4_iht_v8_batch without PhiT / sPhiT"""
    main = declared("clover_hip.h")
    ours = declared("clover_hip_batch_t_v8.h")

    def types(params):
        return [re.sub(r"\s+", " ", re.sub(r"\w+$", "", p.strip())).strip() for p in params.split(",")]
    for name, other in TWO_MATRIX.items():
        assert types(ours[name]) == types(main[other]), name
        assert SIGNATURES_BATCH_T_V8[name] == SIGNATURES[other], name
    two = types(main["clm4_iht_v8_batch"])
    assert types(ours["clm4_iht_v8_batch_one_matrix"]) == two[:2] + two[4:]
    res, args = SIGNATURES["clm4_iht_v8_batch"]
    assert SIGNATURES_BATCH_T_V8["clm4_iht_v8_batch_one_matrix"] == (res, args[:2] + args[4:])


def test_the_kernel_is_a_source_of_the_library_with_constants_the_tests_can_read():
    assert "mvm_t8_batch.hip" in HIP_SOURCES
    single = (repo_root() / "clover_amd" / "csrc" / "mvm_t8.hip").read_text()
    assert W == int(re.search(r"#define\s+MVT8_W\s+(\d+)", single).group(1)) == 2, "the batched kernel keeps the single kernel's output blocks per workgroup"
    assert S_ == 64 and C_ % S_ == 0 and all((C_ // S_) % (2 * u) == 0 for u in U_OF.values()), "a chunk is whole pairs of load groups"
    assert sorted(U_OF) == [2, 4, 8]


def test_a_c99_client_compiles_links_and_gets_the_argument_checks(tmp_path):
    lib = build_hip_library()
    exe = tmp_path / "batch_t_v8_from_c"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{repo_root() / 'include'}",
                    str(repo_root() / "tests" / "c" / "batch_t_v8_from_c.c"), "-o", str(exe), f"-L{lib.parent}", "-lclover_hip",
                    f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "ok=1" in p.stdout, (p.returncode, p.stdout, p.stderr)


# ---------------------------------------------------------------- the argument checks
def mvm(lib, rows=128, cols=256, nvec=2, x=DEFAULT, sx=DEFAULT, r=DEFAULT, sr=DEFAULT, A=addr(0), sA=addr(1)):
    x = arr(addr(2), addr(3)) if x is DEFAULT else x
    sx = arr(addr(4), addr(5)) if sx is DEFAULT else sx
    r = arr(addr(6), addr(7)) if r is DEFAULT else r
    sr = arr(addr(8), addr(9)) if sr is DEFAULT else sr
    return lib.clm4_mvm_v8_transposed_batch(A, sA, rows, cols, nvec, x, sx, r, sr, None, None)


def at(lib, rows=128, cols=256, nvec=2, x=None, sx=None, r=None, sr=None, rng=RNG, base=0, stride=8, commit=16):
    x = x or arr(addr(2), addr(3))
    sx = sx or arr(addr(4), addr(5))
    r = r or arr(addr(6), addr(7))
    sr = sr or arr(addr(8), addr(9))
    return lib.clm4_mvm_v8_transposed_batch_at(addr(0), addr(1), rows, cols, nvec, x, sx, r, sr, rng, base, stride, commit, None)


def fused(lib, rows=128, cols=256, nvec=2, **kw):
    p = dict(x=arr(addr(2), addr(3)), sx=arr(addr(4), addr(5)), qu=arr(addr(10), addr(11)), su=arr(addr(12), addr(13)), t=arr(addr(14), addr(15)),
             st=arr(addr(16), addr(17)), r=arr(addr(6), addr(7)), sr=arr(addr(8), addr(9)))
    p.update(kw)
    return lib.clm4_mvm_v8_transposed_scale_and_add_batch(addr(0), addr(1), rows, cols, nvec, p["x"], p["sx"], p["qu"], p["su"], 0.5, p["t"], p["st"],
                                                       p["r"], p["sr"], None, None)


def iht(lib, m=128, n=256, nvec=2, x_len=256, Phi=addr(0), **kw):
    names = ("x", "sx", "y", "sy", "t1", "st1", "t2", "st2", "t3", "st3")
    p = {k: arr(addr(20 + 2 * i), addr(21 + 2 * i)) for i, k in enumerate(names)}
    p.update(kw)
    return lib.clm4_iht_v8_batch_one_matrix(Phi, addr(1), m, n, nvec, p["x"], p["sx"], x_len, p["y"], p["sy"], p["t1"], p["st1"], p["t2"], p["st2"],
                                         p["t3"], p["st3"], 3, 8, 0.5, 1, None, None)


def test_nvec_zero_and_an_empty_matrix_return_ok(lib):
    before = lib.clv_mvm_batch_launches()
    assert lib.clm4_mvm_v8_transposed_batch(addr(0), addr(1), 128, 256, 0, None, None, None, None, None, None) == 0
    assert lib.clm4_mvm_v8_transposed_batch_at(addr(0), addr(1), 128, 256, 0, None, None, None, None, RNG, 0, 8, 16, None) == 0
    assert lib.clm4_mvm_v8_transposed_scale_and_add_batch(addr(0), addr(1), 128, 256, 0, None, None, None, None, 0.5, None, None, None, None, None,
                                                       None) == 0
    assert iht(lib, nvec=0) == 0
    assert mvm(lib, rows=0) == 0 and at(lib, rows=0) == 0 and fused(lib, rows=0) == 0
    assert mvm(lib, cols=0) == 0 and at(lib, cols=0) == 0 and fused(lib, cols=0) == 0
    assert lib.clv_mvm_batch_launches() == before


def test_size_rules(lib):
    failed(lib, mvm(lib, rows=192), "clm4_mvm_v8_transposed_batch", "multiples of 128")
    failed(lib, mvm(lib, cols=192), "clm4_mvm_v8_transposed_batch", "multiples of 128")
    failed(lib, at(lib, rows=64), "clm4_mvm_v8_transposed_batch_at", "multiples of 128")
    failed(lib, at(lib, cols=320), "clm4_mvm_v8_transposed_batch_at", "multiples of 128")
    failed(lib, fused(lib, rows=100), "clm4_mvm_v8_transposed_scale_and_add_batch", "multiples of 128")
    failed(lib, fused(lib, cols=64), "clm4_mvm_v8_transposed_scale_and_add_batch", "multiples of 128")
    failed(lib, mvm(lib, rows=0, cols=64 << 31), "clm4_mvm_v8_transposed_batch", "too many columns")
    failed(lib, mvm(lib, rows=64 << 31, cols=0), "clm4_mvm_v8_transposed_batch", "too many rows")
    failed(lib, iht(lib, m=64), "clm4_iht_v8_batch_one_matrix", "m=64")
    failed(lib, iht(lib, x_len=257), "clm4_iht_v8_batch_one_matrix", "x_len")


def test_null_arrays_and_null_entries(lib):
    before = lib.clv_mvm_batch_launches()
    failed(lib, mvm(lib, x=None), "clm4_mvm_v8_transposed_batch", "null pointer array")
    failed(lib, mvm(lib, sr=None), "clm4_mvm_v8_transposed_batch", "null pointer array")
    failed(lib, mvm(lib, A=None), "clm4_mvm_v8_transposed_batch", "null")
    failed(lib, mvm(lib, sr=arr(addr(8), None)), "clm4_mvm_v8_transposed_batch", "vector 1")
    failed(lib, mvm(lib, x=arr(None, addr(3))), "clm4_mvm_v8_transposed_batch", "vector 0")
    failed(lib, at(lib, sr=arr(addr(8), None)), "clm4_mvm_v8_transposed_batch_at", "vector 1")
    failed(lib, lib.clm4_mvm_v8_transposed_batch_at(addr(0), addr(1), 128, 256, 2, None, None, None, None, RNG, 0, 8, 16, None),
           "clm4_mvm_v8_transposed_batch_at", "null pointer array")
    failed(lib, fused(lib, qu=None), "clm4_mvm_v8_transposed_scale_and_add_batch", "null pointer array")
    failed(lib, fused(lib, su=arr(addr(12), None)), "clm4_mvm_v8_transposed_scale_and_add_batch", "vector 1")
    failed(lib, fused(lib, t=arr(addr(14), None)), "clm4_mvm_v8_transposed_scale_and_add_batch", "vector 1")
    failed(lib, iht(lib, t2=None), "clm4_iht_v8_batch_one_matrix", "null pointer array")
    failed(lib, iht(lib, st3=arr(addr(38), None)), "clm4_iht_v8_batch_one_matrix", "vector 1")
    failed(lib, iht(lib, Phi=None), "clm4_iht_v8_batch_one_matrix", "null pointer")
    assert lib.clv_mvm_batch_launches() == before


def test_t_and_st_come_together(lib):
    failed(lib, fused(lib, st=None), "clm4_mvm_v8_transposed_scale_and_add_batch", "t and st")
    failed(lib, fused(lib, t=None), "clm4_mvm_v8_transposed_scale_and_add_batch", "t and st")
    assert fused(lib, rows=0, t=None, st=None) == 0


def test_outputs_may_not_overlap_inputs_of_any_vector_nor_each_other(lib):
    """128 x 256: x is rows = 128 bytes, r cols = 256 bytes, sx 8 bytes, sr 16 bytes, the matrix 128 * 256 / 2 = 16384 bytes"""
    before = lib.clv_mvm_batch_launches()
    # r of vector 1 is x of vector 0: another workgroup may still be reading it
    failed(lib, mvm(lib, r=arr(addr(6), addr(2))), "clm4_mvm_v8_transposed_batch", "overlaps", "vector 0", "vector 1")
    failed(lib, mvm(lib, r=arr(addr(6), addr(2) + 127)), "clm4_mvm_v8_transposed_batch", "overlaps")           # x is sized by ROWS: 128 bytes
    assert mvm(lib, rows=0, r=arr(addr(6), addr(2) + 128)) == 0
    failed(lib, mvm(lib, r=arr(addr(6), addr(2) - 255)), "clm4_mvm_v8_transposed_batch", "overlaps")           # r is sized by COLS: 256 bytes
    failed(lib, mvm(lib, r=arr(addr(6), addr(6) + 255)), "clm4_mvm_v8_transposed_batch", "overlaps")
    failed(lib, mvm(lib, sr=arr(addr(8), addr(4))), "clm4_mvm_v8_transposed_batch", "overlaps")
    failed(lib, mvm(lib, sr=arr(addr(8), addr(4) + 4)), "clm4_mvm_v8_transposed_batch", "overlaps")            # sx: rows / 64 * 4 = 8 bytes
    failed(lib, mvm(lib, sr=arr(addr(8), addr(8) + 12)), "clm4_mvm_v8_transposed_batch", "overlaps")           # sr: cols / 64 * 4 = 16 bytes
    failed(lib, mvm(lib, r=arr(addr(6), addr(0))), "clm4_mvm_v8_transposed_batch", "overlaps", "matrix")
    failed(lib, mvm(lib, r=arr(addr(6), addr(0) + 128 * 256 // 2 - 1)), "clm4_mvm_v8_transposed_batch", "overlaps", "matrix")
    failed(lib, mvm(lib, r=arr(addr(6), addr(6))), "clm4_mvm_v8_transposed_batch", "overlaps", "vector 0", "vector 1")      # two equal outputs
    failed(lib, mvm(lib, sr=arr(addr(8), addr(8))), "clm4_mvm_v8_transposed_batch", "overlaps")
    failed(lib, at(lib, r=arr(addr(6), addr(2))), "clm4_mvm_v8_transposed_batch_at", "overlaps", "vector 0", "vector 1")
    failed(lib, at(lib, r=arr(addr(6), addr(0))), "clm4_mvm_v8_transposed_batch_at", "overlaps", "matrix")
    failed(lib, at(lib, rng=None, r=arr(addr(6), addr(2))), "clm4_mvm_v8_transposed_batch_at", "overlaps")     # also without a generator
    failed(lib, fused(lib, t=arr(addr(14), addr(7))), "clm4_mvm_v8_transposed_scale_and_add_batch", "overlaps")
    failed(lib, fused(lib, r=arr(addr(6), addr(10))), "clm4_mvm_v8_transposed_scale_and_add_batch", "overlaps")   # r[1] == qu[0]: not the in-place form
    failed(lib, fused(lib, r=arr(addr(6), addr(2))), "clm4_mvm_v8_transposed_scale_and_add_batch", "overlaps")    # r[1] == x[0]
    failed(lib, fused(lib, r=arr(addr(6), addr(0) + 4096)), "clm4_mvm_v8_transposed_scale_and_add_batch", "overlaps", "matrix")
    failed(lib, iht(lib, t3=arr(addr(36), addr(20))), "clm4_iht_v8_batch_one_matrix", "overlaps")              # t3[1] == x[0]
    failed(lib, iht(lib, t1=arr(addr(28), addr(24))), "clm4_iht_v8_batch_one_matrix", "overlaps")              # t1[1] == y[0]
    failed(lib, iht(lib, x=arr(addr(20), addr(20))), "clm4_iht_v8_batch_one_matrix", "overlaps")
    failed(lib, iht(lib, t2=arr(addr(32), addr(0))), "clm4_iht_v8_batch_one_matrix", "overlaps", "matrix")
    assert lib.clv_mvm_batch_launches() == before


def test_repeated_inputs_and_the_in_place_form_pass_validation(lib):
    # rows == 0: everything is checked (the results keep their cols bytes), nothing runs
    assert mvm(lib, rows=0, x=arr(addr(2), addr(2)), sx=arr(addr(4), addr(4))) == 0
    assert at(lib, rows=0, x=arr(addr(2), addr(2)), sx=arr(addr(4), addr(4))) == 0
    assert fused(lib, rows=0, qu=arr(addr(10), addr(10)), su=arr(addr(12), addr(12))) == 0
    assert fused(lib, rows=0, r=arr(addr(10), addr(11)), sr=arr(addr(12), addr(13))) == 0                  # r[j] == qu[j], sr[j] == su[j]
    # the same in-place call is refused only for a reason of its own: here vector 1's qu is vector 0's in-place result
    failed(lib, fused(lib, r=arr(addr(10), addr(7)), sr=arr(addr(12), addr(9)), qu=arr(addr(10), addr(10)), su=arr(addr(12), addr(12))),
           "clm4_mvm_v8_transposed_scale_and_add_batch", "overlaps")
    # r[j] == qu[j] alone (sr[j] != su[j]) is not the in-place form
    failed(lib, fused(lib, rows=0, r=arr(addr(10), addr(11))), "clm4_mvm_v8_transposed_scale_and_add_batch", "overlaps")


def test_the_position_limit(lib):
    """256 columns: a window is 2 G = 8 draws.  The end of every window and the commit stay below 2^55; the message names the first vector beyond"""
    fn, lim = "clm4_mvm_v8_transposed_batch_at", 1 << 55
    before = lib.clv_mvm_batch_launches()
    failed(lib, at(lib, base=lim), fn, "2^55", "vector 0")
    failed(lib, at(lib, base=lim - 7), fn, "2^55", "vector 0")
    failed(lib, at(lib, base=lim - 16, stride=9), fn, "2^55", "vector 1")
    failed(lib, at(lib, base=0, stride=lim), fn, "2^55", "vector 1")
    failed(lib, at(lib, base=(1 << 64) - 1, stride=(1 << 64) - 1), fn, "2^55", "vector 0")      # no wrap-around
    failed(lib, at(lib, commit=lim), fn, "2^55", "commit_draws")
    # the window is sized by the COLUMNS: 128 rows x 256 columns at lim - 8 is legal, 256 rows x 128 columns would be too
    assert at(lib, rows=0, base=lim - 8, stride=0, commit=lim - 1) == 0
    assert at(lib, rows=0, rng=None, base=lim, stride=lim, commit=lim) == 0
    assert lib.clv_mvm_batch_launches() == before


# ---------------------------------------------------------------- the CPU reference of the GPU tests
@pytest.mark.parametrize("rows,cols", [(128, 128), (256, 128), (128, 256)], ids=lambda v: str(v))
def test_the_cpu_reference_tells_the_failure_modes_apart(oracle, rows, cols):
    """oracle.m4_transpose + oracle.m4_mvm_v8 + oracle.v8_scale_and_add per vector, on the data of mvm_v8_transposed_batch_data.py:
    vectors swapped, a window one draw off and the scale grid read transposed each give other bytes"""
    D = data(oracle, rows, cols)
    nib = np.stack([D.qA >> 4, D.qA & 0xF], axis=1).reshape(rows, cols).astype(np.int8)      # even elements in the high nibble
    A = np.where(nib > 7, nib - 16, nib)
    assert rows != cols or not np.array_equal(A, A.T), "a symmetric matrix hides a forgotten transposition"
    assert np.unique(D.sA).size == D.sA.size, "equal tile scales hide sA[cb][b] read for sA[b][cb]"
    assert not np.any(A[:64, :64]) and not np.any(A[:, cols - 64:]), "the zero tile, the all-zero column group"
    assert A.min() == -7 and A.max() == 7
    t = [D.t(j) for j in range(NVMAX)]
    for j in range(NVMAX):
        assert t[j][0].size == cols and t[j][1].size == cols // 64
        assert not np.any(t[j][0][-64:]) and t[j][1][-1] == 1.0, "the zero column group gives a zero block of scale 1"
    assert not np.any(D.x[1][0]) and not np.any(t[1][0]) and np.all(t[1][1] == 1.0), "the all-zero vector"
    assert D.x[2] is D.x[0] and eq(t[2], t[0]), "the repeated input"
    distinct = [j for j in range(NVMAX) if j != 2]
    for i in distinct:
        for j in distinct:
            assert i == j or not same(t[i][0], t[j][0]), f"vectors {i} and {j} give the same result: a slot mix-up would not show"
    for j in (0, 1, 5):
        r = D.r(j)
        assert not eq(r, t[j]) and (j == 1 or not eq(r, D.u[j])), "the fused result differs from both of its operands (u + a * 0 is u)"
        assert eq(r, oracle.v8_scale_and_add(*D.u[j], *t[j], A_FUSED))
    # the scale grid read transposed (sA[cb][b] for sA[b][cb]): A's own grid, untransposed, in the place of the stored transpose's
    if rows // 64 > 1 or cols // 64 > 1:
        assert not same(D.sA, D.At[1])
        assert not eq(oracle.m4_mvm_v8(D.At[0], D.sA, cols, rows, *D.x[0]), t[0]), "a transposed scale grid gives the same bytes"
    # a window one draw off: the same call from a generator moved by one draw gives other bytes
    o0, o1 = oracle.rng(*KEYS), oracle.rng(*KEYS)
    oracle.rng_draw(o1)
    assert not eq(oracle.m4_mvm_v8(*D.At, cols, rows, *D.x[0], o0), oracle.m4_mvm_v8(*D.At, cols, rows, *D.x[0], o1)), "one draw off gives the same bytes"
    assert not keys_equal(Oracle.rng_keys(o0), Oracle.rng_keys(o1))
    if rows != cols:
        wrong = oracle.m4_mvm_v8(D.qA, D.sA, rows, cols, *D.u[0])                  # A u instead of A' x: another length altogether
        assert wrong[0].size == rows != t[0][0].size
