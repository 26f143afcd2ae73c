"""The batch calls of the pure 8-bit path (clm8_mvm_batch, clm8_mvm_batch_at, clm8_mvm_scale_and_add_batch, clm8_iht_batch) without a GPU:
they are declared, exported and bound, a C99 client compiles with -pedantic and links, and every argument check runs before any device work
-- a bad call returns CLV_ERR_INVALID with a message that names the call (and the vector index where there is one) on a machine that has
no device.  The pointer arrays are HOST arrays of device pointers; the addresses below are never dereferenced (a call that passes
validation has rows == 0 or nvec == 0, so nothing runs).  The matrix is rows x cols BYTES, a vector of n elements n bytes."""
import ctypes as C
import re
import subprocess

import pytest

from clover_amd.build import build_hip_library, repo_root
from clover_amd.lib_binding import SIGNATURES, load_library
from test_mvm_batch_cpu import DEFAULT, addr, arr, failed

BATCH = {"clm8_mvm_batch": 11, "clm8_mvm_batch_at": 14, "clm8_mvm_scale_and_add_batch": 16, "clm8_iht_batch": 24}
RNG = addr(60)


@pytest.fixture(scope="module")
def lib():
    return load_library()


def test_the_four_calls_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", (repo_root() / "include" / "clover_hip.h").read_text(), flags=re.S)
    raw = C.CDLL(str(build_hip_library()))
    for name, arity in BATCH.items():
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared in clover_hip.h"
        assert len(m.group(1).split(",")) == arity, name
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in SIGNATURES and len(SIGNATURES[name][1]) == arity, name


def test_a_c99_client_compiles_links_and_gets_the_argument_checks(tmp_path):
    lib = build_hip_library()
    exe = tmp_path / "m8_mvm_batch_from_c"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{repo_root() / 'include'}",
                    str(repo_root() / "tests" / "c" / "m8_mvm_batch_from_c.c"), "-o", str(exe), f"-L{lib.parent}", "-lclover_hip",
                    f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "ok=1" in p.stdout, (p.returncode, p.stdout, p.stderr)


def mvm(lib, rows=128, cols=128, nvec=2, x=DEFAULT, sx=DEFAULT, r=DEFAULT, sr=DEFAULT, A=addr(0), sA=addr(1)):
    x = arr(addr(2), addr(3)) if x is DEFAULT else x
    sx = arr(addr(4), addr(5)) if sx is DEFAULT else sx
    r = arr(addr(6), addr(7)) if r is DEFAULT else r
    sr = arr(addr(8), addr(9)) if sr is DEFAULT else sr
    return lib.clm8_mvm_batch(A, sA, rows, cols, nvec, x, sx, r, sr, None, None)


def at(lib, rows=128, cols=128, nvec=2, x=None, sx=None, r=None, sr=None, rng=RNG, base=0, stride=4, commit=8):
    x = x or arr(addr(2), addr(3))
    sx = sx or arr(addr(4), addr(5))
    r = r or arr(addr(6), addr(7))
    sr = sr or arr(addr(8), addr(9))
    return lib.clm8_mvm_batch_at(addr(0), addr(1), rows, cols, nvec, x, sx, r, sr, rng, base, stride, commit, None)


def fused(lib, rows=128, cols=128, nvec=2, **kw):
    p = dict(x=arr(addr(2), addr(3)), sx=arr(addr(4), addr(5)), qu=arr(addr(10), addr(11)), su=arr(addr(12), addr(13)), t=arr(addr(14), addr(15)),
             st=arr(addr(16), addr(17)), r=arr(addr(6), addr(7)), sr=arr(addr(8), addr(9)))
    p.update(kw)
    return lib.clm8_mvm_scale_and_add_batch(addr(0), addr(1), rows, cols, nvec, p["x"], p["sx"], p["qu"], p["su"], 0.5, p["t"], p["st"], p["r"],
                                               p["sr"], None, None)


def iht(lib, m=128, n=128, nvec=2, x_len=128, **kw):
    names = ("x", "sx", "y", "sy", "t1", "st1", "t2", "st2", "t3", "st3")
    p = {k: arr(addr(20 + 2 * i), addr(21 + 2 * i)) for i, k in enumerate(names)}
    p.update(kw)
    return lib.clm8_iht_batch(addr(0), addr(1), addr(2), addr(3), m, n, nvec, p["x"], p["sx"], x_len, p["y"], p["sy"], p["t1"], p["st1"],
                                 p["t2"], p["st2"], p["t3"], p["st3"], 3, 8, 0.5, 1, None, None)


def test_nvec_zero_and_rows_zero_return_ok(lib):
    before = lib.clv_mvm_batch_launches()
    assert lib.clm8_mvm_batch(addr(0), addr(1), 128, 128, 0, None, None, None, None, None, None) == 0
    assert lib.clm8_mvm_batch_at(addr(0), addr(1), 128, 128, 0, None, None, None, None, RNG, 0, 4, 8, None) == 0
    assert lib.clm8_mvm_scale_and_add_batch(addr(0), addr(1), 128, 128, 0, None, None, None, None, 0.5, None, None, None, None, None, None) == 0
    assert iht(lib, nvec=0) == 0
    assert mvm(lib, rows=0) == 0 and at(lib, rows=0) == 0 and fused(lib, rows=0) == 0
    assert lib.clv_mvm_batch_launches() == before


def test_size_rules(lib):
    failed(lib, mvm(lib, rows=100), "clm8_mvm_batch", "multiple of 64")
    failed(lib, mvm(lib, cols=64), "clm8_mvm_batch", "multiple of 64")
    failed(lib, at(lib, rows=100), "clm8_mvm_batch_at", "multiple of 64")
    failed(lib, fused(lib, rows=96), "clm8_mvm_scale_and_add_batch", "multiple of 64")
    failed(lib, iht(lib, m=64), "clm8_iht_batch", "m=64")
    failed(lib, iht(lib, x_len=129), "clm8_iht_batch", "x_len")


def test_null_arrays_and_null_entries(lib):
    before = lib.clv_mvm_batch_launches()
    failed(lib, mvm(lib, x=None), "clm8_mvm_batch", "null pointer array")
    failed(lib, mvm(lib, sr=None), "clm8_mvm_batch", "null pointer array")
    failed(lib, mvm(lib, A=None), "clm8_mvm_batch", "null")
    failed(lib, mvm(lib, sr=arr(addr(8), None)), "clm8_mvm_batch", "vector 1")
    failed(lib, mvm(lib, x=arr(None, addr(3))), "clm8_mvm_batch", "vector 0")
    failed(lib, at(lib, sr=arr(addr(8), None)), "clm8_mvm_batch_at", "vector 1")
    failed(lib, lib.clm8_mvm_batch_at(addr(0), addr(1), 128, 128, 2, None, None, None, None, RNG, 0, 4, 8, None), "clm8_mvm_batch_at",
           "null pointer array")
    failed(lib, fused(lib, qu=None), "clm8_mvm_scale_and_add_batch", "null pointer array")
    failed(lib, fused(lib, su=arr(addr(12), None)), "clm8_mvm_scale_and_add_batch", "vector 1")
    failed(lib, fused(lib, t=arr(addr(14), None)), "clm8_mvm_scale_and_add_batch", "vector 1")
    failed(lib, iht(lib, t2=None), "clm8_iht_batch", "null pointer array")
    failed(lib, iht(lib, st3=arr(addr(38), None)), "clm8_iht_batch", "vector 1")
    assert lib.clv_mvm_batch_launches() == before


def test_t_and_st_come_together(lib):
    failed(lib, fused(lib, st=None), "clm8_mvm_scale_and_add_batch", "t and st")
    failed(lib, fused(lib, t=None), "clm8_mvm_scale_and_add_batch", "t and st")
    assert fused(lib, rows=0, t=None, st=None) == 0


def test_outputs_may_not_overlap_inputs_of_any_vector_nor_each_other(lib):
    before = lib.clv_mvm_batch_launches()
    # r of vector 1 is x of vector 0: another workgroup may still be reading it
    failed(lib, mvm(lib, r=arr(addr(6), addr(2))), "clm8_mvm_batch", "overlaps", "vector 0", "vector 1")
    # ... by one byte only: x has cols = 128 bytes
    failed(lib, mvm(lib, r=arr(addr(6), addr(2) + 127)), "clm8_mvm_batch", "overlaps")
    assert mvm(lib, rows=0, r=arr(addr(6), addr(2) + 128)) == 0
    # r has rows = 128 bytes: r[1] may begin right behind r[0], not one byte earlier
    failed(lib, mvm(lib, r=arr(addr(6), addr(6) + 127)), "clm8_mvm_batch", "overlaps")
    failed(lib, mvm(lib, sr=arr(addr(8), addr(4))), "clm8_mvm_batch", "overlaps")
    failed(lib, mvm(lib, sr=arr(addr(8), addr(8) + 4)), "clm8_mvm_batch", "overlaps")          # scales: rows / 64 * 4 = 8 bytes
    failed(lib, mvm(lib, r=arr(addr(6), addr(0))), "clm8_mvm_batch", "overlaps", "matrix")
    failed(lib, mvm(lib, r=arr(addr(6), addr(0) + 128 * 128 - 1)), "clm8_mvm_batch", "overlaps", "matrix")      # the matrix is 16384 bytes
    # two equal outputs
    failed(lib, mvm(lib, r=arr(addr(6), addr(6))), "clm8_mvm_batch", "overlaps", "vector 0", "vector 1")
    failed(lib, mvm(lib, sr=arr(addr(8), addr(8))), "clm8_mvm_batch", "overlaps")
    failed(lib, at(lib, r=arr(addr(6), addr(2))), "clm8_mvm_batch_at", "overlaps", "vector 0", "vector 1")
    failed(lib, at(lib, r=arr(addr(6), addr(0))), "clm8_mvm_batch_at", "overlaps", "matrix")
    failed(lib, at(lib, rng=None, r=arr(addr(6), addr(2))), "clm8_mvm_batch_at", "overlaps")           # also without a generator
    failed(lib, fused(lib, t=arr(addr(14), addr(7))), "clm8_mvm_scale_and_add_batch", "overlaps")
    failed(lib, fused(lib, r=arr(addr(6), addr(10))), "clm8_mvm_scale_and_add_batch", "overlaps")       # r[1] == qu[0]: not the in-place form
    failed(lib, fused(lib, r=arr(addr(6), addr(2))), "clm8_mvm_scale_and_add_batch", "overlaps")        # r[1] == x[0]
    failed(lib, fused(lib, r=arr(addr(6), addr(0) + 4096)), "clm8_mvm_scale_and_add_batch", "overlaps", "matrix")
    # the fused single call's rule, with the vector index: the result must not be the vector being multiplied
    failed(lib, fused(lib, r=arr(addr(6), addr(3))), "clm8_mvm_scale_and_add_batch", "alias", "vector 1")
    failed(lib, fused(lib, sr=arr(addr(4), addr(9))), "clm8_mvm_scale_and_add_batch", "alias", "vector 0")
    failed(lib, iht(lib, t3=arr(addr(36), addr(20))), "clm8_iht_batch", "overlaps")                     # t3[1] == x[0]
    failed(lib, iht(lib, t1=arr(addr(28), addr(24))), "clm8_iht_batch", "overlaps")                     # t1[1] == y[0]
    failed(lib, iht(lib, t1=arr(addr(28), addr(24) + 127)), "clm8_iht_batch", "overlaps")               # y is m = 128 bytes
    failed(lib, iht(lib, x=arr(addr(20), addr(20))), "clm8_iht_batch", "overlaps")
    failed(lib, iht(lib, t2=arr(addr(32), addr(0))), "clm8_iht_batch", "overlaps", "matrix")
    assert lib.clv_mvm_batch_launches() == before


def test_repeated_inputs_and_the_in_place_form_pass_validation(lib):
    # rows == 0: everything is checked, nothing runs
    assert mvm(lib, rows=0, x=arr(addr(2), addr(2)), sx=arr(addr(4), addr(4))) == 0
    assert at(lib, rows=0, x=arr(addr(2), addr(2)), sx=arr(addr(4), addr(4))) == 0
    assert fused(lib, rows=0, qu=arr(addr(10), addr(10)), su=arr(addr(12), addr(12))) == 0
    assert fused(lib, rows=0, r=arr(addr(10), addr(11)), sr=arr(addr(12), addr(13))) == 0                  # r[j] == qu[j], sr[j] == su[j]
    # with rows > 0 the same in-place call is refused only for a reason of its own: here vector 1's qu is vector 0's in-place result
    failed(lib, fused(lib, r=arr(addr(10), addr(7)), sr=arr(addr(12), addr(9)), qu=arr(addr(10), addr(10)), su=arr(addr(12), addr(12))),
           "clm8_mvm_scale_and_add_batch", "overlaps")
    # r[j] == qu[j] alone (sr[j] != su[j]) is not the in-place form
    failed(lib, fused(lib, r=arr(addr(10), addr(11))), "clm8_mvm_scale_and_add_batch", "overlaps")


def test_the_position_limit(lib):
    """128 rows: a window is 4 draws.  The end of every window and the commit stay below 2^55; the message names the first vector beyond"""
    fn, lim = "clm8_mvm_batch_at", 1 << 55
    before = lib.clv_mvm_batch_launches()
    failed(lib, at(lib, base=lim), fn, "2^55", "vector 0")
    failed(lib, at(lib, base=lim - 3), fn, "2^55", "vector 0")
    failed(lib, at(lib, base=lim - 8, stride=5), fn, "2^55", "vector 1")
    failed(lib, at(lib, base=0, stride=lim), fn, "2^55", "vector 1")
    failed(lib, at(lib, base=(1 << 64) - 1, stride=(1 << 64) - 1), fn, "2^55", "vector 0")      # no wrap-around
    failed(lib, at(lib, commit=lim), fn, "2^55", "commit_draws")
    # legal at the limit and without a generator: rows == 0, so that nothing runs
    assert at(lib, rows=0, base=lim, stride=0, commit=lim - 1) == 0
    assert at(lib, rows=0, rng=None, base=lim, stride=lim, commit=lim) == 0
    assert lib.clv_mvm_batch_launches() == before
