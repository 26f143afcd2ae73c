"""The batch calls (clm4_mvm_batch, clm4_mvm_scale_and_add_batch, clv4_threshold_batch, clm4_iht_batch) without a GPU: they are declared,
exported and bound, and every argument check runs before any device work -- a bad call returns CLV_ERR_INVALID with a message that names
the call (and the vector index where there is one) on a machine that has no device.  The pointer arrays are HOST arrays of device pointers;
the addresses below are never dereferenced (a call that passes validation has rows == 0 or nvec == 0, so nothing runs)."""
import ctypes as C
import re

import pytest

from clover_amd.build import build_hip_library, repo_root
from clover_amd.lib_binding import SIGNATURES, load_library

BATCH = {"clm4_mvm_batch": 11, "clm4_mvm_scale_and_add_batch": 16, "clv4_threshold_batch": 8, "clm4_iht_batch": 24}
BASE = 0x10000000          # fake device addresses, 1 MiB apart: far enough for every range of the shapes used here


DEFAULT = object()


def addr(i):
    return BASE + (i << 20)


def arr(*ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


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
    assert re.search(r"#define\s+CLM4_MVM_BATCH_MAX\s+8\b", text)


def mvm(lib, rows=128, cols=128, nvec=2, x=DEFAULT, sx=DEFAULT, r=DEFAULT, sr=DEFAULT, A=addr(0), sA=addr(1)):
    x = arr(addr(2), addr(3)) if x is DEFAULT else x
    sx = arr(addr(4), addr(5)) if sx is DEFAULT else sx
    r = arr(addr(6), addr(7)) if r is DEFAULT else r
    sr = arr(addr(8), addr(9)) if sr is DEFAULT else sr
    return lib.clm4_mvm_batch(A, sA, rows, cols, nvec, x, sx, r, sr, None, None)


def fused(lib, rows=128, cols=128, nvec=2, **kw):
    p = dict(x=arr(addr(2), addr(3)), sx=arr(addr(4), addr(5)), qu=arr(addr(10), addr(11)), su=arr(addr(12), addr(13)), t=arr(addr(14), addr(15)),
             st=arr(addr(16), addr(17)), r=arr(addr(6), addr(7)), sr=arr(addr(8), addr(9)))
    p.update(kw)
    return lib.clm4_mvm_scale_and_add_batch(addr(0), addr(1), rows, cols, nvec, p["x"], p["sx"], p["qu"], p["su"], 0.5, p["t"], p["st"], p["r"], p["sr"],
                                            None, None)


def iht(lib, m=128, n=128, nvec=2, x_len=128, **kw):
    names = ("x", "sx", "y", "sy", "t1", "st1", "t2", "st2", "t3", "st3")
    p = {k: arr(addr(20 + 2 * i), addr(21 + 2 * i)) for i, k in enumerate(names)}
    p.update(kw)
    return lib.clm4_iht_batch(addr(0), addr(1), addr(2), addr(3), m, n, nvec, p["x"], p["sx"], x_len, p["y"], p["sy"], p["t1"], p["st1"], p["t2"],
                              p["st2"], p["t3"], p["st3"], 3, 8, 0.5, 1, None, None)


def thr(lib, nvec=2, n=128, n_pad=128, k=128, mode=0, q=DEFAULT, s=DEFAULT):
    q = arr(addr(2), addr(3)) if q is DEFAULT else q
    s = arr(addr(4), addr(5)) if s is DEFAULT else s
    return lib.clv4_threshold_batch(q, s, nvec, n, n_pad, k, mode, None)


def failed(lib, rc, *words):
    msg = lib.clv_last_error()
    assert rc == -1, (rc, msg)
    for w in words:
        assert w.encode() in msg, (w, msg)


def test_nvec_zero_returns_ok(lib):
    assert lib.clm4_mvm_batch(addr(0), addr(1), 128, 128, 0, None, None, None, None, None, None) == 0
    assert lib.clm4_mvm_scale_and_add_batch(addr(0), addr(1), 128, 128, 0, None, None, None, None, 0.5, None, None, None, None, None, None) == 0
    assert lib.clv4_threshold_batch(None, None, 0, 128, 128, 4, 0, None) == 0
    assert iht(lib, nvec=0) == 0


def test_size_rules(lib):
    failed(lib, mvm(lib, rows=100), "clm4_mvm_batch", "multiple of 64")
    failed(lib, mvm(lib, cols=64), "clm4_mvm_batch", "multiple of 64")
    failed(lib, fused(lib, rows=96), "clm4_mvm_scale_and_add_batch", "multiple of 64")
    failed(lib, thr(lib, n_pad=192, n=100), "clv4_threshold_batch", "n_pad")
    failed(lib, thr(lib, n=129), "clv4_threshold_batch", "n_pad")
    failed(lib, thr(lib, mode=7), "clv4_threshold_batch", "mode")
    failed(lib, iht(lib, m=64), "clm4_iht_batch", "m=64")
    failed(lib, iht(lib, x_len=129), "clm4_iht_batch", "x_len")


def test_null_arrays_and_null_entries(lib):
    failed(lib, mvm(lib, x=None), "clm4_mvm_batch", "null pointer array")
    failed(lib, mvm(lib, sr=None), "clm4_mvm_batch", "null pointer array")
    failed(lib, mvm(lib, A=None), "clm4_mvm_batch", "null")
    failed(lib, mvm(lib, sr=arr(addr(8), None)), "clm4_mvm_batch", "vector 1")
    failed(lib, mvm(lib, x=arr(None, addr(3))), "clm4_mvm_batch", "vector 0")
    failed(lib, fused(lib, qu=None), "clm4_mvm_scale_and_add_batch", "null pointer array")
    failed(lib, fused(lib, su=arr(addr(12), None)), "clm4_mvm_scale_and_add_batch", "vector 1")
    failed(lib, fused(lib, t=arr(addr(14), None)), "clm4_mvm_scale_and_add_batch", "vector 1")
    failed(lib, thr(lib, k=4, q=None), "clv4_threshold_batch", "null pointer array")
    failed(lib, thr(lib, k=4, s=arr(addr(4), None)), "clv4_threshold_batch", "vector 1")
    failed(lib, iht(lib, t2=None), "clm4_iht_batch", "null pointer array")
    failed(lib, iht(lib, st3=arr(addr(38), None)), "clm4_iht_batch", "vector 1")


def test_t_and_st_come_together(lib):
    failed(lib, fused(lib, st=None), "clm4_mvm_scale_and_add_batch", "t and st")
    failed(lib, fused(lib, t=None), "clm4_mvm_scale_and_add_batch", "t and st")
    assert fused(lib, rows=0, t=None, st=None) == 0


def test_outputs_may_not_overlap_inputs_of_any_vector_nor_each_other(lib):
    # r of vector 1 is x of vector 0: another workgroup may still be reading it
    failed(lib, mvm(lib, r=arr(addr(6), addr(2))), "clm4_mvm_batch", "overlaps", "vector 0", "vector 1")
    # ... by one byte only (x has cols / 2 = 64 bytes)
    failed(lib, mvm(lib, r=arr(addr(6), addr(2) + 63)), "clm4_mvm_batch", "overlaps")
    failed(lib, mvm(lib, sr=arr(addr(8), addr(4))), "clm4_mvm_batch", "overlaps")
    failed(lib, mvm(lib, r=arr(addr(6), addr(0))), "clm4_mvm_batch", "overlaps", "matrix")
    # two equal outputs
    failed(lib, mvm(lib, r=arr(addr(6), addr(6))), "clm4_mvm_batch", "overlaps", "vector 0", "vector 1")
    failed(lib, mvm(lib, sr=arr(addr(8), addr(8))), "clm4_mvm_batch", "overlaps")
    failed(lib, fused(lib, t=arr(addr(14), addr(7))), "clm4_mvm_scale_and_add_batch", "overlaps")
    failed(lib, fused(lib, r=arr(addr(6), addr(10))), "clm4_mvm_scale_and_add_batch", "overlaps")          # r[1] == qu[0]: not the in-place form
    failed(lib, fused(lib, r=arr(addr(2), addr(7))), "clm4_mvm_scale_and_add_batch", "overlaps")           # the result may not be x
    failed(lib, thr(lib, k=4, q=arr(addr(2), addr(2))), "clv4_threshold_batch", "overlaps")
    failed(lib, thr(lib, k=4, s=arr(addr(4), addr(2))), "clv4_threshold_batch", "overlaps")
    failed(lib, iht(lib, t3=arr(addr(36), addr(20))), "clm4_iht_batch", "overlaps")                        # t3[1] == x[0]
    failed(lib, iht(lib, t1=arr(addr(28), addr(24))), "clm4_iht_batch", "overlaps")                        # t1[1] == y[0]
    failed(lib, iht(lib, x=arr(addr(20), addr(20))), "clm4_iht_batch", "overlaps")


def test_repeated_inputs_and_the_in_place_form_pass_validation(lib):
    # rows == 0: everything is checked, nothing runs
    assert mvm(lib, rows=0, x=arr(addr(2), addr(2)), sx=arr(addr(4), addr(4))) == 0
    assert fused(lib, rows=0, qu=arr(addr(10), addr(10)), su=arr(addr(12), addr(12))) == 0
    assert fused(lib, rows=0, r=arr(addr(10), addr(11)), sr=arr(addr(12), addr(13))) == 0                  # r[j] == qu[j], sr[j] == su[j]
    # with rows > 0 the same in-place call is refused only for a reason of its own: here vector 1's qu is vector 0's in-place result
    failed(lib, fused(lib, r=arr(addr(10), addr(7)), sr=arr(addr(12), addr(9)), qu=arr(addr(10), addr(10)), su=arr(addr(12), addr(12))),
           "clm4_mvm_scale_and_add_batch", "overlaps")
    assert thr(lib, s=arr(addr(4), addr(4))) == 0                                                          # k >= n: nothing to do
