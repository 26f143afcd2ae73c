"""clm8_mvm_transposed, clm8_mvm_transposed_scale_and_add and clm8_iht_one_matrix without a GPU: declared, exported and bound with the
right arity and the argument lists of clm8_mvm, clm8_mvm_scale_and_add and clm8_iht minus the PhiT pair; a C99 client compiles with
-pedantic -Werror, links and gets CLV_ERR_INVALID from bad calls; every argument check runs before any device work and names the call;
rows == 0 or cols == 0 returns CLV_OK.  The addresses are fake and never dereferenced: a call that passes validation here has an empty
matrix, so nothing runs.  A CloverVector8 of n elements is n bytes, so x (rows = 128) ends 128 bytes behind its address; a CloverMatrix8
of rows x cols is rows * cols bytes."""
import ctypes as C
import re
import subprocess

import pytest

from clover_amd.build import build_hip_library, repo_root
from clover_amd.lib_binding import SIGNATURES, CloverHip, load_library
from test_mvm_batch_cpu import addr, failed

NEW = {"clm8_mvm_transposed": 10, "clm8_mvm_transposed_scale_and_add": 15, "clm8_iht_one_matrix": 21}
PLAIN, FUSED, LOOP = NEW


@pytest.fixture(scope="module")
def lib():
    return load_library()


def test_the_three_calls_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", (repo_root() / "include" / "clover_hip.h").read_text(), flags=re.S)
    raw = C.CDLL(str(build_hip_library()))
    for name, arity in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared in clover_hip.h"
        assert len(m.group(1).split(",")) == arity, name
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in SIGNATURES and len(SIGNATURES[name][1]) == arity, name
    assert SIGNATURES[FUSED][1] == SIGNATURES["clm8_mvm_scale_and_add"][1] and SIGNATURES[PLAIN][1] == SIGNATURES["clm8_mvm"][1]
    iht = SIGNATURES["clm8_iht"][1]
    assert SIGNATURES[LOOP][1] == iht[:2] + iht[4:], "clm8_iht without the PhiT / sPhiT pair"
    for method in ("m8_mvm_transposed", "m8_mvm_transposed_scale_and_add", "m8_iht"):
        assert callable(getattr(CloverHip, method))


def test_a_c99_client_compiles_links_and_gets_the_argument_checks(tmp_path):
    lib = build_hip_library()
    exe = tmp_path / "m8_mvm_transposed_from_c"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{repo_root() / 'include'}",
                    str(repo_root() / "tests" / "c" / "m8_mvm_transposed_from_c.c"), "-o", str(exe), f"-L{lib.parent}", "-lclover_hip",
                    f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "ok=1" in p.stdout, (p.returncode, p.stdout, p.stderr)


P = dict(A=addr(0), sA=addr(1), x=addr(2), sx=addr(3), qu=addr(4), su=addr(5), t=addr(6), st=addr(7), r=addr(8), sr=addr(9))


def plain(lib, rows=128, cols=128, **kw):
    p = dict(P, **kw)
    return lib.clm8_mvm_transposed(p["A"], p["sA"], rows, cols, p["x"], p["sx"], p["r"], p["sr"], None, None)


def fused(lib, rows=128, cols=128, **kw):
    p = dict(P, **kw)
    return lib.clm8_mvm_transposed_scale_and_add(p["A"], p["sA"], rows, cols, p["x"], p["sx"], p["qu"], p["su"], 0.5, p["t"], p["st"], p["r"],
                                                 p["sr"], None, None)


LOOP_NAMES = ("Phi", "sPhi", "x", "sx", "y", "sy", "t1", "st1", "t2", "st2", "t3", "st3")


def loop(lib, m=128, n=128, x_len=128, **kw):
    p = {k: addr(20 + i) for i, k in enumerate(LOOP_NAMES)}
    p.update(kw)
    return lib.clm8_iht_one_matrix(p["Phi"], p["sPhi"], m, n, p["x"], p["sx"], x_len, p["y"], p["sy"], p["t1"], p["st1"], p["t2"], p["st2"],
                                   p["t3"], p["st3"], 3, 8, 0.5, 1, None, None)


def test_sizes_must_be_multiples_of_128(lib):
    for call, name in ((plain, PLAIN), (fused, FUSED)):
        failed(lib, call(lib, rows=64), name + ":", "multiples of 128")
        failed(lib, call(lib, cols=192), name + ":", "multiples of 128")
        failed(lib, call(lib, rows=100), name + ":", "rows=100")
    failed(lib, loop(lib, m=64), LOOP, "m=64")
    failed(lib, loop(lib, n=192), LOOP, "n=192")
    failed(lib, loop(lib, x_len=129), LOOP, "x_len")


def test_every_null_pointer_is_refused(lib):
    for k in ("A", "sA", "x", "sx", "r", "sr"):
        failed(lib, plain(lib, **{k: None}), PLAIN + ":", "null pointer")
        failed(lib, fused(lib, **{k: None}), FUSED + ":", "null pointer")
    for k in ("qu", "su"):
        failed(lib, fused(lib, **{k: None}), FUSED + ":", "null pointer")
    for k in LOOP_NAMES:
        failed(lib, loop(lib, **{k: None}), LOOP + ":", "null pointer")
    # also with an empty matrix: the pointers are checked first
    failed(lib, plain(lib, rows=0, r=None), PLAIN + ":", "null pointer")
    failed(lib, fused(lib, cols=0, su=None), FUSED + ":", "null pointer")


def test_t_and_st_come_together(lib):
    failed(lib, fused(lib, st=None), FUSED + ":", "t and st")
    failed(lib, fused(lib, t=None), FUSED + ":", "t and st")
    assert fused(lib, rows=0, t=None, st=None) == 0


def test_outputs_may_not_overlap_the_inputs_nor_each_other(lib):
    failed(lib, plain(lib, r=P["x"]), PLAIN + ":", "overlaps", "`x`")
    failed(lib, plain(lib, r=P["x"] + 127), PLAIN + ":", "overlaps")                # by one byte: x has rows = 128 bytes
    assert plain(lib, rows=0, r=P["x"] + 128) == 0
    failed(lib, plain(lib, r=P["x"] - 127), PLAIN + ":", "overlaps")                # by one byte: r has cols = 128 bytes
    failed(lib, plain(lib, r=P["A"]), PLAIN + ":", "overlaps", "matrix")
    failed(lib, plain(lib, sr=P["sA"] + 12), PLAIN + ":", "overlaps", "`sA`")
    failed(lib, plain(lib, sr=P["sx"]), PLAIN + ":", "overlaps", "`sx`")
    failed(lib, plain(lib, sr=P["sx"] + 7), PLAIN + ":", "overlaps")                # the last byte of sx (two floats)
    # A is rows * cols bytes, twice a CloverMatrix4's: its last byte, and the byte in front of it
    failed(lib, plain(lib, rows=256, cols=128, r=P["A"] + 256 * 128 - 1), PLAIN + ":", "overlaps")
    failed(lib, plain(lib, rows=256, cols=128, r=P["A"] + 256 * 64), PLAIN + ":", "overlaps")         # inside the second half of A
    failed(lib, plain(lib, rows=256, cols=128, r=P["A"] - 127), PLAIN + ":", "overlaps")
    failed(lib, fused(lib, rows=256, cols=128, r=P["A"] + 256 * 128 - 1), FUSED + ":", "overlaps")
    failed(lib, fused(lib, r=P["x"]), FUSED + ":", "overlaps")
    failed(lib, fused(lib, r=P["A"]), FUSED + ":", "overlaps")
    failed(lib, fused(lib, t=P["x"]), FUSED + ":", "overlaps")
    failed(lib, fused(lib, t=P["r"]), FUSED + ":", "overlaps")
    failed(lib, fused(lib, t=P["r"] + 127), FUSED + ":", "overlaps")
    failed(lib, fused(lib, t=P["qu"]), FUSED + ":", "overlaps")                     # the in-place exception covers r == qu only
    failed(lib, fused(lib, r=P["qu"] + 1), FUSED + ":", "overlaps")                 # overlapping, not in place
    failed(lib, fused(lib, r=P["qu"] + 127), FUSED + ":", "overlaps")


def test_empty_matrices_return_ok(lib):
    assert plain(lib, rows=0) == 0 and plain(lib, cols=0) == 0
    assert fused(lib, rows=0) == 0 and fused(lib, cols=0) == 0
    assert fused(lib, rows=0, r=P["qu"], sr=P["su"]) == 0                           # the in-place form passes validation
