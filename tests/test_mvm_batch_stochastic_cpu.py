"""clm4_mvm_batch_at and clv_mvm_batch_launches without a GPU: declared, exported and bound with the right arity; a C99 client compiles with
-pedantic and links; the argument checks of the positioned call (NULL entries, overlap, the position limit) answer CLV_ERR_INVALID before
any device work, with the vector index in clv_last_error.  The addresses are fake and never dereferenced (test_mvm_batch_cpu.py).  Also the
GF(2) power the GPU tests move the generator with (tests/gf2.py) against burnt draws of the oracle."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import gf2
from clover_amd.build import build_hip_library, repo_root
from clover_amd.lib_binding import SIGNATURES, load_library
from oracle.binding import Oracle
from test_mvm_batch_cpu import addr, arr, failed

NEW = {"clm4_mvm_batch_at": 14, "clv_mvm_batch_launches": 1}          # a (void) parameter list splits into one piece
RNG = addr(60)


@pytest.fixture(scope="module")
def lib():
    return load_library()


def test_the_two_calls_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", (repo_root() / "include" / "clover_hip.h").read_text(), flags=re.S)
    raw = C.CDLL(str(build_hip_library()))
    for name, arity in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared in clover_hip.h"
        params = [p for p in m.group(1).split(",")]
        assert len(params) == arity, name
        assert hasattr(raw, name), f"{name} is not exported"
        want = 0 if params == ["void"] else arity
        assert name in SIGNATURES and len(SIGNATURES[name][1]) == want, name
    assert SIGNATURES["clv_mvm_batch_launches"][0] is C.c_uint64


def test_a_c99_client_compiles_links_and_gets_the_argument_checks(tmp_path):
    lib = build_hip_library()
    exe = tmp_path / "mvm_batch_at_from_c"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{repo_root() / 'include'}",
                    str(repo_root() / "tests" / "c" / "mvm_batch_at_from_c.c"), "-o", str(exe), f"-L{lib.parent}", "-lclover_hip",
                    f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "ok=1" in p.stdout, (p.returncode, p.stdout, p.stderr)


def at(lib, rows=128, cols=128, nvec=2, x=None, sx=None, r=None, sr=None, rng=RNG, base=0, stride=4, commit=8):
    x = x or arr(addr(2), addr(3))
    sx = sx or arr(addr(4), addr(5))
    r = r or arr(addr(6), addr(7))
    sr = sr or arr(addr(8), addr(9))
    return lib.clm4_mvm_batch_at(addr(0), addr(1), rows, cols, nvec, x, sx, r, sr, rng, base, stride, commit, None)


def test_the_checks_of_clm4_mvm_batch(lib):
    fn = "clm4_mvm_batch_at"
    failed(lib, at(lib, rows=100), fn, "multiple of 64")
    failed(lib, at(lib, sr=arr(addr(8), None)), fn, "vector 1")
    failed(lib, at(lib, x=arr(None, addr(3))), fn, "vector 0")
    failed(lib, lib.clm4_mvm_batch_at(addr(0), addr(1), 128, 128, 2, None, None, None, None, RNG, 0, 4, 8, None), fn, "null pointer array")
    failed(lib, at(lib, r=arr(addr(6), addr(2))), fn, "overlaps", "vector 0", "vector 1")
    failed(lib, at(lib, r=arr(addr(6), addr(6))), fn, "overlaps", "vector 0", "vector 1")
    failed(lib, at(lib, r=arr(addr(6), addr(0))), fn, "overlaps", "matrix")
    failed(lib, at(lib, rng=None, r=arr(addr(6), addr(2))), fn, "overlaps")           # also without a generator
    assert at(lib, nvec=0) == 0 and at(lib, rows=0) == 0
    assert at(lib, rows=0, x=arr(addr(2), addr(2)), sx=arr(addr(4), addr(4))) == 0    # repeated inputs pass


def test_the_position_limit(lib):
    """128 rows: a window is 4 draws.  The end of every window and the commit stay below 2^55; the message names the first vector beyond"""
    fn, lim = "clm4_mvm_batch_at", 1 << 55
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


@pytest.mark.parametrize("e", [0, 1, 2, 7, 1000])
def test_the_gf2_power_moves_the_keys_like_burnt_draws(oracle, e):
    o = oracle.rng(777, 4242)
    fresh = Oracle.rng_keys(o)
    for _ in range(e):
        oracle.rng_draw(o)
    want, got = Oracle.rng_keys(o), gf2.advance_keys(fresh, e)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    a = int(fresh[1][0])
    assert gf2.apply(gf2.power((1 << 40) + 3), a) == gf2.apply(gf2.power(3), gf2.apply(gf2.power(1 << 40), a))
