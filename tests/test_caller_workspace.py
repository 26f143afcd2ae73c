"""Every function of the C ABI that takes a `workspace`, given one: a scratch region of EXACTLY the bytes its query function returns, at a
256-byte boundary of a guarded arena (tests/guarded.py, the harness of tests/test_guard_bands.py).  Everywhere else in the repository the
argument is NULL and the work runs in the library's grow-only scratch, which only grows and keeps the leftovers of earlier calls: a size
formula that is short, or a kernel that relies on what the scratch holds, cannot show there.

Each case runs twice, with the workspace prefilled with 0x00 and with 0xFF (NaN as floats, huge as counters): both runs equal the CPU
reference bit for bit -- the header's "no initialisation" -- and the guards, the inputs and the padding behind n survive.  A formula
that returns too little writes into the guard behind the region and is reported with its offset.

What a pass proves is the contract as published: the kernels stay inside the bytes the query returns.  Every formula ends in 256 or
512 bytes of slack behind its layout terms (threshold4.hip, vector4.hip), and the region includes that slack, so a pass does NOT prove
that the layout terms alone are tight -- only that terms plus slack are enough for every form run here."""
import re

import numpy as np
import pytest

from clover_amd.build import repo_root
from clover_amd.lib_binding import DOT_EXACT, DOT_FAST, THRESHOLD_FAST, THRESHOLD_REFERENCE
from half16_helpers import rh  # noqa: F401
from matrix8_helpers import m8  # noqa: F401
import test_guard_bands as G
from test_guard_bands import CAND, HEAP, KS, SIX, refs, run_case, threshold_name, v4, v8  # noqa: F401

CASES = {}


def case(name):
    def reg(build):
        assert name not in CASES, name
        CASES[name] = build
        return build
    return reg


# ---------------------------------------------------------------- dots (the builders of test_guard_bands.py, with a workspace)
def _dot(fn, n, data, mode, exact, fast):
    return G._dot(fn, n, data, mode, exact, fast, ws=lambda L: getattr(L, fn + "_workspace_bytes")(n))


def _dot16(n, mode):
    def ws_bytes(L):
        assert L.clv_f16_dot_workspace_bytes(n) == 0
        return 0                                                            # a pointer with nothing behind it but guard
    return G._f16_vec("dot", n, mode=mode, ws=ws_bytes)


# the chain kernel of the EXACT dots walks blocks of 16 fma steps, DOTX_D = 10 blocks per loop iteration, and reads one iteration past the
# end: a step is a block pair (128 elements) for 4 bits and a block (64 elements) for 8, so the padding unit is 20480 / 10240 elements
for _n in (128, 20480 - 128, 20480, 20480 + 128, 99968):
    case(f"clv4_dot EXACT n_pad={_n}")(_dot("clv4_dot", _n, v4, DOT_EXACT, lambda R: R.oracle.v4_dot, None))
for _n in (128, 10240 - 128, 10240, 10240 + 128, 99968):
    case(f"clv8_dot EXACT n_pad={_n}")(_dot("clv8_dot", _n, v8, DOT_EXACT, lambda R: R.oracle.v8_dot, None))
for _n in (128, 99968):
    case(f"clv4_dot FAST n_pad={_n}")(_dot("clv4_dot", _n, v4, DOT_FAST, None, lambda hip: hip.v4_dot))
    case(f"clv8_dot FAST n_pad={_n}")(_dot("clv8_dot", _n, v8, DOT_FAST, None, lambda hip: hip.v8_dot))
    for _m, _mn in ((DOT_EXACT, "EXACT"), (DOT_FAST, "FAST")):
        case(f"clv_f16_dot {_mn} n_pad={_n}")(_dot16(_n, _m))


# ---------------------------------------------------------------- thresholds
def _threshold(bits, mode, n_pad, n, k_of, ws_bytes, env=None, plain=False, untouched=False):
    return G._threshold(bits, mode, n_pad, k_of, env=env, plain=plain, n=n, ws=ws_bytes, untouched=untouched)


FAST_WS = {4: lambda L, n_pad, k: L.clv4_threshold_workspace_bytes(n_pad), 8: lambda L, n_pad, k: L.clv8_threshold_workspace_bytes(n_pad),
           16: lambda L, n_pad, k: L.clv_f16_threshold_workspace_bytes(n_pad)}


def ref_ws_k(L, n_pad, k):
    return L.clv_threshold_reference_workspace_bytes_k(n_pad, k)


def ref_ws_any(L, n_pad, k):
    return L.clv_threshold_reference_workspace_bytes(n_pad)


# 4-bit FAST beyond one workgroup: the three-launch form (candidate words in registers, and through the workspace), the six-launch form
for _pad in (131072 + 128, 1 << 18):
    for _kn, _kf in KS.items():
        case(f"clv4_threshold n_pad={_pad} k={_kn} three launches")(_threshold(4, THRESHOLD_FAST, _pad, _pad - 37, _kf, FAST_WS[4], plain=True))
        case(f"clv4_threshold_mode FAST n_pad={_pad} k={_kn} candidate words through memory")(
            _threshold(4, THRESHOLD_FAST, _pad, _pad - 37, _kf, FAST_WS[4], env=CAND))
        case(f"clv4_threshold_mode FAST n_pad={_pad} k={_kn} six launches")(_threshold(4, THRESHOLD_FAST, _pad, _pad - 37, _kf, FAST_WS[4], env=SIX))
for _pad, _n in ((32768 + 128, 32768 + 128 - 37), (65536, 65536 - 37)):
    for _kn, _kf in KS.items():
        case(f"clv8_threshold n_pad={_pad} k={_kn}")(_threshold(8, THRESHOLD_FAST, _pad, _n, _kf, FAST_WS[8], plain=True))
    case(f"clv8_threshold_mode FAST n_pad={_pad} k=n/4")(_threshold(8, THRESHOLD_FAST, _pad, _n, KS["n/4"], FAST_WS[8]))
for _pad in (128, 8192 + 128):
    for _kn, _kf in KS.items():
        case(f"clv_f16_threshold_mode FAST n_pad={_pad} k={_kn}")(_threshold(16, THRESHOLD_FAST, _pad, _pad - 37, _kf, FAST_WS[16]))
# one workgroup: the kernel works in LDS and registers, the workspace is left alone
case("clv4_threshold n_pad=131072 k=n/4 one workgroup")(_threshold(4, THRESHOLD_FAST, 131072, 131072 - 37, KS["n/4"], FAST_WS[4], plain=True, untouched=True))
case("clv8_threshold n_pad=32768 k=n/4 one workgroup")(_threshold(8, THRESHOLD_FAST, 32768, 32768 - 37, KS["n/4"], FAST_WS[8], plain=True, untouched=True))
# REFERENCE mode and the heap forms: the heap lives in LDS up to k = 20000 (no heap region in the size), in the workspace beyond
for _bits in (4, 8, 16):
    for _mode in (THRESHOLD_REFERENCE, HEAP):
        _nm = threshold_name(_bits, _mode)
        case(f"{_nm} n_pad=4096 k=512 workspace for this k")(_threshold(_bits, _mode, 4096, 4096 - 37, lambda n: 512, ref_ws_k))
        case(f"{_nm} n_pad=32768 n=32765 k=20001 workspace for this k")(_threshold(_bits, _mode, 32768, 32765, lambda n: 20001, ref_ws_k))
        case(f"{_nm} n_pad=4096 k=512 workspace for any k")(_threshold(_bits, _mode, 4096, 4096 - 37, lambda n: 512, ref_ws_any))


# ================================================================ the tests
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_call_on_an_exact_uninitialised_workspace(hip, refs, name):  # noqa: F811
    c = CASES[name](refs)
    zero = run_case(hip, c, seed=11, scratch_fill=0x00)
    ones = run_case(hip, c, seed=11, scratch_fill=0xFF)
    for region in zero:
        if region != "ws":
            assert np.array_equal(zero[region], ones[region]), (region, "the result depends on what the workspace held")


def _header_functions():
    text = (repo_root() / "include" / "clover_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(\w+)\s*\(([^;{]*)\)\s*;", text)}


def test_the_case_list_covers_every_entry_point_with_a_workspace():
    takes = {name for name, params in _header_functions().items() if re.search(r"\bvoid\s*\*\s*workspace\b", params)}
    assert len(takes) == 11, takes
    assert takes == {c.split()[0] for c in CASES}


# ---------------------------------------------------------------- the alignment rule, without a device
def test_a_misaligned_workspace_is_rejected_before_anything_touches_the_device():
    """integer pointers: the argument checks answer before any pointer is used (test_f16_argument_checks_answer_without_a_device)"""
    from clover_amd.lib_binding import load_library
    lib = load_library()
    err = lambda: lib.clv_last_error().decode()                                # noqa: E731
    for ws in (4096 + 8, 4096 + 4, 4096 + 1):
        calls = {
            "clv4_dot": lambda: lib.clv4_dot(16, 16, 32, 32, 128, 0, 48, ws, None),
            "clv8_dot": lambda: lib.clv8_dot(16, 16, 32, 32, 128, 1, 48, ws, None),
            "clv_f16_dot": lambda: lib.clv_f16_dot(16, 32, 128, 0, 48, ws, None),
            "clv4_threshold": lambda: lib.clv4_threshold(16, 32, 100, 128, 10, ws, None),
            "clv4_threshold_mode": lambda: lib.clv4_threshold_mode(16, 32, 100, 128, 10, 1, ws, None),
            "clv4_threshold_heap": lambda: lib.clv4_threshold_heap(16, 32, 100, 128, 10, 48, ws, None),
            "clv8_threshold": lambda: lib.clv8_threshold(16, 32, 100, 128, 10, ws, None),
            "clv8_threshold_mode": lambda: lib.clv8_threshold_mode(16, 32, 100, 128, 10, 1, ws, None),
            "clv8_threshold_heap": lambda: lib.clv8_threshold_heap(16, 32, 100, 128, 10, 48, ws, None),
            "clv_f16_threshold_mode": lambda: lib.clv_f16_threshold_mode(16, 100, 128, 10, 0, ws, None),
            "clv_f16_threshold_heap": lambda: lib.clv_f16_threshold_heap(16, 100, 128, 10, 48, ws, None),
        }
        assert set(calls) == {name for name, params in _header_functions().items() if "workspace" in params}
        for name, call in calls.items():
            assert call() == -1 and f"{name}: workspace must be 16-byte aligned" in err(), (name, ws, err())
    # the FAST modes of the _mode forms pass the workspace on: rejected there too
    assert lib.clv4_threshold_mode(16, 32, 100, 128, 10, 0, 4104, None) == -1 and "workspace must be 16-byte aligned" in err()
    assert lib.clv8_threshold_mode(16, 32, 100, 128, 10, 0, 4104, None) == -1 and "workspace must be 16-byte aligned" in err()
    # the other argument checks still answer first or alike, and an aligned workspace with nothing to do is accepted
    assert lib.clv4_threshold(16, 32, 200, 128, 10, 4104, None) == -1 and "n=200" in err()
    assert lib.clv4_threshold(16, 32, 100, 128, 100, 4096, None) == 0           # k >= n: everything survives, no device work
    assert lib.clv_f16_threshold_mode(16, 100, 128, 100, 0, 4096, None) == 0
