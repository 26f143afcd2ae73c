"""Shared by the transposed half-precision mvm tests: the column-walk restatement (tests/half16_t_restate.c, which includes
half16_restate.c, so one library has both rt_* and rh_*), and per shape the references every GPU test compares with, computed once."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

from f16_transposed_data import A_VALUES, case
from half16_helpers import Restate, h16

RESTATE_T = Path(__file__).parent / "half16_t_restate.c"
RIGHT, ENDS_LEFT_TO_RIGHT, ONE_CHAIN, SIXTEEN_CHAINS = 0, 1, 2, 3
WRONG = {"chain ends left to right": ENDS_LEFT_TO_RIGHT, "one chain": ONE_CHAIN, "16 chains": SIXTEEN_CHAINS}

_u16 = C.POINTER(C.c_uint16)
_fp = C.POINTER(C.c_float)
_u64 = C.c_uint64


def _p(a, t):
    return a.ctypes.data_as(t)


class RestateT(Restate):
    """Restate (the rh_* row forms) plus the rt_* column walk"""

    def columns(self, A, rows, cols, x, order=RIGHT):
        A, x = h16(A), h16(x)
        d = np.zeros(cols, np.float32)
        self.L.rt_columns(_p(A, _u16), _u64(rows), _u64(cols), _p(x, _u16), C.c_int(order), _p(d, _fp))
        return d

    def mvm_transposed(self, A, rows, cols, x, order=RIGHT):
        A, x = h16(A), h16(x)
        r = np.zeros(cols, np.uint16)
        self.L.rt_mvm_transposed(_p(A, _u16), _u64(rows), _u64(cols), _p(x, _u16), C.c_int(order), _p(r, _u16))
        return r

    def mvm_f32_transposed(self, A, rows, cols, x, order=RIGHT):
        A, x = h16(A), np.ascontiguousarray(x, dtype=np.float32)
        r = np.zeros(cols, np.float32)
        self.L.rt_mvm_f32_transposed(_p(A, _u16), _u64(rows), _u64(cols), _p(x, _fp), C.c_int(order), _p(r, _fp))
        return r

    def mvm_transposed_scale_and_add(self, A, rows, cols, x, u, a, order=RIGHT):
        A, x, u = h16(A), h16(x), h16(u)
        t, r = np.zeros(cols, np.uint16), np.zeros(cols, np.uint16)
        self.L.rt_mvm_transposed_scale_and_add(_p(A, _u16), _u64(rows), _u64(cols), _p(x, _u16), _p(u, _u16), C.c_float(a), C.c_int(order),
                                               _p(t, _u16), _p(r, _u16))
        return t, r


@functools.lru_cache(maxsize=None)
def _build(out: Path) -> Path:
    subprocess.run(["cc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-o", str(out), str(RESTATE_T), "-lm"], check=True)
    return out


@pytest.fixture(scope="module")
def rt(tmp_path_factory):
    return RestateT(_build(tmp_path_factory.getbasetemp() / "librt16.so"))


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


class Refs:
    """one shape on the device: the matrix uploaded once, the restatement's results and those of the device pair clm_f16_transpose +
    clm_f16_mvm / clm_f16_mvm_f32 / clm_f16_mvm_scale_and_add on the stored transpose"""

    def __init__(self, hip, rt, rows, cols):  # noqa: F811
        S = self.S = case(rows, cols)
        self.dA = hip.to_device(S.A)
        self.cpu_t = rt.mvm_transposed(S.A, rows, cols, S.x)
        self.cpu_f32 = rt.mvm_f32_transposed(S.A, rows, cols, S.xf)
        self.cpu_fused = {a: rt.mvm_transposed_scale_and_add(S.A, rows, cols, S.x, S.u, a) for a in A_VALUES}
        At = hip.mf16_transpose(S.A, rows, cols)
        assert rt.is_transpose(S.A, rows, cols, At)
        self.dAt = hip.to_device(At)
        self.dev_t = hip.mf16_mvm(At, cols, rows, S.x)
        self.dev_f32 = hip.mf16_mvm_f32(At, cols, rows, S.xf)
        self.dev_fused = {a: hip.mf16_mvm_scale_and_add(self.dAt, cols, rows, S.x, S.u, a) for a in A_VALUES}


_refs = {}


def refs(hip, rt, rows, cols):  # noqa: F811
    if (rows, cols) not in _refs:
        _refs[(rows, cols)] = Refs(hip, rt, rows, cols)
    return _refs[(rows, cols)]
