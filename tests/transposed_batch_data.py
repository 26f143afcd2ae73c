"""Data and references shared by the tests of the batched transposed 4-bit mvm (test_mvm_transposed_batch*.py, test_iht_batch_one_matrix.py).

The reference side is never the new kernel: it is the CPU oracle -- oracle.m4_transpose, then oracle.m4_mvm on the stored transpose, then
oracle.v4_scale_and_add for the fused form, per vector -- and, on the device, the single calls clm4_mvm_transposed /
clm4_mvm_transposed_scale_and_add in order.

Data (matrix, vector: test_mvm_transposed.py): nibbles in [-7, 7], all tile scales distinct, one zero tile, one all-zero column group (its
result block is all zero with scale 1), square matrices not symmetric.  Of the NVMAX vectors, vector 1 is all zero and vector 2 IS vector 0
(the same device pointers twice); every other pair differs, so a result landing in the wrong slot shows.

C = MVTB_CHUNK (rows staged in LDS per pass), U = MVTB_U(NV) (128-row steps per group of loads) and W = MVT_W (output blocks per workgroup)
are read from the sources."""
import math
import re
from pathlib import Path

import numpy as np

from test_mvm_batch import get, pairs
from test_mvm_transposed import eq, matrix, same, vector  # noqa: F401

ROOT = Path(__file__).resolve().parent.parent
SRC = (ROOT / "clover_amd" / "csrc" / "mvm_t4_batch.hip").read_text()
C_ = int(re.search(r"#define\s+MVTB_CHUNK\s+(\d+)u", SRC).group(1))
W = int(re.search(r"#define\s+MVT_W\s+(\d+)", (ROOT / "clover_amd" / "csrc" / "mvm_t4.hip").read_text()).group(1))
WB = int(re.search(r"#define\s+MVTB_W\s+(\d+)", (ROOT / "clover_amd" / "csrc" / "mvm_t4_batch.h").read_text()).group(1))
_u = re.search(r"#define\s+MVTB_U\(NV\)\s+\(\(NV\)\s*<=\s*(\d+)\s*\?\s*(\d+)\s*:\s*(\d+)\)", SRC)
U_OF = {nv: (int(_u.group(2)) if nv <= int(_u.group(1)) else int(_u.group(3))) for nv in (2, 4, 8)}
US = sorted(set(U_OF.values()))
NVMAX = 17
A_FUSED = 0.37
KEYS = (4711, 13)

FIRST4 = [(128, 128), (256, 128), (128, 256), (384, 640)]
SMALL = FIRST4 + [(128 * (u + 1), 128) for u in US if (128 * (u + 1), 128) not in FIRST4] + [(128, 64 * (W + 2)), (256, 64 * (2 * W + 2))]
ODD = (C_ + 128 * (math.lcm(*US) + 1), 384)
CHUNKY = [(C_ - 128, 128), (C_, 128), (C_ + 128, 128), (2 * C_ + 128, 128), ODD]
assert ODD[0] % C_ and all((ODD[0] // 128) % u for u in US if u > 1) and (64 * (W + 2)) % 128 == 0


class Data:
    """host side, once per shape: the matrix, NVMAX vectors x (rows elements) and u (cols elements), the oracle's t = A' x and
    r = u + A_FUSED t per vector (computed on first use)"""

    def __init__(self, oracle, rows, cols):
        rng = np.random.default_rng(rows * 1000003 + cols + 1)
        self.oracle, self.rows, self.cols = oracle, rows, cols
        self.qA, self.sA = matrix(rng, rows, cols)
        self.x = [vector(rng, rows, zero_block=None if j % 3 else (0 if rows == 128 else 1)) for j in range(NVMAX)]
        self.x[1] = (np.zeros(rows // 2, np.uint8), self.x[1][1])           # all zero
        self.x[2] = self.x[0]                                               # the same object: uploaded once, the same pointers twice
        self.u = [vector(rng, cols) for _ in range(NVMAX)]
        self.At = oracle.m4_transpose(self.qA, self.sA, rows, cols)
        self._t, self._r = {}, {}

    def t(self, j):
        if j not in self._t:
            self._t[j] = self._t[0] if j == 2 and 0 in self._t else self.oracle.m4_mvm(*self.At, self.cols, self.rows, *self.x[j])
        return self._t[j]

    def r(self, j, a=A_FUSED):
        if (j, a) not in self._r:
            self._r[(j, a)] = self.oracle.v4_scale_and_add(*self.u[j], *self.t(j), a)
        return self._r[(j, a)]


class Dev:
    """device side, once per shape: the buffers and the results of the single calls in order"""

    def __init__(self, hip, D):
        L, rows, cols = hip.lib, D.rows, D.cols
        self.D = D
        self.dA, self.dsA = hip.to_device(D.qA), hip.to_device(D.sA)
        self.dx = [(hip.to_device(q), hip.to_device(s)) for q, s in D.x]
        self.dx[2] = self.dx[0]
        self.du = [(hip.to_device(q), hip.to_device(s)) for q, s in D.u]
        out = pairs(hip, NVMAX, cols)
        for (dq, ds), (r, sr) in zip(self.dx, out):
            hip.check(L.clm4_mvm_transposed(self.dA.ptr, self.dsA.ptr, rows, cols, dq.ptr, ds.ptr, r.ptr, sr.ptr, None, None))
        hip.sync()
        self.single = [get(o, cols) for o in out]


_data, _dev = {}, {}


def data(oracle, rows, cols):
    if (rows, cols) not in _data:
        _data[(rows, cols)] = Data(oracle, rows, cols)
    return _data[(rows, cols)]


def dev(hip, oracle, rows, cols):
    if (rows, cols) not in _dev:
        _dev[(rows, cols)] = Dev(hip, data(oracle, rows, cols))
    return _dev[(rows, cols)]
