"""Data and references shared by the tests of the batched transposed mixed mvm, CloverMatrix4 x CloverVector8
(test_mvm_v8_transposed_batch*.py, test_iht_v8_batch_one_matrix.py).

The reference side is never the new kernel: on the CPU it is oracle.m4_transpose, then oracle.m4_mvm_v8 on the stored transpose, then
oracle.v8_scale_and_add for the fused form, per vector; on the device, the single calls clm4_mvm_v8_transposed /
clm4_mvm_v8_transposed_scale_and_add in order and clm4_mvm_v8_batch / clm4_mvm_v8_scale_and_add_batch on clm4_transpose(A).

Data (matrix, vector: test_mvm_v8_transposed.py): nibbles in [-7, 7] with -7 and 7 at known places, all tile scales distinct, one zero
tile, one all-zero column group (its result block is all zero with scale 1), square matrices not symmetric.  Of the NVMAX vectors, vector 1
is all zero and vector 2 IS vector 0 (the same device pointers twice); every other pair differs, so a result landing in the wrong slot shows.

C = MVT8B_CHUNK (rows staged in LDS per pass), S = MVT8B_STEP (rows per block), U = MVT8B_U(NV) (blocks per register set) are read from
clover_amd/csrc/mvm_t8_batch.hip, W = MVT8B_W (output blocks per workgroup) from mvm_t8_batch.h."""
import re
from pathlib import Path

import numpy as np

from test_m8_mvm_batch import get8, pairs8
from test_mvm_batch import batch_kernel, pa
from test_mvm_v8_transposed import eq, matrix, same, vector  # noqa: F401

ROOT = Path(__file__).resolve().parent.parent
SRC = (ROOT / "clover_amd" / "csrc" / "mvm_t8_batch.hip").read_text()
C_ = int(re.search(r"#define\s+MVT8B_CHUNK\s+(\d+)u", SRC).group(1))
S_ = int(re.search(r"#define\s+MVT8B_STEP\s+(\d+)u", SRC).group(1))
W = int(re.search(r"#define\s+MVT8B_W\s+(\d+)", (ROOT / "clover_amd" / "csrc" / "mvm_t8_batch.h").read_text()).group(1))
_u = re.search(r"#define\s+MVT8B_U\(NV\)\s+\(\(NV\)\s*<=\s*(\d+)\s*\?\s*(\d+)\s*:\s*(\d+)\)", SRC)
U_OF = {nv: (int(_u.group(2)) if nv <= int(_u.group(1)) else int(_u.group(3))) for nv in (2, 4, 8)}
US = sorted(set(U_OF.values()))
NVMAX = 17
NVECS = (1, 2, 3, 5, 8, 9, 17)
A_FUSED = 0.37
KEYS = (4711, 13)

FIRST4 = [(128, 128), (256, 128), (128, 256), (384, 640)]
# one whole register set, one and two whole rounds of the two sets, a round and a partial set, for the U of every NV (rows are
# multiples of 128, so S U = 64 at U = 1 is no shape)
_WALK = sorted({(r, 128) for u in US for r in (S_ * u, 2 * S_ * u, S_ * (2 * u + 2), 4 * S_ * u) if r % 128 == 0})
SMALL = FIRST4 + [s for s in _WALK if s not in FIRST4] + [s for s in [(128, 64 * (W + 2)), (256, 64 * (2 * W + 2))] if s not in FIRST4]
ODD = (C_ + 2 * S_ * max(US) + 128, 384)
CHUNKY = [(C_ - 128, 128), (C_, 128), (C_ + 128, 128), (2 * C_ + 128, 128), ODD]
assert all(r % 128 == 0 and c % 128 == 0 for r, c in SMALL + CHUNKY) and ODD[0] % C_ and (64 * (W + 2)) % 128 == 0


class Data:
    """host side, once per shape: the matrix, NVMAX vectors x (rows elements) and u (cols elements), the CPU's t = A' x and
    r = u + a t per vector (computed on first use)"""

    def __init__(self, oracle, rows, cols):
        rng = np.random.default_rng(rows * 1000003 + cols + 2)
        self.oracle, self.rows, self.cols = oracle, rows, cols
        self.qA, self.sA = matrix(rng, rows, cols)
        self.x = [vector(rng, rows, zero_block=None if j % 3 else (0 if rows == 128 else 1)) for j in range(NVMAX)]
        self.x[1] = (np.zeros(rows, np.int8), self.x[1][1])                 # all zero
        self.x[2] = self.x[0]                                               # the same object: the same pointers twice
        self.u = [vector(rng, cols) for _ in range(NVMAX)]
        self.At = oracle.m4_transpose(self.qA, self.sA, rows, cols)
        self._t, self._r = {}, {}

    def t(self, j, o=None):
        """A' x[j] on the CPU; with a generator o: with its draws, not kept"""
        if o is not None:
            return self.oracle.m4_mvm_v8(*self.At, self.cols, self.rows, *self.x[j], o)
        if j not in self._t:
            self._t[j] = self._t[0] if j == 2 and 0 in self._t else self.oracle.m4_mvm_v8(*self.At, self.cols, self.rows, *self.x[j])
        return self._t[j]

    def r(self, j, a=A_FUSED):
        if (j, a) not in self._r:
            self._r[(j, a)] = self.oracle.v8_scale_and_add(*self.u[j], *self.t(j), a)
        return self._r[(j, a)]


class Dev:
    """device side, once per shape: the buffers, the results of the single calls in order and of clm4_mvm_v8_batch on clm4_transpose(A)"""

    def __init__(self, hip, D):
        L, rows, cols = hip.lib, D.rows, D.cols
        self.D = D
        self.dA, self.dsA = hip.to_device(D.qA), hip.to_device(D.sA)
        self.dAt = (hip.alloc(rows * cols // 2), hip.alloc((rows // 64) * (cols // 64) * 4))
        hip.check(L.clm4_transpose(self.dA.ptr, self.dsA.ptr, rows, cols, self.dAt[0].ptr, self.dAt[1].ptr, None))
        self.dx = [(hip.to_device(q), hip.to_device(s)) for q, s in D.x]
        self.dx[2] = self.dx[0]
        self.du = [(hip.to_device(q), hip.to_device(s)) for q, s in D.u]
        out, held = pairs8(hip, NVMAX, cols), pairs8(hip, NVMAX, cols)
        for (dq, ds), (r, sr) in zip(self.dx, out):
            hip.check(L.clm4_mvm_v8_transposed(self.dA.ptr, self.dsA.ptr, rows, cols, dq.ptr, ds.ptr, r.ptr, sr.ptr, None, None))
        with batch_kernel("1"):
            hip.check(L.clm4_mvm_v8_batch(self.dAt[0].ptr, self.dAt[1].ptr, cols, rows, NVMAX, *self.xs(NVMAX), pa([o[0] for o in held]),
                                          pa([o[1] for o in held]), None, None))
        hip.sync()
        self.single = [get8(o, cols) for o in out]
        self.held = [get8(o, cols) for o in held]

    def xs(self, nvec):
        return pa([d[0] for d in self.dx[:nvec]]), pa([d[1] for d in self.dx[:nvec]])


_data, _dev = {}, {}


def data(oracle, rows, cols):
    if (rows, cols) not in _data:
        _data[(rows, cols)] = Data(oracle, rows, cols)
    return _data[(rows, cols)]


def dev(hip, oracle, rows, cols):
    if (rows, cols) not in _dev:
        _dev[(rows, cols)] = Dev(hip, data(oracle, rows, cols))
    return _dev[(rows, cols)]
