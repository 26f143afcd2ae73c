"""Shared pieces of the CloverMatrix8 x fp32-vector tests (include/clover_hip_m8_f32.h; tests/test_m8_f32_*.py).

- Restate: tests/m8_f32_t_restate.c, the transposed product as a column walk of the stated definition, built with cc -O2 -ffp-contract=off
  (its only fused operation is the explicit fmaf).  test_m8_f32_cpu.py pins it on m8.transpose + m8.mvm_f32 of tests/matrix8_helpers.py,
  the restatement that is pinned on the reference's fixtures;
- the constants of the transposed kernel, read from clover_amd/csrc/matrix8_f32_t.hip and the header, and the shapes the GPU tests use;
- data: full-range random bytes (-128 included) with tile scales in [0.5, 2), normal-distributed fp32 vectors, the scale edges (a tile
  scale near FLT_MAX, subnormal factors f32(s / 127) with subnormal products x f), the loop problems re-quantized to 8 bits;
- loop_reference: the Python composition of the loop (m8.mvm_f32 + rf of tests/fp32_helpers.py), with the transposed product as a
  parameter: a stored transpose or the column walk."""
import ctypes as C
import functools
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from clover_amd.build import repo_root
from fp32_helpers import fast_threshold_model, iht_problem

ROOT = repo_root()
SRC = (ROOT / "clover_amd" / "csrc" / "matrix8_f32_t.hip").read_text()
HEADER = (ROOT / "include" / "clover_hip_m8_f32.h").read_text()
COLS = int(re.search(r"#define\s+M8FT_COLS\s+(\d+)", SRC).group(1))          # columns per workgroup
U = int(re.search(r"#define\s+M8FT_U\s+(\d+)", SRC).group(1))                # 32-row blocks per register set
CHUNK = int(re.search(r"#define\s+CLM8_F32_T_CHUNK\s+(\d+)", HEADER).group(1))      # rows of x staged per pass: exported by the header
M8_UNROLL = 8                # 64-column blocks per round of k_m8_mvm_f32 (matrix8.hip: constexpr int U = 8)

# transposed product (rows, cols): one block; three strips at 128 columns; three row blocks of 128; a ragged last group of loads and five
# strips; the second staging chunk with a ragged last group of loads
T_SHAPES = [(128, 128), (128, 384), (384, 128), (256, 640), (CHUNK + 128, 384)]
# row-major fused (rows, cols): one row group; several, cols / 64 = 10 past one round of the unroll; two rounds and a ragged third
R_SHAPES = [(128, 128), (256, 640), (128, 1152)]
LOOP_SHAPES = [(128, 256), (256, 384), (384, 128)]
A_VALUES = (-1.0, 0.37)

_fp = C.POINTER(C.c_float)
_i8p = C.POINTER(C.c_int8)
_u64 = C.c_uint64


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


class Restate:
    def __init__(self, so: Path):
        self.L = C.CDLL(str(so))

    def mvm_f32_transposed(self, qA, sA, rows, cols, x, chains=32):
        qA, sA, x = np.ascontiguousarray(qA, np.int8), np.ascontiguousarray(sA, np.float32), np.ascontiguousarray(x, np.float32)
        assert qA.size == rows * cols and sA.size == (rows // 64) * (cols // 64) and x.size == rows
        r = np.zeros(cols, np.float32)
        self.L.m8rt_mvm_f32_transposed(qA.ctypes.data_as(_i8p), sA.ctypes.data_as(_fp), _u64(rows), _u64(cols), x.ctypes.data_as(_fp),
                                       r.ctypes.data_as(_fp), C.c_int(chains))
        return r


@functools.lru_cache(maxsize=None)
def _build(out: Path) -> Path:
    subprocess.run(["cc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fPIC", "-shared", "-o",
                    str(out), str(Path(__file__).parent / "m8_f32_t_restate.c"), "-lm"], check=True)
    return out


@pytest.fixture(scope="module")
def m8rt(tmp_path_factory):
    return Restate(_build(tmp_path_factory.getbasetemp() / "libm8_f32_t_restate.so"))


# ---------------------------------------------------------------- data
def matrix(rng, rows, cols):
    """(bytes over the whole range, -128 included; tile scales in [0.5, 2))"""
    q = np.frombuffer(rng.bytes(rows * cols), np.int8).copy()
    q[:4] = (-128, 127, -128, -1)                                # whatever the draw: the byte a quantiser never writes is there
    return q, rng.uniform(0.5, 2.0, size=(rows // 64) * (cols // 64)).astype(np.float32)


def vector(rng, n):
    return rng.normal(size=n).astype(np.float32)


def problem(rows, cols, seed=0):
    """(qA, sA, x[rows], xc[cols], u_rows[rows], u_cols[cols]) of one shape"""
    rng = np.random.default_rng(1000 * rows + cols + seed)
    qA, sA = matrix(rng, rows, cols)
    return qA, sA, vector(rng, rows), vector(rng, cols), vector(rng, rows), vector(rng, cols)


def cancel_u(d, a):
    """u = -f32(a d): fma(d, a, u) is then the rounding error of the product and nothing else; a separately rounded product gives +0"""
    return (-(np.float32(a) * d.astype(np.float32))).astype(np.float32)


TINY = float(np.finfo(np.float32).tiny)      # 2^-126: below it a float is subnormal


def edge_problem():
    """the scale edges on A's grid for the TRANSPOSED walk, in the first and in the second row chunk: a tile scale near FLT_MAX, and tiles
    whose factor f32(s / 127) is subnormal (1e-37, 3e-38) down to a few units of the last subnormal place (1e-42).  x over the huge
    tiles' rows is scaled down so that the results stay finite; over the tiny tiles' rows x stays of order one, so that the products
    x f are subnormal too.  The column tiles that hold tiny tiles are zero in every other row tile, so that their results ARE the tiny
    tiles' products: subnormals that a flushing multiply or fma would lose."""
    rows, cols = CHUNK + 128, 384
    rng = np.random.default_rng(77)
    qA, sA = matrix(rng, rows, cols)
    g = sA.reshape(rows // 64, cols // 64)
    q = qA.reshape(rows, cols)
    x = vector(rng, rows)
    c2 = CHUNK // 64                                            # the first row tile of the second chunk
    huge = [(1, 0, 3e38), (c2 + 1, 4, 2.9e38)]                  # (row tile, column tile, scale)
    tiny = [(2, 1, 1e-37), (c2, 1, 3e-38), (3, 2, 1e-42), (c2, 2, 1e-42)]
    for rt, ct, s in huge:
        g[rt, ct] = np.float32(s)
        x[64 * rt:64 * rt + 64] *= np.float32(1e-30)
    for ct in sorted({ct for _, ct, _ in tiny}):
        keep = np.zeros(rows, bool)
        for rt in (rt for rt, c, _ in tiny if c == ct):
            keep[64 * rt:64 * rt + 64] = True
        q[~keep, 64 * ct:64 * ct + 64] = 0
    for rt, ct, s in tiny:
        g[rt, ct] = np.float32(s)
    return rows, cols, q.reshape(-1), sA, x, huge, tiny


def loop_problem(m8, m, n, ties):
    """iht_problem of tests/fp32_helpers.py re-quantized to 8 bits: (qPhi, sPhi, y, mu)"""
    Phi, _, y, mu = iht_problem(m, n, 17 * m + n + ties, ties=ties)
    qPhi, sPhi = m8.quantize(Phi.reshape(m, n))
    return qPhi, sPhi, y, mu


def loop_reference(m8, rf, qPhi, sPhi, m, n, y, iterations, K, mu, threshold, x_len, transposed_product, prefill=0x55):
    """the five calls one by one on the CPU: m8.mvm_f32, rf.scale_and_add, the threshold of the mode (0 none, 1 FAST: the
    lowest-index model, 2 REFERENCE: rf.threshold); transposed_product(t2) gives Phi' t2.  Untouched temporaries keep the prefill."""
    fill = np.frombuffer(bytes([prefill]) * 4, np.float32)[0]
    v = {"x": np.zeros(n, np.float32), "t1": np.full(m, fill, np.float32), "t2": np.full(m, fill, np.float32), "t3": np.full(n, fill, np.float32)}
    for _ in range(iterations):
        v["t1"] = m8.mvm_f32(qPhi, sPhi, m, n, v["x"])
        v["t2"] = rf.scale_and_add(y, v["t1"], -1.0)
        v["t3"] = transposed_product(v["t2"])
        v["x"] = rf.scale_and_add(v["x"], v["t3"], mu)
        if threshold == 1:
            v["x"] = fast_threshold_model(v["x"], x_len, K)
        elif threshold == 2:
            v["x"] = rf.threshold(v["x"], x_len, K)
    return v


def tie_K(m8, rf, qPhi, sPhi, qT, sT, m, n, y, mu, x_len):
    """a K near n / 8 at which the FIRST threshold cuts between two equal magnitudes"""
    first = loop_reference(m8, rf, qPhi, sPhi, m, n, y, 1, 0, mu, 0, x_len, lambda t2: m8.mvm_f32(qT, sT, n, m, t2))["x"]
    mags = np.sort(np.abs(first[:x_len]))[::-1]
    for K in range(n // 8, x_len - 1):
        if mags[K - 1] == mags[K] and mags[K] > 0:
            return K
    raise AssertionError("the data has no tie to cut")
