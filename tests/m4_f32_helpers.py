"""Shared pieces of the CloverMatrix4 x fp32-vector tests (include/clover_hip_m4_f32.h; tests/test_m4_f32_*.py).

- Restate: tests/m4_f32_t_restate.c, the transposed product as a column walk of the stated definition, built with cc -O2 -ffp-contract=off
  (its only fused operation is the explicit fmaf).  test_m4_f32_cpu.py pins it on oracle.m4_transpose + oracle.m4_mvm_f32.
- the constants of the transposed kernel, read from clover_amd/csrc/mvm_f32_t.hip and the header, and the shapes the GPU tests use;
- data: random nibbles with tile scales in [0.5, 2), normal-distributed fp32 vectors, the scale edges of the (q / 16) (16 c) shortcut,
  the loop problems re-quantized to 4 bits;
- loop_reference: the Python composition of the loop (oracle product + rf of tests/fp32_helpers.py), with the transposed product as a
  parameter: a stored transpose or the column walk."""
import ctypes as C
import functools
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from clover_amd.build import repo_root
from conftest import random_packed
from fp32_helpers import fast_threshold_model, iht_problem

ROOT = repo_root()
SRC = (ROOT / "clover_amd" / "csrc" / "mvm_f32_t.hip").read_text()
HEADER = (ROOT / "include" / "clover_hip_m4_f32.h").read_text()
COLS = int(re.search(r"#define\s+M4FT_COLS\s+(\d+)", SRC).group(1))          # columns per workgroup
U = int(re.search(r"#define\s+M4FT_U\s+(\d+)", SRC).group(1))                # 32-row blocks per register set
CHUNK = int(re.search(r"#define\s+CLM4_F32_T_CHUNK\s+(\d+)", HEADER).group(1))      # rows of x staged per pass: exported by the header
MVF_CHUNK = int(re.search(r"#define\s+MVF_CHUNK\s+(\d+)u", (ROOT / "clover_amd" / "csrc" / "mvm_f32.hip").read_text()).group(1))

# transposed product (rows, cols): one block; a masked last strip at 256 columns / three strips at 128; three row blocks of 128; a ragged
# last group of loads and two / five strips; the second staging chunk
T_SHAPES = [(128, 128), (128, 384), (384, 128), (256, 640), (CHUNK + 128, 384)]
# row-major fused (rows, cols): one row group; several; the second x chunk of k_m4_mvm_f32
R_SHAPES = [(128, 128), (256, 640), (384, MVF_CHUNK + 128)]
LOOP_SHAPES = [(128, 256), (256, 384), (384, 128)]
A_VALUES = (-1.0, 0.37)

_fp = C.POINTER(C.c_float)
_u8p = C.POINTER(C.c_uint8)
_u64 = C.c_uint64


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


class Restate:
    def __init__(self, so: Path):
        self.L = C.CDLL(str(so))

    def mvm_f32_transposed(self, qA, sA, rows, cols, x, chains=32):
        qA, sA, x = np.ascontiguousarray(qA, np.uint8), np.ascontiguousarray(sA, np.float32), np.ascontiguousarray(x, np.float32)
        assert qA.size == rows * cols // 2 and sA.size == (rows // 64) * (cols // 64) and x.size == rows
        r = np.zeros(cols, np.float32)
        self.L.m4rt_mvm_f32_transposed(qA.ctypes.data_as(_u8p), sA.ctypes.data_as(_fp), _u64(rows), _u64(cols), x.ctypes.data_as(_fp),
                                       r.ctypes.data_as(_fp), C.c_int(chains))
        return r


@functools.lru_cache(maxsize=None)
def _build(out: Path) -> Path:
    subprocess.run(["cc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fPIC", "-shared", "-o",
                    str(out), str(Path(__file__).parent / "m4_f32_t_restate.c"), "-lm"], check=True)
    return out


@pytest.fixture(scope="module")
def m4rt(tmp_path_factory):
    return Restate(_build(tmp_path_factory.getbasetemp() / "libm4_f32_t_restate.so"))


# ---------------------------------------------------------------- data
def matrix(rng, rows, cols):
    """(nibbles, tile scales in [0.5, 2))"""
    return random_packed(rng, rows * cols)[0], rng.uniform(0.5, 2.0, size=(rows // 64) * (cols // 64)).astype(np.float32)


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


def edge_problem():
    """the scale edges of test_gpu_mixed_mvm_f32_tiny_and_huge_scales on A's grid for the TRANSPOSED walk, in the first and in the second
    row chunk: a tile whose 16 f32(s / 7) overflows (the chunk of its strip takes the plain conversion), a subnormal factor, 1e-42.  The x
    values over the huge tiles' rows are scaled down so that the results stay finite, over the tiny tiles' rows up; the column tiles that
    hold tiny tiles are zero in every other row tile, so that their results ARE the tiny tiles' products."""
    rows, cols = CHUNK + 128, 384
    rng = np.random.default_rng(77)
    qA, sA = matrix(rng, rows, cols)
    g = sA.reshape(rows // 64, cols // 64)
    q = qA.reshape(rows, cols // 2)
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
        q[~keep, 32 * ct:32 * ct + 32] = 0
    for rt, ct, s in tiny:
        g[rt, ct] = np.float32(s)
    for rt in sorted({rt for rt, _, _ in tiny}):
        x[64 * rt:64 * rt + 64] *= np.float32(1e35)
    return rows, cols, q.reshape(-1), sA, x, huge, tiny


def loop_problem(oracle, m, n, ties):
    """iht_problem of tests/fp32_helpers.py re-quantized to 4 bits: (qPhi, sPhi, y, mu)"""
    Phi, _, y, mu = iht_problem(m, n, 17 * m + n + ties, ties=ties)
    qPhi, sPhi = oracle.m4_quantize(Phi.reshape(m, n))
    return qPhi, sPhi, y, mu


def loop_reference(oracle, rf, qPhi, sPhi, m, n, y, iterations, K, mu, threshold, x_len, transposed_product, prefill=0x55):
    """the five calls one by one on the CPU: oracle.m4_mvm_f32, rf.scale_and_add, the threshold of the mode (0 none, 1 FAST: the
    lowest-index model, 2 REFERENCE: rf.threshold); transposed_product(t2) gives Phi' t2.  Untouched temporaries keep the prefill."""
    fill = np.frombuffer(bytes([prefill]) * 4, np.float32)[0]
    v = {"x": np.zeros(n, np.float32), "t1": np.full(m, fill, np.float32), "t2": np.full(m, fill, np.float32), "t3": np.full(n, fill, np.float32)}
    for _ in range(iterations):
        v["t1"] = oracle.m4_mvm_f32(qPhi, sPhi, m, n, v["x"])
        v["t2"] = rf.scale_and_add(y, v["t1"], -1.0)
        v["t3"] = transposed_product(v["t2"])
        v["x"] = rf.scale_and_add(v["x"], v["t3"], mu)
        if threshold == 1:
            v["x"] = fast_threshold_model(v["x"], x_len, K)
        elif threshold == 2:
            v["x"] = rf.threshold(v["x"], x_len, K)
    return v


def tie_K(oracle, rf, qPhi, sPhi, qT, sT, m, n, y, mu, x_len):
    """a K near n / 8 at which the FIRST threshold cuts between two equal magnitudes"""
    first = loop_reference(oracle, rf, qPhi, sPhi, m, n, y, 1, 0, mu, 0, x_len, lambda t2: oracle.m4_mvm_f32(qT, sT, n, m, t2))["x"]
    mags = np.sort(np.abs(first[:x_len]))[::-1]
    for K in range(n // 8, x_len - 1):
        if mags[K - 1] == mags[K] and mags[K] > 0:
            return K
    raise AssertionError("the data has no tie to cut")
