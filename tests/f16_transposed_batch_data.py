"""Shapes and vectors of the batched transposed half-precision mvm tests (test_f16_mvm_transposed_batch*.py,
test_f16_iht_batch_one_matrix.py).  The matrices and the first vector of a shape are those of f16_transposed_data.py (data built to CANCEL
across chains, so that a wrong summation order reaches the f16 bits); vector j >= 1 is built the same way from a seed of its own.
test_f16_mvm_transposed_batch_cpu.py asserts, for every shape and vector used here, that every wrong order changes at least one result.

The edge shapes come from the kernel's own constants in clover_amd/csrc/half16_t_batch.hip: the strip width F16TB_COLS and the look-ahead
depth F16TB_U (plain numbers or functions of NV) and the chunk F16TB_CHUNK."""
import re
from pathlib import Path

import numpy as np

from f16_transposed_data import BASIC, case, pad128, vector_cols, vector_rows

SRC = (Path(__file__).resolve().parent.parent / "clover_amd" / "csrc" / "half16_t_batch.hip").read_text()
NVS = (2, 4, 8)                                         # the instantiations
COLS_RE = r"#define\s+F16TB_COLS(?:\(NV\))?\s+(\d+|\(\(NV\) == \d+ \? \d+ : \d+\))"
U_RE = r"#define\s+F16TB_U(?:\(NV\))?\s+(\d+|\(\(NV\) == \d+ \? \d+ : \d+\))"
CHUNK_RE = r"#define\s+F16TB_CHUNK(?:\(NV\))?\s+(\d+u|\(\(NV\) == \d+ \? \d+u : \d+u\))"


def per_nv(regex):
    """{NV: value} of a constant written as a number or as ((NV) == k ? a : b)"""
    body = re.search(regex, SRC).group(1).replace("u", "")
    m = re.fullmatch(r"\(\(NV\) == (\d+) \? (\d+) : (\d+)\)", body)
    if not m:
        return {nv: int(body) for nv in NVS}
    k, a, b = map(int, m.groups())
    return {nv: a if nv == k else b for nv in NVS}


COLS, U, CHUNK = per_nv(COLS_RE), per_nv(U_RE), per_nv(CHUNK_RE)
WIDTHS, CHUNKS_ = sorted(set(COLS.values())), sorted(set(CHUNK.values()))
ROUND = 64 * max(U.values())                            # two register sets of U 32-row blocks

# one set, one round, a round plus a set, a partial set and two rounds for every U in {1, 2, 4, 8}
SETS = [(r, 128) for r in (128, 256, 384, 512, 640, 768, 1024)]
# the masked last workgroup (strips wider than 128 columns) and several workgroups, for every strip width
STRIPS = [(r, pad128(c)) for w in WIDTHS for c in (w - 128, w, w + 128, 2 * w + 128) if c > 0 for r in (128, 256)]
# the x re-staging barriers, for every chunk
CHUNKS = [(r, 128) for c in CHUNKS_ for r in (c - 128, c, c + 128, 2 * c + 128) if r > 0]
# a multiple of neither the chunk nor the round, three workgroups or more at every strip width
ODD = (max(CHUNKS_) + ROUND + 128, pad128(2 * max(WIDTHS) + 1))
EDGES = sorted(set(SETS + STRIPS + CHUNKS + [ODD]) - set(BASIC))
SHAPES = sorted(set(BASIC + EDGES))
assert all(r % 128 == 0 and c % 128 == 0 and r > 0 and c > 0 for r, c in SHAPES)
assert all(ODD[0] % c for c in CHUNKS_) and ODD[0] % ROUND and all(-(-ODD[1] // w) >= 3 for w in WIDTHS)

NVECS = [1, 2, 3, 4, 5, 8, 9, 17]                       # every instantiation full and partly filled; remainder groups of one
EDGE_NVECS = [2, 3, 5, 8]
NVMAX = max(NVECS)


def x_of(rows, cols, j):
    """vector j of a shape: the shape's own x, then vectors of the same build with seeds of their own"""
    return case(rows, cols).x if j == 0 else vector_rows(np.random.default_rng(rows * 1000003 + cols + 7919 * j), rows)


def u_of(rows, cols, j):
    return case(rows, cols).u if j == 0 else vector_cols(np.random.default_rng(rows * 1000003 + cols + 104729 * j + 1), cols)


def count_for(shape):
    """how many vectors the GPU tests use on a shape"""
    return NVMAX if tuple(shape) in BASIC else max(EDGE_NVECS)
