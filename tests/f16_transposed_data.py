"""Data and shapes of the transposed half-precision mvm tests (test_f16_mvm_transposed*.py, test_f16_iht_one_matrix.py).

Why the data is built: on ordinary random f16 data a wrong summation order (chain ends summed left to right, one chain, 16 chains) changes
most fp32 column values but almost none of the f16 results, so a comparison of f16 bits would pass a kernel that sums in another order.
The data here CANCELS across chains: in every 32-row block, row b + 16 + k holds the bits of row b + k with the sign flipped, a random
third of those elements with their last mantissa bit flipped as well, and x[b + 16 + k] = x[b + k].  Chains 0 .. 15 then carry large
sums that chains 16 .. 31 nearly undo, and what is left depends on the order of the additions down to the last f16 bit.
test_f16_mvm_transposed_cpu.py asserts that condition for every shape below instead of trusting it.

Also placed: a few subnormals, both zeros, one all-zero column (its result is +0)."""
import re
from pathlib import Path

import numpy as np

from half16_helpers import random_f16_bits

SRC = (Path(__file__).resolve().parent.parent / "clover_amd" / "csrc" / "half16_t.hip").read_text()
COLS = int(re.search(r"#define\s+F16T_COLS\s+(\d+)", SRC).group(1))       # columns per workgroup
U = int(re.search(r"#define\s+F16T_U\s+(\d+)", SRC).group(1))             # 32-row blocks per register set; a round is the two sets
C_ = int(re.search(r"#define\s+F16T_CHUNK\s+(\d+)u", SRC).group(1))       # rows of x staged per pass
ROUND = 64 * U


def pad128(n):
    return (n + 127) // 128 * 128


BASIC = [(128, 128), (256, 128), (128, 256), (384, 640)]
# one register set, one round, a round plus a partial set, two rounds
SETS = [(pad128(32 * U), 128), (pad128(64 * U), 128), (pad128(32 * (2 * U + 1)), 128), (pad128(128 * U), 128)]
# the masked last workgroup (strips wider than 128 columns) and several workgroups
STRIPS = [(r, pad128(c)) for c in (COLS - 128, COLS, COLS + 128, 2 * COLS + 128) if c > 0 for r in (128, 256)]
# the x re-staging barriers
CHUNKS = [(C_ - 128, 128), (C_, 128), (C_ + 128, 128), (2 * C_ + 128, 128)]
# a multiple of neither the chunk nor the round, three workgroups or more
ODD = (C_ + ROUND + 128, pad128(2 * COLS + 1))
SHAPES = sorted(set(BASIC + SETS + STRIPS + CHUNKS + [ODD]))
IHT_SHAPES = [(128, 256), (256, 128), (384, 640)]
NT_SHAPE = (8192, 16512)                                                   # one 128-column strip over 256 MiB
assert all(r % 128 == 0 and c % 128 == 0 and r > 0 and c > 0 for r, c in SHAPES)
assert ODD[0] % C_ and ODD[0] % ROUND and -(-ODD[1] // COLS) >= 3
assert NT_SHAPE[0] * NT_SHAPE[1] * 2 > (256 << 20) >= NT_SHAPE[0] * (NT_SHAPE[1] - 128) * 2

ZERO_COLUMN = 5                     # the all-zero column of every matrix
A_VALUES = (0.37, -1.0)             # the fused call's a


def _mirror_rows(M, rng):
    """row b + 16 + k = row b + k with the sign flipped, a random third with the last mantissa bit flipped too (in place; M is rows x cols
    uint16)"""
    rows, cols = M.shape
    B = M.reshape(rows // 32, 32, cols)
    flip = (rng.random((rows // 32, 16, cols)) < 1.0 / 3.0).astype(np.uint16)
    B[:, 16:, :] = (B[:, :16, :] ^ np.uint16(0x8000)) ^ flip


def _mirror_vec(v):
    B = v.reshape(v.size // 32, 32)
    B[:, 16:] = B[:, :16]


def matrix(rng, rows, cols):
    """rows x cols f16 bit patterns, magnitudes 2^-4 .. 2^4, built to cancel across chains (module docstring); not symmetric"""
    M = random_f16_bits(rng, rows * cols, -4, 4).reshape(rows, cols)
    # a few subnormals and both zeros in the first halves of blocks: the mirror gives them their negated twins
    M[0, 1], M[1, 2], M[2, 3], M[3, 4] = 0x0001, 0x83FF, 0x0000, 0x8000
    M[rows - 32, cols - 1], M[rows - 31, cols - 2] = 0x0200, 0x8000
    _mirror_rows(M, rng)
    M[:, ZERO_COLUMN] = 0
    assert rows != cols or not np.array_equal(M, M.T)
    return np.ascontiguousarray(M.reshape(-1))


def vector_rows(rng, rows):
    """x of `rows` elements with x[b + 16 + k] = x[b + k]; a subnormal and both zeros among them"""
    x = random_f16_bits(rng, rows, -4, 4)
    x[[2, 7, 9]] = [0x0000, 0x8000, 0x0003]
    _mirror_vec(x)
    return x


def vector_rows_f32(rng, rows):
    """the fp32 x of the _f32 form: full 24-bit significands, the same mirror"""
    x = (rng.choice([-1.0, 1.0], size=rows) * np.exp2(rng.uniform(-4, 4, size=rows))).astype(np.float32)
    x[[2, 7]] = [0.0, -0.0]
    _mirror_vec(x)
    return x


def vector_cols(rng, cols):
    """u of the fused call: of the size of the results, which are small after the cancellation"""
    u = random_f16_bits(rng, cols, -6, 0)
    u[[1, 6]] = [0x8000, 0x0002]
    return u


def big_matrix(rng, rows, cols, period=384):
    """a rows x cols matrix for the nontemporal shape in well under a second: matrix(rows, period) repeated along the columns, every
    column with a random sign of its own, so that no two 128-column strips hold the same bits"""
    M = np.tile(matrix(rng, rows, period).reshape(rows, period), (1, -(-cols // period)))[:, :cols]
    M = M ^ (rng.integers(0, 2, size=cols).astype(np.uint16) << np.uint16(15))[None, :]
    return np.ascontiguousarray(M.reshape(-1))


class Case:
    """the matrix and vectors of one shape; the same bytes wherever the shape is used"""

    def __init__(self, rows, cols):
        rng = np.random.default_rng(rows * 1000003 + cols)
        self.rows, self.cols = rows, cols
        self.A = matrix(rng, rows, cols)
        self.x = vector_rows(rng, rows)
        self.xf = vector_rows_f32(rng, rows)
        self.u = vector_cols(rng, cols)


_cases = {}


def case(rows, cols):
    if (rows, cols) not in _cases:
        _cases[(rows, cols)] = Case(rows, cols)
    return _cases[(rows, cols)]
