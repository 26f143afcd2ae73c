"""The transposed 8-bit mvm on the GPU: clm8_mvm_transposed, clm8_mvm_transposed_scale_and_add and clm8_iht_one_matrix give, BYTE FOR
BYTE, what a stored transpose gives -- against the CPU (tests/matrix8_restate.c: transpose, then mvm, then oracle.v8_scale_and_add for
the fused form) and against the device (clm8_transpose + clm8_mvm / clm8_mvm_scale_and_add, clm8_iht with PhiT = clm8_transpose(Phi), and
that loop composed call by call), the XORShift state left behind included.  Every comparison is of bytes.

Shapes (rows x cols): the smallest at which each thing can go wrong.  C = M8T_CHUNK (rows staged in LDS per pass), S = M8T_STEP (rows
per block), U = M8T_U (blocks per register set = blocks of loads ahead; a round is the two sets, 2 U blocks) and W = M8T_W (output
blocks per workgroup) are read from clover_amd/csrc/matrix8_t.hip:
  128 x 128                       half a register set, one output pair
  256 x 128, 128 x 256            non-square both ways: a product that forgets to transpose, or reads sA[cb][b] for sA[b][cb], fails
  384 x 640                       one set and a half, ten column tiles
  S U x 128, 2 S U x 128, S (2 U + 2) x 128, 4 S U x 128
                                  one whole set (the tail form of the walk), one and two whole rounds (the look-ahead loads of
                                  every group but the last), a round and a partial set
  128 x 64 (W + 2), 256 x 64 (2 W + 2)     more than one workgroup (W = 2: cols is a multiple of 128, every workgroup is whole, MASKED
                                  below is empty)
  C - 128, C, C + 128, 2 C + 128 (x 128)   the x re-staging barriers, a partial set at the end of a chunk and as a whole chunk
  C + 2 S U + 128 x 384           a multiple of neither C nor the round, three workgroups
Data: bytes in [-127, 127] with -127 and 127 at known places, all tile scales distinct in [0.5, 2), one zero tile, one all-zero column
group (its result block is all zero with scale 1.0: fix_zero_max); x and u are int8 in [-127, 127] with -127 and 127 at known places, x
with one zero block at 1 (at 0 for the 128-row shapes, whose block 0 meets the zero tile); the square matrices are not symmetric.
The nontemporal instantiations run at 16384 x 16512 (one 128-column strip more than the 256 MiB Infinity Cache holds; 129 workgroups):
the launcher has no switch that forces them at a small shape."""
import re
from pathlib import Path

import numpy as np
import pytest

from clover_amd.lib_binding import THRESHOLD_FAST
from matrix8_helpers import m8, m8p  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SRC = (ROOT / "clover_amd" / "csrc" / "matrix8_t.hip").read_text()
C_ = int(re.search(r"#define\s+M8T_CHUNK\s+(\d+)u", SRC).group(1))
S_ = int(re.search(r"#define\s+M8T_STEP\s+(\d+)u", SRC).group(1))
U = int(re.search(r"#define\s+M8T_U\s+(\d+)", SRC).group(1))
W = int(re.search(r"#define\s+M8T_W\s+(\d+)", SRC).group(1))
ROUND = 2 * S_ * U
SMALL = sorted({(128, 128), (256, 128), (128, 256), (384, 640), (S_ * U, 128), (ROUND, 128), (S_ * (2 * U + 2), 128), (2 * ROUND, 128),
                (128, 64 * (W + 2)), (256, 64 * (2 * W + 2))})
ODD = (C_ + ROUND + 128, 384)
CHUNKY = [(C_ - 128, 128), (C_, 128), (C_ + 128, 128), (2 * C_ + 128, 128), ODD]
ST_SHAPES = SMALL + [(C_ + 128, 128)]
IHT_SHAPES = [(128, 256), (256, 128), (384, 640)]
KEYS = (4711, 13)
A_FUSED = 0.37
T = 256 << 20
assert all(r % 128 == 0 and c % 128 == 0 for r, c in SMALL + CHUNKY)
assert ODD[0] % C_ and ODD[0] % ROUND and ODD[1] // (64 * W) == 3 and (64 * (W + 2)) % 128 == 0
MASKED = [c for _, c in SMALL + CHUNKY if (c // 64) % W]      # shapes whose last workgroup is masked (none while W divides 128 / 64)
assert not MASKED or W != 2


def same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


def eq(p, q):
    return same(p[0], q[0]) and same(p[1], q[1])


def vector(rng, n, zero_block=None):
    q = rng.integers(-127, 128, size=n).astype(np.int8)
    q[[3, n - 2]] = [127, -127]
    if zero_block is not None:
        q[64 * zero_block:64 * zero_block + 64] = 0
    return q, rng.uniform(0.5, 2.0, size=n // 64).astype(np.float32)


def matrix(rng, rows, cols):
    A = rng.integers(-127, 128, size=(rows, cols)).astype(np.int8)
    A[:64, :64] = 0                                                         # a zero tile
    A[:, cols - 64:] = 0                                                    # an all-zero column group: its result block is zero
    A[rows - 1, 5], A[rows - 1, 6], A[70, 0], A[67, 1] = 127, -127, -127, 127
    tiles = (rows // 64) * (cols // 64)
    s = (0.5 + 1.5 * rng.permutation(tiles) / tiles).astype(np.float32)     # all distinct
    assert np.unique(s).size == tiles and (rows != cols or not np.array_equal(A, A.T))
    return A.reshape(-1), s


def keys_equal(hip, st, o, oracle):
    k1, k2 = hip.rng_get(st)
    w1, w2 = oracle.rng_keys(o)
    return np.array_equal(k1, w1) and np.array_equal(k2, w2)


def dev_fused(hip, dA, dsA, rows, cols, x, u, a, rng=None):
    """(t, st, r, sr) of clm8_mvm_scale_and_add on device matrix buffers: the existing call, on a stored transpose"""
    b = [hip.to_device(v) for v in (*x, *u)]
    out = [hip.alloc(rows), hip.alloc(rows // 16), hip.alloc(rows), hip.alloc(rows // 16)]
    hip.check(hip.lib.clm8_mvm_scale_and_add(dA.ptr, dsA.ptr, rows, cols, b[0].ptr, b[1].ptr, b[2].ptr, b[3].ptr, a, out[0].ptr, out[1].ptr,
                                             out[2].ptr, out[3].ptr, rng.ptr if rng else None, None))
    return (out[0].download(np.int8, rows), out[1].download(np.float32, rows // 64), out[2].download(np.int8, rows),
            out[3].download(np.float32, rows // 64))


def dev_mvm(hip, dA, dsA, rows, cols, x, rng=None):
    b = [hip.to_device(v) for v in x]
    out = [hip.alloc(rows), hip.alloc(rows // 16)]
    hip.check(hip.lib.clm8_mvm(dA.ptr, dsA.ptr, rows, cols, b[0].ptr, b[1].ptr, out[0].ptr, out[1].ptr, rng.ptr if rng else None, None))
    return out[0].download(np.int8, rows), out[1].download(np.float32, rows // 64)


class Shape:
    """one matrix, x and u, the CPU's and the stored-transpose device results: computed once per shape"""

    def __init__(self, hip, oracle, m8, rows, cols):  # noqa: F811
        rng = np.random.default_rng(rows * 1000003 + cols)
        self.rows, self.cols = rows, cols
        self.qA, self.sA = matrix(rng, rows, cols)
        self.x = vector(rng, rows, zero_block=0 if rows == 128 else 1)        # 128 rows: block 0 meets the zero tile, block 1 stays
        self.u = vector(rng, cols)
        self.At = m8.transpose(self.qA, self.sA, rows, cols)
        self.dA, self.dsA = hip.to_device(self.qA), hip.to_device(self.sA)
        self.cpu_t = m8.mvm(*self.At, cols, rows, *self.x)
        self.cpu_r = oracle.v8_scale_and_add(*self.u, *self.cpu_t, A_FUSED)
        dAt = hip.m8_transpose(self.qA, self.sA, rows, cols)
        assert eq(dAt, self.At)
        self.dAt = [hip.to_device(v) for v in dAt]
        self.dev_t = dev_mvm(hip, *self.dAt, cols, rows, self.x)
        f = dev_fused(hip, *self.dAt, cols, rows, self.x, self.u, A_FUSED)
        self.dev_fused = (f[0:2], f[2:4])


_shapes = {}


def shape(hip, oracle, m8, rows, cols):  # noqa: F811
    if (rows, cols) not in _shapes:
        _shapes[(rows, cols)] = Shape(hip, oracle, m8, rows, cols)
    return _shapes[(rows, cols)]


@pytest.mark.parametrize("rows,cols", SMALL + CHUNKY, ids=lambda v: str(v))
def test_transposed_mvm_equals_transpose_then_mvm(hip, oracle, m8, rows, cols):  # noqa: F811
    S = shape(hip, oracle, m8, rows, cols)
    got = hip.m8_mvm_transposed(S.dA, S.dsA, rows, cols, *S.x)
    assert eq(got, S.cpu_t), "against the restatement's transpose + mvm"
    assert eq(got, S.dev_t), "against clm8_transpose + clm8_mvm"
    assert np.any(S.cpu_t[0]) and not np.any(S.cpu_t[0][-64:]) and S.cpu_t[1][-1] == 1.0, "the zero column group gives a zero block of scale 1"
    assert not np.any(got[0][-64:]) and got[1][-1] == 1.0


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("want_t", [True, False], ids=["t", "no_t"])
@pytest.mark.parametrize("rows,cols", SMALL + CHUNKY, ids=lambda v: str(v))
def test_fused_transposed_mvm_equals_the_fused_call_on_a_stored_transpose(hip, oracle, m8, rows, cols, want_t, in_place):  # noqa: F811
    S = shape(hip, oracle, m8, rows, cols)
    t, st, r, sr = hip.m8_mvm_transposed_scale_and_add(S.dA, S.dsA, rows, cols, *S.x, *S.u, A_FUSED, in_place=in_place, want_t=want_t)
    assert eq((r, sr), S.cpu_r), "r against the CPU"
    assert eq((r, sr), S.dev_fused[1]), "r against clm8_mvm_scale_and_add on the stored transpose"
    assert (t is None) != want_t
    if want_t:
        assert eq((t, st), S.cpu_t) and eq((t, st), S.dev_fused[0]), "t"
    assert not same(r, S.u[0])


@pytest.mark.parametrize("rows,cols", ST_SHAPES, ids=lambda v: str(v))
def test_stochastic_rounding_takes_the_draws_of_mvm_on_the_transpose(hip, oracle, m8, rows, cols):  # noqa: F811
    """a plain call, then a fused one on the same state: the second continues the stream where two reference calls would; bytes and
    clv_rng_get equal the restatement's walk and the device's calls on a stored transpose"""
    S = shape(hip, oracle, m8, rows, cols)
    st, o = hip.new_rng(*KEYS), oracle.rng(*KEYS)
    got1 = hip.m8_mvm_transposed(S.dA, S.dsA, rows, cols, *S.x, rng=st)
    want1 = m8.mvm(*S.At, cols, rows, *S.x, o)
    assert eq(got1, want1) and keys_equal(hip, st, o, oracle), "the plain call"
    assert not eq(want1, S.cpu_t), "the noise changed nothing: the comparison shows less than it should"
    got2 = hip.m8_mvm_transposed_scale_and_add(S.dA, S.dsA, rows, cols, *S.x, *S.u, A_FUSED, rng=st)
    want_t = m8.mvm(*S.At, cols, rows, *S.x, o)
    want_r = oracle.v8_scale_and_add(*S.u, *want_t, A_FUSED, o)
    assert eq(got2[0:2], want_t) and eq(got2[2:4], want_r) and keys_equal(hip, st, o, oracle), "the fused call behind it"
    st2 = hip.new_rng(*KEYS)
    assert eq(dev_mvm(hip, *S.dAt, cols, rows, S.x, rng=st2), got1)
    dev2 = dev_fused(hip, *S.dAt, cols, rows, S.x, S.u, A_FUSED, rng=st2)
    assert eq(dev2[0:2], got2[0:2]) and eq(dev2[2:4], got2[2:4])
    assert all(np.array_equal(a, b) for a, b in zip(hip.rng_get(st), hip.rng_get(st2)))


def composed_loop(hip, Phi, PhiT, m, n, y, iterations, K, mu, threshold, x_len, rng, prefill=0x55):
    """clm8_iht's loop call by call from the existing ABI on the stored transpose: clear, then per iteration the two fused calls and the
    threshold"""
    L = hip.lib
    b = [hip.to_device(v) for v in (*Phi, *PhiT, *y)]
    lens = {"x": n, "t1": m, "t2": m, "t3": n}
    v = {}
    for name, ln in lens.items():
        v[name] = (hip.alloc(ln), hip.alloc(ln // 16))
        for d in v[name]:
            hip.check(L.clv_memset(d.ptr, prefill, d.nbytes, None))
    v["x"] = (hip.to_device(np.zeros(n, np.int8)), hip.to_device(np.ones(n // 64, np.float32)))       # x.clear(): zero bytes, scales 1.0
    r = rng.ptr if rng else None
    for _ in range(iterations):
        hip.check(L.clm8_mvm_scale_and_add(b[0].ptr, b[1].ptr, m, n, v["x"][0].ptr, v["x"][1].ptr, b[4].ptr, b[5].ptr, -1.0, v["t1"][0].ptr,
                                           v["t1"][1].ptr, v["t2"][0].ptr, v["t2"][1].ptr, r, None))
        hip.check(L.clm8_mvm_scale_and_add(b[2].ptr, b[3].ptr, n, m, v["t2"][0].ptr, v["t2"][1].ptr, v["x"][0].ptr, v["x"][1].ptr, mu,
                                           v["t3"][0].ptr, v["t3"][1].ptr, v["x"][0].ptr, v["x"][1].ptr, r, None))
        if threshold:
            hip.check(L.clv8_threshold_mode(v["x"][0].ptr, v["x"][1].ptr, x_len, n, K, THRESHOLD_FAST, None, None))
    return {name: (v[name][0].download(np.int8, ln), v[name][1].download(np.float32, ln // 64)) for name, ln in lens.items()}


@pytest.mark.parametrize("generator", [False, True], ids=["deterministic", "generator"])
@pytest.mark.parametrize("threshold", [0, 1], ids=["GD", "IHT_FAST"])
@pytest.mark.parametrize("m,n", IHT_SHAPES, ids=lambda v: str(v))
def test_the_one_matrix_loop_equals_the_two_matrix_loop(hip, m, n, threshold, generator):
    rng = np.random.default_rng(m * 7 + n)
    Phi = matrix(rng, m, n)
    PhiT = hip.m8_transpose(*Phi, m, n)
    y = vector(rng, m)
    args = dict(iterations=3, K=n // 4, mu=0.0002, threshold=threshold, x_len=n - 5)
    st1, st2, st3 = (hip.new_rng(*KEYS), hip.new_rng(*KEYS), hip.new_rng(*KEYS)) if generator else (None, None, None)
    two = hip.m8_iht(*Phi, *PhiT, m, n, *y, rng=st1, **args)
    one = hip.m8_iht(*Phi, None, None, m, n, *y, rng=st2, **args)
    step = composed_loop(hip, Phi, PhiT, m, n, y, rng=st3, **args)
    for name in ("x", "t1", "t2", "t3"):
        assert eq(one[name], two[name]), name
        assert eq(one[name], step[name]), name + " against the loop composed call by call"
    assert np.any(two["x"][0]) and np.any(two["t3"][0])
    if generator:
        assert all(np.array_equal(a, b) for a, b in zip(hip.rng_get(st1), hip.rng_get(st2)))
        assert all(np.array_equal(a, b) for a, b in zip(hip.rng_get(st3), hip.rng_get(st2)))
        assert not np.array_equal(hip.rng_get(st1)[0], hip.rng_get(hip.new_rng(*KEYS))[0])


def test_the_nontemporal_instantiations(hip, oracle, m8p):  # noqa: F811
    """k_m8_mvm_t<M8T_U, true, ST, FUSE> for all four (ST, FUSE).  The STORED TRANSPOSE is drawn on the host, so the references are the
    OpenMP restatement's mvm on it and nothing else; the matrix under test is clm8_transpose of it (a wrong transposition fails here, it
    cannot pass).  258 output blocks: 129 workgroups of W = 2"""
    L = hip.lib
    rows, cols = 16384, 16512
    assert rows * cols > T and rows * (cols - 128) <= T and (cols // 64) % W == 0
    rng = np.random.default_rng(rows + cols)
    qt = np.frombuffer(rng.bytes(rows * cols), np.int8).copy()
    np.maximum(qt, -127, out=qt)                                            # as a quantiser leaves them
    At = (qt, rng.uniform(0.5, 2.0, size=(rows // 64) * (cols // 64)).astype(np.float32))
    dA, dsA = hip.alloc(rows * cols), hip.alloc((rows // 64) * (cols // 64) * 4)
    dAt = [hip.to_device(v) for v in At]
    hip.check(L.clm8_transpose(dAt[0].ptr, dAt[1].ptr, cols, rows, dA.ptr, dsA.ptr, None))
    hip.sync()
    del dAt
    x, u = vector(rng, rows, zero_block=1), vector(rng, cols)
    want_t = m8p.mvm(*At, cols, rows, *x)
    assert eq(hip.m8_mvm_transposed(dA, dsA, rows, cols, *x), want_t), "deterministic, plain"
    got = hip.m8_mvm_transposed_scale_and_add(dA, dsA, rows, cols, *x, *u, A_FUSED)
    assert eq(got[0:2], want_t) and eq(got[2:4], oracle.v8_scale_and_add(*u, *want_t, A_FUSED)), "deterministic, fused"
    st, o = hip.new_rng(*KEYS), oracle.rng(*KEYS)
    want1 = m8p.mvm(*At, cols, rows, *x, o)
    assert eq(hip.m8_mvm_transposed(dA, dsA, rows, cols, *x, rng=st), want1) and keys_equal(hip, st, o, oracle), "generator, plain"
    got = hip.m8_mvm_transposed_scale_and_add(dA, dsA, rows, cols, *x, *u, A_FUSED, rng=st, in_place=True, want_t=False)
    want2 = m8p.mvm(*At, cols, rows, *x, o)
    assert eq(got[2:4], oracle.v8_scale_and_add(*u, *want2, A_FUSED, o)) and keys_equal(hip, st, o, oracle), "generator, fused"
    assert np.any(want_t[0]) and not eq(want1, want_t)
