"""The transposed mixed mvm on the GPU: clm4_mvm_v8_transposed, clm4_mvm_v8_transposed_scale_and_add and clm4_iht_v8_one_matrix give, BYTE
FOR BYTE, what a stored transpose gives -- against the CPU (oracle.m4_transpose, then oracle.m4_mvm_v8, then oracle.v8_scale_and_add for
the fused form) and against the device (clm4_transpose + clm4_mvm_v8 / clm4_mvm_v8_scale_and_add, clm4_iht_v8 with PhiT =
clm4_transpose(Phi), and that loop composed call by call), the XORShift state left behind included.  Every comparison is of bytes.

Shapes (rows x cols): the smallest at which each thing can go wrong.  C = MVT8_CHUNK (rows staged in LDS per pass), S = MVT8_STEP (rows
per round: one 64-row block per wave), U = MVT8_U (rounds of loads ahead) and W = MVT8_W (output blocks per workgroup) are read from
clover_amd/csrc/mvm_t8.hip:
  128 x 128                       half a round (two of the four waves have a block), one output pair
  256 x 128, 128 x 256            non-square both ways: a product that forgets to transpose, or reads sA[cb][b] for sA[b][cb], fails
  384 x 640                       one round and a half, ten column tiles
  S (U + 1) x 128                 whole rounds: the look-ahead loads of every round but the last
  128 x 64 (W + 2), 256 x 64 (2 W + 2)     more than one workgroup; a masked last workgroup where W does not divide 2 (W = 2: cols is a
                                  multiple of 128, every workgroup is whole, MASKED below is empty)
  C - 128, C, C + 128, 2 C + 128 (x 128)   the x re-staging barriers, a half round at the end of a chunk and as a whole chunk
  C + S (U + 1) + 128 x 384       a multiple of neither C nor S U, three workgroups (W = 4: the last one masked)
Data: nibbles in [-7, 7] with -7 and 7 at known places, all tile scales distinct in [0.5, 2), one zero tile, one all-zero column group
(its result block is all zero: fix_zero_max); x and u are int8 in [-127, 127] with -127 and 127 at known places, x with one zero block
at 1 (at 0 for the 128-row shapes, whose block 0 meets the zero tile); the square matrices are not symmetric.
The nontemporal instantiations run at 16384 x 32896 (one byte row more than the 256 MiB Infinity Cache holds; 257 workgroups: one beyond
the whole groups of 16 that the kernel's XCD pairing renumbers),
as tests/test_streaming_instantiations.py does for the other kernels: the launchers have no switch that forces them at a small shape."""
import re
from pathlib import Path

import numpy as np
import pytest

from clover_amd.lib_binding import THRESHOLD_FAST

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SRC = (ROOT / "clover_amd" / "csrc" / "mvm_t8.hip").read_text()
C_ = int(re.search(r"#define\s+MVT8_CHUNK\s+(\d+)u", SRC).group(1))
S_ = int(re.search(r"#define\s+MVT8_STEP\s+(\d+)u", SRC).group(1))
U = int(re.search(r"#define\s+MVT8_U\s+(\d+)", SRC).group(1))
W = int(re.search(r"#define\s+MVT8_W\s+(\d+)", SRC).group(1))
SMALL = [(128, 128), (256, 128), (128, 256), (384, 640), (S_ * (U + 1), 128), (128, 64 * (W + 2)), (256, 64 * (2 * W + 2))]
ODD = (C_ + S_ * (U + 1) + 128, 384)
CHUNKY = [(C_ - 128, 128), (C_, 128), (C_ + 128, 128), (2 * C_ + 128, 128), ODD]
ST_SHAPES = SMALL + [(C_ + 128, 128)]
IHT_SHAPES = [(128, 256), (256, 128), (384, 640)]
KEYS = (4711, 13)
A_FUSED = 0.37
T = 256 << 20
assert ODD[0] % 128 == 0 and ODD[0] % C_ and ODD[0] % (S_ * max(U, 1)) and (64 * (W + 2)) % 128 == 0
MASKED = [c for _, c in SMALL + CHUNKY if (c // 64) % W]      # shapes whose last workgroup is masked (none while W divides 128 / 64)


def same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


def eq(p, q):
    return same(p[0], q[0]) and same(p[1], q[1])


def pack(q):
    return (((q[0::2].astype(np.uint8) & 0xF) << 4) | (q[1::2].astype(np.uint8) & 0xF)).astype(np.uint8)


def vector(rng, n, zero_block=None):
    q = rng.integers(-127, 128, size=n).astype(np.int8)
    q[[3, n - 2]] = [127, -127]
    if zero_block is not None:
        q[64 * zero_block:64 * zero_block + 64] = 0
    return q, rng.uniform(0.5, 2.0, size=n // 64).astype(np.float32)


def matrix(rng, rows, cols):
    A = rng.integers(-7, 8, size=(rows, cols)).astype(np.int8)
    A[:64, :64] = 0                                                         # a zero tile
    A[:, cols - 64:] = 0                                                    # an all-zero column group: its result block is zero
    A[rows - 1, 5], A[rows - 1, 6], A[70, 0] = 7, -7, -7
    tiles = (rows // 64) * (cols // 64)
    s = (0.5 + 1.5 * rng.permutation(tiles) / tiles).astype(np.float32)     # all distinct
    assert np.unique(s).size == tiles and (rows != cols or not np.array_equal(A, A.T))
    return pack(A.reshape(-1)), s


def keys_equal(hip, st, o, oracle):
    k1, k2 = hip.rng_get(st)
    w1, w2 = oracle.rng_keys(o)
    return np.array_equal(k1, w1) and np.array_equal(k2, w2)


def dev_fused_v8(hip, dA, dsA, rows, cols, x, u, a, rng=None):
    """(t, st, r, sr) of clm4_mvm_v8_scale_and_add on device matrix buffers: the existing call, on a stored transpose"""
    b = [hip.to_device(v) for v in (*x, *u)]
    out = [hip.alloc(rows), hip.alloc(rows // 16), hip.alloc(rows), hip.alloc(rows // 16)]
    hip.check(hip.lib.clm4_mvm_v8_scale_and_add(dA.ptr, dsA.ptr, rows, cols, b[0].ptr, b[1].ptr, b[2].ptr, b[3].ptr, a, out[0].ptr, out[1].ptr,
                                                out[2].ptr, out[3].ptr, rng.ptr if rng else None, None))
    return (out[0].download(np.int8, rows), out[1].download(np.float32, rows // 64), out[2].download(np.int8, rows),
            out[3].download(np.float32, rows // 64))


class Shape:
    """one matrix, x and u, the CPU's and the stored-transpose device results: computed once per shape"""

    def __init__(self, hip, oracle, rows, cols):
        rng = np.random.default_rng(rows * 1000003 + cols)
        self.rows, self.cols = rows, cols
        self.qA, self.sA = matrix(rng, rows, cols)
        self.x = vector(rng, rows, zero_block=0 if rows == 128 else 1)        # 128 rows: block 0 meets the zero tile, block 1 stays
        self.u = vector(rng, cols)
        self.At = oracle.m4_transpose(self.qA, self.sA, rows, cols)
        self.dA, self.dsA = hip.to_device(self.qA), hip.to_device(self.sA)
        self.cpu_t = oracle.m4_mvm_v8(*self.At, cols, rows, *self.x)
        self.cpu_r = oracle.v8_scale_and_add(*self.u, *self.cpu_t, A_FUSED)
        dAt = hip.m4_transpose(self.qA, self.sA, rows, cols)
        assert eq(dAt, self.At)
        self.dAt = [hip.to_device(v) for v in dAt]
        self.dev_t = hip.m4_mvm_v8(*dAt, cols, rows, *self.x)
        f = dev_fused_v8(hip, *self.dAt, cols, rows, self.x, self.u, A_FUSED)
        self.dev_fused = (f[0:2], f[2:4])


_shapes = {}


def shape(hip, oracle, rows, cols):
    if (rows, cols) not in _shapes:
        _shapes[(rows, cols)] = Shape(hip, oracle, rows, cols)
    return _shapes[(rows, cols)]


@pytest.mark.parametrize("rows,cols", SMALL + CHUNKY, ids=lambda v: str(v))
def test_transposed_mvm_equals_transpose_then_mvm(hip, oracle, rows, cols):
    S = shape(hip, oracle, rows, cols)
    got = hip.m4_mvm_v8_transposed(S.dA, S.dsA, rows, cols, *S.x)
    assert eq(got, S.cpu_t), "against oracle.m4_transpose + oracle.m4_mvm_v8"
    assert eq(got, S.dev_t), "against clm4_transpose + clm4_mvm_v8"
    assert np.any(S.cpu_t[0]) and not np.any(S.cpu_t[0][-64:]) and S.cpu_t[1][-1] == 1.0, "the zero column group gives a zero block of scale 1"


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("want_t", [True, False], ids=["t", "no_t"])
@pytest.mark.parametrize("rows,cols", SMALL + CHUNKY, ids=lambda v: str(v))
def test_fused_transposed_mvm_equals_the_fused_call_on_a_stored_transpose(hip, oracle, rows, cols, want_t, in_place):
    S = shape(hip, oracle, rows, cols)
    t, st, r, sr = hip.m4_mvm_v8_transposed_scale_and_add(S.dA, S.dsA, rows, cols, *S.x, *S.u, A_FUSED, in_place=in_place, want_t=want_t)
    assert eq((r, sr), S.cpu_r), "r against the CPU"
    assert eq((r, sr), S.dev_fused[1]), "r against clm4_mvm_v8_scale_and_add on the stored transpose"
    assert (t is None) != want_t
    if want_t:
        assert eq((t, st), S.cpu_t) and eq((t, st), S.dev_fused[0]), "t"
    assert not same(r, S.u[0])


@pytest.mark.parametrize("rows,cols", ST_SHAPES, ids=lambda v: str(v))
def test_stochastic_rounding_takes_the_draws_of_mvm_v8_on_the_transpose(hip, oracle, rows, cols):
    """a plain call, then a fused one on the same state: the second continues the stream where two reference calls would; bytes and
    clv_rng_get equal the oracle's walk and the device's calls on a stored transpose"""
    S = shape(hip, oracle, rows, cols)
    st, o = hip.new_rng(*KEYS), oracle.rng(*KEYS)
    got1 = hip.m4_mvm_v8_transposed(S.dA, S.dsA, rows, cols, *S.x, rng=st)
    want1 = oracle.m4_mvm_v8(*S.At, cols, rows, *S.x, o)
    assert eq(got1, want1) and keys_equal(hip, st, o, oracle), "the plain call"
    assert not eq(want1, S.cpu_t), "the noise changed nothing: the comparison shows less than it should"
    got2 = hip.m4_mvm_v8_transposed_scale_and_add(S.dA, S.dsA, rows, cols, *S.x, *S.u, A_FUSED, rng=st)
    want_t = oracle.m4_mvm_v8(*S.At, cols, rows, *S.x, o)
    want_r = oracle.v8_scale_and_add(*S.u, *want_t, A_FUSED, o)
    assert eq(got2[0:2], want_t) and eq(got2[2:4], want_r) and keys_equal(hip, st, o, oracle), "the fused call behind it"
    st2 = hip.new_rng(*KEYS)
    assert eq(hip.m4_mvm_v8(*S.At, cols, rows, *S.x, rng=st2), got1)
    dev2 = dev_fused_v8(hip, *S.dAt, cols, rows, S.x, S.u, A_FUSED, rng=st2)
    assert eq(dev2[0:2], got2[0:2]) and eq(dev2[2:4], got2[2:4])
    assert all(np.array_equal(a, b) for a, b in zip(hip.rng_get(st), hip.rng_get(st2)))


def composed_loop(hip, Phi, PhiT, m, n, y, iterations, K, mu, threshold, x_len, rng, prefill=0x55):
    """clm4_iht_v8's loop call by call from the existing ABI on the stored transpose: clear, then per iteration the two fused calls and the
    threshold -- the reference that does not rest on the persistent kernel"""
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
        hip.check(L.clm4_mvm_v8_scale_and_add(b[0].ptr, b[1].ptr, m, n, v["x"][0].ptr, v["x"][1].ptr, b[4].ptr, b[5].ptr, -1.0, v["t1"][0].ptr,
                                              v["t1"][1].ptr, v["t2"][0].ptr, v["t2"][1].ptr, r, None))
        hip.check(L.clm4_mvm_v8_scale_and_add(b[2].ptr, b[3].ptr, n, m, v["t2"][0].ptr, v["t2"][1].ptr, v["x"][0].ptr, v["x"][1].ptr, mu,
                                              v["t3"][0].ptr, v["t3"][1].ptr, v["x"][0].ptr, v["x"][1].ptr, r, None))
        if threshold:
            hip.check(L.clv8_threshold_mode(v["x"][0].ptr, v["x"][1].ptr, x_len, n, K, THRESHOLD_FAST, None, None))
    return {name: (v[name][0].download(np.int8, ln), v[name][1].download(np.float32, ln // 64)) for name, ln in lens.items()}


@pytest.mark.parametrize("generator", [False, True], ids=["deterministic", "generator"])
@pytest.mark.parametrize("threshold", [0, 1], ids=["GD", "IHT_FAST"])
@pytest.mark.parametrize("m,n", IHT_SHAPES, ids=lambda v: str(v))
def test_the_one_matrix_loop_equals_the_two_matrix_loop(hip, oracle, m, n, threshold, generator):
    rng = np.random.default_rng(m * 7 + n)
    Phi = matrix(rng, m, n)
    PhiT = hip.m4_transpose(*Phi, m, n)
    y = vector(rng, m)
    args = dict(iterations=3, K=n // 4, mu=0.002, threshold=threshold, x_len=n - 5)
    st1, st2, st3 = (hip.new_rng(*KEYS), hip.new_rng(*KEYS), hip.new_rng(*KEYS)) if generator else (None, None, None)
    two = hip.m4_iht_v8(*Phi, *PhiT, m, n, *y, rng=st1, **args)
    one = hip.m4_iht_v8(*Phi, None, None, m, n, *y, rng=st2, **args)
    step = composed_loop(hip, Phi, PhiT, m, n, y, rng=st3, **args)
    for name in ("x", "t1", "t2", "t3"):
        assert eq(one[name], two[name]), name
        assert eq(one[name], step[name]), name + " against the loop composed call by call"
    assert np.any(two["x"][0]) and np.any(two["t3"][0])
    if generator:
        assert all(np.array_equal(a, b) for a, b in zip(hip.rng_get(st1), hip.rng_get(st2)))
        assert all(np.array_equal(a, b) for a, b in zip(hip.rng_get(st3), hip.rng_get(st2)))
        assert not np.array_equal(hip.rng_get(st1)[0], hip.rng_get(hip.new_rng(*KEYS))[0])


def test_the_nontemporal_instantiations(hip, oracle):
    """k_m4_mvm8_t<MVT8_U, true, ST, FUSE> for all four (ST, FUSE).  The STORED TRANSPOSE is drawn on the host, so the references are the
    oracle's mvm on it and nothing else; the matrix under test is clm4_transpose of it (a wrong transposition fails here, it cannot pass).
    514 output blocks: 257 workgroups of W = 2, the last one outside the renumbered groups of 16"""
    L = hip.lib
    rows, cols = 16384, 32896
    assert rows * (cols // 2) > T and (W == 2 or (cols // 64) % W)
    rng = np.random.default_rng(rows + cols)
    qt = np.frombuffer(rng.bytes(rows * cols // 2), np.uint8).copy()
    qt[(qt >> 4) == 8] ^= 0x80                                              # nibbles in [-7, 7], as a quantiser leaves them
    qt[(qt & 0xF) == 8] ^= 0x08
    At = (qt, rng.uniform(0.5, 2.0, size=(rows // 64) * (cols // 64)).astype(np.float32))
    dA, dsA = hip.alloc(rows * cols // 2), hip.alloc((rows // 64) * (cols // 64) * 4)
    dAt = [hip.to_device(v) for v in At]
    hip.check(L.clm4_transpose(dAt[0].ptr, dAt[1].ptr, cols, rows, dA.ptr, dsA.ptr, None))
    hip.sync()
    del dAt
    x, u = vector(rng, rows, zero_block=1), vector(rng, cols)
    want_t = oracle.m4_mvm_v8(*At, cols, rows, *x)
    assert eq(hip.m4_mvm_v8_transposed(dA, dsA, rows, cols, *x), want_t), "deterministic, plain"
    got = hip.m4_mvm_v8_transposed_scale_and_add(dA, dsA, rows, cols, *x, *u, A_FUSED)
    assert eq(got[0:2], want_t) and eq(got[2:4], oracle.v8_scale_and_add(*u, *want_t, A_FUSED)), "deterministic, fused"
    st, o = hip.new_rng(*KEYS), oracle.rng(*KEYS)
    want1 = oracle.m4_mvm_v8(*At, cols, rows, *x, o)
    assert eq(hip.m4_mvm_v8_transposed(dA, dsA, rows, cols, *x, rng=st), want1) and keys_equal(hip, st, o, oracle), "generator, plain"
    got = hip.m4_mvm_v8_transposed_scale_and_add(dA, dsA, rows, cols, *x, *u, A_FUSED, rng=st, in_place=True, want_t=False)
    want2 = oracle.m4_mvm_v8(*At, cols, rows, *x, o)
    assert eq(got[2:4], oracle.v8_scale_and_add(*u, *want2, A_FUSED, o)) and keys_equal(hip, st, o, oracle), "generator, fused"
    assert np.any(want_t[0]) and not eq(want1, want_t)
