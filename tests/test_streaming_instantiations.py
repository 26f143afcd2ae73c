"""The nontemporal (NT = true) instantiation of every kernel that has one, each against a reference that is not a device kernel.

A launcher in clover_amd/csrc picks the streaming instantiation once its operands exceed the 256 MiB Infinity Cache (T = 268 435 456
below); the NT arm is separate code.  The map: every NT = true instantiation in the tree, crossed with the template arguments its
launcher varies, against the test id that launches it and compares the WHOLE result (or, where said, sampled rows) bit for bit with the
scalar oracle or a CPU restatement -- or "unreachable".  Ids without a file are in this file.  CU-dependent entries assume the 256 CUs
of an MI355X, and the cases below assert the launcher's predicate on their shape, so a shape that stops selecting the streaming form
fails instead of passing on the cached kernel.

transpose4.hip, clm4_transpose, rows cols > T:
- k_m4_transpose<true>, per-XCD tile order, masked tile column / row: test_m4_transpose_streaming[16384x18304]
- k_m4_transpose<true>, plain tile order: test_m4_transpose_streaming[16384x16512]
  (k_m4_transpose<false> in the per-XCD order with both edges masked and with bx = 3: test_m4_transpose_per_xcd_order_ragged[...])
matrix4.hip:
- k_m4_restore<true> (rows cols 4 > T): test_m4_restore_streaming
- k_m4_mvm64<16, true, false, false, 8> and <16, true, false, true, 8> (no generator, rows / 64 <= 2 CUs):
  test_gpu_large.py::test_mvm_few_row_groups_streaming_matrix
- k_m4_mvm64<8, true, false, false> (no generator, rows / 64 > 2 CUs): test_gpu_large.py::test_c3_mvm_65536_sampled_and_sharded,
  test_c5_whole_matrix_and_its_eight_shards_on_one_gpu (sampled row groups against the oracle)
- k_m4_mvm64<8, true, false, true>: test_m4_mvm_fused_four_wave_streaming[t] and [no_t]
- k_m4_mvm64<8, true, true, false>: test_m4_mvm_streaming_with_generator
- k_m4_mvm64<8, true, true, true>: test_m4_mvm_scale_and_add_streaming_with_generator
vector4.hip:
- k_v4_restore<true> (n_pad 4 > T): test_v4_restore_streaming
scale_add4.hip, clv4_scale_and_add, 3 n_pad / 2 > T:
- k_v4_scale_and_add_blk<true>: test_gpu_large.py::test_scale_and_add_2p28_streaming_kernels_whole_result[False]
- k_v4_scale_and_add_st<64, true>: test_gpu_large.py::test_scale_and_add_2p28_streaming_kernels_whole_result[True]
- k_v4_scale_and_add<true, 1>: unreachable (it needed n_pad / 64 < 4096 as well, i.e. 3 n_pad / 2 < 393 216); the arm is deleted
mvm_f32.hip:
- k_m4_mvm_f32<true>: test_gpu_large.py::test_mvm_f32_streaming_kernel_whole_result
mvm_batch4.hip, rows cols / 2 > T.  test_mvm_batch.py, test_mvm_batch_widths.py and test_mvm_batch_stochastic.py compare these with
the single device calls only, so:
- k_m4_mvm_batch<2, 8, true, false, false>, <4, 8, ...>, <8, 4, ...>: test_m4_mvm_batch_streaming[plain-deterministic-g] g = 2, 3, 8
- k_m4_mvm_batch<NV, U, true, true, false>: test_m4_mvm_batch_streaming[fused-deterministic-g]
- k_m4_mvm_batch<NV, U, true, false, true>: test_m4_mvm_batch_streaming[plain-generator-g]
- k_m4_mvm_batch<NV, U, true, true, true>: test_m4_mvm_batch_streaming[fused-generator-g]
mixed8.hip:
- k_v8_restore<true> (n_pad 4 > T): test_v8_restore_streaming
- k_v8_scale_and_add<true> (3 n_pad > T and n_pad / 64 < 2^21): test_v8_scale_and_add_streaming_plain_kernel
- k_v8_scale_and_add_blk<true>: test_gpu_large.py::test_v8_scale_and_add_2p27_block_kernel_whole_result
- k_m4_mvm8<MVM8_U, true, false, false>: test_m4_mvm_v8_streaming[deterministic]
- k_m4_mvm8<MVM8_U, true, true, false>: test_m4_mvm_v8_streaming[generator]
- k_m4_mvm8<MVM8_U, true, false, true>: test_m4_mvm_v8_scale_and_add_streaming[deterministic]
- k_m4_mvm8<MVM8_U, true, true, true>: test_m4_mvm_v8_scale_and_add_streaming[generator]
matrix8.hip:
- k_m8_restore<true>: test_matrix8_scale.py::test_gpu_restore_threshold[shape1]
- k_m8_mvm<true, false>, k_m8_mvm<true, true>, k_m8_mvm_f32<true>: test_matrix8_scale.py::test_gpu_mvm_threshold[shape1], test_gpu_mvm_65536
- k_m8_transpose<true>: test_matrix8_scale.py::test_gpu_transpose_threshold[shape1..3], test_gpu_transpose_65536_and_back
- k_m8_mvm_saa<true, false>: test_m8_mvm_scale_and_add_streaming[deterministic]
- k_m8_mvm_saa<true, true>: test_m8_mvm_scale_and_add_streaming[generator]
  (k_m8_quantize<true> is the stochastic form, not a streaming one)
half16.hip:
- k_f16_quantize<true>: test_half16_scale.py::test_matrix_quantize_at_32768_squared
- k_f16_restore<true>: test_f16_restore_streaming
- k_f16_scale_and_add<true>: test_f16_scale_and_add_streaming
- k_f16_mvm<4, true, false>, <4, true, true>: test_half16_scale.py::test_mvm_f16_at_65536_squared, test_mvm_f32_at_65536_squared
- k_f16_mvm<1, true, false>: test_half16_fused.py::test_gpu_fused_streaming_loads[shape0] (its clm_f16_mvm call)
- k_f16_mvm<1, true, true>: test_f16_mvm_f32_one_wave_streaming
- k_f16_mvm<1, true, false, F16Fuse>, <4, true, false, F16Fuse>: test_half16_fused.py::test_gpu_fused_streaming_loads[shape0], [shape1]
- k_f16_transpose<true>: test_half16_scale.py::test_transpose_at_65536_squared
fp32.hip:
- k_f32_scale_and_add<true>: test_f32_scale_and_add_streaming
- k_f32_mvm<1, true, false>: test_fp32_device.py::test_mvm_streams_a_matrix_beyond_the_infinity_cache_with_one_wave_workgroups
- k_f32_mvm<4, true, false>: test_fp32_device.py::test_mvm_addresses_rows_beyond_4_gib (its last 128 rows against the restatement)
- k_f32_mvm<1, true, true>: test_f32_mvm_scale_and_add_streaming[one_wave]
- k_f32_mvm<4, true, true>: test_f32_mvm_scale_and_add_streaming[four_waves]
- k_f32_transpose<true>: test_f32_transpose_streaming

Large operands are filled on the device where the existing large tests do so and downloaded once; the 4-bit matrix of 192 x 2 796 288
(3 row groups, rows no multiple of 128, 268 443 648 bytes, 85 full LDS chunks of 32768 columns and a ragged one) is shared by every
case that can use it.  Peak host memory stays below 2 GiB."""
import numpy as np
import pytest

from fp32_helpers import make_axpy, make_ops, rfp  # noqa: F401
from half16_helpers import rhp  # noqa: F401
from matrix8_helpers import binade_scales, full_range_bytes, m8p, same_keys  # noqa: F401
from test_half16_scale import finite_f16_bits
from test_mvm_batch import batch_kernel, get, pa, pairs

pytestmark = pytest.mark.gpu

T = 256 << 20
ROWS, COLS = 192, 2796288
NVEC = 8
KEYS = (2027, 9)
A_FUSED = -0.37


def same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


def eq(p, q):
    return same(p[0], q[0]) and same(p[1], q[1])


def cus(hip):
    return hip.device_info()["compute_units"]


def raw_nibbles(rng, n):
    """n / 2 random bytes: every nibble value, -8 included"""
    return np.frombuffer(rng.bytes(n // 2), np.uint8).copy()


def clover_nibbles(rng, n):
    """n / 2 random bytes whose nibbles lie in [-7, 7], as a quantiser leaves them"""
    q = raw_nibbles(rng, n)
    q[(q >> 4) == 8] ^= 0x80
    q[(q & 0xF) == 8] ^= 0x08
    return q


def extreme_scales(rng, n):
    """positive scales over 40 binades with the ends of the fp32 range and subnormals among them"""
    s = binade_scales(rng, n)
    ends = np.array([1e-45, 1e-39, 1.1754944e-38, 3.0e38, 3.4028235e38], np.float32)
    idx = rng.integers(0, n, size=max(n // 50, 5))
    s[idx] = ends[rng.integers(0, ends.size, size=idx.size)]
    return s


# ---------------------------------------------------------------- clm4_transpose
def check_m4_transpose(hip, oracle, rows, cols):
    rng = np.random.default_rng(rows + 3 * cols)
    q = raw_nibbles(rng, rows * cols)
    s = (np.arange((rows // 64) * (cols // 64), dtype=np.float32) + np.float32(0.5))       # every scale tile its own value
    qt, st = hip.m4_transpose(q, s, rows, cols)
    qo, so = oracle.m4_transpose(q, s, rows, cols)
    assert same(qt, qo) and same(st, so)
    del qo, so
    q2, s2 = hip.m4_transpose(qt, st, cols, rows)
    assert same(q2, q) and same(s2, s)


def tile_order(rows, cols):
    """(tile rows, tile columns, whether k_m4_transpose walks them in per-XCD 8 x 8 blocks)"""
    ty, tx = -(-rows // 256), -(-cols // 256)
    return ty, tx, (ty * tx) % 8 == 0 and tx % 8 == 0 and ty % 8 == 0


@pytest.mark.parametrize("rows,cols,per_xcd", [(16384, 18304, True), (16384, 16512, False)], ids=["16384x18304", "16384x16512"])
def test_m4_transpose_streaming(hip, oracle, rows, cols, per_xcd):
    """16384 x 18304: 64 x 72 tiles, the per-XCD order, the last tile column half masked; back as 18304 x 16384, the same order with a
    masked tile row.  16384 x 16512: 65 tile columns, the plain order"""
    assert rows * cols > T and cols % 256 == 128
    assert tile_order(rows, cols)[2] == per_xcd and tile_order(cols, rows)[2] == per_xcd
    check_m4_transpose(hip, oracle, rows, cols)


@pytest.mark.parametrize("rows,cols", [(1920, 1920), (2048, 6016)], ids=["1920x1920", "2048x6016"])
def test_m4_transpose_per_xcd_order_ragged(hip, oracle, rows, cols):
    """the per-XCD order is a bijection where the tiles are not all full (1920 x 1920: both edges masked) and where the blocks per tile
    row are no power of two (2048 x 6016: 24 tile columns, bx = 3); cached loads"""
    assert rows * cols <= T and tile_order(rows, cols)[2] and (rows % 256 or cols % 256)
    assert (rows, cols) != (2048, 6016) or tile_order(rows, cols)[1] // 8 == 3
    check_m4_transpose(hip, oracle, rows, cols)


# ---------------------------------------------------------------- restore
def test_m4_restore_streaming(hip, oracle):
    rows, cols = 8192, 8320
    assert rows * cols * 4 > T
    rng = np.random.default_rng(rows + cols)
    q, s = clover_nibbles(rng, rows * cols), extreme_scales(rng, (rows // 64) * (cols // 64))
    assert same(hip.m4_restore(q, s, rows, cols), oracle.m4_restore(q, s, rows, cols))


def test_v4_restore_streaming(hip, oracle):
    n = (1 << 26) + 128
    assert n * 4 > T
    rng = np.random.default_rng(n)
    q, s = clover_nibbles(rng, n), extreme_scales(rng, n // 64)
    assert same(hip.v4_restore(q, s), oracle.v4_restore(q, s))


def test_v8_restore_streaming(hip, oracle):
    n = (1 << 26) + 128
    assert n * 4 > T
    rng = np.random.default_rng(n + 8)
    q, s = full_range_bytes(rng, n), extreme_scales(rng, n // 64)
    assert same(hip.v8_restore(q, s), oracle.v8_restore(q, s))


# ---------------------------------------------------------------- clv8_scale_and_add, the plain kernel
def test_v8_scale_and_add_streaming_plain_kernel(hip, oracle):
    """n_pad = 128 x 699051: 3 n_pad = T + 128 and 1 398 102 blocks, fewer than the 2^21 from which the block kernel takes over; out of
    place, then with u aliased as the result"""
    n = 89478528
    assert 3 * n > T and n // 64 < 1 << 21
    rng = np.random.default_rng(n)
    qu, qv = full_range_bytes(rng, n), full_range_bytes(rng, n)
    su, sv = binade_scales(rng, n // 64, -10, 10), binade_scales(rng, n // 64, -10, 10)
    ro, sro = oracle.v8_scale_and_add(qu, su, qv, sv, -0.75)
    for in_place in (False, True):
        r, sr = hip.v8_scale_and_add(qu, su, qv, sv, -0.75, in_place=in_place)
        assert same(r, ro) and same(sr, sro), in_place


# ---------------------------------------------------------------- the shared 4-bit matrix
class Shared:
    def __init__(self, hip):
        L = hip.lib
        self.dA, self.dsA = hip.alloc(ROWS * COLS // 2), hip.alloc((ROWS // 64) * (COLS // 64) * 4)
        hip.check(L.clv_fill_random_nibbles(self.dA.ptr, self.dA.nbytes, 0x57, 0, None))
        hip.check(L.clv_fill_random_scales(self.dsA.ptr, self.dsA.nbytes // 4, 0x58, 0, None))
        self.dx, self.du = pairs(hip, NVEC, COLS), pairs(hip, NVEC, ROWS)              # CloverVector4 x and u, one pair per batch slot
        for j in range(NVEC):
            for (q, s), seed in ((self.dx[j], 300 + j), (self.du[j], 500 + j)):
                hip.check(L.clv_fill_random_nibbles(q.ptr, q.nbytes, seed, 0, None))
                hip.check(L.clv_fill_random_scales(s.ptr, s.nbytes // 4, seed + 100, 0, None))
        self.qA, self.sA = self.dA.download(np.uint8), self.dsA.download(np.float32)
        self.x, self.u = [get(p, COLS) for p in self.dx], [get(p, ROWS) for p in self.du]
        rng = np.random.default_rng(COLS)
        self.x8 = (full_range_bytes(rng, COLS), binade_scales(rng, COLS // 64, -4, 4))   # CloverVector8 x and u
        self.u8 = (full_range_bytes(rng, ROWS), binade_scales(rng, ROWS // 64, -4, 4))
        self.dx8 = [hip.to_device(v) for v in self.x8]
        self._seq = {}

    def sequence(self, oracle, fused, generator):
        """the oracle's results for the NVEC vectors in stream order on ONE generator (what the batch call and the sequence of single
        calls both give), as [(t, r or None, keys after the vector or None)]; computed once"""
        key = (fused, generator)
        if key not in self._seq:
            o = oracle.rng(*KEYS) if generator else None
            if not generator and (False, False) in self._seq:
                ts = [v[0] for v in self._seq[(False, False)]]
            else:
                ts = None
            out = []
            for j in range(NVEC):
                t = ts[j] if ts else oracle.m4_mvm(self.qA, self.sA, ROWS, COLS, *self.x[j], o)
                r = oracle.v4_scale_and_add(*self.u[j], *t, A_FUSED, o) if fused else None
                out.append((t, r, oracle.rng_keys(o) if generator else None))
            self._seq[key] = out
        return self._seq[key]


@pytest.fixture(scope="module")
def shared(hip):
    assert ROWS * (COLS // 2) > T and ROWS % 128 == 64 and COLS % 32768 != 0
    s = Shared(hip)
    yield s
    del s


def keys_equal(hip, st, keys):
    k1, k2 = hip.rng_get(st)
    return np.array_equal(k1, keys[0]) and np.array_equal(k2, keys[1])


# ---------------------------------------------------------------- 4-bit matrix x CloverVector8
@pytest.mark.parametrize("generator", [False, True], ids=["deterministic", "generator"])
def test_m4_mvm_v8_streaming(hip, oracle, shared, generator):
    assert ROWS * (COLS // 2) > T
    st, o = (hip.new_rng(*KEYS), oracle.rng(*KEYS)) if generator else (None, None)
    dr, dsr = hip.alloc(ROWS), hip.alloc(ROWS // 16)
    hip.check(hip.lib.clm4_mvm_v8(shared.dA.ptr, shared.dsA.ptr, ROWS, COLS, shared.dx8[0].ptr, shared.dx8[1].ptr, dr.ptr, dsr.ptr,
                                  st.ptr if st else None, None))
    ro, sro = oracle.m4_mvm_v8(shared.qA, shared.sA, ROWS, COLS, *shared.x8, o)
    assert same(dr.download(np.int8, ROWS), ro) and same(dsr.download(np.float32, ROWS // 64), sro)
    assert np.any(ro) and (not generator or same_keys(hip, st, oracle, o))


@pytest.mark.parametrize("generator", [False, True], ids=["deterministic", "generator"])
def test_m4_mvm_v8_scale_and_add_streaming(hip, oracle, shared, generator):
    assert ROWS * (COLS // 2) > T
    st, o = (hip.new_rng(*KEYS), oracle.rng(*KEYS)) if generator else (None, None)
    du, dsu = hip.to_device(shared.u8[0]), hip.to_device(shared.u8[1])
    dt, dst, dr, dsr = hip.alloc(ROWS), hip.alloc(ROWS // 16), hip.alloc(ROWS), hip.alloc(ROWS // 16)
    hip.check(hip.lib.clm4_mvm_v8_scale_and_add(shared.dA.ptr, shared.dsA.ptr, ROWS, COLS, shared.dx8[0].ptr, shared.dx8[1].ptr, du.ptr, dsu.ptr,
                                                A_FUSED, dt.ptr, dst.ptr, dr.ptr, dsr.ptr, st.ptr if st else None, None))
    to, sto = oracle.m4_mvm_v8(shared.qA, shared.sA, ROWS, COLS, *shared.x8, o)
    ro, sro = oracle.v8_scale_and_add(*shared.u8, to, sto, A_FUSED, o)
    assert same(dt.download(np.int8, ROWS), to) and same(dst.download(np.float32, ROWS // 64), sto)
    assert same(dr.download(np.int8, ROWS), ro) and same(dsr.download(np.float32, ROWS // 64), sro)
    assert np.any(to) and not same(ro, shared.u8[0]) and (not generator or same_keys(hip, st, oracle, o))


# ---------------------------------------------------------------- 4-bit matrix x CloverVector4 with a generator (excludes the 8-lane kernel)
def test_m4_mvm_streaming_with_generator(hip, oracle, shared):
    assert ROWS * (COLS // 2) > T
    want = shared.sequence(oracle, False, True)[0]
    st, out = hip.new_rng(*KEYS), pairs(hip, 1, ROWS)[0]
    hip.check(hip.lib.clm4_mvm(shared.dA.ptr, shared.dsA.ptr, ROWS, COLS, shared.dx[0][0].ptr, shared.dx[0][1].ptr, out[0].ptr, out[1].ptr,
                               st.ptr, None))
    assert eq(get(out, ROWS), want[0]) and keys_equal(hip, st, want[2])
    assert not eq(want[0], shared.sequence(oracle, False, False)[0][0]), "the noise changed nothing: the comparison shows less than it should"


def test_m4_mvm_scale_and_add_streaming_with_generator(hip, oracle, shared):
    assert ROWS * (COLS // 2) > T
    want = shared.sequence(oracle, True, True)[0]
    st, t, r = hip.new_rng(*KEYS), pairs(hip, 1, ROWS)[0], pairs(hip, 1, ROWS)[0]
    du = shared.du[0]
    hip.check(hip.lib.clm4_mvm_scale_and_add(shared.dA.ptr, shared.dsA.ptr, ROWS, COLS, shared.dx[0][0].ptr, shared.dx[0][1].ptr, du[0].ptr, du[1].ptr,
                                             A_FUSED, t[0].ptr, t[1].ptr, r[0].ptr, r[1].ptr, st.ptr, None))
    assert eq(get(t, ROWS), want[0]) and eq(get(r, ROWS), want[1]) and keys_equal(hip, st, want[2])


# ---------------------------------------------------------------- the batched kernel
@pytest.mark.parametrize("g", [2, 3, 8])
@pytest.mark.parametrize("generator", [False, True], ids=["deterministic", "generator"])
@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
def test_m4_mvm_batch_streaming(hip, oracle, shared, fused, generator, g):
    """groups of 2, 3 and 8 vectors run as NV = 2, 4 and 8 (CLV_MVM_BATCH=1: the batched kernel whatever the measured rule says); every
    vector against the oracle's sequence, and the state left behind"""
    assert ROWS * (COLS // 2) > T
    L = hip.lib
    want = shared.sequence(oracle, fused, generator)
    st = hip.new_rng(*KEYS) if generator else None
    x, sx = pa([d[0] for d in shared.dx[:g]]), pa([d[1] for d in shared.dx[:g]])
    t = pairs(hip, g, ROWS)
    launches = L.clv_mvm_batch_launches()
    with batch_kernel("1"):
        if fused:
            r = pairs(hip, g, ROWS)
            hip.check(L.clm4_mvm_scale_and_add_batch(shared.dA.ptr, shared.dsA.ptr, ROWS, COLS, g, x, sx, pa([d[0] for d in shared.du[:g]]),
                                                     pa([d[1] for d in shared.du[:g]]), A_FUSED, pa([d[0] for d in t]), pa([d[1] for d in t]),
                                                     pa([d[0] for d in r]), pa([d[1] for d in r]), st.ptr if st else None, None))
        else:
            hip.check(L.clm4_mvm_batch(shared.dA.ptr, shared.dsA.ptr, ROWS, COLS, g, x, sx, pa([d[0] for d in t]), pa([d[1] for d in t]),
                                       st.ptr if st else None, None))
    hip.sync()
    assert L.clv_mvm_batch_launches() - launches == 1
    for j in range(g):
        assert eq(get(t[j], ROWS), want[j][0]), f"A x of vector {j}"
        if fused:
            assert eq(get(r[j], ROWS), want[j][1]), f"r of vector {j}"
            assert eq(get(shared.du[j], ROWS), shared.u[j]), f"u of vector {j} was written"
    assert not eq(want[0][0], want[1][0])
    if generator:
        assert keys_equal(hip, st, want[g - 1][2])


# ---------------------------------------------------------------- streaming, fused, four waves per row group, deterministic
@pytest.mark.parametrize("want_t", [True, False], ids=["t", "no_t"])
def test_m4_mvm_fused_four_wave_streaming(hip, oracle, want_t):
    """one row group more than two per CU: past the 8-lane kernel's rule"""
    L = hip.lib
    rows, cols = 64 * (2 * cus(hip) + 1), 16384
    assert rows * (cols // 2) > T and rows // 64 > 2 * cus(hip)
    dA, dsA = hip.alloc(rows * cols // 2), hip.alloc((rows // 64) * (cols // 64) * 4)
    hip.check(L.clv_fill_random_nibbles(dA.ptr, dA.nbytes, 0x61, 0, None))
    hip.check(L.clv_fill_random_scales(dsA.ptr, dsA.nbytes // 4, 0x62, 0, None))
    rng = np.random.default_rng(rows)
    (qx, sx), (qu, su) = ((clover_nibbles(rng, n), rng.uniform(0.5, 2, n // 64).astype(np.float32)) for n in (cols, rows))
    dx, dsx, du, dsu = (hip.to_device(v) for v in (qx, sx, qu, su))
    t, r = (pairs(hip, 1, rows)[0] if want_t else None), pairs(hip, 1, rows)[0]
    hip.check(L.clm4_mvm_scale_and_add(dA.ptr, dsA.ptr, rows, cols, dx.ptr, dsx.ptr, du.ptr, dsu.ptr, A_FUSED, t[0].ptr if t else None,
                                       t[1].ptr if t else None, r[0].ptr, r[1].ptr, None, None))
    to = oracle.m4_mvm(dA.download(np.uint8), dsA.download(np.float32), rows, cols, qx, sx)
    ro = oracle.v4_scale_and_add(qu, su, *to, A_FUSED)
    assert eq(get(r, rows), ro) and (t is None or eq(get(t, rows), to))
    assert np.any(to[0]) and not same(ro[0], qu)


# ---------------------------------------------------------------- CloverMatrix8, fused
@pytest.mark.parametrize("generator", [False, True], ids=["deterministic", "generator"])
def test_m8_mvm_scale_and_add_streaming(hip, oracle, m8p, generator):  # noqa: F811
    rows, cols = 16384, 16512
    assert rows * cols > T
    rng = np.random.default_rng(rows + cols)
    qA, sA = full_range_bytes(rng, rows * cols), binade_scales(rng, (rows // 64) * (cols // 64), -4, 4)
    qx, sx = full_range_bytes(rng, cols), binade_scales(rng, cols // 64, -4, 4)
    qu, su = full_range_bytes(rng, rows), binade_scales(rng, rows // 64, -4, 4)
    st, o = (hip.new_rng(*KEYS), oracle.rng(*KEYS)) if generator else (None, None)
    t, s_t, r, sr = hip.m8_mvm_scale_and_add(qA, sA, rows, cols, qx, sx, qu, su, A_FUSED, rng=st)
    to, sto = m8p.mvm(qA, sA, rows, cols, qx, sx, o)
    ro, sro = oracle.v8_scale_and_add(qu, su, to, sto, A_FUSED, o)
    assert same(t, to) and same(s_t, sto) and same(r, ro) and same(sr, sro)
    assert np.any(to) and (not generator or same_keys(hip, st, oracle, o))


# ---------------------------------------------------------------- fp32
def test_f32_scale_and_add_streaming(hip, rfp):  # noqa: F811
    n = 22369664
    assert n * 12 > T and n % 128 == 0
    for kind in ("magnitudes", "cancel"):
        u, v, a = make_axpy(kind, n, n)
        want = rfp.scale_and_add(u, v, a)
        assert same(hip.f32_scale_and_add(u, v, float(a)), want), kind
        assert same(hip.f32_scale_and_add(u, v, float(a), in_place=True), want), kind


def test_f32_transpose_streaming(hip):
    """4096 x 8196: the last tile column is 4 elements wide; every element carries its own bit pattern"""
    rows, cols = 4096, 8196
    assert rows * cols * 8 > T and cols % 64 == 4
    A = np.arange(rows * cols, dtype=np.uint32)
    got = hip.f32_transpose(A.view(np.float32), rows, cols)
    assert np.array_equal(got.view(np.uint32).reshape(cols, rows), A.reshape(rows, cols).T)


@pytest.mark.parametrize("form", ["one_wave", "four_waves"])
def test_f32_mvm_scale_and_add_streaming(hip, rfp, form):  # noqa: F811
    """one random block of 1 000 003 values (a prime: no two rows start at the same place in it) repeated: the case is about the load
    path, every row still has its own sum"""
    rows, cols = (128, (1 << 19) + 128) if form == "one_wave" else (32 * 2 * cus(hip), 4224)
    assert rows * cols * 4 > T and (rows // 32 >= 2 * cus(hip)) == (form == "four_waves")
    block = make_ops("magnitudes", 1, 1000003, rows)[0]
    A = np.tile(block, rows * cols // block.size + 1)[:rows * cols]
    x, u = make_ops("magnitudes", 1, cols, 2)[0], make_ops("magnitudes", 1, rows, 3)[0]
    a = 0.37
    d = rfp.mvm(A, rows, cols, x)
    r = rfp.scale_and_add(u, d, a)
    dA = hip.to_device(A)
    for want_t in (False, True):
        t, r2 = hip.f32_mvm_scale_and_add(dA, rows, cols, x, u, a, in_place=True, want_t=want_t)
        assert same(r2, r) and (t is None) != want_t and (t is None or same(t, d)), want_t
    assert np.unique(d).size > rows // 2


# ---------------------------------------------------------------- f16
def test_f16_restore_streaming(hip, rhp):  # noqa: F811
    n = 44739328
    assert n * 6 > T and n % 128 == 0
    h = finite_f16_bits(np.random.default_rng(n), n)
    got, want = hip.f16_restore(h), rhp.restore(h)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_f16_scale_and_add_streaming(hip, rhp):  # noqa: F811
    n = 44739328
    assert n * 6 > T
    rng = np.random.default_rng(n + 1)
    u, v = finite_f16_bits(rng, n), finite_f16_bits(rng, n)
    want = rhp.scale_and_add(u, v, np.float32(-1.25))
    for in_place in (False, True):
        assert np.array_equal(hip.f16_scale_and_add(u, v, -1.25, in_place=in_place), want), in_place


def test_f16_mvm_f32_one_wave_streaming(hip, rhp):  # noqa: F811
    """clm_f16_mvm_f32 past 256 MiB with fewer than two four-wave workgroups per CU: 16440 rows leave the last one-wave workgroup 8 of
    its 16 rows"""
    rows, cols = 16440, 8320
    assert rows * cols * 2 > T and rows // 64 < 2 * cus(hip)
    rng = np.random.default_rng(rows)
    A = finite_f16_bits(rng, rows * cols)
    x = rng.standard_normal(cols, dtype=np.float32)
    got, want = hip.mf16_mvm_f32(A, rows, cols, x), rhp.mvm_f32(A, rows, cols, x)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.flatnonzero(got != want)[:8]
