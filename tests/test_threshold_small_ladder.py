"""The one-workgroup threshold kernels of clover_amd/csrc/threshold4.hip at EVERY compiled width, FAST mode.

W, the words a thread owns, is a template parameter of k_thresh_small / k_thresh_small_batch (CloverVector4), k_thresh8_small
(CloverVector8) and k_f32_thresh_small (CloverVector32): every value is differently unrolled code, chosen by the launcher as
ceil(ceil(n / EPW) / TS_THREADS) with EPW elements per 32-bit word.  The sizes below are DERIVED from TS_THREADS, TS_MAXW and TS8_MAXW as
the source states them, so that a changed ladder moves the cases with it: for every W its last size, the one before, the first of the
next W, one ragged size that ends inside a word and inside a block; the sizes around a word and around one and two blocks; and n = 100
inside the largest eligible n_pad (W comes from n, eligibility from n_pad).

Every FAST result is held to
  (a) the CPU restatement of the lowest-index rule, over the whole buffer, padding included;
  (b) the multiset of NON-ZERO magnitudes that the reference's heap walk keeps (with zero scales and tau = 0 the two sides may keep
      different zero-magnitude elements: the reference's choice among equal values is its heap's history, so zeros are left out);
  (c) idempotence: the call on its own result changes nothing;
  (d) the padding, filled with non-zero values, is untouched;
and k >= n gives the input back.  Infinite and NaN values or scales are left out where the header states no order for them (4- and 8-bit;
NaN in fp32).  The CPU test at the end checks the derived size list and (a) against (b) on the restatements alone."""
import os
import re
from pathlib import Path

import numpy as np
import pytest

from clover_amd.lib_binding import THRESHOLD_FAST
from fp32_helpers import fast_threshold_model, pad128, rf, threshold_data  # noqa: F401
from test_mixed8 import _threshold8_lowest_index
from test_mvm_batch import clustered, get, pa, pairs
from test_threshold_large3 import lowest_index_rule, make, nibbles

ROOT = Path(__file__).resolve().parent.parent
_SRC = (ROOT / "clover_amd" / "csrc" / "threshold4.hip").read_text()


def _define(name):
    return int(re.search(rf"#define\s+{name}\s+(\d+)\b", _SRC).group(1))


TS_THREADS, TS_MAXW, TS8_MAXW, TS_BATCH_GROUP = (_define(n) for n in ("TS_THREADS", "TS_MAXW", "TS8_MAXW", "TS_BATCH_GROUP"))
EPW = {4: 8, 8: 4, 32: 1}                                    # elements per 32-bit word
MAXW = {4: TS_MAXW, 8: TS8_MAXW, 32: TS_MAXW}


def ladder(bits):
    return [1 << i for i in range(MAXW[bits].bit_length()) if (1 << i) <= MAXW[bits]]


def last_size(bits, W):
    return TS_THREADS * W * EPW[bits]


def ragged_size(bits, W):
    return last_size(bits, W) - 3 * EPW[bits] - 1           # ends inside a word (EPW > 1) and inside a block of 64


def words_per_thread(bits, n):
    """the launcher's selection, rounded up to the compiled width"""
    w = -(-((n + EPW[bits] - 1) // EPW[bits]) // TS_THREADS)
    return next(W for W in ladder(bits) if w <= W)


def cases(bits):
    e = EPW[bits]
    ns = {1, 2, e - 1, e, e + 1, 63, 64, 65, 127, 128, 129}
    for W in ladder(bits):
        ns |= {last_size(bits, W) - 1, last_size(bits, W), ragged_size(bits, W)}
        if W < MAXW[bits]:
            ns.add(last_size(bits, W) + 1)
    return [(n, pad128(n)) for n in sorted(ns) if n >= 1] + [(100, last_size(bits, MAXW[bits]))]


CASES = {bits: cases(bits) for bits in EPW}


def _ids(cs):
    return [f"{n}in{n_pad}" for n, n_pad in cs]


def ks(n, nz):
    """0, 1, a quarter, all but one, past the non-zero elements (tau = 0), and the two that leave the input alone"""
    return sorted({0, 1, n // 4, n - 1, min(n - 1, nz + 5), n, n + 5})


def same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


def nonzero_sorted(m):
    return np.sort(m[m > 0])


# ---------------------------------------------------------------- CloverVector4
KINDS4 = ["uniform", "sparse", "equal", "wide", "subnormal", "edge", "zeroscale", "integers", "fields"]


def pack(nib):
    return (((nib[0::2] & 0xF) << 4) | (nib[1::2] & 0xF)).astype(np.uint8)


def vector4(oracle, kind, n, n_pad, seed=0):
    """(packed nibbles, scales) of n_pad elements; the elements from n on are non-zero.  Kinds: `make` of test_threshold_large3 (raw
    nibbles, -8 included), the reference's test data quantized, and `fields`: blocks with 16 .. 64 elements of |q| = 4 (the 7-bit count
    whose field straddles bit 32 of the packed counts, filled to its top) and blocks of 64 equal nibbles, under a pool of four scales"""
    rng = np.random.default_rng(1000003 * seed + 131 * n + KINDS4.index(kind))
    if kind == "integers":
        q, s = oracle.v4_quantize(rng.integers(-40, 41, size=n_pad).astype(np.float32))
        nib = nibbles(q)
    elif kind == "fields":
        nib = np.empty((n_pad // 64, 64), np.int32)
        others = np.array([-8, -7, -6, -5, -3, -2, -1, 0, 1, 2, 3, 5, 6, 7])
        for b in range(n_pad // 64):
            if rng.random() < 0.4:
                nib[b] = rng.choice(np.array([-8, -7, -4, -1, 1, 4, 7]))
            else:
                c = int(rng.integers(16, 65))
                blk = np.concatenate([rng.choice(np.array([-4, 4]), size=c), rng.choice(others, size=64 - c)])
                nib[b] = rng.permutation(blk)
        nib = nib.reshape(-1)
        s = np.array([0.5, 1.0, 1.0, 2.0], np.float32)[rng.integers(0, 4, size=n_pad // 64)]
    else:
        q, s = make(rng, n_pad, kind)
        nib = nibbles(q)
    tail = nib[n:]
    tail[tail == 0] = 5
    return pack(nib), s


def expect4(oracle, q, s, n, k):
    """(the lowest-index rule's buffer, the sorted non-zero magnitudes the reference's heap walk keeps or None where k leaves no choice)"""
    if k >= n:
        return q.copy(), None
    if k == 0:
        nib = nibbles(q)
        nib[:n] = 0
        return pack(nib), None
    mags = np.abs(oracle.v4_restore(q, s))[:n]
    return lowest_index_rule(oracle, q, s, n, k), nonzero_sorted(mags[nibbles(oracle.v4_threshold(q, s, n, k))[:n] != 0])


def check4(oracle, q, s, n, k, got, expect, what):
    want, ref_mags = expect
    assert same(got, want), (what, "lowest-index rule", np.flatnonzero(got != want)[:8])
    tail = nibbles(got)[n:]
    assert np.array_equal(tail, nibbles(q)[n:]) and np.all(tail != 0), (what, "padding")
    if ref_mags is not None:
        mags = np.abs(oracle.v4_restore(q, s))[:n]
        assert np.array_equal(nonzero_sorted(mags[nibbles(got)[:n] != 0]), ref_mags), (what, "the reference's surviving magnitudes")


@pytest.mark.gpu
@pytest.mark.parametrize("n,n_pad", CASES[4], ids=_ids(CASES[4]))
def test_gpu_v4_small_threshold_at_every_width(hip, oracle, n, n_pad):
    for kind in KINDS4:
        q, s = vector4(oracle, kind, n, n_pad)
        for k in ks(n, int(np.count_nonzero(nibbles(q)[:n]))):
            what = (kind, n, n_pad, k)
            got = hip.v4_threshold(q, s, n, k)
            check4(oracle, q, s, n, k, got, expect4(oracle, q, s, n, k), what)
            if k >= n:
                assert same(got, q), (what, "k >= n changes nothing")
            assert same(hip.v4_threshold(got, s, n, k), got), (what, "idempotent")


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["last", "ragged"])
@pytest.mark.parametrize("W", ladder(4))
def test_gpu_v4_threshold_batch_at_every_width(hip, oracle, W, which):
    """k_thresh_small_batch<W>: vectors of different kinds in one call (vector 1 is one magnitude everywhere), a group that is not full,
    a full one, and a full one plus a second launch; every vector against the restatement and the reference, not the single call"""
    L = hip.lib
    n = last_size(4, W) if which == "last" else ragged_size(4, W)
    n_pad = pad128(n)
    assert words_per_thread(4, n) == W
    vecs = [vector4(oracle, KINDS4[j % len(KINDS4)], n, n_pad, seed=j + 1) for j in range(TS_BATCH_GROUP + 1)]
    vecs[1] = clustered(n_pad, 0, all_equal=True)
    src = [(hip.to_device(q), hip.to_device(s)) for q, s in vecs]
    expect = {}
    for nvec in (2, 3, TS_BATCH_GROUP, TS_BATCH_GROUP + 1):
        for k in (sorted({0, 1, n // 4, n - 1, n}) if nvec == 3 else (n // 4,)):
            w = pairs(hip, nvec, n_pad)
            for (wq, ws), (pq, ps) in zip(w, src):
                hip.check(L.clv_memcpy_d2d(wq.ptr, pq.ptr, n_pad // 2, None))
                hip.check(L.clv_memcpy_d2d(ws.ptr, ps.ptr, n_pad // 16, None))
            hip.check(L.clv4_threshold_batch(pa([d[0] for d in w]), pa([d[1] for d in w]), nvec, n, n_pad, k, THRESHOLD_FAST, None))
            hip.sync()
            for j in range(nvec):
                q, s = vecs[j]
                if (j, k) not in expect:
                    expect[j, k] = expect4(oracle, q, s, n, k)
                got, got_s = get(w[j], n_pad)
                check4(oracle, q, s, n, k, got, expect[j, k], (W, which, nvec, k, j))
                assert same(got_s, s), (W, which, nvec, k, j, "scales")
    kept = np.count_nonzero(nibbles(expect[1, n // 4][0])[:n])
    assert kept == n // 4, "the all-equal vector keeps exactly k"


# ---------------------------------------------------------------- CloverVector8
KINDS8 = ["raw", "integers", "sparse", "equal", "wide", "subnormal", "zeroscale"]


def vector8(oracle, kind, n, n_pad):
    """(int8 bytes over -128 .. 127, scales); 127 s stays finite; the elements from n on are non-zero"""
    rng = np.random.default_rng(977 * n + KINDS8.index(kind))
    q = rng.integers(-128, 128, size=n_pad).astype(np.int8)
    s = rng.uniform(0.5, 2, size=n_pad // 64).astype(np.float32)
    if kind == "integers":
        q, s = oracle.v8_quantize(rng.integers(-40, 41, size=n_pad).astype(np.float32))
    elif kind == "sparse":
        q[rng.random(q.size) < 0.9] = 0
    elif kind == "equal":
        q[:] = -128
        s[:] = 1.25
    elif kind == "wide":
        s = np.exp2(rng.uniform(-30, 30, size=s.size)).astype(np.float32)
    elif kind == "subnormal":
        s = (rng.uniform(0.5, 2, size=s.size) * 1e-39).astype(np.float32)
    elif kind == "zeroscale":
        s[rng.random(s.size) < 0.5] = 0.0
    tail = q[n:]
    tail[tail == 0] = 5
    return q, s


def mags8(q, s, n):
    """CloverVector8::get: ((float) q * s) / 127"""
    return np.abs((q.astype(np.float32) * np.repeat(s, 64)) / np.float32(127.0))[:n]


def expect8(oracle, q, s, n, k):
    want = _threshold8_lowest_index(q, s, n, k)
    if k == 0 or k >= n:
        return want, None
    return want, nonzero_sorted(mags8(q, s, n)[oracle.v8_threshold(q, s, n, k)[:n] != 0])


def check8(q, s, n, k, got, expect, what):
    want, ref_mags = expect
    assert same(got, want), (what, "lowest-index rule", np.flatnonzero(got != want)[:8])
    assert np.array_equal(got[n:], q[n:]) and np.all(got[n:] != 0), (what, "padding")
    if ref_mags is not None:
        assert np.array_equal(nonzero_sorted(mags8(q, s, n)[got[:n] != 0]), ref_mags), (what, "the reference's surviving magnitudes")


@pytest.mark.gpu
@pytest.mark.parametrize("n,n_pad", CASES[8], ids=_ids(CASES[8]))
def test_gpu_v8_small_threshold_at_every_width(hip, oracle, n, n_pad):
    for kind in KINDS8:
        q, s = vector8(oracle, kind, n, n_pad)
        for k in ks(n, int(np.count_nonzero(q[:n]))):
            what = (kind, n, n_pad, k)
            got = hip.v8_threshold(q, s, n, k)
            check8(q, s, n, k, got, expect8(oracle, q, s, n, k), what)
            if k >= n:
                assert same(got, q), (what, "k >= n changes nothing")
            assert same(hip.v8_threshold(got, s, n, k), got), (what, "idempotent")


# ---------------------------------------------------------------- CloverVector32
KINDS32 = ["distinct", "ties", "equal", "zeros", "inf"]
PAD32 = np.float32(-5.5)


def vector32(kind, n, n_pad):
    rng = np.random.default_rng(31 * n + KINDS32.index(kind))
    sign = (rng.integers(0, 2, size=n_pad).astype(np.uint32) << 31)
    if kind in ("distinct", "ties"):
        x = threshold_data(kind, n_pad, n)
    elif kind == "equal":
        x = (np.full(n_pad, np.float32(1.5).view(np.uint32), np.uint32) | sign).view(np.float32)
    elif kind == "zeros":                                            # +-0 and subnormals
        x = (np.where(rng.random(n_pad) < 0.6, 0, rng.integers(1, 0x800000, size=n_pad)).astype(np.uint32) | sign).view(np.float32)
    else:                                                            # +-inf among finite values
        x = threshold_data("distinct", n_pad, n + 1)
        x[rng.integers(0, n_pad, size=max(n // 50, 1))] = np.inf
        x[rng.integers(0, n_pad, size=max(n // 50, 1))] = -np.inf
    x = np.ascontiguousarray(x, dtype=np.float32).copy()
    x[n:] = PAD32
    return x


def expect32(rf, x, n, k):
    want = fast_threshold_model(x, n, k)
    if k == 0 or k >= n:
        return want, None
    return want, nonzero_sorted(np.abs(rf.threshold(x, n, k)[:n]))


def check32(x, n, k, got, expect, what):
    want, ref_mags = expect
    assert same(got, want), (what, "lowest-index rule", np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:8])
    assert same(got[n:], x[n:]) and np.all(got[n:] == PAD32), (what, "padding")
    if ref_mags is not None:
        assert np.array_equal(nonzero_sorted(np.abs(got[:n])), ref_mags), (what, "the reference's surviving magnitudes")


def _f32_large_path(hip, x, n, k):
    os.environ["CLV_F32_THRESHOLD_SMALL"] = "0"
    try:
        return hip.f32_threshold(x, n, k, THRESHOLD_FAST)
    finally:
        del os.environ["CLV_F32_THRESHOLD_SMALL"]


@pytest.mark.gpu
@pytest.mark.parametrize("n,n_pad", CASES[32], ids=_ids(CASES[32]))
def test_gpu_f32_small_threshold_at_every_width(hip, rf, n, n_pad):
    for kind in KINDS32:
        x = vector32(kind, n, n_pad)
        for k in ks(n, int(np.count_nonzero(x[:n]))):
            what = (kind, n, n_pad, k)
            got = hip.f32_threshold(x, n, k, THRESHOLD_FAST)
            check32(x, n, k, got, expect32(rf, x, n, k), what)
            if k >= n:
                assert same(got, x), (what, "k >= n changes nothing")
            assert same(hip.f32_threshold(got, n, k, THRESHOLD_FAST), got), (what, "idempotent")
            assert same(_f32_large_path(hip, x, n, k), got), (what, "CLV_F32_THRESHOLD_SMALL=0")


# ---------------------------------------------------------------- CPU: the size list and the two references against each other
def test_the_size_list_walks_every_width_and_the_restatements_agree(oracle, rf):
    for bits in EPW:
        ns = [n for n, _ in CASES[bits]]
        assert ladder(bits)[-1] == MAXW[bits] and len(ladder(bits)) == MAXW[bits].bit_length()
        for W in ladder(bits):
            first = last_size(bits, W // 2) + 1 if W > 1 else 1
            rag = ragged_size(bits, W)
            assert {first, last_size(bits, W), rag} <= set(ns), (bits, W)
            assert [words_per_thread(bits, m) for m in (first, rag, last_size(bits, W))] == [W, W, W], (bits, W)
            assert rag % 64 and (EPW[bits] == 1 or rag % EPW[bits]), (bits, W)
        assert all(n <= n_pad <= last_size(bits, MAXW[bits]) and n_pad % 128 == 0 for n, n_pad in CASES[bits])
        assert (100, last_size(bits, MAXW[bits])) in CASES[bits]
    assert last_size(4, TS_MAXW) == 131072 and last_size(8, TS8_MAXW) == 32768 and last_size(32, TS_MAXW) == 16384   # what the headers document

    def survivors(mags, kept):
        return nonzero_sorted(mags[kept])
    for n, n_pad in CASES[4]:
        for kind in KINDS4:
            q, s = vector4(oracle, kind, n, n_pad)
            mags = np.abs(oracle.v4_restore(q, s))[:n]
            for k in sorted({n // 4, min(n - 1, int(np.count_nonzero(nibbles(q)[:n])) + 5)} - {0}):
                want, ref_mags = expect4(oracle, q, s, n, k)
                assert np.array_equal(nibbles(want)[n:], nibbles(q)[n:]), (4, kind, n, k)
                assert np.array_equal(survivors(mags, nibbles(want)[:n] != 0), ref_mags), (4, kind, n, k)
                assert np.count_nonzero(nibbles(want)[:n]) <= k, (4, kind, n, k)
    for n, n_pad in CASES[8]:
        for kind in KINDS8:
            q, s = vector8(oracle, kind, n, n_pad)
            assert np.all(np.isfinite(np.float32(127.0) * s)), kind
            for k in sorted({n // 4, min(n - 1, int(np.count_nonzero(q[:n])) + 5)} - {0}):
                want, ref_mags = expect8(oracle, q, s, n, k)
                assert np.array_equal(want[n:], q[n:]), (8, kind, n, k)
                assert np.array_equal(survivors(mags8(q, s, n), want[:n] != 0), ref_mags), (8, kind, n, k)
    for n, n_pad in CASES[32]:
        for kind in KINDS32:
            x = vector32(kind, n, n_pad)
            for k in sorted({n // 4, min(n - 1, int(np.count_nonzero(x[:n])) + 5)} - {0}):
                want, ref_mags = expect32(rf, x, n, k)
                assert same(want[n:], x[n:]), (32, kind, n, k)
                assert np.array_equal(nonzero_sorted(np.abs(want[:n])), ref_mags), (32, kind, n, k)
