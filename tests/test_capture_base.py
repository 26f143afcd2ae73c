"""Every entry point of the 4-bit, mixed (CloverVector8) and CloverMatrix8 C ABI (include/clover_hip.h) that enqueues work on a stream,
captured once into a hipGraph in global mode and replayed on changing operands -- the table tests/test_fp32_capture.py and
tests/test_half16_capture.py keep for their widths.

A row is (operands per seed, enqueue, output bytes).  One ordinary call is made on the stream first (the library's scratch, the hand-over
slots and every once-per-device attribute are set up outside the capture), then the call is captured, then replayed three times on freshly
uploaded operands with the outputs prefilled with 0xA5: every replay equals the eager call on the same operands byte for byte, the
replays differ from one another, and on the first operand set the replayed bytes also equal the CPU reference the suite uses for that
entry (the oracle, tests/matrix8_restate.c) -- so a row cannot pass on "eager and replay are wrong alike".  A launch on the wrong stream,
a host-side value baked into a kernel argument or an allocation inside the call, invisible to every stream=None test, fails here.

Rows without a byte reference: dot FAST (a tolerance against the float64 dot, the one of tests/test_graph_capture.py), the three
synthetic-data fills (the binding has no CPU form of them).  The fills take no operand that a replay could change, only host arguments,
which a graph replays by design: their replays are equal, and only the prefill shows that they ran.

The GEMM rows run in this process on the workgroup tile the library picks for 128 x 256 x 384 (128 x 128: fewer tiles than CUs) and once
more in a child process under CLV_GEMM_TILE=256 (read once per process).  The loop rows run with CLV_IHT_PERSISTENT=0, read per call: the
graph holds the launch-per-step kernels, and clv_iht_persistent_launches() does not move.

Stochastic rows: two generator states seeded alike, A in graph mode (clv_rng_graph_mode) inside the graph, B on eager calls; after every
replay the outputs and clv_rng_get of A equal those of B.

The tests at the end are about the library's scratch under capture (clv_internal_workspace, clover_amd/csrc/runtime.hip), and the CPU test
before them holds the three dicts that account for every name of lib_binding.SIGNATURES."""
import contextlib
import ctypes as C
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from capture_helpers import Graph, fresh_graph
from clover_amd.lib_binding import DOT_EXACT, DOT_FAST, SIGNATURES, THRESHOLD_FAST, THRESHOLD_REFERENCE
from conftest import random_packed

ROOT = Path(__file__).resolve().parent.parent
_CSRC = ROOT / "clover_amd" / "csrc"


def _define(source, name):
    return int(re.search(rf"#define\s+{name}\s+(\d+)u?\b", (_CSRC / source).read_text()).group(1))


# the sizes at which the launchers change kernels, as the sources state them
SAA_BLK_MIN_BLOCKS = _define("scale_add4.hip", "SAA_BLK_MIN_BLOCKS")
TS_THREADS, TS_MAXW, TS8_MAXW = (_define("threshold4.hip", n) for n in ("TS_THREADS", "TS_MAXW", "TS8_MAXW"))
SMALL_LAST = {4: TS_THREADS * TS_MAXW * 8, 8: TS_THREADS * TS8_MAXW * 4}       # ThreshHost<BITS>: n_pad <= TS_THREADS * MAXW * EPW is one workgroup

N = 8192 + 128
NBLK = 64 * SAA_BLK_MIN_BLOCKS                                                # the first size of k_v4_scale_and_add_blk
ROWS, COLS = 256, 512
GM, GN, GK = 128, 256, 384                                                    # GEMM: A is GM x GK, B is GN x GK
M_IHT, N_IHT, ITERS = 128, 256, 3
K_REF = 700
A_SAA = 0.37
NVEC = 3


def same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


def u8(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def layout(**sizes):
    """name -> byte offset of each output inside one buffer (256-byte aligned), and the buffer's size"""
    off, at = {}, 0
    for name, size in sizes.items():
        off[name] = at
        at += (size + 255) & ~255
    return off, at


class Refs:
    """the CPU references: the oracle, and the CloverMatrix8 and 8-bit GEMM restatements built on first use"""

    def __init__(self, oracle, tmp_path_factory):
        self.oracle, self._tmp, self._m8, self._g8 = oracle, tmp_path_factory, None, None

    @property
    def g8(self):
        if self._g8 is None:
            from gemm8_helpers import build_restate
            self._g8 = build_restate(self._tmp.getbasetemp(), parallel=False)
        return self._g8

    @property
    def m8(self):
        if self._m8 is None:
            from matrix8_helpers import build_restate
            self._m8 = build_restate(self._tmp.getbasetemp(), parallel=False)
        return self._m8


class Case:
    """make(seed) -> the operand arrays; enqueue(b, out, stream, rng) with b the operands' device buffers, out the address of the output
    buffer and rng a generator state's address or None; ref(arrays) -> [(offset, expected array)] or None; check(arrays, got bytes): a
    row's own assertion where no byte reference exists; setup(hip) / teardown(): device state of the row that no replay changes"""

    def __init__(self, make, enqueue, nbytes, ref=None, check=None, varies=True, env=None, setup=None, teardown=None):
        self.make, self.enqueue, self.nbytes, self.ref, self.check = make, enqueue, nbytes, ref, check
        self.varies, self.env, self.setup, self.teardown = varies, env or {}, setup, teardown


@contextlib.contextmanager
def environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---------------------------------------------------------------- operands
def vec4(rng, n):
    return random_packed(rng, n)


def vec8(rng, n):
    return rng.integers(-127, 128, size=n).astype(np.int8), rng.uniform(0.5, 2.0, size=n // 64).astype(np.float32)


def floats(rng, n):
    return (rng.standard_normal(n) * 3).astype(np.float32)


def tiles(rng, rows, cols):
    return rng.uniform(0.5, 2.0, size=(rows // 64) * (cols // 64)).astype(np.float32)


def mat4(rng, rows, cols):
    return random_packed(rng, rows * cols)[0], tiles(rng, rows, cols)


def mat8(rng, rows, cols):
    return rng.integers(-127, 128, size=rows * cols).astype(np.int8), tiles(rng, rows, cols)


def tied4(rng, n_pad):
    """raw nibbles, -8 included, under ONE scale: nine magnitudes, so the k-th is tied many times over"""
    return rng.integers(0, 256, size=n_pad // 2, dtype=np.uint8), np.full(n_pad // 64, 1.25, np.float32)


def tied8(rng, n_pad):
    return rng.integers(-20, 21, size=n_pad).astype(np.int8), np.full(n_pad // 64, 1.25, np.float32)


VEC = {4: vec4, 8: vec8}
QBYTES = {4: lambda n: n // 2, 8: lambda n: n}


def lvec(bits, n, *names):
    """layout of CloverVector4 / 8 outputs: for every name its values and its scales ("s" + name)"""
    sizes = {}
    for nm in names:
        sizes[nm] = QBYTES[bits](n)
        sizes["s" + nm] = n // 16
    return layout(**sizes)


# ---------------------------------------------------------------- CPU loops (test/performance/01_measure.h:923-946, 999-1021)
def lowest_index4(oracle, q, s, n, k):
    from test_threshold_large3 import lowest_index_rule
    return lowest_index_rule(oracle, q, s, n, k)


def lowest_index8(q, s, n, k):
    from test_mixed8 import _threshold8_lowest_index
    return _threshold8_lowest_index(q, s, n, k)


def cpu_iht(R, kind, Phi, PhiT, y, m, n, x_len, iters, K, mu, thr):
    """x, t1, t2, t3 as (values, scales) after the deterministic loop; kind: "m4v4", "m4v8" or "m8v8"; thr: 0 none, 1 FAST"""
    o = R.oracle
    if kind == "m4v4":
        x = (np.zeros(n // 2, np.uint8), np.ones(n // 64, np.float32))
        mvm, saa = o.m4_mvm, o.v4_scale_and_add
        cut = lambda q, s: lowest_index4(o, q, s, x_len, K)                    # noqa: E731
    else:
        x = (np.zeros(n, np.int8), np.ones(n // 64, np.float32))
        mvm, saa = (o.m4_mvm_v8 if kind == "m4v8" else R.m8.mvm), o.v8_scale_and_add
        cut = lambda q, s: lowest_index8(q, s, x_len, K)                       # noqa: E731
    t1 = t2 = t3 = None
    for _ in range(iters):
        t1 = mvm(*Phi, m, n, *x)
        t2 = saa(*y, *t1, -1.0)
        t3 = mvm(*PhiT, n, m, *t2)
        x = saa(*x, *t3, float(mu))
        if thr and K < x_len:
            x = (cut(*x), x[1])
    return x, t1, t2, t3


# ---------------------------------------------------------------- the rows
def _vector_rows(hip, R):
    L, o = hip.lib, R.oracle
    rows = {}

    def simple(name, make, call, sizes, ref, **kw):
        off, total = layout(**sizes)
        rows[name] = lambda: Case(make, lambda b, out, s, rng=None: hip.check(call(b, {k: out + v for k, v in off.items()}, s)), total,
                                  ref=lambda a: [(off[k], v) for k, v in ref(a).items()], **kw)

    def mk(*parts):
        def make(seed):
            rng = np.random.default_rng(seed)
            out = []
            for p in parts:
                r = p(rng)
                out.extend(r if isinstance(r, tuple) else (r,))
            return tuple(out)
        return make

    q4, q8, s_ = N // 2, N, N // 16
    simple("clv4_quantize", mk(lambda r: floats(r, N)), lambda b, p, s: L.clv4_quantize(b[0].ptr, N, p["q"], p["s"], None, s), dict(q=q4, s=s_),
           lambda a: dict(zip("qs", o.v4_quantize(a[0]))))
    simple("clv4_restore", mk(lambda r: vec4(r, N)), lambda b, p, s: L.clv4_restore(b[0].ptr, b[1].ptr, N, p["x"], s), dict(x=4 * N),
           lambda a: dict(x=o.v4_restore(*a)))
    simple("clv4_word_isums", mk(lambda r: vec4(r, N)[0], lambda r: vec4(r, N)[0]), lambda b, p, s: L.clv4_word_isums(b[0].ptr, b[1].ptr, N, p["i"], s),
           dict(i=N // 2), lambda a: dict(i=o.v4_word_isums(*a)))
    simple("clv8_quantize", mk(lambda r: floats(r, N)), lambda b, p, s: L.clv8_quantize(b[0].ptr, N, p["q"], p["s"], None, s), dict(q=q8, s=s_),
           lambda a: dict(zip("qs", o.v8_quantize(a[0]))))
    simple("clv8_restore", mk(lambda r: vec8(r, N)), lambda b, p, s: L.clv8_restore(b[0].ptr, b[1].ptr, N, p["x"], s), dict(x=4 * N),
           lambda a: dict(x=o.v8_restore(*a)))

    def saa(bits, n, in_place):
        fn, cpu = (L.clv4_scale_and_add, o.v4_scale_and_add) if bits == 4 else (L.clv8_scale_and_add, o.v8_scale_and_add)
        qb = QBYTES[bits](n)

        def call(b, p, s):
            if not in_place:
                return fn(b[0].ptr, b[1].ptr, b[2].ptr, b[3].ptr, A_SAA, n, p["q"], p["s"], None, s)
            hip.check(L.clv_memcpy_d2d(p["q"], b[0].ptr, qb, s))           # r == qu: u += a v on a copy of u
            hip.check(L.clv_memcpy_d2d(p["s"], b[1].ptr, n // 16, s))
            return fn(p["q"], p["s"], b[2].ptr, b[3].ptr, A_SAA, n, p["q"], p["s"], None, s)
        return (mk(lambda r: VEC[bits](r, n), lambda r: VEC[bits](r, n)), call, dict(q=qb, s=n // 16), lambda a: dict(zip("qs", cpu(*a, A_SAA))))

    simple("clv4_scale_and_add", *saa(4, N, False))
    simple("clv4_scale_and_add in-place", *saa(4, N, True))
    simple("clv4_scale_and_add block", *saa(4, NBLK, False))                 # k_v4_scale_and_add_blk from its first size on
    simple("clv4_scale_and_add block in-place", *saa(4, NBLK, True))
    simple("clv8_scale_and_add", *saa(8, N, False))
    simple("clv8_scale_and_add in-place", *saa(8, N, True))

    def dot(bits, mode):
        fn = L.clv4_dot if bits == 4 else L.clv8_dot
        exact, f64 = (o.v4_dot, o.v4_dot_f64) if bits == 4 else (o.v8_dot, o.v8_dot_f64)

        def call(b, p, s):
            return fn(b[0].ptr, b[1].ptr, b[2].ptr, b[3].ptr, N, mode, p["d"], None, s)

        def close_to_f64(a, got):                                          # the bound tests/test_graph_capture.py holds FAST to
            d64 = f64(*a)
            assert abs(float(got[:4].view(np.float32)[0]) - d64) <= 2e-5 * max(abs(d64), 1.0) + 2e-6 * N
        make = mk(lambda r: VEC[bits](r, N), lambda r: VEC[bits](r, N))
        if mode == DOT_EXACT:
            return make, call, dict(d=4), lambda a: dict(d=np.array([exact(*a)], np.float32))
        return make, call, dict(d=4), lambda a: {}, close_to_f64

    for bits in (4, 8):
        simple(f"clv{bits}_dot exact", *dot(bits, DOT_EXACT))
        make, call, sizes, ref, chk = dot(bits, DOT_FAST)
        simple(f"clv{bits}_dot fast", make, call, sizes, ref, check=chk)

    # no operand: the host arguments are replayed as they were captured
    nothing = lambda seed: ()                                              # noqa: E731
    simple("clv_fill_random_nibbles", nothing, lambda b, p, s: L.clv_fill_random_nibbles(p["q"], N // 2, 11, 256, s), dict(q=N // 2), lambda a: {},
           varies=False)
    simple("clv_fill_random_scales", nothing, lambda b, p, s: L.clv_fill_random_scales(p["s"], N // 64, 12, 64, s), dict(s=N // 16), lambda a: {},
           varies=False)
    simple("clv_fill_random_ints_f32", nothing, lambda b, p, s: L.clv_fill_random_ints_f32(p["x"], N, 40, 13, 128, s), dict(x=4 * N), lambda a: {},
           varies=False)
    simple("clv_memcpy_d2d", mk(lambda r: r.integers(0, 256, size=N, dtype=np.uint8)), lambda b, p, s: L.clv_memcpy_d2d(p["x"], b[0].ptr, N, s),
           dict(x=N), lambda a: dict(x=a[0]))
    return rows


def _threshold_rows(hip, R):
    L, o = hip.lib, R.oracle
    rows = {}

    def row(name, bits, n_pad, k, how):
        """how: "plain" (clvN_threshold), "fast" / "reference" (clvN_threshold_mode), "heap" (clvN_threshold_heap); in place, so every call
        works on a copy of the operand made on the stream, inside the graph"""
        n, qb = n_pad - 100, QBYTES[bits](n_pad)
        off, total = layout(q=qb, heap=8 * k if how == "heap" else 0)
        plain, mode, heap = ((L.clv4_threshold, L.clv4_threshold_mode, L.clv4_threshold_heap) if bits == 4 else
                             (L.clv8_threshold, L.clv8_threshold_mode, L.clv8_threshold_heap))

        def enqueue(b, out, s, rng=None):
            hip.check(L.clv_memcpy_d2d(out, b[0].ptr, qb, s))
            if how == "plain":
                hip.check(plain(out, b[1].ptr, n, n_pad, k, None, s))
            elif how == "heap":
                hip.check(heap(out, b[1].ptr, n, n_pad, k, out + off["heap"], None, s))
            else:
                hip.check(mode(out, b[1].ptr, n, n_pad, k, THRESHOLD_FAST if how == "fast" else THRESHOLD_REFERENCE, None, s))

        def ref(a):
            if how in ("plain", "fast"):
                return [(0, lowest_index4(o, *a, n, k) if bits == 4 else lowest_index8(*a, n, k))]
            return [(0, o.v4_threshold(*a, n, k) if bits == 4 else o.v8_threshold(*a, n, k))]   # the heap itself: replay == eager

        data = tied4 if bits == 4 else tied8
        rows[name] = lambda: Case(lambda seed: data(np.random.default_rng(seed), n_pad), enqueue, total, ref=ref)

    for bits in (4, 8):
        last = SMALL_LAST[bits]
        row(f"clv{bits}_threshold_mode fast last-small", bits, last, last // 4, "fast")
        row(f"clv{bits}_threshold_mode fast first-large", bits, last + 128, last // 4, "fast")
        row(f"clv{bits}_threshold_mode reference", bits, N, K_REF, "reference")
        row(f"clv{bits}_threshold_heap", bits, N, K_REF, "heap")
        row(f"clv{bits}_threshold", bits, N, N // 4, "plain")
    return rows


def _matrix_rows(hip, R):
    L, o = hip.lib, R.oracle
    rows = {}
    nt = (ROWS // 64) * (COLS // 64)

    def simple(name, make, call, sizes, ref):
        off, total = layout(**sizes)
        rows[name] = lambda: Case(lambda seed: make(np.random.default_rng(seed)),
                                  lambda b, out, s, rng=None: hip.check(call(b, {k: out + v for k, v in off.items()}, s, rng)), total,
                                  ref=lambda a: [(off[k], v) for k, v in ref(a).items()])

    def A32(r):
        return ((r.standard_normal((ROWS, COLS)) * 2).astype(np.float32),)

    simple("clm4_quantize", A32, lambda b, p, s, g: L.clm4_quantize(b[0].ptr, ROWS, COLS, p["q"], p["s"], g, s), dict(q=ROWS * COLS // 2, s=4 * nt),
           lambda a: dict(zip("qs", o.m4_quantize(a[0]))))
    simple("clm4_restore", lambda r: mat4(r, ROWS, COLS), lambda b, p, s, g: L.clm4_restore(b[0].ptr, b[1].ptr, ROWS, COLS, p["A"], s),
           dict(A=4 * ROWS * COLS), lambda a: dict(A=o.m4_restore(*a, ROWS, COLS)))
    simple("clm4_transpose", lambda r: mat4(r, ROWS, COLS), lambda b, p, s, g: L.clm4_transpose(b[0].ptr, b[1].ptr, ROWS, COLS, p["q"], p["s"], s),
           dict(q=ROWS * COLS // 2, s=4 * nt), lambda a: dict(zip("qs", o.m4_transpose(*a, ROWS, COLS))))
    simple("clm8_quantize", A32, lambda b, p, s, g: L.clm8_quantize(b[0].ptr, ROWS, COLS, p["q"], p["s"], g, s), dict(q=ROWS * COLS, s=4 * nt),
           lambda a: dict(zip("qs", R.m8.quantize(a[0]))))
    simple("clm8_restore", lambda r: mat8(r, ROWS, COLS), lambda b, p, s, g: L.clm8_restore(b[0].ptr, b[1].ptr, ROWS, COLS, p["A"], s),
           dict(A=4 * ROWS * COLS), lambda a: dict(A=R.m8.restore(*a, ROWS, COLS)))
    simple("clm8_transpose", lambda r: mat8(r, ROWS, COLS), lambda b, p, s, g: L.clm8_transpose(b[0].ptr, b[1].ptr, ROWS, COLS, p["q"], p["s"], s),
           dict(q=ROWS * COLS, s=4 * nt), lambda a: dict(zip("qs", R.m8.transpose(*a, ROWS, COLS))))

    # the mvm family: (matrix width, vector width) -> the entry, its CPU form, the vector's scaleAndAdd
    fam = {"m4v4": (mat4, 4, L.clm4_mvm, o.m4_mvm, L.clm4_mvm_scale_and_add, o.v4_scale_and_add),
           "m4v8": (mat4, 8, L.clm4_mvm_v8, o.m4_mvm_v8, L.clm4_mvm_v8_scale_and_add, o.v8_scale_and_add),
           "m8v8": (mat8, 8, L.clm8_mvm, lambda *a: R.m8.mvm(*a), L.clm8_mvm_scale_and_add, o.v8_scale_and_add)}

    def mvm(kind, nrows):
        mat, bits, fn, cpu, _, _ = fam[kind]
        off, _ = lvec(bits, nrows, "r")
        return (lambda r: (*mat(r, nrows, COLS), *VEC[bits](r, COLS)),
                lambda b, p, s, g: fn(b[0].ptr, b[1].ptr, nrows, COLS, b[2].ptr, b[3].ptr, p["r"], p["sr"], g, s),
                {k: (QBYTES[bits](nrows) if k == "r" else nrows // 16) for k in off}, lambda a: dict(zip(("r", "sr"), cpu(a[0], a[1], nrows, COLS, a[2], a[3]))))

    def fused(kind):
        mat, bits, _, cpu, fn, saa = fam[kind]
        qb = QBYTES[bits](ROWS)

        def ref(a):
            t = cpu(a[0], a[1], ROWS, COLS, a[2], a[3])
            return dict(zip(("t", "st", "r", "sr"), (*t, *saa(a[4], a[5], *t, A_SAA))))
        return (lambda r: (*mat(r, ROWS, COLS), *VEC[bits](r, COLS), *VEC[bits](r, ROWS)),
                lambda b, p, s, g: fn(b[0].ptr, b[1].ptr, ROWS, COLS, b[2].ptr, b[3].ptr, b[4].ptr, b[5].ptr, A_SAA, p["t"], p["st"], p["r"], p["sr"], g, s),
                dict(t=qb, st=ROWS // 16, r=qb, sr=ROWS // 16), ref)

    simple("clm4_mvm", *mvm("m4v4", ROWS))
    simple("clm4_mvm shard", *mvm("m4v4", 192))                               # rows % 128 == 64: a 64-row shard's last group
    simple("clm4_mvm_v8", *mvm("m4v8", ROWS))
    simple("clm8_mvm", *mvm("m8v8", ROWS))
    simple("clm4_mvm_scale_and_add", *fused("m4v4"))
    simple("clm4_mvm_v8_scale_and_add", *fused("m4v8"))
    simple("clm8_mvm_scale_and_add", *fused("m8v8"))
    simple("clm4_rowdots", lambda r: (*mat4(r, ROWS, COLS), *vec4(r, COLS)),
           lambda b, p, s, g: L.clm4_rowdots(b[0].ptr, b[1].ptr, ROWS, COLS, b[2].ptr, b[3].ptr, p["d"], s), dict(d=4 * ROWS),
           lambda a: dict(d=o.m4_rowdots(a[0], a[1], ROWS, COLS, a[2], a[3])))
    simple("clm4_rowdots_v8", lambda r: (*mat4(r, ROWS, COLS), *vec8(r, COLS)),
           lambda b, p, s, g: L.clm4_rowdots_v8(b[0].ptr, b[1].ptr, ROWS, COLS, b[2].ptr, b[3].ptr, p["d"], s), dict(d=4 * ROWS),
           lambda a: dict(d=o.m4_rowdots_v8(a[0], a[1], ROWS, COLS, a[2], a[3])))
    simple("clm4_mvm_f32", lambda r: (*mat4(r, ROWS, COLS), floats(r, COLS)),
           lambda b, p, s, g: L.clm4_mvm_f32(b[0].ptr, b[1].ptr, ROWS, COLS, b[2].ptr, p["d"], s), dict(d=4 * ROWS),
           lambda a: dict(d=o.m4_mvm_f32(a[0], a[1], ROWS, COLS, a[2])))
    simple("clm8_mvm_f32", lambda r: (*mat8(r, ROWS, COLS), floats(r, COLS)),
           lambda b, p, s, g: L.clm8_mvm_f32(b[0].ptr, b[1].ptr, ROWS, COLS, b[2].ptr, p["d"], s), dict(d=4 * ROWS),
           lambda a: dict(d=R.m8.mvm_f32(a[0], a[1], ROWS, COLS, a[2])))

    # the transposed fused forms: A is ROWS x COLS, x has ROWS elements, u, t and r have COLS.  Their deterministic captures are in the
    # *_transposed_capture.py files; these rows exist for the stochastic table below (and cost nothing to run deterministically too)
    def fused_t(kind, fn, transpose):
        mat, bits, _, cpu, _, saa = fam[kind]
        qb = QBYTES[bits](COLS)

        def ref(a):
            t = cpu(*transpose(a[0], a[1], ROWS, COLS), COLS, ROWS, a[2], a[3])
            return dict(zip(("t", "st", "r", "sr"), (*t, *saa(a[4], a[5], *t, A_SAA))))
        return (lambda r: (*mat(r, ROWS, COLS), *VEC[bits](r, ROWS), *VEC[bits](r, COLS)),
                lambda b, p, s, g: fn(b[0].ptr, b[1].ptr, ROWS, COLS, b[2].ptr, b[3].ptr, b[4].ptr, b[5].ptr, A_SAA, p["t"], p["st"], p["r"], p["sr"], g, s),
                dict(t=qb, st=COLS // 16, r=qb, sr=COLS // 16), ref)

    simple("clm4_mvm_transposed_scale_and_add", *fused_t("m4v4", L.clm4_mvm_transposed_scale_and_add, o.m4_transpose))
    simple("clm4_mvm_v8_transposed_scale_and_add", *fused_t("m4v8", L.clm4_mvm_v8_transposed_scale_and_add, o.m4_transpose))
    simple("clm8_mvm_transposed_scale_and_add", *fused_t("m8v8", L.clm8_mvm_transposed_scale_and_add, lambda *a: R.m8.transpose(*a)))
    return rows


def _gemm_rows(hip, R):
    L, o = hip.lib, R.oracle
    rows = {}
    nbytes = 4 * GM * GN
    EVEN, ODD = (2, 4), (1, 3)                                                # K-block ranges: the matrix kernel, the VALU kernel

    def A_(r):
        return mat4(r, GM, GK)

    def B_(r):
        return mat4(r, GN, GK)

    def isums(qA, qB, kb):
        return o.m4_gemm_isums(qA, GM, GK, qB, GN)[:, :, kb[0]:kb[0] + kb[1]].sum(2).astype(np.int32)

    rows["clm4_gemm"] = lambda: Case(
        lambda seed: (lambda r: (*A_(r), *B_(r)))(np.random.default_rng(seed)),
        lambda b, out, s, rng=None: hip.check(L.clm4_gemm(b[0].ptr, b[1].ptr, GM, GK, b[2].ptr, b[3].ptr, GN, out, s)), nbytes,
        ref=lambda a: [(0, o.m4_gemm(a[0], a[1], GM, GK, a[2], a[3], GN))])

    def i32(kb):
        return lambda: Case(
            lambda seed: (lambda r: (A_(r)[0], B_(r)[0]))(np.random.default_rng(seed)),
            lambda b, out, s, rng=None: hip.check(L.clm4_gemm_i32(b[0].ptr, GM, GK, b[1].ptr, GN, kb[0], kb[1], out, s)), nbytes,
            ref=lambda a: [(0, isums(a[0], a[1], kb))])
    # any begin and any count run on the int8 matrix cores; the other two 8-bit GEMM entries are captured in tests/test_gemm8.py
    rows["clm8_gemm_i32"] = lambda: Case(
        lambda seed: (lambda r: (mat8(r, GM, GK)[0], mat8(r, GN, GK)[0]))(np.random.default_rng(seed)),
        lambda b, out, s, rng=None: hip.check(L.clm8_gemm_i32(b[0].ptr, GM, GK, b[1].ptr, GN, ODD[0], ODD[1], out, s)), nbytes,
        ref=lambda a: [(0, R.g8.gemm_i32(a[0], GM, GK, a[1], GN, *ODD))])
    rows["clm4_gemm_i32 even"] = i32(EVEN)
    rows["clm4_gemm_i32 odd"] = i32(ODD)

    def prepared(kb):
        """B, the weights, is re-coded once outside the capture (clm4_gemm_prepare allocates); A changes from replay to replay.  kb None:
        the fp32 product; else the integer sums of that K-block range (an odd range reads B's nibbles besides its image)"""
        st = {}

        def setup(hip_):
            st["B"] = B_(np.random.default_rng(7))
            st["qB"], st["sB"], st["op"] = hip_.to_device(st["B"][0]), hip_.to_device(st["B"][1]), C.c_void_p()
            hip_.check(L.clm4_gemm_prepare(st["qB"].ptr, GN, GK, C.byref(st["op"]), None))
            hip_.sync()

        def teardown():
            hip.check(L.clm4_gemm_release(st["op"]))

        def enqueue(b, out, s, rng=None):
            if kb is None:
                hip.check(L.clm4_gemm_prepared(None, b[0].ptr, b[1].ptr, GM, GK, st["op"], None, st["sB"].ptr, GN, out, s))
            else:
                hip.check(L.clm4_gemm_i32_prepared(None, b[0].ptr, GM, GK, st["op"], st["qB"].ptr, GN, kb[0], kb[1], out, s))
        ref = ((lambda a: [(0, o.m4_gemm(a[0], a[1], GM, GK, *st["B"], GN))]) if kb is None else
               (lambda a: [(0, isums(a[0], st["B"][0], kb))]))
        return lambda: Case(lambda seed: A_(np.random.default_rng(seed)), enqueue, nbytes, ref=ref, setup=setup, teardown=teardown)
    rows["clm4_gemm_prepared"] = prepared(None)
    rows["clm4_gemm_i32_prepared even"] = prepared(EVEN)
    rows["clm4_gemm_i32_prepared odd"] = prepared(ODD)
    return rows


LOOP_ENV = {"CLV_IHT_PERSISTENT": "0"}


def _loop_rows(hip, R):
    L, o = hip.lib, R.oracle
    rows = {}
    m, n, x_len, K = M_IHT, N_IHT, N_IHT - 10, N_IHT // 4
    kinds = {"m4v4": (mat4, 4, o.m4_transpose, 0.002), "m4v8": (mat4, 8, o.m4_transpose, 0.002),
             "m8v8": (mat8, 8, lambda *a: R.m8.transpose(*a), 0.0002)}

    def loop(name, kind, fn, thr, one_matrix=False):
        mat, bits, transpose, mu = kinds[kind]
        off, total = lvec(bits, max(m, n), "x", "t1", "t2", "t3")

        def make(seed):
            r = np.random.default_rng(seed)
            Phi = mat(r, m, n)
            return (*Phi, *transpose(*Phi, m, n), *VEC[bits](r, m))

        def enqueue(b, out, s, rng=None):
            p = {k: out + v for k, v in off.items()}
            head = (b[0].ptr, b[1].ptr, m, n) if one_matrix else (b[0].ptr, b[1].ptr, b[2].ptr, b[3].ptr, m, n)
            hip.check(fn(*head, p["x"], p["sx"], x_len, b[4].ptr, b[5].ptr, p["t1"], p["st1"], p["t2"], p["st2"], p["t3"], p["st3"], ITERS, K, mu,
                         thr, rng, s))

        def ref(a):
            x, t1, t2, t3 = cpu_iht(R, kind, a[0:2], a[2:4], a[4:6], m, n, x_len, ITERS, K, mu, thr)
            return [(off[k], v) for k, v in zip(("x", "sx", "t1", "st1", "t2", "st2", "t3", "st3"), (*x, *t1, *t2, *t3))]
        rows[name] = lambda: Case(make, enqueue, total, ref=ref, env=LOOP_ENV)

    for label, thr in (("gd", 0), ("fast", 1)):
        loop(f"clm4_iht {label}", "m4v4", L.clm4_iht, thr)
        loop(f"clm4_iht_v8 {label}", "m4v8", L.clm4_iht_v8, thr)
    # for the stochastic table: the loops whose deterministic captures live elsewhere
    loop("clm8_iht fast", "m8v8", L.clm8_iht, 1)
    loop("clm4_iht_one_matrix fast", "m4v4", L.clm4_iht_one_matrix, 1, one_matrix=True)
    loop("clm4_iht_v8_one_matrix fast", "m4v8", L.clm4_iht_v8_one_matrix, 1, one_matrix=True)
    loop("clm8_iht_one_matrix fast", "m8v8", L.clm8_iht_one_matrix, 1, one_matrix=True)
    return rows


BATCH_ENV = {"CLV_MVM_BATCH": "1", "CLV_IHT_PERSISTENT": "0"}                 # every group of two or more vectors runs the one-pass kernel


def _batch_rows(hip, R):
    """the batch entries no other test captures, NVEC vectors each: the pointer arrays are host arrays read during the call, the graph
    holds the device pointers"""
    L, o = hip.lib, R.oracle
    rows = {}
    pa = hip.ptr_array
    brows, bcols = 128, 256
    fam = {"m4v4": (mat4, 4, o.m4_mvm), "m4v8": (mat4, 8, o.m4_mvm_v8), "m8v8": (mat8, 8, lambda *a: R.m8.mvm(*a))}

    def mvm(name, kind, fn, at):
        mat, bits, cpu = fam[kind]
        off, total = lvec(bits, brows, *[f"r{j}" for j in range(NVEC)])

        def make(seed):
            r = np.random.default_rng(seed)
            return (*mat(r, brows, bcols), *[v for _ in range(NVEC) for v in VEC[bits](r, bcols)])

        def enqueue(b, out, s, rng=None):
            x, sx = pa([b[2 + 2 * j].ptr for j in range(NVEC)]), pa([b[3 + 2 * j].ptr for j in range(NVEC)])
            r, sr = pa([out + off[f"r{j}"] for j in range(NVEC)]), pa([out + off[f"sr{j}"] for j in range(NVEC)])
            extra = (0, 2 * (brows // 64), NVEC * 2 * (brows // 64)) if at else ()
            hip.check(fn(b[0].ptr, b[1].ptr, brows, bcols, NVEC, x, sx, r, sr, rng, *extra, s))

        def ref(a):
            out = []
            for j in range(NVEC):
                q, s = cpu(a[0], a[1], brows, bcols, a[2 + 2 * j], a[3 + 2 * j])
                out += [(off[f"r{j}"], q), (off[f"sr{j}"], s)]
            return out
        rows[name] = lambda: Case(make, enqueue, total, ref=ref, env=BATCH_ENV)

    mvm("clm4_mvm_batch_at", "m4v4", L.clm4_mvm_batch_at, True)
    mvm("clm4_mvm_v8_batch", "m4v8", L.clm4_mvm_v8_batch, False)
    mvm("clm4_mvm_v8_batch_at", "m4v8", L.clm4_mvm_v8_batch_at, True)
    mvm("clm8_mvm_batch", "m8v8", L.clm8_mvm_batch, False)
    mvm("clm8_mvm_batch_at", "m8v8", L.clm8_mvm_batch_at, True)

    def threshold(name, bits, fn):
        n_pad, n, k, qb = N, N - 100, N // 4, QBYTES[bits](N)
        off, total = layout(**{f"q{j}": qb for j in range(NVEC)})
        data = tied4 if bits == 4 else tied8

        def make(seed):
            r = np.random.default_rng(seed)
            return tuple(v for _ in range(NVEC) for v in data(r, n_pad))

        def enqueue(b, out, s, rng=None):
            for j in range(NVEC):
                hip.check(L.clv_memcpy_d2d(out + off[f"q{j}"], b[2 * j].ptr, qb, s))
            hip.check(fn(pa([out + off[f"q{j}"] for j in range(NVEC)]), pa([b[2 * j + 1].ptr for j in range(NVEC)]), NVEC, n, n_pad, k, THRESHOLD_FAST, s))

        def ref(a):
            return [(off[f"q{j}"], lowest_index4(o, a[2 * j], a[2 * j + 1], n, k) if bits == 4 else lowest_index8(a[2 * j], a[2 * j + 1], n, k))
                    for j in range(NVEC)]
        rows[name] = lambda: Case(make, enqueue, total, ref=ref, env=BATCH_ENV)

    threshold("clv4_threshold_batch", 4, L.clv4_threshold_batch)
    threshold("clv8_threshold_batch", 8, L.clv8_threshold_batch)

    def loop(name, kind, fn, transpose, mu):
        mat, bits, _ = fam[kind]
        m, n, x_len, K = M_IHT, N_IHT, N_IHT - 10, N_IHT // 4
        names = ("x", "t1", "t2", "t3")
        off, total = lvec(bits, max(m, n), *[f"{k}{j}" for j in range(NVEC) for k in names])

        def make(seed):
            r = np.random.default_rng(seed)
            Phi = mat(r, m, n)
            return (*Phi, *transpose(*Phi, m, n), *[v for _ in range(NVEC) for v in VEC[bits](r, m)])

        def enqueue(b, out, s, rng=None):
            arr = lambda k: (pa([out + off[f"{k}{j}"] for j in range(NVEC)]), pa([out + off[f"s{k}{j}"] for j in range(NVEC)]))   # noqa: E731
            y, sy = pa([b[4 + 2 * j].ptr for j in range(NVEC)]), pa([b[5 + 2 * j].ptr for j in range(NVEC)])
            hip.check(fn(b[0].ptr, b[1].ptr, b[2].ptr, b[3].ptr, m, n, NVEC, *arr("x"), x_len, y, sy, *arr("t1"), *arr("t2"), *arr("t3"), ITERS, K,
                         mu, 1, rng, s))

        def ref(a):
            out = []
            for j in range(NVEC):
                vs = cpu_iht(R, kind, a[0:2], a[2:4], a[4 + 2 * j:6 + 2 * j], m, n, x_len, ITERS, K, mu, 1)
                for k, (q, s) in zip(names, vs):
                    out += [(off[f"{k}{j}"], q), (off[f"s{k}{j}"], s)]
            return out
        rows[name] = lambda: Case(make, enqueue, total, ref=ref, env=BATCH_ENV)

    loop("clm4_iht_v8_batch", "m4v8", L.clm4_iht_v8_batch, o.m4_transpose, 0.002)
    loop("clm8_iht_batch", "m8v8", L.clm8_iht_batch, lambda *a: R.m8.transpose(*a), 0.0002)
    return rows


def all_rows(hip, R):
    rows = {}
    for part in (_vector_rows, _threshold_rows, _matrix_rows, _gemm_rows, _loop_rows, _batch_rows):
        rows.update(part(hip, R))
    return rows


CASES = [
    "clv4_quantize", "clv4_restore", "clv4_scale_and_add", "clv4_scale_and_add in-place", "clv4_scale_and_add block", "clv4_scale_and_add block in-place",
    "clv4_dot exact", "clv4_dot fast", "clv4_word_isums", "clv8_quantize", "clv8_restore", "clv8_scale_and_add", "clv8_scale_and_add in-place",
    "clv8_dot exact", "clv8_dot fast", "clv_fill_random_nibbles", "clv_fill_random_scales", "clv_fill_random_ints_f32", "clv_memcpy_d2d",
    "clv4_threshold_mode fast last-small", "clv4_threshold_mode fast first-large", "clv4_threshold_mode reference", "clv4_threshold_heap",
    "clv4_threshold", "clv8_threshold_mode fast last-small", "clv8_threshold_mode fast first-large", "clv8_threshold_mode reference",
    "clv8_threshold_heap", "clv8_threshold",
    "clm4_quantize", "clm4_restore", "clm4_transpose", "clm4_mvm", "clm4_mvm shard", "clm4_rowdots", "clm4_mvm_scale_and_add", "clm4_mvm_v8",
    "clm4_mvm_v8_scale_and_add", "clm4_rowdots_v8", "clm4_mvm_f32", "clm8_quantize", "clm8_restore", "clm8_transpose", "clm8_mvm", "clm8_mvm_f32",
    "clm4_gemm", "clm4_gemm_prepared", "clm4_gemm_i32 even", "clm4_gemm_i32 odd", "clm4_gemm_i32_prepared even", "clm4_gemm_i32_prepared odd",
    "clm8_gemm_i32", "clm4_iht gd", "clm4_iht fast", "clm4_iht_v8 gd", "clm4_iht_v8 fast",
    "clm4_mvm_batch_at", "clm4_mvm_v8_batch", "clm4_mvm_v8_batch_at", "clm8_mvm_batch", "clm8_mvm_batch_at", "clv4_threshold_batch",
    "clv8_threshold_batch", "clm4_iht_v8_batch", "clm8_iht_batch",
]
GEMM_CASES = [c for c in CASES if c.startswith("clm4_gemm")]

# the header's STOCHASTIC CALLS that no other test replays on a state in graph mode: stochastic name -> the row it runs with a generator
STOCHASTIC = {
    "clm4_mvm_v8_scale_and_add stochastic": "clm4_mvm_v8_scale_and_add",
    "clm8_mvm_scale_and_add stochastic": "clm8_mvm_scale_and_add",
    "clm4_mvm_transposed_scale_and_add stochastic": "clm4_mvm_transposed_scale_and_add",
    "clm4_mvm_v8_transposed_scale_and_add stochastic": "clm4_mvm_v8_transposed_scale_and_add",
    "clm8_mvm_transposed_scale_and_add stochastic": "clm8_mvm_transposed_scale_and_add",
    "clm4_iht stochastic": "clm4_iht fast",
    "clm4_iht_v8 stochastic": "clm4_iht_v8 fast",
    "clm8_iht stochastic": "clm8_iht fast",
    "clm4_iht_one_matrix stochastic": "clm4_iht_one_matrix fast",
    "clm4_iht_v8_one_matrix stochastic": "clm4_iht_v8_one_matrix fast",
    "clm8_iht_one_matrix stochastic": "clm8_iht_one_matrix fast",
}
# rows that only the stochastic table runs (their deterministic captures are in other files); with CASES, every name all_rows() builds
STOCHASTIC_ONLY_ROWS = ["clm8_mvm_scale_and_add", "clm4_mvm_transposed_scale_and_add", "clm4_mvm_v8_transposed_scale_and_add",
                        "clm8_mvm_transposed_scale_and_add", "clm8_iht fast", "clm4_iht_one_matrix fast", "clm4_iht_v8_one_matrix fast",
                        "clm8_iht_one_matrix fast"]
KEYS = (2718, 2818)


def compare(got, expected, what):
    for off, want in expected:
        w = u8(want)
        assert np.array_equal(got[off:off + w.size], w), (*what, "the CPU reference", off, np.flatnonzero(got[off:off + w.size] != w)[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_captured_call_replays_to_the_eager_bits(hip, oracle, tmp_path_factory, name):
    rows = all_rows(hip, Refs(oracle, tmp_path_factory))
    assert set(rows) == set(CASES) | set(STOCHASTIC_ONLY_ROWS)                 # the lists the CPU check reads are the table
    case = rows[name]()
    launches = hip.lib.clv_iht_persistent_launches()
    with environment(case.env):
        if case.setup:
            case.setup(hip)
        bufs = [hip.to_device(a) for a in case.make(1)]
        out, eager = hip.alloc(case.nbytes), hip.alloc(case.nbytes)
        g = Graph()
        g.capture(lambda s: case.enqueue(bufs, out.ptr, s))
        results = []
        for rep in range(3):
            arrays = case.make(10 + rep)
            for b, a in zip(bufs, arrays):
                b.upload(a, g.stream)
            hip.check(hip.lib.clv_memset(out.ptr, 0xA5, case.nbytes, g.stream))
            hip.check(hip.lib.clv_memset(eager.ptr, 0xA5, case.nbytes, g.stream))   # the gaps between the outputs too
            g.replay()
            got = out.download(np.uint8)
            case.enqueue(bufs, eager.ptr, g.stream)
            g.sync()
            assert np.array_equal(got, eager.download(np.uint8)), (name, rep)
            if rep == 0:
                compare(got, case.ref(arrays), (name,))
                if case.check:
                    case.check(arrays, got)
            results.append(got)
        if case.varies:
            assert not np.array_equal(results[0], results[1])              # the replays did compute from the new operands
        else:
            assert not np.all(results[0] == 0xA5)
        g.close(hip.lib)
        if case.teardown:
            case.teardown()
    assert hip.lib.clv_iht_persistent_launches() == launches


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(STOCHASTIC))
def test_captured_stochastic_call_draws_what_the_eager_calls_draw(hip, oracle, tmp_path_factory, name):
    case = all_rows(hip, Refs(oracle, tmp_path_factory))[STOCHASTIC[name]]()
    L = hip.lib
    launches = L.clv_iht_persistent_launches()
    with environment(case.env):
        bufs = [hip.to_device(a) for a in case.make(1)]
        out, eager = hip.alloc(case.nbytes), hip.alloc(case.nbytes)
        A, B = hip.new_rng(*KEYS), hip.new_rng(*KEYS)
        fresh = hip.rng_get(A)
        g = Graph()
        # ordinary (host-stamped) calls first, one per state: the generator tables and the stream's scratch are built outside the capture
        for d in (out, eager):
            hip.check(L.clv_memset(d.ptr, 0xA5, case.nbytes, g.stream))      # the gaps between the outputs compare too
        case.enqueue(bufs, out.ptr, g.stream, A.ptr)
        case.enqueue(bufs, eager.ptr, g.stream, B.ptr)
        g.sync()
        assert np.array_equal(out.download(np.uint8), eager.download(np.uint8)), (name, "ordinary")
        hip.check(L.clv_rng_graph_mode(A.ptr, 1, g.stream))
        g.sync()
        g.record(lambda s: case.enqueue(bufs, out.ptr, s, A.ptr))
        results = []
        for rep in range(3):
            for b, a in zip(bufs, case.make(10 + rep)):
                b.upload(a, g.stream)
            hip.check(L.clv_memset(out.ptr, 0xA5, case.nbytes, g.stream))
            hip.check(L.clv_memset(eager.ptr, 0xA5, case.nbytes, g.stream))
            g.replay()
            got = out.download(np.uint8)
            case.enqueue(bufs, eager.ptr, g.stream, B.ptr)
            g.sync()
            assert np.array_equal(got, eager.download(np.uint8)), (name, rep)
            ka, kb = hip.rng_get(A), hip.rng_get(B)
            assert np.array_equal(ka[0], kb[0]) and np.array_equal(ka[1], kb[1]), (name, rep, "the generator state")
            results.append((got, ka))
        assert not np.array_equal(results[0][0], results[1][0])
        assert not np.array_equal(results[0][1][0], results[1][1][0]) and not np.array_equal(results[0][1][0], fresh[0])   # the stream moved
        hip.check(L.clv_rng_graph_mode(A.ptr, 0, g.stream))
        g.close(L)
    assert L.clv_iht_persistent_launches() == launches


@pytest.mark.gpu
def test_gemm_rows_on_the_256_tile():
    """CLV_GEMM_TILE is read once per process: the GEMM rows once more in a child that forces the 256 x 256 workgroup tile (this process runs
    them on the tile the library picks for the shape, 128 x 128)"""
    assert "CLV_GEMM_TILE" not in os.environ
    cmd = [sys.executable, *(["-s"] if sys.flags.no_user_site else []), "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu",
           f"{Path(__file__).name}::test_captured_call_replays_to_the_eager_bits", "-k", "clm4_gemm"]
    p = subprocess.run(cmd, cwd=Path(__file__).parent, env=dict(os.environ, CLV_GEMM_TILE="256"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and f"{len(GEMM_CASES)} passed" in p.stdout, (p.stdout[-3000:], p.stderr[-1500:])


# ---------------------------------------------------------------- every name of the binding is accounted for (CPU)
# entry -> the rows of this file that enqueue it between hipStreamBeginCapture and hipStreamEndCapture
CAPTURED = {
    "clv4_quantize": ["clv4_quantize"],
    "clv4_restore": ["clv4_restore"],
    "clv4_scale_and_add": ["clv4_scale_and_add", "clv4_scale_and_add in-place", "clv4_scale_and_add block", "clv4_scale_and_add block in-place"],
    "clv4_dot": ["clv4_dot exact", "clv4_dot fast"],
    "clv4_word_isums": ["clv4_word_isums"],
    "clv8_quantize": ["clv8_quantize"],
    "clv8_restore": ["clv8_restore"],
    "clv8_scale_and_add": ["clv8_scale_and_add", "clv8_scale_and_add in-place"],
    "clv8_dot": ["clv8_dot exact", "clv8_dot fast"],
    "clv_fill_random_nibbles": ["clv_fill_random_nibbles"],
    "clv_fill_random_scales": ["clv_fill_random_scales"],
    "clv_fill_random_ints_f32": ["clv_fill_random_ints_f32"],
    "clv_memcpy_d2d": ["clv_memcpy_d2d"],
    "clv4_threshold": ["clv4_threshold"],
    "clv4_threshold_mode": ["clv4_threshold_mode fast last-small", "clv4_threshold_mode fast first-large", "clv4_threshold_mode reference"],
    "clv4_threshold_heap": ["clv4_threshold_heap"],
    "clv8_threshold": ["clv8_threshold"],
    "clv8_threshold_mode": ["clv8_threshold_mode fast last-small", "clv8_threshold_mode fast first-large", "clv8_threshold_mode reference"],
    "clv8_threshold_heap": ["clv8_threshold_heap"],
    "clm4_quantize": ["clm4_quantize"],
    "clm4_restore": ["clm4_restore"],
    "clm4_transpose": ["clm4_transpose"],
    "clm4_mvm": ["clm4_mvm", "clm4_mvm shard"],
    "clm4_rowdots": ["clm4_rowdots"],
    "clm4_mvm_scale_and_add": ["clm4_mvm_scale_and_add"],
    "clm4_mvm_v8": ["clm4_mvm_v8"],
    "clm4_mvm_v8_scale_and_add": ["clm4_mvm_v8_scale_and_add", "clm4_mvm_v8_scale_and_add stochastic"],
    "clm4_rowdots_v8": ["clm4_rowdots_v8"],
    "clm4_mvm_f32": ["clm4_mvm_f32"],
    "clm8_quantize": ["clm8_quantize"],
    "clm8_restore": ["clm8_restore"],
    "clm8_transpose": ["clm8_transpose"],
    "clm8_mvm": ["clm8_mvm"],
    "clm8_mvm_f32": ["clm8_mvm_f32"],
    "clm8_mvm_scale_and_add": ["clm8_mvm_scale_and_add stochastic"],
    "clm4_gemm": ["clm4_gemm"],
    "clm4_gemm_prepared": ["clm4_gemm_prepared"],
    "clm4_gemm_i32": ["clm4_gemm_i32 even", "clm4_gemm_i32 odd"],
    "clm4_gemm_i32_prepared": ["clm4_gemm_i32_prepared even", "clm4_gemm_i32_prepared odd"],
    "clm8_gemm_i32": ["clm8_gemm_i32"],
    "clm4_iht": ["clm4_iht gd", "clm4_iht fast", "clm4_iht stochastic"],
    "clm4_iht_v8": ["clm4_iht_v8 gd", "clm4_iht_v8 fast", "clm4_iht_v8 stochastic"],
    "clm8_iht": ["clm8_iht stochastic"],
    "clm4_mvm_transposed_scale_and_add": ["clm4_mvm_transposed_scale_and_add stochastic"],
    "clm4_mvm_v8_transposed_scale_and_add": ["clm4_mvm_v8_transposed_scale_and_add stochastic"],
    "clm8_mvm_transposed_scale_and_add": ["clm8_mvm_transposed_scale_and_add stochastic"],
    "clm4_iht_one_matrix": ["clm4_iht_one_matrix stochastic"],
    "clm4_iht_v8_one_matrix": ["clm4_iht_v8_one_matrix stochastic"],
    "clm8_iht_one_matrix": ["clm8_iht_one_matrix stochastic"],
    "clm4_mvm_batch_at": ["clm4_mvm_batch_at"],
    "clm4_mvm_v8_batch": ["clm4_mvm_v8_batch"],
    "clm4_mvm_v8_batch_at": ["clm4_mvm_v8_batch_at"],
    "clm8_mvm_batch": ["clm8_mvm_batch"],
    "clm8_mvm_batch_at": ["clm8_mvm_batch_at"],
    "clv4_threshold_batch": ["clv4_threshold_batch"],
    "clv8_threshold_batch": ["clv8_threshold_batch"],
    "clm4_iht_v8_batch": ["clm4_iht_v8_batch"],
    "clm8_iht_batch": ["clm8_iht_batch"],
}

# entry -> file::test that enqueues it inside a capture (the deterministic form; the fused transposed calls and the one-matrix loops with
# a generator are rows above, so they stand in CAPTURED)
CAPTURED_ELSEWHERE = {
    "clm4_mvm_transposed": "test_mvm_transposed_capture.py::test_the_deterministic_calls_capture_and_replay",
    "clm4_mvm_v8_transposed": "test_mvm_v8_transposed_capture.py::test_the_deterministic_calls_capture_and_replay",
    "clm8_mvm_transposed": "test_m8_mvm_transposed_capture.py::test_the_deterministic_calls_capture_and_replay",
    "clm4_mvm_batch": "test_mvm_batch_stochastic.py::test_a_stochastic_batch_call_captures_into_a_graph_when_the_state_is_in_graph_mode",
    "clm4_mvm_scale_and_add_batch": "test_mvm_batch.py::test_the_deterministic_batch_calls_capture_into_a_graph",
    "clm4_iht_batch": "test_mvm_batch.py::test_the_deterministic_batch_calls_capture_into_a_graph",
    "clm4_mvm_v8_scale_and_add_batch": "test_mvm_v8_batch.py::test_the_fused_v8_batch_call_captures_into_a_graph",
    "clm8_mvm_scale_and_add_batch": "test_m8_mvm_batch_capture.py::test_the_fused_m8_batch_call_captures_into_a_graph",
    "clm8_gemm": "test_gemm8.py::test_gpu_captured_call_replays",
    "clm4_gemm_m8": "test_gemm8.py::test_gpu_captured_call_replays",
}

_NO_WORK = "no stream argument, enqueues no work"
_SHARDED = "runs on streams of its own across devices"
NOT_CAPTURED = {
    **{n: _NO_WORK for n in (
        "clv_version", "clv_last_error", "clv_device_count", "clv_set_device", "clv_get_device", "clv_device_info", "clv_malloc", "clv_free",
        "clv_host_alloc", "clv_host_free", "clv_stream_create", "clv_stream_destroy", "clv_device_sync", "clv_event_create", "clv_event_destroy",
        "clv_event_sync", "clv_event_elapsed_ms", "clv_rng_set_segments", "clv4_dot_workspace_bytes", "clv8_dot_workspace_bytes",
        "clv4_threshold_workspace_bytes", "clv8_threshold_workspace_bytes", "clv_threshold_reference_workspace_bytes",
        "clv_threshold_reference_workspace_bytes_k", "clv_iht_persistent_launches", "clv_mvm_batch_launches", "clm4_shard_partition")},
    "clv_stream_sync": "synchronises by contract",
    "clv_memcpy_d2h": "synchronises by contract",
    "clv_rng_get": "synchronises by contract",
    "clv_rng_set": "synchronises by contract: its source is a stack buffer",
    "clv_rng_seed": "synchronises by contract: clv_rng_set behind it",
    "clv_rng_graph_mode": "by contract called outside the capture, before it; leaving the mode synchronises",
    "clv_memcpy_h2d": "the source is pageable host memory read when the copy runs: a graph would replay a host address the caller no longer owns",
    "clv_memset": "memory function: hipMemsetAsync and nothing else, no kernel and no state of the library; every row here uses it for its prefill",
    "clv_event_record": "enqueues no work of the library; an event recorded under capture belongs to the graph, not to the caller",
    "clm4_gemm_prepare": "allocates by contract",
    "clm4_gemm_release": "frees by contract",
    **{n: _SHARDED for n in SIGNATURES if n.startswith("clm4_sharded_")},
}
# also not captured, and no entry of its own: the persistent one-launch form of clm4_iht / clm4_iht_v8 -- every workgroup must be
# co-resident and the cross-stream chain is skipped under capture (PersistChain::begin); CLV_IHT_PERSISTENT=0 is the capturable form


def test_every_entry_point_is_captured_or_says_why_not():
    tests = Path(__file__).parent
    sets = {k: set(v) for k, v in dict(CAPTURED=CAPTURED, CAPTURED_ELSEWHERE=CAPTURED_ELSEWHERE, NOT_CAPTURED=NOT_CAPTURED).items()}
    for a, b in (("CAPTURED", "CAPTURED_ELSEWHERE"), ("CAPTURED", "NOT_CAPTURED"), ("CAPTURED_ELSEWHERE", "NOT_CAPTURED")):
        assert not sets[a] & sets[b], (a, b, sets[a] & sets[b])
    entries = {n for n in SIGNATURES if "_f16_" not in n}                      # the f16 names: tests/test_half16_capture.py
    union = sets["CAPTURED"] | sets["CAPTURED_ELSEWHERE"] | sets["NOT_CAPTURED"]
    assert union == entries, (sorted(entries - union), sorted(union - entries))
    # every row runs, belongs to the entry it is filed under, and is filed
    names = set(CASES) | set(STOCHASTIC)
    assert len(CASES) == len(set(CASES))
    for entry, rows in CAPTURED.items():
        assert rows and set(rows) <= names and all(r.split()[0] == entry for r in rows), entry
    assert names == {r for rows in CAPTURED.values() for r in rows}
    assert set(STOCHASTIC.values()) <= set(CASES) | set(STOCHASTIC_ONLY_ROWS) and not set(CASES) & set(STOCHASTIC_ONLY_ROWS)
    for entry, where in CAPTURED_ELSEWHERE.items():
        file, test = where.split("::")
        text = (tests / file).read_text()
        assert f"def {test}(" in text and re.search(rf"\b{entry}\b", text) and "hipStreamBeginCapture" in text, (entry, where)
    assert all(isinstance(r, str) and r for r in NOT_CAPTURED.values())
    # the sizes the rows derive from the sources are the ones the headers document
    assert NBLK == 1 << 18 and SMALL_LAST == {4: 131072, 8: 32768}


# ---------------------------------------------------------------- the library's scratch under capture
def _reference_problem(oracle, seed, n_pad):
    q, s = tied4(np.random.default_rng(seed), n_pad)
    return q, s, n_pad - 100


@pytest.mark.gpu
def test_a_first_scratch_call_under_capture_is_refused_with_advice(hip, oracle):
    """REFERENCE mode with workspace == NULL takes the stream's scratch; a stream that is capturing and has none must get CLV_ERR_INVALID
    and the advice BEFORE the library allocates or waits (illegal under a global-mode capture, which they would invalidate): the capture
    still ends well, and the same call made eagerly afterwards gives the oracle's bytes."""
    L = hip.lib
    q, s, n = _reference_problem(oracle, 5, N)
    dq, ds = hip.to_device(q), hip.to_device(s)
    g = fresh_graph(L)
    g.begin()
    rc = L.clv4_threshold_mode(dq.ptr, ds.ptr, n, N, K_REF, THRESHOLD_REFERENCE, None, g.stream)
    message = L.clv_last_error().decode()
    end = g.end()
    print("first scratch call under capture: rc", rc, "| message:", message, "| hipStreamEndCapture:", end)
    assert rc == -1, (rc, message)                                             # CLV_ERR_INVALID
    assert "make one ordinary call of this size on the stream before hipStreamBeginCapture" in message
    assert end == 0
    hip.check(L.clv4_threshold_mode(dq.ptr, ds.ptr, n, N, K_REF, THRESHOLD_REFERENCE, None, g.stream))
    g.sync()
    assert same(dq.download(np.uint8), oracle.v4_threshold(q, s, n, K_REF))
    g.close(L)


@pytest.mark.gpu
def test_a_captured_scratch_call_that_needs_more_than_the_stream_has_is_refused(hip, oracle):
    """the same for growth: the stream has the 1 MiB a small call left it, the captured call needs more"""
    L = hip.lib
    big = 1 << 19
    q, s, n = _reference_problem(oracle, 6, big)
    dq, ds = hip.to_device(q), hip.to_device(s)
    small = _reference_problem(oracle, 7, N)
    dq0, ds0 = hip.to_device(small[0]), hip.to_device(small[1])
    g = fresh_graph(L)
    hip.check(L.clv4_threshold_mode(dq0.ptr, ds0.ptr, small[2], N, K_REF, THRESHOLD_REFERENCE, None, g.stream))
    g.sync()
    assert L.clv_threshold_reference_workspace_bytes_k(big, K_REF) > 1 << 20 >= L.clv_threshold_reference_workspace_bytes_k(N, K_REF)
    g.begin()
    rc = L.clv4_threshold_mode(dq.ptr, ds.ptr, n, big, K_REF, THRESHOLD_REFERENCE, None, g.stream)
    message = L.clv_last_error().decode()
    end = g.end()
    assert rc == -1 and "before hipStreamBeginCapture" in message, (rc, message)
    assert end == 0
    assert same(dq.download(np.uint8), q)                                      # nothing was enqueued
    g.close(L)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["clm4_iht", "clm4_iht_v8"])
def test_the_persistent_loop_passes_the_refusal_on(hip, entry):
    """the persistent one-launch loop takes scratch too: captured on a stream that has none it returns the scratch's CLV_ERR_INVALID and
    advice, not CLV_ERR_HIP, enqueues nothing and leaves the capture valid (the persistent form is not meant for capture; this is what a
    caller who tries gets told)"""
    L = hip.lib
    assert "CLV_IHT_PERSISTENT" not in os.environ
    m, n = 256, 512                                                            # a shape tests/test_iht_persistent.py runs persistently, both widths
    rng = np.random.default_rng(3)
    bits = 4 if entry == "clm4_iht" else 8
    Phi, PhiT, y = mat4(rng, m, n), mat4(rng, n, m), VEC[bits](rng, m)
    b = [hip.to_device(a) for a in (*Phi, *PhiT, *y)]
    off, total = lvec(bits, n, "x", "t1", "t2", "t3")
    out = hip.alloc(total)
    hip.check(L.clv_memset(out.ptr, 0xA5, total, None))
    hip.sync()
    p = {k: out.ptr + v for k, v in off.items()}
    launches = L.clv_iht_persistent_launches()
    g = fresh_graph(L)
    g.begin()
    rc = getattr(L, entry)(b[0].ptr, b[1].ptr, b[2].ptr, b[3].ptr, m, n, p["x"], p["sx"], n, b[4].ptr, b[5].ptr, p["t1"], p["st1"], p["t2"], p["st2"],
                           p["t3"], p["st3"], ITERS, n // 4, 0.002, 1, None, g.stream)
    message = L.clv_last_error().decode()
    end = g.end()
    assert rc == -1 and "before hipStreamBeginCapture" in message, (rc, message)
    assert end == 0
    assert L.clv_iht_persistent_launches() == launches
    assert np.all(out.download(np.uint8) == 0xA5)
    g.close(L)


@pytest.mark.gpu
def test_b_scratch_growth_after_a_capture_leaves_the_captured_buffer_alive(hip, oracle):
    """A graph holds the address of the scratch it was captured with.  A later, larger eager call on the stream makes the scratch grow: the
    captured buffer must be retired (kept until clv_stream_destroy), not freed, or the next replay works in freed device memory."""
    L = hip.lib
    big = 1 << 19
    assert L.clv_threshold_reference_workspace_bytes_k(big, K_REF) > 1 << 20 >= L.clv_threshold_reference_workspace_bytes_k(N, K_REF)
    q, s, n = _reference_problem(oracle, 1, N)
    dq, ds, out, eager = hip.to_device(q), hip.to_device(s), hip.alloc(N // 2), hip.alloc(N // 2)

    def enqueue(dst, stream):
        hip.check(L.clv_memcpy_d2d(dst.ptr, dq.ptr, N // 2, stream))
        hip.check(L.clv4_threshold_mode(dst.ptr, ds.ptr, n, N, K_REF, THRESHOLD_REFERENCE, None, stream))
    g = Graph()
    g.capture(lambda st: enqueue(out, st))
    qb, sb, nb = _reference_problem(oracle, 2, big)
    dqb, dsb = hip.to_device(qb), hip.to_device(sb)
    hip.check(L.clv4_threshold_mode(dqb.ptr, dsb.ptr, nb, big, K_REF, THRESHOLD_REFERENCE, None, g.stream))     # the scratch grows here
    g.sync()
    assert same(dqb.download(np.uint8), oracle.v4_threshold(qb, sb, nb, K_REF))
    seen = []
    for rep in range(2):
        q, s, _ = _reference_problem(oracle, 20 + rep, N)
        dq.upload(q, g.stream)
        ds.upload(s, g.stream)
        hip.check(L.clv_memset(out.ptr, 0xA5, N // 2, g.stream))
        g.replay()
        got = out.download(np.uint8)
        enqueue(eager, g.stream)
        g.sync()
        assert same(got, eager.download(np.uint8)), rep
        assert same(got, oracle.v4_threshold(q, s, n, K_REF)), rep
        seen.append(got)
    assert not same(seen[0], seen[1])
    g.close(L)
