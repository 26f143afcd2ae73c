"""The batch calls for CloverVector8 vectors on the GPU: clm4_mvm_v8_batch, clm4_mvm_v8_batch_at, clm4_mvm_v8_scale_and_add_batch,
clv8_threshold_batch and clm4_iht_v8_batch equal the sequence of single calls (clm4_mvm_v8, clm4_mvm_v8_scale_and_add, clv8_threshold_mode,
clm4_iht_v8) BIT FOR BIT -- results, t1 .. t3 and the XORShift state left behind -- and the mvm and its fused form also equal the CPU oracle
(oracle.m4_mvm_v8, oracle.v8_scale_and_add).  Every comparison is of bytes.

Shapes: the smallest at which each thing can go wrong (C = MVMB8_CHUNK, the columns k_m4_mvm8_batch stages in LDS per pass, read from
clover_amd/csrc/mvm_batch8.hip):
  (64, 128)          one row group, one step (the unroll tail only)
  (128, 384)         three steps: fewer than U
  (192, 256)         a row shard: rows no multiple of 128
  (64, C - 128), (64, C), (64, C + 128), (128, 2 C + 128)     one chunk short of full, exactly full, re-staged once with a one-step rest,
                     re-staged twice: U-steps and tail inside a chunk, the barriers between chunks
  (128, 32768 + 128) crosses the SINGLE kernel's chunk as well
nvec: 1 (forwards), 2 (a pass that is not full), 3 and 5 (masked slots of the 4- and 8-vector instantiations), 8 (a full pass), 9 and 17
(full passes plus a remainder of 1; with a generator the state is handed over between the groups).  x holds the int8 values -128, -127 and
127; vector 1 is all zero (its result block is zero: fix_zero_max), vector 2 is vector 0's POINTER again, the matrix has a zero tile and,
from two row groups on, a zero row group.  Every case runs with CLV_MVM_BATCH=1 (the batched kernel, whatever the measured rule says) and,
at the small shapes, with the measured rule as well.  The nontemporal instantiations: test_mvm_v8_batch_streaming.py."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import gf2
import test_guard_bands as gb
from clover_amd.lib_binding import THRESHOLD_FAST, THRESHOLD_REFERENCE
from conftest import random_packed
from oracle.binding import Oracle
from test_mvm_batch import KEYS, NVMAX, assert_same_vectors, batch_kernel, fresh, pa, same
from test_mvm_batch_stochastic import keys_equal, moved, orng_at, set_state

ROOT = Path(__file__).resolve().parent.parent
CHUNK = int(re.search(r"#define\s+MVMB8_CHUNK\s+(\d+)u", (ROOT / "clover_amd" / "csrc" / "mvm_batch8.hip").read_text()).group(1))
SMALL = [(64, 128), (128, 384), (192, 256)]
CHUNKY = [(64, CHUNK - 128), (64, CHUNK), (64, CHUNK + 128), (128, 2 * CHUNK + 128), (128, 32768 + 128)]
ST_SHAPES = [(64, 128), (192, 256), (128, CHUNK + 128)]
NVECS = (1, 2, 3, 5, 8, 9, 17)
A_FUSED = 0.37


def pairs8(hip, count, n, fill=0x5A):
    """count x (n bytes, n / 64 scales), prefilled"""
    return [(fresh(hip, n, fill), fresh(hip, n // 16, fill)) for _ in range(count)]


def get8(pair, n):
    return pair[0].download(np.int8, n), pair[1].download(np.float32, n // 64)


def eq(p, q):
    return same(p[0], q[0]) and same(p[1], q[1])


def v8(rng, n):
    """n int8 over the whole range with -128, -127 and 127 at known places, positive scales"""
    q = rng.integers(-128, 128, size=n).astype(np.int8)
    q[[3, n // 2 + 1, n - 1]] = [-128, 127, -127]
    return q, rng.uniform(0.5, 2.0, size=n // 64).astype(np.float32)


def copies_of(hip, src, count, n):
    w = pairs8(hip, count, n)
    for (wq, ws), (pq, ps) in zip(w, src):
        hip.check(hip.lib.clv_memcpy_d2d(wq.ptr, pq.ptr, n, None))
        hip.check(hip.lib.clv_memcpy_d2d(ws.ptr, ps.ptr, n // 16, None))
    return w


class Shape:
    """one matrix and NVMAX vectors on the device, the oracle's and the single call's results per vector: computed once per shape"""

    def __init__(self, hip, oracle, rows, cols):
        rng = np.random.default_rng(rows * 1000003 + cols + 8)
        self.rows, self.cols = rows, cols
        qA, sA = random_packed(rng, rows * cols)[0], rng.uniform(0.5, 2.0, size=(rows // 64) * (cols // 64)).astype(np.float32)
        A = qA.reshape(rows, cols // 2)
        A[:64, :32] = 0                                                     # a zero tile
        if rows > 64:
            A[rows - 64:, :] = 0                                            # a zero row group: its result block is all zero
        self.qA, self.sA = qA, sA
        self.x = [v8(rng, cols) for _ in range(NVMAX)]
        self.x[1] = (np.zeros(cols, np.int8), self.x[1][1])                 # all zero
        self.x[2] = self.x[0]
        self.u = [v8(rng, rows) for _ in range(NVMAX)]
        self.dA, self.dsA = hip.to_device(qA), hip.to_device(sA)
        self.dx = [(hip.to_device(q), hip.to_device(s)) for q, s in self.x]
        self.dx[2] = self.dx[0]                                             # the same pointers twice
        self.du = [(hip.to_device(q), hip.to_device(s)) for q, s in self.u]
        self.oracle = [oracle.m4_mvm_v8(qA, sA, rows, cols, *x) for x in self.x]
        out = pairs8(hip, NVMAX, rows)
        for (dq, ds), (r, sr) in zip(self.dx, out):
            hip.check(hip.lib.clm4_mvm_v8(self.dA.ptr, self.dsA.ptr, rows, cols, dq.ptr, ds.ptr, r.ptr, sr.ptr, None, None))
        hip.sync()
        self.single = [get8(o, rows) for o in out]
        self._st = None

    def xs(self, nvec):
        return pa([d[0] for d in self.dx[:nvec]]), pa([d[1] for d in self.dx[:nvec]])

    def stochastic(self, hip, oracle):
        """once: the oracle sequence and the single device calls for NVMAX vectors from KEYS, plain and fused, with the state after every vector"""
        if self._st is None:
            self._st = Stochastic(hip, oracle, self)
        return self._st


class Stochastic:
    def __init__(self, hip, oracle, S):
        L, rows, cols = hip.lib, S.rows, S.cols
        self.fresh = Oracle.rng_keys(oracle.rng(*KEYS))
        o = oracle.rng(*KEYS)
        self.o_mvm, self.o_mvm_keys = [], []
        for x in S.x:
            self.o_mvm.append(oracle.m4_mvm_v8(S.qA, S.sA, rows, cols, *x, o))
            self.o_mvm_keys.append(Oracle.rng_keys(o))
        o = oracle.rng(*KEYS)
        self.o_t, self.o_r, self.o_fused_keys = [], [], []
        for x, u in zip(S.x, S.u):
            t = oracle.m4_mvm_v8(S.qA, S.sA, rows, cols, *x, o)
            self.o_t.append(t)
            self.o_r.append(oracle.v8_scale_and_add(*u, *t, A_FUSED, o))
            self.o_fused_keys.append(Oracle.rng_keys(o))
        st, out = hip.new_rng(*KEYS), pairs8(hip, NVMAX, rows)
        self.d_mvm_keys = []
        for (dq, ds), (r, sr) in zip(S.dx, out):
            hip.check(L.clm4_mvm_v8(S.dA.ptr, S.dsA.ptr, rows, cols, dq.ptr, ds.ptr, r.ptr, sr.ptr, st.ptr, None))
            self.d_mvm_keys.append(hip.rng_get(st))
        self.d_mvm = [get8(p, rows) for p in out]
        st, t, r = hip.new_rng(*KEYS), pairs8(hip, NVMAX, rows), pairs8(hip, NVMAX, rows)
        self.d_fused_keys = []
        for j in range(NVMAX):
            hip.check(L.clm4_mvm_v8_scale_and_add(S.dA.ptr, S.dsA.ptr, rows, cols, S.dx[j][0].ptr, S.dx[j][1].ptr, S.du[j][0].ptr, S.du[j][1].ptr,
                                                  A_FUSED, t[j][0].ptr, t[j][1].ptr, r[j][0].ptr, r[j][1].ptr, st.ptr, None))
            self.d_fused_keys.append(hip.rng_get(st))
        self.d_t, self.d_r = [get8(p, rows) for p in t], [get8(p, rows) for p in r]


_shapes = {}


def shape(hip, oracle, rows, cols):
    if (rows, cols) not in _shapes:
        _shapes[(rows, cols)] = Shape(hip, oracle, rows, cols)
    return _shapes[(rows, cols)]


def groups(nvec):
    return (nvec + 7) // 8


# ---------------------------------------------------------------- mvm
MVM_CASES = [(r, c, nv, f) for r, c in SMALL for nv in NVECS for f in ("1", None)] + [(r, c, nv, "1") for r, c in CHUNKY for nv in (3, 8, 9)]


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,nvec,force", MVM_CASES)
def test_mvm_v8_batch_equals_the_single_calls_and_the_oracle(hip, oracle, rows, cols, nvec, force):
    S = shape(hip, oracle, rows, cols)
    L = hip.lib
    for j in range(nvec):
        assert eq(S.single[j], S.oracle[j]), f"clm4_mvm_v8 itself differs from the oracle, vector {j}"
    out = pairs8(hip, nvec, rows)
    before = L.clv_mvm_batch_launches()
    with batch_kernel(force):
        hip.check(L.clm4_mvm_v8_batch(S.dA.ptr, S.dsA.ptr, rows, cols, nvec, *S.xs(nvec), pa([o[0] for o in out]), pa([o[1] for o in out]), None, None))
    hip.sync()
    if force:
        assert L.clv_mvm_batch_launches() - before == nvec // 8 + (nvec % 8 >= 2), "one batched launch per group of two or more"
    for j in range(nvec):
        got = get8(out[j], rows)
        assert eq(got, S.single[j]), f"vector {j} differs from clm4_mvm_v8"
        assert eq(got, S.oracle[j]), f"vector {j} differs from the oracle"
    if nvec >= 2:
        assert not np.any(get8(out[1], rows)[0]) and np.all(get8(out[1], rows)[1] == 1.0), "the zero vector: zero bytes, scales 1.0"
    if rows > 64:
        assert not np.any(get8(out[0], rows)[0][-64:]) and get8(out[0], rows)[1][-1] == 1.0, "the zero row group"
    if nvec >= 3:
        assert eq(get8(out[2], rows), get8(out[0], rows)), "the same x twice"


# ---------------------------------------------------------------- the fused form
@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", SMALL + CHUNKY)
@pytest.mark.parametrize("nvec", [2, 5, 9])
def test_fused_v8_batch_equals_the_single_calls(hip, oracle, rows, cols, nvec):
    S = shape(hip, oracle, rows, cols)
    L = hip.lib
    for a, with_t, in_place in ((-1.0, True, False), (A_FUSED, False, False), (A_FUSED, True, True), (-1.0, False, True)):
        def run(batch):
            u = copies_of(hip, S.du, nvec, rows)                            # working copies of u: the in-place form overwrites them
            t = pairs8(hip, nvec, rows) if with_t else None
            r = u if in_place else pairs8(hip, nvec, rows)
            dx = S.dx[:nvec]
            if batch:
                with batch_kernel("1"):
                    hip.check(L.clm4_mvm_v8_scale_and_add_batch(
                        S.dA.ptr, S.dsA.ptr, rows, cols, nvec, *S.xs(nvec), pa([d[0] for d in u]), pa([d[1] for d in u]), a,
                        pa([d[0] for d in t]) if t else None, pa([d[1] for d in t]) if t else None, pa([d[0] for d in r]), pa([d[1] for d in r]),
                        None, None))
            else:
                for j in range(nvec):
                    hip.check(L.clm4_mvm_v8_scale_and_add(S.dA.ptr, S.dsA.ptr, rows, cols, dx[j][0].ptr, dx[j][1].ptr, u[j][0].ptr, u[j][1].ptr, a,
                                                          t[j][0].ptr if t else None, t[j][1].ptr if t else None, r[j][0].ptr, r[j][1].ptr, None, None))
            hip.sync()
            return [get8(p, rows) for p in r], ([get8(p, rows) for p in t] if t else None), (None if in_place else [get8(p, rows) for p in u])
        what = f"a={a} t={with_t} in_place={in_place}"
        (r1, t1, u1), (r2, t2, u2) = run(False), run(True)
        for j in range(nvec):
            assert eq(r2[j], r1[j]), f"{what}: r of vector {j}"
            want = oracle.v8_scale_and_add(*S.u[j], *S.oracle[j], a)
            assert eq(r2[j], want), f"{what}: r of vector {j} against the oracle"
            if with_t:
                assert eq(t2[j], t1[j]), f"{what}: t of vector {j}"
                assert eq(t2[j], S.oracle[j]), f"{what}: t of vector {j} against the oracle"
            if not in_place:
                assert eq(u2[j], S.u[j]), f"{what}: u of vector {j} was written"


# ---------------------------------------------------------------- with a generator: contiguous windows
CONTIG = [(r, c, nv, "1") for r, c in ST_SHAPES for nv in NVECS[1:]] + [(r, c, nv, None) for r, c in ST_SHAPES[:2] for nv in NVECS[1:]]


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,nvec,force", CONTIG)
def test_stochastic_mvm_v8_batch_equals_the_oracle_sequence_and_the_single_calls(hip, oracle, rows, cols, nvec, force):
    S = shape(hip, oracle, rows, cols)
    T = S.stochastic(hip, oracle)
    L = hip.lib
    st, out = hip.new_rng(*KEYS), pairs8(hip, nvec, rows)
    before = L.clv_mvm_batch_launches()
    with batch_kernel(force):
        hip.check(L.clm4_mvm_v8_batch(S.dA.ptr, S.dsA.ptr, rows, cols, nvec, *S.xs(nvec), pa([o[0] for o in out]), pa([o[1] for o in out]), st.ptr, None))
    hip.sync()
    if force:
        assert L.clv_mvm_batch_launches() - before == groups(nvec), "forced, with a generator: every group on the batched kernel, a group of one too"
    for j in range(nvec):
        got = get8(out[j], rows)
        assert eq(T.d_mvm[j], T.o_mvm[j]), f"clm4_mvm_v8 itself differs from the oracle, vector {j}"
        assert eq(got, T.o_mvm[j]), f"vector {j} differs from the oracle sequence"
        assert eq(got, T.d_mvm[j]), f"vector {j} differs from the single calls"
    keys = hip.rng_get(st)
    assert keys_equal(keys, T.o_mvm_keys[nvec - 1]), "the state left behind differs from the oracle's"
    assert keys_equal(keys, T.d_mvm_keys[nvec - 1]), "the state left behind differs from the single calls'"
    assert not keys_equal(keys, T.fresh)
    assert not eq(T.o_mvm[0], S.oracle[0]), "the noise changed nothing: the comparison shows less than it should"


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,nvec,force", CONTIG)
def test_stochastic_fused_v8_batch_equals_the_oracle_sequence_and_the_single_calls(hip, oracle, rows, cols, nvec, force):
    """t stored, t not stored, in place: r is the same in all three"""
    S = shape(hip, oracle, rows, cols)
    T = S.stochastic(hip, oracle)
    L = hip.lib
    for with_t, in_place in ((True, False), (False, False), (True, True)):
        u = copies_of(hip, S.du, nvec, rows)
        t = pairs8(hip, nvec, rows) if with_t else None
        r = u if in_place else pairs8(hip, nvec, rows)
        st = hip.new_rng(*KEYS)
        with batch_kernel(force):
            hip.check(L.clm4_mvm_v8_scale_and_add_batch(S.dA.ptr, S.dsA.ptr, rows, cols, nvec, *S.xs(nvec), pa([d[0] for d in u]), pa([d[1] for d in u]),
                                                        A_FUSED, pa([d[0] for d in t]) if t else None, pa([d[1] for d in t]) if t else None,
                                                        pa([d[0] for d in r]), pa([d[1] for d in r]), st.ptr, None))
        hip.sync()
        what = f"t={with_t} in_place={in_place}"
        for j in range(nvec):
            got = get8(r[j], rows)
            assert eq(got, T.o_r[j]), f"{what}: r of vector {j} against the oracle sequence"
            assert eq(got, T.d_r[j]), f"{what}: r of vector {j} against the single calls"
            if with_t:
                gt = get8(t[j], rows)
                assert eq(gt, T.o_t[j]) and eq(gt, T.d_t[j]), f"{what}: t of vector {j}"
            if not in_place:
                assert eq(get8(u[j], rows), S.u[j]), f"{what}: u of vector {j} was written"
        keys = hip.rng_get(st)
        assert keys_equal(keys, T.o_fused_keys[nvec - 1]) and keys_equal(keys, T.d_fused_keys[nvec - 1]), f"{what}: the state left behind"


# ---------------------------------------------------------------- clm4_mvm_v8_batch_at
def at_call(hip, S, nvec, st, base, stride, commit):
    out = pairs8(hip, nvec, S.rows)
    rc = hip.lib.clm4_mvm_v8_batch_at(S.dA.ptr, S.dsA.ptr, S.rows, S.cols, nvec, *S.xs(nvec), pa([o[0] for o in out]), pa([o[1] for o in out]),
                                      st.ptr if st else None, base, stride, commit, None)
    return rc, out


def windows(G):
    """(base, stride, commit): every vector on the same draws and the state untouched; odd positions and a commit unrelated to the windows;
    bases that need the table rounds of the jump-ahead beyond 8 and beyond 16 bits, up to bit 54"""
    return [(0, 0, 0), (7, 2 * G + 3, 5), ((1 << 33) + 12345, 2 * G, (1 << 20) + 1), (1 << 54, 1, (1 << 54) + 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,force", [(r, c, "1") for r, c in ST_SHAPES] + [(64, 128, None), (192, 256, "0")])
@pytest.mark.parametrize("nvec", [1, 3, 9])
def test_v8_batch_at_places_every_window_where_it_is_told(hip, oracle, rows, cols, nvec, force):
    """vector j against the oracle and against clm4_mvm_v8, each on a generator moved to base + j * stride on the test side (tests/gf2.py
    beyond 4096 draws); the state afterwards is the initial one moved by commit -- untouched for commit_draws == 0.  CLV_MVM_BATCH=0 changes
    nothing: the positioned call always runs the batched kernel, one launch per group."""
    S = shape(hip, oracle, rows, cols)
    T = S.stochastic(hip, oracle)
    L = hip.lib
    assert keys_equal(gf2.advance_keys(T.fresh, 5), moved(oracle, T.fresh, 5))
    for base, stride, commit in windows(rows // 64):
        st = hip.new_rng(*KEYS)
        before = L.clv_mvm_batch_launches()
        with batch_kernel(force):
            rc, out = at_call(hip, S, nvec, st, base, stride, commit)
        hip.check(rc)
        hip.sync()
        assert L.clv_mvm_batch_launches() - before == groups(nvec), "the positioned call did not run the batched kernel"
        what = f"(base, stride, commit) = ({base}, {stride}, {commit})"
        assert keys_equal(hip.rng_get(st), moved(oracle, T.fresh, commit)), f"{what}: the state left behind"
        one, single = hip.new_rng(*KEYS), pairs8(hip, 1, rows)[0]
        for j in range(nvec):
            at = moved(oracle, T.fresh, base + j * stride)
            want = oracle.m4_mvm_v8(S.qA, S.sA, rows, cols, *S.x[j], orng_at(at))
            set_state(hip, one, at)
            hip.check(L.clm4_mvm_v8(S.dA.ptr, S.dsA.ptr, rows, cols, S.dx[j][0].ptr, S.dx[j][1].ptr, single[0].ptr, single[1].ptr, one.ptr, None))
            hip.sync()
            got = get8(out[j], rows)
            assert eq(got, want), f"{what}: vector {j} against the oracle at its window"
            assert eq(got, get8(single, rows)), f"{what}: vector {j} against clm4_mvm_v8 at its window"
        if (base, stride) == (0, 0):
            assert eq(get8(out[0], rows), T.o_mvm[0]), "stride 0: vector 0 is the first single call from the fresh state"


@pytest.mark.gpu
def test_v8_batch_at_with_the_contiguous_windows_without_a_generator_and_beyond_the_tables(hip, oracle):
    rows, cols, nvec = 192, 256, 9
    S = shape(hip, oracle, rows, cols)
    T = S.stochastic(hip, oracle)
    G = rows // 64
    st = hip.new_rng(*KEYS)
    rc, out = at_call(hip, S, nvec, st, 0, 2 * G, nvec * 2 * G)             # the windows of clm4_mvm_v8_batch
    hip.check(rc)
    hip.sync()
    assert all(eq(get8(out[j], rows), T.d_mvm[j]) for j in range(nvec)) and keys_equal(hip.rng_get(st), T.d_mvm_keys[nvec - 1])
    rc, out = at_call(hip, S, nvec, None, 1 << 60, 1 << 60, 1 << 60)        # ignored without an rng
    hip.check(rc)
    hip.sync()
    assert all(eq(get8(out[j], rows), S.single[j]) for j in range(nvec))
    st = hip.new_rng(*KEYS)
    before = hip.lib.clv_mvm_batch_launches()
    for base, stride, commit in (((1 << 55) - 5, 0, 0), (0, 1 << 53, 0), (0, 6, 1 << 55), ((1 << 64) - 1, (1 << 64) - 1, 0)):
        rc, out = at_call(hip, S, nvec, st, base, stride, commit)
        assert rc == -1 and b"clm4_mvm_v8_batch_at" in hip.lib.clv_last_error() and b"2^55" in hip.lib.clv_last_error(), (base, stride, commit)
        hip.sync()
        assert all(np.all(get8(o, rows)[0] == 0x5A) for o in out), "a refused call wrote a result"
    assert hip.lib.clv_mvm_batch_launches() == before, "a refused call launched"
    assert keys_equal(hip.rng_get(st), T.fresh)


@pytest.mark.gpu
def test_the_launch_counter_rises_by_one_per_group(hip, oracle):
    """17 vectors: forced with a generator 8 + 8 + 1 (the remainder of one runs batched too), forced without 8 + 8 and one single call;
    under CLV_MVM_BATCH=0 none"""
    rows, cols, nvec = 192, 256, 17
    S = shape(hip, oracle, rows, cols)
    T = S.stochastic(hip, oracle)
    L = hip.lib
    for force, rng, want in (("1", True, 3), ("1", False, 2), ("0", True, 0), ("0", False, 0)):
        st, out = (hip.new_rng(*KEYS) if rng else None), pairs8(hip, nvec, rows)
        before = L.clv_mvm_batch_launches()
        with batch_kernel(force):
            hip.check(L.clm4_mvm_v8_batch(S.dA.ptr, S.dsA.ptr, rows, cols, nvec, *S.xs(nvec), pa([o[0] for o in out]), pa([o[1] for o in out]),
                                          st.ptr if st else None, None))
        hip.sync()
        assert L.clv_mvm_batch_launches() - before == want, (force, rng)
        assert all(eq(get8(out[j], rows), (T.d_mvm if rng else S.single)[j]) for j in range(nvec)), (force, rng)
        assert not rng or keys_equal(hip.rng_get(st), T.d_mvm_keys[nvec - 1])


# ---------------------------------------------------------------- threshold
def clustered8(n_pad, seed, all_equal=False):
    """few distinct magnitudes (bytes of a small range x a pool of 4 scales), so that the k-th largest has many ties; all_equal: one magnitude"""
    rng = np.random.default_rng(seed)
    if all_equal:
        return np.where(np.arange(n_pad) % 3 == 0, -33, 33).astype(np.int8), np.ones(n_pad // 64, np.float32)
    q = rng.integers(-12, 13, size=n_pad).astype(np.int8)
    q[rng.integers(0, n_pad, size=max(n_pad // 64, 3))] = [-128, 127, -127][seed % 3]
    return q, np.array([0.5, 1.0, 1.0, 2.0], np.float32)[rng.integers(0, 4, size=n_pad // 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [THRESHOLD_FAST, THRESHOLD_REFERENCE])
@pytest.mark.parametrize("n_pad,n", [(128, 128), (4096, 4096 - 37), (8192, 8192), (16384, 16384 - 1), (32768, 32768), (32768 + 128, 32768 + 128)])
def test_threshold_v8_batch_equals_the_single_calls(hip, n_pad, n, mode):
    """n_pad 128 / 4096 / 8192 / 16384 / 32768: k_thresh8_small<W> for W = 1, 1, 2, 4, 8 (4096 - 37 and 16384 - 1: ragged n); 32768 is the
    last size of the one-launch form, 32768 + 128 is forwarded to the single calls (as is REFERENCE mode).  nvec 65: two groups."""
    L = hip.lib
    big = n_pad > 32768
    nvecs = (3,) if big or mode == THRESHOLD_REFERENCE else (1, 3, 65)
    vecs = [clustered8(n_pad, n_pad + j, all_equal=(j == 1)) for j in range(max(nvecs))]
    src = [(hip.to_device(q), hip.to_device(s)) for q, s in vecs]
    ks = (n // 4,) if big or (mode == THRESHOLD_REFERENCE and n_pad > 4096) else (1, n // 4, n - 1, n, n + 5)
    for k in ks:
        for nvec in nvecs:
            if nvec == 65 and k not in (1, n // 4):
                continue

            def run(batch):
                w = copies_of(hip, src, nvec, n_pad)
                if batch:
                    hip.check(L.clv8_threshold_batch(pa([d[0] for d in w]), pa([d[1] for d in w]), nvec, n, n_pad, k, mode, None))
                else:
                    for q, s in w:
                        hip.check(L.clv8_threshold_mode(q.ptr, s.ptr, n, n_pad, k, mode, None, None))
                hip.sync()
                return [get8(p, n_pad) for p in w]
            one, many = run(False), run(True)
            for j in range(nvec):
                assert same(many[j][0], one[j][0]) and same(many[j][1], vecs[j][1]), (k, nvec, j)
                kept = np.count_nonzero(many[j][0][:n])
                if k >= n:
                    assert same(many[j][0], vecs[j][0]), "k >= n: everything survives"
                else:
                    assert kept <= k and (j == 1) <= (kept == k), (k, nvec, j, kept)
                    if j == 1 and mode == THRESHOLD_FAST:
                        assert np.all(many[j][0][:k] != 0) and not np.any(many[j][0][k:n]), "equal magnitudes: the lowest indices survive"


# ---------------------------------------------------------------- IHT / GD
def iht_data(hip, oracle, m, n, nvec, seed=5):
    rng = np.random.default_rng(seed + m * 7 + n)
    qP, sP = random_packed(rng, m * n)[0], rng.uniform(0.5, 2.0, size=(m // 64) * (n // 64)).astype(np.float32)
    qT, sT = oracle.m4_transpose(qP, sP, m, n)
    mats = [hip.to_device(v) for v in (qP, sP, qT, sT)]
    ys = [v8(rng, m) for _ in range(nvec)]
    return mats, [(hip.to_device(q), hip.to_device(s)) for q, s in ys]


def iht_run(hip, mats, dy, m, n, thr, batch, rng=None, iters=3, stream=None, bufs=None):
    L = hip.lib
    nvec = len(dy)
    lens = dict(x=n, t1=m, t2=m, t3=n)
    v = bufs or {k: pairs8(hip, nvec, ln, 0x55) for k, ln in lens.items()}
    x_len, K, mu = n - 5, n // 8, 0.002
    head = [b.ptr for b in mats] + [m, n]
    if batch:
        arrs = {k: (pa([d[0] for d in v[k]]), pa([d[1] for d in v[k]])) for k in v}
        hip.check(L.clm4_iht_v8_batch(*head, nvec, arrs["x"][0], arrs["x"][1], x_len, pa([d[0] for d in dy]), pa([d[1] for d in dy]), arrs["t1"][0],
                                      arrs["t1"][1], arrs["t2"][0], arrs["t2"][1], arrs["t3"][0], arrs["t3"][1], iters, K, mu, thr,
                                      rng.ptr if rng else None, stream))
    else:
        for j in range(nvec):
            hip.check(L.clm4_iht_v8(*head, v["x"][j][0].ptr, v["x"][j][1].ptr, x_len, dy[j][0].ptr, dy[j][1].ptr, v["t1"][j][0].ptr, v["t1"][j][1].ptr,
                                    v["t2"][j][0].ptr, v["t2"][j][1].ptr, v["t3"][j][0].ptr, v["t3"][j][1].ptr, iters, K, mu, thr,
                                    rng.ptr if rng else None, stream))
    return v, lens


def iht_read(v, lens):
    return {k: [get8(p, lens[k]) for p in v[k]] for k in v}


@pytest.mark.gpu
@pytest.mark.parametrize("m,n", [(128, 256), (256, 128)])
@pytest.mark.parametrize("nvec", [2, 3, 8, 9])
@pytest.mark.parametrize("with_rng", [False, True], ids=["deterministic", "generator"])
def test_iht_v8_batch_equals_clm4_iht_v8_per_vector(hip, oracle, m, n, nvec, with_rng):
    """three iterations, thresholds none / FAST / REFERENCE, forced and with the measured rule: x, t1 .. t3 and, with a generator, the
    state equal clm4_iht_v8 for vector 0, then 1, ... on one state.  Forced, a group of g >= 2 is 2 batched launches per iteration."""
    mats, dy = iht_data(hip, oracle, m, n, nvec)
    L = hip.lib
    for thr in (0, 1, 2):
        st1 = hip.new_rng(*KEYS) if with_rng else None
        v1, lens = iht_run(hip, mats, dy, m, n, thr, batch=False, rng=st1)
        hip.sync()
        one, keys1 = iht_read(v1, lens), (hip.rng_get(st1) if with_rng else None)
        for force in ("1", None):
            st2 = hip.new_rng(*KEYS) if with_rng else None
            before = L.clv_mvm_batch_launches()
            with batch_kernel(force):
                v2, _ = iht_run(hip, mats, dy, m, n, thr, batch=True, rng=st2)
            hip.sync()
            if force:
                assert L.clv_mvm_batch_launches() - before == 6 * (nvec // 8 + (nvec % 8 >= 2)), "two batched launches per iteration and group"
            assert_same_vectors(iht_read(v2, lens), one, f"threshold={thr} CLV_MVM_BATCH={force}:")
            assert not with_rng or keys_equal(hip.rng_get(st2), keys1), f"threshold={thr} CLV_MVM_BATCH={force}: the state left behind"
        assert any(np.any(x[0]) for x in one["x"]), "the loop left every x zero: the comparison shows nothing"
        assert not with_rng or not keys_equal(keys1, Oracle.rng_keys(oracle.rng(*KEYS)))
    if with_rng:
        st = hip.new_rng(*KEYS)
        with batch_kernel("1"):
            v0, lens = iht_run(hip, mats, dy, m, n, 1, batch=True, rng=st, iters=0)
        hip.sync()
        assert keys_equal(hip.rng_get(st), Oracle.rng_keys(oracle.rng(*KEYS))), "no iterations: nothing drawn, nothing committed"
        got = iht_read(v0, lens)
        assert all(not np.any(x[0]) and np.all(x[1] == 1.0) for x in got["x"]), "no iterations: every x cleared"


# ---------------------------------------------------------------- graph capture
@pytest.mark.gpu
@pytest.mark.parametrize("generator", [False, True], ids=["deterministic", "generator"])
def test_the_fused_v8_batch_call_captures_into_a_graph(hip, oracle, generator):
    """clm4_mvm_v8_scale_and_add_batch, nvec = 5: no pointer table on the device, nothing allocated.  Captured once (after a warm-up call
    outside the capture), replayed twice on changed inputs; every replay equals the eager single calls on the same inputs -- with a
    generator (the state in clv_rng_graph_mode) the single calls continue the same stream on a second state."""
    L = hip.lib
    rt = C.CDLL("libamdhip64.so")
    stream, graph, gexec = C.c_void_p(), C.c_void_p(), C.c_void_p()

    def ok(rc):
        assert rc == 0, f"HIP runtime call failed: {rc}"
    rows, cols, nvec = 192, 256, 5
    S = shape(hip, oracle, rows, cols)
    dx, du = pairs8(hip, nvec, cols), S.du[:nvec]
    t, r = pairs8(hip, nvec, rows), pairs8(hip, nvec, rows)
    captured, eager = (hip.new_rng(*KEYS), hip.new_rng(*KEYS)) if generator else (None, None)

    def fill(seed):
        rng = np.random.default_rng(seed)
        for q, s in dx:
            xq, xs = v8(rng, cols)
            q.upload(xq)
            s.upload(xs)
        hip.sync()

    def enqueue(st):
        hip.check(L.clm4_mvm_v8_scale_and_add_batch(S.dA.ptr, S.dsA.ptr, rows, cols, nvec, pa([d[0] for d in dx]), pa([d[1] for d in dx]),
                                                    pa([d[0] for d in du]), pa([d[1] for d in du]), -1.0, pa([d[0] for d in t]), pa([d[1] for d in t]),
                                                    pa([d[0] for d in r]), pa([d[1] for d in r]), captured.ptr if captured else None, st))

    def singles():
        wt, wr = pairs8(hip, nvec, rows), pairs8(hip, nvec, rows)
        for j in range(nvec):
            hip.check(L.clm4_mvm_v8_scale_and_add(S.dA.ptr, S.dsA.ptr, rows, cols, dx[j][0].ptr, dx[j][1].ptr, du[j][0].ptr, du[j][1].ptr, -1.0,
                                                  wt[j][0].ptr, wt[j][1].ptr, wr[j][0].ptr, wr[j][1].ptr, eager.ptr if eager else None, None))
        hip.sync()
        return {"t": [get8(p, rows) for p in wt], "r": [get8(p, rows) for p in wr]}

    def got():
        return {"t": [get8(p, rows) for p in t], "r": [get8(p, rows) for p in r]}

    with batch_kernel("1"):
        fill(1)
        ok(rt.hipStreamCreate(C.byref(stream)))
        if generator:
            hip.check(L.clv_rng_graph_mode(captured.ptr, 1, stream))
        enqueue(stream)                                                     # warm-up outside the capture
        ok(rt.hipStreamSynchronize(stream))
        assert_same_vectors(got(), singles(), "the warm-up call:")
        ok(rt.hipStreamBeginCapture(stream, 0))
        enqueue(stream)
        ok(rt.hipStreamEndCapture(stream, C.byref(graph)))
        ok(rt.hipGraphInstantiate(C.byref(gexec), graph, None, None, 0))
        seen = []
        for rep in range(2):
            fill(50 + 10 * rep)
            ok(rt.hipGraphLaunch(gexec, stream))
            ok(rt.hipStreamSynchronize(stream))
            replay = got()
            assert_same_vectors(replay, singles(), f"replay {rep}:")
            seen.append(replay)
        assert not eq(seen[0]["r"][0], seen[1]["r"][0]), "the replays saw the same inputs"
        if generator:
            hip.check(L.clv_rng_graph_mode(captured.ptr, 0, stream))
            assert keys_equal(hip.rng_get(captured), hip.rng_get(eager)), "the state after two replays"
        ok(rt.hipGraphExecDestroy(gexec))
        ok(rt.hipGraphDestroy(graph))
        ok(rt.hipStreamDestroy(stream))


# ---------------------------------------------------------------- guard bands: the five calls in test_guard_bands' table
GB_ENV = {"CLV_MVM_BATCH": "1"}


def _burnt(orc, draws):
    o = orc.rng(*gb.KEYS)
    for _ in range(draws):
        orc.rng_draw(o)
    return o


def _gb_mvm(rows, cols, nvec, st, fused=False, with_t=True, in_place=False, at=False):
    """at: clm4_mvm_v8_batch_at -- deterministic: the positions are ignored; stochastic: windows at 3 + j (2 G + 1), the state moved by 5"""
    def build(R):
        orc = R.oracle
        G = rows // 64
        base, stride, commit = (3, 2 * G + 1, 5) if st else (1 << 60, 1 << 60, 1 << 60)
        qA, sA = gb.m4(rows * cols + 81, rows, cols)
        regs, want = [("A", "input", qA), ("sA", "input", sA)] + ([("rng", "state", None)] if st else []), {}
        o = orc.rng(*gb.KEYS) if st and not at else None
        for j in range(nvec):
            qx, sx = gb.v8(cols + 30 + j, cols)
            regs += [(f"x{j}", "input", qx), (f"sx{j}", "input", sx)]
            t = orc.m4_mvm_v8(qA, sA, rows, cols, qx, sx, _burnt(orc, base + j * stride) if st and at else o)
            if not fused:
                regs += [(f"r{j}", "output", rows), (f"sr{j}", "output", rows // 16)]
                want.update({f"r{j}": t[0], f"sr{j}": t[1]})
                continue
            qu, su = gb.v8(rows + 50 + j, rows)
            r = orc.v8_scale_and_add(qu, su, *t, -0.5, o)
            if with_t:
                regs += [(f"t{j}", "output", rows), (f"st{j}", "output", rows // 16)]
                want.update({f"t{j}": t[0], f"st{j}": t[1]})
            if in_place:
                regs += [(f"u{j}", "inout", qu), (f"su{j}", "inout", su)]
                want.update({f"u{j}": r[0], f"su{j}": r[1]})
            else:
                regs += [(f"u{j}", "input", qu), (f"su{j}", "input", su), (f"r{j}", "output", rows), (f"sr{j}", "output", rows // 16)]
                want.update({f"r{j}": r[0], f"sr{j}": r[1]})
        if st and at:
            o = _burnt(orc, commit)

        def call(L, p):
            a = lambda name: pa([p[f"{name}{j}"] for j in range(nvec)])  # noqa: E731
            before = L.clv_mvm_batch_launches()
            if at:
                rc = L.clm4_mvm_v8_batch_at(p["A"], p["sA"], rows, cols, nvec, a("x"), a("sx"), a("r"), a("sr"), p.get("rng"), base, stride, commit, None)
            elif not fused:
                rc = L.clm4_mvm_v8_batch(p["A"], p["sA"], rows, cols, nvec, a("x"), a("sx"), a("r"), a("sr"), p.get("rng"), None)
            else:
                rc = L.clm4_mvm_v8_scale_and_add_batch(p["A"], p["sA"], rows, cols, nvec, a("x"), a("sx"), a("u"), a("su"), -0.5,
                                                       a("t") if with_t else None, a("st") if with_t else None, a("u" if in_place else "r"),
                                                       a("su" if in_place else "sr"), p.get("rng"), None)
            # without a generator a remainder group of one vector is forwarded to the single call
            want_launches = groups(nvec) if st else nvec // 8 + (nvec % 8 >= 2)
            assert L.clv_mvm_batch_launches() - before == want_launches, "the call did not take the batched kernel"
            return rc
        return gb.Case(regs, call, want, orng=o, env=GB_ENV)
    return build


def _gb_threshold(n_pad, nvec, mode):
    def build(R):
        n, k = n_pad - 37, (n_pad - 37) // 4
        regs, want = [], {}
        for j in range(nvec):
            q, s = gb.threshold_data(8, n_pad, n_pad + 4 + 10 * j)
            regs += [(f"q{j}", "inout", q), (f"s{j}", "input", s)]
            want[f"q{j}"] = gb.threshold_reference(R, 8, q, s, n, k, mode)[0]
        return gb.Case(regs, lambda L, p: L.clv8_threshold_batch(pa([p[f"q{j}"] for j in range(nvec)]), pa([p[f"s{j}"] for j in range(nvec)]), nvec, n,
                                                                 n_pad, k, mode, None), want)
    return build


def _gb_iht(m, n, nvec, thr, st, iters=3):
    """the oracle's loop per vector, vector after vector on ONE generator: the order of the single calls"""
    def build(R):
        orc = R.oracle
        x_len, K, mu = n - 5, n // 4, np.float32(0.002)
        qP, sP = gb.m4(m * n + 13, m, n)
        qT, sT = orc.m4_transpose(qP, sP, m, n)
        regs, want = [("Phi", "input", qP), ("sPhi", "input", sP), ("PhiT", "input", qT), ("sPhiT", "input", sT)], {}
        regs += [("rng", "state", None)] if st else []
        o = orc.rng(*gb.KEYS) if st else None
        for j in range(nvec):
            y = gb.v8(m + 14 + j, m)
            x = (np.zeros(n, np.int8), np.ones(n // 64, np.float32))
            t1 = t2 = t3 = None
            for _ in range(iters):
                t1 = orc.m4_mvm_v8(qP, sP, m, n, *x, o)
                t2 = orc.v8_scale_and_add(*y, *t1, -1.0, o)
                t3 = orc.m4_mvm_v8(qT, sT, n, m, *t2, o)
                x = orc.v8_scale_and_add(*x, *t3, float(mu), o)
                if thr:
                    x = (gb.threshold_reference(R, 8, x[0], x[1], x_len, K, THRESHOLD_REFERENCE if thr == 2 else THRESHOLD_FAST)[0], x[1])
            w = {f"x{j}": x[0], f"sx{j}": x[1], f"t1{j}": t1[0], f"st1{j}": t1[1], f"t2{j}": t2[0], f"st2{j}": t2[1], f"t3{j}": t3[0], f"st3{j}": t3[1]}
            regs += [(f"y{j}", "input", y[0]), (f"sy{j}", "input", y[1])] + [(k, "output", v.nbytes) for k, v in w.items()]
            want.update(w)

        def call(L, p):
            a = lambda name: pa([p[f"{name}{j}"] for j in range(nvec)])  # noqa: E731
            before = L.clv_mvm_batch_launches()
            rc = L.clm4_iht_v8_batch(p["Phi"], p["sPhi"], p["PhiT"], p["sPhiT"], m, n, nvec, a("x"), a("sx"), x_len, a("y"), a("sy"), a("t1"), a("st1"),
                                     a("t2"), a("st2"), a("t3"), a("st3"), iters, K, float(mu), thr, p.get("rng"), None)
            assert L.clv_mvm_batch_launches() - before == 2 * iters, "the call did not take the batched loop"
            return rc
        return gb.Case(regs, call, want, orng=o, env=GB_ENV)
    return build


V8_CASES = []
for _st in (False, True):
    _how = "stochastic" if _st else "rounding disabled"
    V8_CASES.append((f"clm4_mvm_v8_batch 192x640 nvec=3 {_how}", _gb_mvm(192, 640, 3, _st)))
    V8_CASES.append((f"clm4_mvm_v8_batch_at 192x640 nvec=3 {_how}", _gb_mvm(192, 640, 3, _st, at=True)))
    V8_CASES.append((f"clm4_mvm_v8_scale_and_add_batch 192x640 nvec=3 {_how}", _gb_mvm(192, 640, 3, _st, fused=True)))
    V8_CASES.append((f"clm4_mvm_v8_scale_and_add_batch 64x128 nvec=5 t=False in_place=True {_how}",
                     _gb_mvm(64, 128, 5, _st, fused=True, with_t=False, in_place=True)))
    V8_CASES.append((f"clm4_iht_v8_batch 128x256 nvec=3 threshold=1 {_how}", _gb_iht(128, 256, 3, 1, _st)))
V8_CASES.append((f"clm4_mvm_v8_batch 64x{CHUNK + 128} nvec=9 rounding disabled", _gb_mvm(64, CHUNK + 128, 9, False)))
V8_CASES.append((f"clm4_mvm_v8_batch_at 64x{CHUNK + 128} nvec=9 stochastic", _gb_mvm(64, CHUNK + 128, 9, True, at=True)))
V8_CASES.append(("clm4_iht_v8_batch 128x256 nvec=3 threshold=0 rounding disabled", _gb_iht(128, 256, 3, 0, False)))
for _pad in (128, 4096, 32768):
    V8_CASES.append((f"clv8_threshold_batch FAST n_pad={_pad} nvec=3", _gb_threshold(_pad, 3, THRESHOLD_FAST)))
V8_CASES.append(("clv8_threshold_batch REFERENCE n_pad=384 nvec=3", _gb_threshold(384, 3, THRESHOLD_REFERENCE)))
for _name, _build in V8_CASES:
    if _name not in gb.CASES:                 # the coverage test of test_guard_bands.py reads its table when it runs, after every module is imported
        gb.case(_name)(_build)


@pytest.fixture(scope="module")
def refs(oracle):
    return gb.Refs(oracle, None, None)          # the oracle's 4-bit matrix and CloverVector8 routines only


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, _ in V8_CASES])
def test_v8_batch_calls_write_their_outputs_and_nothing_else(hip, refs, name):
    gb.run_case(hip, dict(V8_CASES)[name](refs))
