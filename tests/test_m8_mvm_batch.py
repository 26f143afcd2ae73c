"""The batch calls of the pure 8-bit path on the GPU: clm8_mvm_batch, clm8_mvm_batch_at, clm8_mvm_scale_and_add_batch and clm8_iht_batch
equal the sequence of single calls (clm8_mvm, clm8_mvm_scale_and_add, clm8_iht) BIT FOR BIT -- results, t1 .. t3 and the XORShift state left
behind -- and the CPU references: tests/matrix8_restate.c (Restate.mvm) for the mvm, followed by oracle.v8_scale_and_add for the fused form,
and the CPU loop of test_matrix8_fused.py for the IHT.  Every comparison is of bytes.

Shapes: the smallest at which each thing can go wrong (C = M8B_CHUNK, the columns k_m8_mvm_batch stages in LDS per pass, read from
clover_amd/csrc/matrix8_batch.hip; the unrolled body covers M8B_U blocks = 512 columns):
  (64, 128)          one row group, two blocks (the unroll tail only)
  (128, 384)         six blocks: fewer than U
  (192, 256)         a row shard: rows no multiple of 128
  (64, C - 128), (64, C), (64, C + 128), (128, 2 C + 128)     one chunk short of full, exactly full, re-staged once with a two-block rest,
                     re-staged twice: U-steps and tail inside a chunk, the barriers between chunks
  (128, C + 640)     a multiple of neither the U-step nor C: a re-staged chunk with one U-step AND a tail
nvec: 1 (forwards), 2 (a pass that is not full), 3 and 5 (masked slots of the 4- and 8-vector instantiations), 8 (a full pass), 9 and 17
(full passes plus a remainder of 1; with a generator the state is handed over between the groups).  Bytes lie in [-127, 127] (-128 is
excluded as in full_range_bytes: the restatement does not define the reference's maddubs form for it) with -127 and 127 at known places,
scales in [0.5, 2); vector 1 is all zero (its result block is zero: fix_zero_max), vector 2 is vector 0's POINTER again, the matrix has a
zero tile and, from two row groups on, a zero row group.  Every case runs with CLV_MVM_BATCH=1 (the batched kernel, whatever the measured
rule says) and, at the small shapes, with the measured rule as well.  The nontemporal instantiations: test_m8_mvm_batch_streaming.py."""
import re
from pathlib import Path

import numpy as np
import pytest

import gf2
from clover_amd.lib_binding import THRESHOLD_FAST, THRESHOLD_REFERENCE  # noqa: F401
from matrix8_helpers import full_range_bytes, m8  # noqa: F401
from oracle.binding import Oracle
from test_matrix8_fused import MU, _cpu_loop
from test_mvm_batch import KEYS, NVMAX, assert_same_vectors, batch_kernel, fresh, pa, same
from test_mvm_batch_stochastic import keys_equal, moved, orng_at, set_state

ROOT = Path(__file__).resolve().parent.parent
SRC = (ROOT / "clover_amd" / "csrc" / "matrix8_batch.hip").read_text()
CHUNK = int(re.search(r"#define\s+M8B_CHUNK\s+(\d+)u", SRC).group(1))
USTEP = 64 * int(re.search(r"#define\s+M8B_U\s+(\d+)", SRC).group(1))
SMALL = [(64, 128), (128, 384), (192, 256)]
ODD = (128, CHUNK + USTEP + 128)
CHUNKY = [(64, CHUNK - 128), (64, CHUNK), (64, CHUNK + 128), (128, 2 * CHUNK + 128), ODD]
ST_SHAPES = [(64, 128), (192, 256), (128, CHUNK + 128)]
NVECS = (1, 2, 3, 5, 8, 9, 17)
A_FUSED = 0.37
assert ODD[1] % USTEP and ODD[1] % CHUNK


def pairs8(hip, count, n, fill=0x5A):
    """count x (n bytes, n / 64 scales), prefilled"""
    return [(fresh(hip, n, fill), fresh(hip, n // 16, fill)) for _ in range(count)]


def get8(pair, n):
    return pair[0].download(np.int8, n), pair[1].download(np.float32, n // 64)


def eq(p, q):
    return same(p[0], q[0]) and same(p[1], q[1])


def v8(rng, n):
    """n int8 in [-127, 127] with -127 and 127 at known places, scales in [0.5, 2)"""
    q = full_range_bytes(rng, n)
    q[[3, n // 2 + 1, n - 1]] = [-127, 127, -127]
    return q, rng.uniform(0.5, 2.0, size=n // 64).astype(np.float32)


def matrix8(rng, rows, cols):
    qA, sA = full_range_bytes(rng, rows * cols), rng.uniform(0.5, 2.0, size=(rows // 64) * (cols // 64)).astype(np.float32)
    A = qA.reshape(rows, cols)
    A[0, 5], A[rows // 2, cols - 1] = 127, -127
    A[:64, 64:128] = 0                                                      # a zero tile
    if rows > 64:
        A[rows - 64:, :] = 0                                                # a zero row group: its result block is all zero
    return qA, sA


def copies_of(hip, src, count, n):
    w = pairs8(hip, count, n)
    for (wq, ws), (pq, ps) in zip(w, src):
        hip.check(hip.lib.clv_memcpy_d2d(wq.ptr, pq.ptr, n, None))
        hip.check(hip.lib.clv_memcpy_d2d(ws.ptr, ps.ptr, n // 16, None))
    return w


class Shape:
    """one matrix and NVMAX vectors on the device, the restatement's and the single call's results per vector: computed once per shape"""

    def __init__(self, hip, cpu, rows, cols):
        rng = np.random.default_rng(rows * 1000003 + cols + 88)
        self.rows, self.cols = rows, cols
        self.qA, self.sA = matrix8(rng, rows, cols)
        self.x = [v8(rng, cols) for _ in range(NVMAX)]
        self.x[1] = (np.zeros(cols, np.int8), self.x[1][1])                 # all zero
        self.x[2] = self.x[0]
        self.u = [v8(rng, rows) for _ in range(NVMAX)]
        self.dA, self.dsA = hip.to_device(self.qA), hip.to_device(self.sA)
        self.dx = [(hip.to_device(q), hip.to_device(s)) for q, s in self.x]
        self.dx[2] = self.dx[0]                                             # the same pointers twice
        self.du = [(hip.to_device(q), hip.to_device(s)) for q, s in self.u]
        self.cpu = [cpu.mvm(self.qA, self.sA, rows, cols, *x) for x in self.x]
        out = pairs8(hip, NVMAX, rows)
        for (dq, ds), (r, sr) in zip(self.dx, out):
            hip.check(hip.lib.clm8_mvm(self.dA.ptr, self.dsA.ptr, rows, cols, dq.ptr, ds.ptr, r.ptr, sr.ptr, None, None))
        hip.sync()
        self.single = [get8(o, rows) for o in out]
        self._st = None

    def xs(self, nvec):
        return pa([d[0] for d in self.dx[:nvec]]), pa([d[1] for d in self.dx[:nvec]])

    def stochastic(self, hip, oracle, cpu):
        """once: the CPU sequence and the single device calls for NVMAX vectors from KEYS, plain and fused, with the state after every vector"""
        if self._st is None:
            self._st = Stochastic(hip, oracle, cpu, self)
        return self._st


class Stochastic:
    def __init__(self, hip, oracle, cpu, S):
        L, rows, cols = hip.lib, S.rows, S.cols
        self.fresh = Oracle.rng_keys(oracle.rng(*KEYS))
        o = oracle.rng(*KEYS)
        self.o_mvm, self.o_mvm_keys = [], []
        for x in S.x:
            self.o_mvm.append(cpu.mvm(S.qA, S.sA, rows, cols, *x, o))
            self.o_mvm_keys.append(Oracle.rng_keys(o))
        o = oracle.rng(*KEYS)
        self.o_t, self.o_r, self.o_fused_keys = [], [], []
        for x, u in zip(S.x, S.u):
            t = cpu.mvm(S.qA, S.sA, rows, cols, *x, o)
            self.o_t.append(t)
            self.o_r.append(oracle.v8_scale_and_add(*u, *t, A_FUSED, o))
            self.o_fused_keys.append(Oracle.rng_keys(o))
        st, out = hip.new_rng(*KEYS), pairs8(hip, NVMAX, rows)
        self.d_mvm_keys = []
        for (dq, ds), (r, sr) in zip(S.dx, out):
            hip.check(L.clm8_mvm(S.dA.ptr, S.dsA.ptr, rows, cols, dq.ptr, ds.ptr, r.ptr, sr.ptr, st.ptr, None))
            self.d_mvm_keys.append(hip.rng_get(st))
        self.d_mvm = [get8(p, rows) for p in out]
        st, t, r = hip.new_rng(*KEYS), pairs8(hip, NVMAX, rows), pairs8(hip, NVMAX, rows)
        self.d_fused_keys = []
        for j in range(NVMAX):
            hip.check(L.clm8_mvm_scale_and_add(S.dA.ptr, S.dsA.ptr, rows, cols, S.dx[j][0].ptr, S.dx[j][1].ptr, S.du[j][0].ptr, S.du[j][1].ptr,
                                               A_FUSED, t[j][0].ptr, t[j][1].ptr, r[j][0].ptr, r[j][1].ptr, st.ptr, None))
            self.d_fused_keys.append(hip.rng_get(st))
        self.d_t, self.d_r = [get8(p, rows) for p in t], [get8(p, rows) for p in r]


_shapes = {}


def shape(hip, cpu, rows, cols):
    if (rows, cols) not in _shapes:
        _shapes[(rows, cols)] = Shape(hip, cpu, rows, cols)
    return _shapes[(rows, cols)]


def groups(nvec):
    return (nvec + 7) // 8


# ---------------------------------------------------------------- mvm
MVM_CASES = [(r, c, nv, f) for r, c in SMALL for nv in NVECS for f in ("1", None)] + [(r, c, nv, "1") for r, c in CHUNKY for nv in NVECS]


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,nvec,force", MVM_CASES)
def test_m8_mvm_batch_equals_the_single_calls_and_the_restatement(hip, m8, rows, cols, nvec, force):  # noqa: F811
    S = shape(hip, m8, rows, cols)
    L = hip.lib
    for j in range(nvec):
        assert eq(S.single[j], S.cpu[j]), f"clm8_mvm itself differs from the restatement, vector {j}"
    out = pairs8(hip, nvec, rows)
    before = L.clv_mvm_batch_launches()
    with batch_kernel(force):
        hip.check(L.clm8_mvm_batch(S.dA.ptr, S.dsA.ptr, rows, cols, nvec, *S.xs(nvec), pa([o[0] for o in out]), pa([o[1] for o in out]), None, None))
    hip.sync()
    if force:
        assert L.clv_mvm_batch_launches() - before == nvec // 8 + (nvec % 8 >= 2), "one batched launch per group of two or more"
    for j in range(nvec):
        got = get8(out[j], rows)
        assert eq(got, S.single[j]), f"vector {j} differs from clm8_mvm"
        assert eq(got, S.cpu[j]), f"vector {j} differs from the restatement"
    if nvec >= 2:
        assert not np.any(get8(out[1], rows)[0]) and np.all(get8(out[1], rows)[1] == 1.0), "the zero vector: zero bytes, scales 1.0"
    if rows > 64:
        assert not np.any(get8(out[0], rows)[0][-64:]) and get8(out[0], rows)[1][-1] == 1.0, "the zero row group"
    if nvec >= 3:
        assert eq(get8(out[2], rows), get8(out[0], rows)), "the same x twice"
    assert np.any(S.cpu[0][0]), "every result is zero: the comparison shows nothing"


# ---------------------------------------------------------------- the fused form
@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", SMALL + CHUNKY)
@pytest.mark.parametrize("nvec", NVECS)
def test_m8_fused_batch_equals_the_single_calls_and_the_cpu(hip, m8, oracle, rows, cols, nvec):  # noqa: F811
    """with t, without t, in place; the launch counter under CLV_MVM_BATCH=1; the small shapes with the measured rule too"""
    S = shape(hip, m8, rows, cols)
    L = hip.lib
    for a, with_t, in_place in ((-1.0, True, False), (A_FUSED, False, False), (A_FUSED, True, True), (-1.0, False, True)):
        def run(how):
            u = copies_of(hip, S.du, nvec, rows)                            # working copies of u: the in-place form overwrites them
            t = pairs8(hip, nvec, rows) if with_t else None
            r = u if in_place else pairs8(hip, nvec, rows)
            dx = S.dx[:nvec]
            if how != "single":
                before = L.clv_mvm_batch_launches()
                with batch_kernel(how):
                    hip.check(L.clm8_mvm_scale_and_add_batch(
                        S.dA.ptr, S.dsA.ptr, rows, cols, nvec, *S.xs(nvec), pa([d[0] for d in u]), pa([d[1] for d in u]), a,
                        pa([d[0] for d in t]) if t else None, pa([d[1] for d in t]) if t else None, pa([d[0] for d in r]), pa([d[1] for d in r]),
                        None, None))
                if how == "1":
                    assert L.clv_mvm_batch_launches() - before == nvec // 8 + (nvec % 8 >= 2), "one batched launch per group of two or more"
            else:
                for j in range(nvec):
                    hip.check(L.clm8_mvm_scale_and_add(S.dA.ptr, S.dsA.ptr, rows, cols, dx[j][0].ptr, dx[j][1].ptr, u[j][0].ptr, u[j][1].ptr, a,
                                                       t[j][0].ptr if t else None, t[j][1].ptr if t else None, r[j][0].ptr, r[j][1].ptr, None, None))
            hip.sync()
            return [get8(p, rows) for p in r], ([get8(p, rows) for p in t] if t else None), (None if in_place else [get8(p, rows) for p in u])
        r1, t1, _ = run("single")
        for how in ("1", None) if (rows, cols) in SMALL else ("1",):
            what = f"a={a} t={with_t} in_place={in_place} CLV_MVM_BATCH={how}"
            r2, t2, u2 = run(how)
            for j in range(nvec):
                assert eq(r2[j], r1[j]), f"{what}: r of vector {j}"
                want = oracle.v8_scale_and_add(*S.u[j], *S.cpu[j], a)
                assert eq(r2[j], want), f"{what}: r of vector {j} against the CPU"
                if with_t:
                    assert eq(t2[j], t1[j]), f"{what}: t of vector {j}"
                    assert eq(t2[j], S.cpu[j]), f"{what}: t of vector {j} against the restatement"
                if not in_place:
                    assert eq(u2[j], S.u[j]), f"{what}: u of vector {j} was written"


# ---------------------------------------------------------------- with a generator: contiguous windows
CONTIG = [(r, c, nv, "1") for r, c in ST_SHAPES for nv in NVECS[1:]] + [(r, c, nv, None) for r, c in ST_SHAPES[:2] for nv in NVECS[1:]]


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,nvec,force", CONTIG)
def test_stochastic_m8_mvm_batch_equals_the_cpu_sequence_and_the_single_calls(hip, m8, oracle, rows, cols, nvec, force):  # noqa: F811
    S = shape(hip, m8, rows, cols)
    T = S.stochastic(hip, oracle, m8)
    L = hip.lib
    st, out = hip.new_rng(*KEYS), pairs8(hip, nvec, rows)
    before = L.clv_mvm_batch_launches()
    with batch_kernel(force):
        hip.check(L.clm8_mvm_batch(S.dA.ptr, S.dsA.ptr, rows, cols, nvec, *S.xs(nvec), pa([o[0] for o in out]), pa([o[1] for o in out]), st.ptr, None))
    hip.sync()
    if force:
        assert L.clv_mvm_batch_launches() - before == groups(nvec), "forced, with a generator: every group on the batched kernel, a group of one too"
    for j in range(nvec):
        got = get8(out[j], rows)
        assert eq(T.d_mvm[j], T.o_mvm[j]), f"clm8_mvm itself differs from the restatement, vector {j}"
        assert eq(got, T.o_mvm[j]), f"vector {j} differs from the CPU sequence"
        assert eq(got, T.d_mvm[j]), f"vector {j} differs from the single calls"
    keys = hip.rng_get(st)
    assert keys_equal(keys, T.o_mvm_keys[nvec - 1]), "the state left behind differs from the oracle generator's"
    assert keys_equal(keys, T.d_mvm_keys[nvec - 1]), "the state left behind differs from the single calls'"
    assert not keys_equal(keys, T.fresh)
    assert not eq(T.o_mvm[0], S.cpu[0]), "the noise changed nothing: the comparison shows less than it should"


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,nvec,force", CONTIG)
def test_stochastic_m8_fused_batch_equals_the_cpu_sequence_and_the_single_calls(hip, m8, oracle, rows, cols, nvec, force):  # noqa: F811
    """t stored, t not stored, in place: r is the same in all three"""
    S = shape(hip, m8, rows, cols)
    T = S.stochastic(hip, oracle, m8)
    L = hip.lib
    for with_t, in_place in ((True, False), (False, False), (True, True)):
        u = copies_of(hip, S.du, nvec, rows)
        t = pairs8(hip, nvec, rows) if with_t else None
        r = u if in_place else pairs8(hip, nvec, rows)
        st = hip.new_rng(*KEYS)
        with batch_kernel(force):
            hip.check(L.clm8_mvm_scale_and_add_batch(S.dA.ptr, S.dsA.ptr, rows, cols, nvec, *S.xs(nvec), pa([d[0] for d in u]), pa([d[1] for d in u]),
                                                     A_FUSED, pa([d[0] for d in t]) if t else None, pa([d[1] for d in t]) if t else None,
                                                     pa([d[0] for d in r]), pa([d[1] for d in r]), st.ptr, None))
        hip.sync()
        what = f"t={with_t} in_place={in_place}"
        for j in range(nvec):
            got = get8(r[j], rows)
            assert eq(got, T.o_r[j]), f"{what}: r of vector {j} against the CPU sequence"
            assert eq(got, T.d_r[j]), f"{what}: r of vector {j} against the single calls"
            if with_t:
                gt = get8(t[j], rows)
                assert eq(gt, T.o_t[j]) and eq(gt, T.d_t[j]), f"{what}: t of vector {j}"
            if not in_place:
                assert eq(get8(u[j], rows), S.u[j]), f"{what}: u of vector {j} was written"
        keys = hip.rng_get(st)
        assert keys_equal(keys, T.o_fused_keys[nvec - 1]) and keys_equal(keys, T.d_fused_keys[nvec - 1]), f"{what}: the state left behind"


# ---------------------------------------------------------------- clm8_mvm_batch_at
def at_call(hip, S, nvec, st, base, stride, commit):
    out = pairs8(hip, nvec, S.rows)
    rc = hip.lib.clm8_mvm_batch_at(S.dA.ptr, S.dsA.ptr, S.rows, S.cols, nvec, *S.xs(nvec), pa([o[0] for o in out]), pa([o[1] for o in out]),
                                   st.ptr if st else None, base, stride, commit, None)
    return rc, out


def windows(G):
    """(base, stride, commit): stride 0 and commit_draws == 0 -- every vector on the same draws and the state untouched; odd positions, a
    stride that is not the natural 2 G and a commit unrelated to the windows; bases that need the table rounds of the jump-ahead beyond 8
    and beyond 16 bits, up to bit 54"""
    return [(0, 0, 0), (7, 2 * G + 3, 5), ((1 << 33) + 12345, 2 * G, (1 << 20) + 1), (1 << 54, 1, (1 << 54) + 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,force", [(r, c, "1") for r, c in ST_SHAPES] + [(64, 128, None), (192, 256, "0")])
@pytest.mark.parametrize("nvec", [1, 3, 9])
def test_m8_batch_at_places_every_window_where_it_is_told(hip, m8, oracle, rows, cols, nvec, force):  # noqa: F811
    """vector j against the restatement and against clm8_mvm, each on a generator moved to base + j * stride on the test side (tests/gf2.py
    beyond 4096 draws); the state afterwards is the initial one moved by commit -- untouched for commit_draws == 0.  CLV_MVM_BATCH=0 changes
    nothing: the positioned call always runs the batched kernel, one launch per group, at nvec == 1 too."""
    S = shape(hip, m8, rows, cols)
    T = S.stochastic(hip, oracle, m8)
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
            want = m8.mvm(S.qA, S.sA, rows, cols, *S.x[j], orng_at(at))
            set_state(hip, one, at)
            hip.check(L.clm8_mvm(S.dA.ptr, S.dsA.ptr, rows, cols, S.dx[j][0].ptr, S.dx[j][1].ptr, single[0].ptr, single[1].ptr, one.ptr, None))
            hip.sync()
            got = get8(out[j], rows)
            assert eq(got, want), f"{what}: vector {j} against the restatement at its window"
            assert eq(got, get8(single, rows)), f"{what}: vector {j} against clm8_mvm at its window"
        if (base, stride) == (0, 0):
            assert eq(get8(out[0], rows), T.o_mvm[0]), "stride 0: vector 0 is the first single call from the fresh state"


@pytest.mark.gpu
def test_m8_batch_at_with_the_contiguous_windows_without_a_generator_and_beyond_the_tables(hip, m8, oracle):  # noqa: F811
    rows, cols, nvec = 192, 256, 9
    S = shape(hip, m8, rows, cols)
    T = S.stochastic(hip, oracle, m8)
    G = rows // 64
    st = hip.new_rng(*KEYS)
    rc, out = at_call(hip, S, nvec, st, 0, 2 * G, nvec * 2 * G)             # the windows of clm8_mvm_batch
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
        assert rc == -1 and b"clm8_mvm_batch_at" in hip.lib.clv_last_error() and b"2^55" in hip.lib.clv_last_error(), (base, stride, commit)
        hip.sync()
        assert all(np.all(get8(o, rows)[0] == 0x5A) for o in out), "a refused call wrote a result"
    assert hip.lib.clv_mvm_batch_launches() == before, "a refused call launched"
    assert keys_equal(hip.rng_get(st), T.fresh)


@pytest.mark.gpu
def test_the_launch_counter_rises_by_one_per_group_of_the_8_bit_calls(hip, m8, oracle):  # noqa: F811
    """17 vectors: forced with a generator 8 + 8 + 1 (the remainder of one runs batched too), forced without 8 + 8 and one single call;
    under CLV_MVM_BATCH=0 none"""
    rows, cols, nvec = 192, 256, 17
    S = shape(hip, m8, rows, cols)
    T = S.stochastic(hip, oracle, m8)
    L = hip.lib
    for force, rng, want in (("1", True, 3), ("1", False, 2), ("0", True, 0), ("0", False, 0)):
        st, out = (hip.new_rng(*KEYS) if rng else None), pairs8(hip, nvec, rows)
        before = L.clv_mvm_batch_launches()
        with batch_kernel(force):
            hip.check(L.clm8_mvm_batch(S.dA.ptr, S.dsA.ptr, rows, cols, nvec, *S.xs(nvec), pa([o[0] for o in out]), pa([o[1] for o in out]),
                                       st.ptr if st else None, None))
        hip.sync()
        assert L.clv_mvm_batch_launches() - before == want, (force, rng)
        assert all(eq(get8(out[j], rows), (T.d_mvm if rng else S.single)[j]) for j in range(nvec)), (force, rng)
        assert not rng or keys_equal(hip.rng_get(st), T.d_mvm_keys[nvec - 1])


# ---------------------------------------------------------------- IHT / GD
IHT_K = 16
_iht = {}


def iht_data(hip, cpu, m, n, nvec):
    """Phi, its transpose and nvec measurements; vector 1 is all zero, vector 2 is vector 0's pointers again"""
    if (m, n) not in _iht:
        rng = np.random.default_rng(5 + m * 7 + n)
        Phi = matrix8(rng, m, n)
        PhiT = cpu.transpose(*Phi, m, n)
        ys = [v8(rng, m) for _ in range(9)]
        ys[1] = (np.zeros(m, np.int8), ys[1][1])
        ys[2] = ys[0]
        dy = [(hip.to_device(q), hip.to_device(s)) for q, s in ys]
        dy[2] = dy[0]
        _iht[(m, n)] = (Phi, PhiT, ys, [hip.to_device(v) for v in (*Phi, *PhiT)], dy)
    Phi, PhiT, ys, mats, dy = _iht[(m, n)]
    return Phi, PhiT, ys[:nvec], mats, dy[:nvec]


def iht_run(hip, mats, dy, m, n, x_len, thr, batch, rng=None, iters=3):
    L = hip.lib
    nvec = len(dy)
    lens = dict(x=n, t1=m, t2=m, t3=n)
    v = {k: pairs8(hip, nvec, ln, 0x55) for k, ln in lens.items()}
    head = [b.ptr for b in mats] + [m, n]
    if batch:
        arrs = {k: (pa([d[0] for d in v[k]]), pa([d[1] for d in v[k]])) for k in v}
        hip.check(L.clm8_iht_batch(*head, nvec, arrs["x"][0], arrs["x"][1], x_len, pa([d[0] for d in dy]), pa([d[1] for d in dy]), arrs["t1"][0],
                                   arrs["t1"][1], arrs["t2"][0], arrs["t2"][1], arrs["t3"][0], arrs["t3"][1], iters, IHT_K, MU, thr,
                                   rng.ptr if rng else None, None))
    else:
        for j in range(nvec):
            hip.check(L.clm8_iht(*head, v["x"][j][0].ptr, v["x"][j][1].ptr, x_len, dy[j][0].ptr, dy[j][1].ptr, v["t1"][j][0].ptr, v["t1"][j][1].ptr,
                                 v["t2"][j][0].ptr, v["t2"][j][1].ptr, v["t3"][j][0].ptr, v["t3"][j][1].ptr, iters, IHT_K, MU, thr,
                                 rng.ptr if rng else None, None))
    hip.sync()
    return {k: [get8(p, lens[k]) for p in v[k]] for k in v}


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,x_len", [(128, 256, 200), (256, 128, 128)])
@pytest.mark.parametrize("nvec", [3, 9])
@pytest.mark.parametrize("with_rng", [False, True], ids=["deterministic", "generator"])
def test_m8_iht_batch_equals_clm8_iht_per_vector_and_the_cpu_loop(hip, m8, oracle, m, n, x_len, nvec, with_rng):  # noqa: F811
    """three iterations, K = 16, thresholds none / FAST / REFERENCE, forced and with the measured rule: x, t1 .. t3 and, with a generator,
    the state equal clm8_iht for vector 0, then 1, ... on one state, and the CPU loop of test_matrix8_fused.py on one oracle generator.
    Forced, a group of g >= 2 is 2 batched launches per iteration."""
    Phi, PhiT, ys, mats, dy = iht_data(hip, m8, m, n, nvec)
    L = hip.lib
    for thr in (0, 1, 2):
        st1 = hip.new_rng(*KEYS) if with_rng else None
        one = iht_run(hip, mats, dy, m, n, x_len, thr, batch=False, rng=st1)
        keys1 = hip.rng_get(st1) if with_rng else None
        o = oracle.rng(*KEYS) if with_rng else None
        cpu = [_cpu_loop(m8, oracle, Phi, PhiT, y, m, n, x_len, 3, IHT_K, thr, o) for y in ys]
        assert_same_vectors({k: [c[k] for c in cpu] for k in one}, one, f"threshold={thr}: clm8_iht itself against the CPU loop:")
        for force in ("1", None):
            st2 = hip.new_rng(*KEYS) if with_rng else None
            before = L.clv_mvm_batch_launches()
            with batch_kernel(force):
                got = iht_run(hip, mats, dy, m, n, x_len, thr, batch=True, rng=st2)
            if force:
                assert L.clv_mvm_batch_launches() - before == 6 * (nvec // 8 + (nvec % 8 >= 2)), "two batched launches per iteration and group"
            assert_same_vectors(got, one, f"threshold={thr} CLV_MVM_BATCH={force}:")
            if with_rng:
                assert keys_equal(hip.rng_get(st2), keys1), f"threshold={thr} CLV_MVM_BATCH={force}: the state left behind"
                assert keys_equal(keys1, Oracle.rng_keys(o)), "clm8_iht's state against the oracle generator's"
        assert any(np.any(x[0]) for x in one["x"]), "the loop left every x zero: the comparison shows nothing"
        assert not np.any(one["x"][1][0]), "the zero measurement"
    if with_rng:
        st = hip.new_rng(*KEYS)
        with batch_kernel("1"):
            got = iht_run(hip, mats, dy, m, n, x_len, 1, batch=True, rng=st, iters=0)
        assert keys_equal(hip.rng_get(st), Oracle.rng_keys(oracle.rng(*KEYS))), "no iterations: nothing drawn, nothing committed"
        assert all(not np.any(x[0]) and np.all(x[1] == 1.0) for x in got["x"]), "no iterations: every x cleared"
