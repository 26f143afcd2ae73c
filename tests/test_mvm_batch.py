"""The batch calls on the GPU: clm4_mvm_batch, clm4_mvm_scale_and_add_batch, clv4_threshold_batch and clm4_iht_batch equal the sequence
of single calls (clm4_mvm, clm4_mvm_scale_and_add, clv4_threshold_mode, clm4_iht) BIT FOR BIT, and the mvm also equals the CPU oracle.

Shapes: the smallest at which each thing can go wrong (C = MVMB_CHUNK, the columns the batched kernel stages in LDS per pass, read from
clover_amd/csrc/mvm_batch4.hip):
  (64, 128)          one row group, one block pair (the unroll tail only)
  (128, 384)         odd pair count: the tail behind ... nothing (3 pairs < U)
  (192, 256)         a row shard: rows no multiple of 128
  (64, C - 128), (64, C), (64, C + 128), (128, 2 C + 128)     one chunk short of full, exactly full, re-staged once with a one-pair rest,
                     re-staged twice: U-steps and tail inside a chunk, the barriers between chunks
  (128, 65536 + 128) crosses the SINGLE kernel's chunk as well
  8192 x 131072      512 MiB: the nontemporal instantiation (the 256 MiB rule of launch_mvm)
nvec: 1 (forwards), 2 (a pass that is not full), 3 and 5 (masked slots of the 4- and 8-vector instantiations), 8 (a full pass), 9 and 17
(full passes plus a remainder of 1).  Vector 1 is all zero (its result block is zero: fix_zero_max), vector 2 is vector 0's POINTER again
(repeated inputs are allowed and give identical results), the matrix has a zero tile and, from two row groups on, a zero row group.
The launcher may forward a group to single launches where the batched kernel was measured slower: every case runs with
CLV_MVM_BATCH=1 (the batched kernel, whatever the rule says) and, at the first three shapes, with the measured rule as well."""
import contextlib
import ctypes as C
import os
import re
from pathlib import Path

import numpy as np
import pytest

import test_guard_bands as gb
from clover_amd.lib_binding import SIGNATURES, THRESHOLD_FAST, THRESHOLD_REFERENCE  # noqa: F401
from conftest import random_packed

ROOT = Path(__file__).resolve().parent.parent
CHUNK = int(re.search(r"#define\s+MVMB_CHUNK\s+(\d+)u", (ROOT / "clover_amd" / "csrc" / "mvm_batch4.hip").read_text()).group(1))
SMALL = [(64, 128), (128, 384), (192, 256)]
CHUNKY = [(64, CHUNK - 128), (64, CHUNK), (64, CHUNK + 128), (128, 2 * CHUNK + 128), (128, 65536 + 128)]
NVMAX = 17
KEYS = (777, 4242)


def same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


@contextlib.contextmanager
def batch_kernel(force):
    """force: "1" = the batched kernel for every group, "0" = single launches, None = the measured rule"""
    old = os.environ.pop("CLV_MVM_BATCH", None)
    if force is not None:
        os.environ["CLV_MVM_BATCH"] = force
    try:
        yield
    finally:
        os.environ.pop("CLV_MVM_BATCH", None)
        if old is not None:
            os.environ["CLV_MVM_BATCH"] = old


def pa(bufs):
    return (C.c_void_p * len(bufs))(*[b if isinstance(b, int) else b.ptr for b in bufs])


def fresh(hip, nbytes, fill=0x5A):
    b = hip.alloc(nbytes)
    hip.check(hip.lib.clv_memset(b.ptr, fill, nbytes, None))
    return b


def pairs(hip, count, n, fill=0x5A):
    """count x (n / 2 bytes, n / 64 scales), prefilled"""
    return [(fresh(hip, n // 2, fill), fresh(hip, n // 16, fill)) for _ in range(count)]


def get(pair, n):
    return pair[0].download(np.uint8, n // 2), pair[1].download(np.float32, n // 64)


class Shape:
    """one matrix and NVMAX vectors on the device, the oracle's and the single call's results per vector: computed once per shape"""

    def __init__(self, hip, oracle, rows, cols):
        rng = np.random.default_rng(rows * 1000003 + cols)
        self.rows, self.cols = rows, cols
        qA, sA = random_packed(rng, rows * cols)[0], rng.uniform(0.5, 2.0, size=(rows // 64) * (cols // 64)).astype(np.float32)
        A = qA.reshape(rows, cols // 2)
        A[:64, :32] = 0                                                     # a zero tile
        if rows > 64:
            A[rows - 64:, :] = 0                                            # a zero row group: its result block is all zero
        self.qA, self.sA = qA, sA
        self.x = [random_packed(rng, cols) for _ in range(NVMAX)]
        self.x[1] = (np.zeros(cols // 2, np.uint8), self.x[1][1])           # all zero
        self.x[2] = self.x[0]
        self.u = [random_packed(rng, rows) for _ in range(NVMAX)]
        self.dA, self.dsA = hip.to_device(qA), hip.to_device(sA)
        self.dx = [(hip.to_device(q), hip.to_device(s)) for q, s in self.x]
        self.dx[2] = self.dx[0]                                             # the same pointers twice
        self.du = [(hip.to_device(q), hip.to_device(s)) for q, s in self.u]
        self.oracle = [oracle.m4_mvm(qA, sA, rows, cols, *x) for x in self.x]
        out = pairs(hip, NVMAX, rows)
        for (dq, ds), (r, sr) in zip(self.dx, out):
            hip.check(hip.lib.clm4_mvm(self.dA.ptr, self.dsA.ptr, rows, cols, dq.ptr, ds.ptr, r.ptr, sr.ptr, None, None))
        hip.sync()
        self.single = [get(o, rows) for o in out]


_shapes = {}


def shape(hip, oracle, rows, cols):
    if (rows, cols) not in _shapes:
        _shapes[(rows, cols)] = Shape(hip, oracle, rows, cols)
    return _shapes[(rows, cols)]


# ---------------------------------------------------------------- mvm
MVM_CASES = [(r, c, nv, f) for r, c in SMALL for nv in (1, 2, 3, 5, 8, 9, 17) for f in ("1", None)] + \
            [(r, c, nv, "1") for r, c in CHUNKY for nv in (3, 8, 9)]


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,nvec,force", MVM_CASES)
def test_mvm_batch_equals_the_single_calls_and_the_oracle(hip, oracle, rows, cols, nvec, force):
    S = shape(hip, oracle, rows, cols)
    for j in range(nvec):
        assert same(S.single[j][0], S.oracle[j][0]) and same(S.single[j][1], S.oracle[j][1]), f"clm4_mvm itself differs from the oracle, vector {j}"
    out = pairs(hip, nvec, rows)
    with batch_kernel(force):
        hip.check(hip.lib.clm4_mvm_batch(S.dA.ptr, S.dsA.ptr, rows, cols, nvec, pa([d[0] for d in S.dx[:nvec]]), pa([d[1] for d in S.dx[:nvec]]),
                                         pa([o[0] for o in out]), pa([o[1] for o in out]), None, None))
    hip.sync()
    for j in range(nvec):
        r, sr = get(out[j], rows)
        assert same(r, S.single[j][0]) and same(sr, S.single[j][1]), f"vector {j} differs from clm4_mvm"
        assert same(r, S.oracle[j][0]) and same(sr, S.oracle[j][1]), f"vector {j} differs from the oracle"
    if nvec >= 2:
        assert not np.any(get(out[1], rows)[0]) and np.all(get(out[1], rows)[1] == 1.0), "the zero vector: zero nibbles, scales 1.0"
    if rows > 64:
        assert not np.any(get(out[0], rows)[0][-32:]) and get(out[0], rows)[1][-1] == 1.0, "the zero row group"
    if nvec >= 3:
        assert same(get(out[2], rows)[0], get(out[0], rows)[0]) and same(get(out[2], rows)[1], get(out[0], rows)[1]), "the same x twice"


# ---------------------------------------------------------------- the fused form
@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", SMALL + CHUNKY)
@pytest.mark.parametrize("nvec", [2, 5, 9])
def test_fused_batch_equals_the_single_calls(hip, oracle, rows, cols, nvec):
    S = shape(hip, oracle, rows, cols)
    L = hip.lib
    for a in (-1.0, 0.37):
        for with_t in (True, False):
            for in_place in (False, True):
                def run(batch):
                    u = pairs(hip, nvec, rows)                               # working copies of u: the in-place form overwrites them
                    for (wq, ws), (pq, ps) in zip(u, S.du):
                        hip.check(L.clv_memcpy_d2d(wq.ptr, pq.ptr, rows // 2, None))
                        hip.check(L.clv_memcpy_d2d(ws.ptr, ps.ptr, rows // 16, None))
                    t = pairs(hip, nvec, rows) if with_t else None
                    r = u if in_place else pairs(hip, nvec, rows)
                    dx = S.dx[:nvec]
                    if batch:
                        with batch_kernel("1"):
                            hip.check(L.clm4_mvm_scale_and_add_batch(
                                S.dA.ptr, S.dsA.ptr, rows, cols, nvec, pa([d[0] for d in dx]), pa([d[1] for d in dx]), pa([d[0] for d in u]),
                                pa([d[1] for d in u]), a, pa([d[0] for d in t]) if t else None, pa([d[1] for d in t]) if t else None,
                                pa([d[0] for d in r]), pa([d[1] for d in r]), None, None))
                    else:
                        for j in range(nvec):
                            hip.check(L.clm4_mvm_scale_and_add(S.dA.ptr, S.dsA.ptr, rows, cols, dx[j][0].ptr, dx[j][1].ptr, u[j][0].ptr, u[j][1].ptr, a,
                                                               t[j][0].ptr if t else None, t[j][1].ptr if t else None, r[j][0].ptr, r[j][1].ptr, None, None))
                    hip.sync()
                    return [get(p, rows) for p in r], ([get(p, rows) for p in t] if t else None), (None if in_place else [get(p, rows) for p in u])
                what = f"a={a} t={with_t} in_place={in_place}"
                (r1, t1, u1), (r2, t2, u2) = run(False), run(True)
                for j in range(nvec):
                    assert same(r2[j][0], r1[j][0]) and same(r2[j][1], r1[j][1]), f"{what}: r of vector {j}"
                    if with_t:
                        assert same(t2[j][0], t1[j][0]) and same(t2[j][1], t1[j][1]), f"{what}: t of vector {j}"
                        assert same(t2[j][0], S.oracle[j][0]) and same(t2[j][1], S.oracle[j][1]), f"{what}: t of vector {j} against the oracle"
                    if not in_place:
                        assert same(u2[j][0], S.u[j][0]) and same(u2[j][1], S.u[j][1]), f"{what}: u of vector {j} was written"
                r0 = oracle.v4_scale_and_add(*S.u[0], *S.oracle[0], a)
                assert same(r2[0][0], r0[0]) and same(r2[0][1], r0[1]), f"{what}: r of vector 0 against the oracle"


# ---------------------------------------------------------------- the streaming branch
@pytest.mark.gpu
def test_mvm_batch_beyond_the_infinity_cache(hip):
    """8192 x 131072 = 512 MiB: nontemporal loads, 16 chunks of x per row, 8 vectors in one pass; against clm4_mvm on the same buffers"""
    L = hip.lib
    rows, cols, nvec = 8192, 131072, 8
    dA, dsA = hip.alloc(rows * cols // 2), hip.alloc((rows // 64) * (cols // 64) * 4)
    hip.check(L.clv_fill_random_nibbles(dA.ptr, dA.nbytes, 11, 0, None))
    hip.check(L.clv_fill_random_scales(dsA.ptr, dsA.nbytes // 4, 12, 0, None))
    dx = pairs(hip, nvec, cols)
    for j, (q, s) in enumerate(dx):
        hip.check(L.clv_fill_random_nibbles(q.ptr, q.nbytes, 100 + j, 0, None))
        hip.check(L.clv_fill_random_scales(s.ptr, s.nbytes // 4, 200 + j, 0, None))
    one, many = pairs(hip, nvec, rows), pairs(hip, nvec, rows)
    for j in range(nvec):
        hip.check(L.clm4_mvm(dA.ptr, dsA.ptr, rows, cols, dx[j][0].ptr, dx[j][1].ptr, one[j][0].ptr, one[j][1].ptr, None, None))
    with batch_kernel("1"):
        hip.check(L.clm4_mvm_batch(dA.ptr, dsA.ptr, rows, cols, nvec, pa([d[0] for d in dx]), pa([d[1] for d in dx]), pa([d[0] for d in many]),
                                   pa([d[1] for d in many]), None, None))
    hip.sync()
    for j in range(nvec):
        (r1, s1), (r2, s2) = get(one[j], rows), get(many[j], rows)
        assert np.any(r1) and same(r2, r1) and same(s2, s1), j


# ---------------------------------------------------------------- threshold
def clustered(n_pad, seed, all_equal=False):
    """few distinct magnitudes (nibbles x a pool of 4 scales), so that the k-th largest has many ties; all_equal: one magnitude only"""
    rng = np.random.default_rng(seed)
    if all_equal:
        return np.full(n_pad // 2, 0x33, np.uint8), np.ones(n_pad // 64, np.float32)
    q = random_packed(rng, n_pad)[0]
    return q, np.array([0.5, 1.0, 1.0, 2.0], np.float32)[rng.integers(0, 4, size=n_pad // 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [THRESHOLD_FAST, THRESHOLD_REFERENCE])
@pytest.mark.parametrize("n_pad,n", [(128, 128), (384, 384 - 37), (8192 + 128, 8192 + 128), (131072, 131072), (131072 + 128, 131072 + 128)])
def test_threshold_batch_equals_the_single_calls(hip, n_pad, n, mode):
    """n_pad = 131072 is the last size of the one-launch form, 131072 + 128 is forwarded to the single calls (as is REFERENCE mode)"""
    L = hip.lib
    big = n_pad > 131072
    vecs = [clustered(n_pad, n_pad + j, all_equal=(j == 1)) for j in range(9)]
    src = [(hip.to_device(q), hip.to_device(s)) for q, s in vecs]
    for k in ((n // 4,) if big else (0, 1, n // 4, n)):
        for nvec in ((9,) if big else (2, 9)):
            def run(batch):
                w = pairs(hip, nvec, n_pad)
                for (wq, ws), (pq, ps) in zip(w, src):
                    hip.check(L.clv_memcpy_d2d(wq.ptr, pq.ptr, n_pad // 2, None))
                    hip.check(L.clv_memcpy_d2d(ws.ptr, ps.ptr, n_pad // 16, None))
                if batch:
                    hip.check(L.clv4_threshold_batch(pa([d[0] for d in w]), pa([d[1] for d in w]), nvec, n, n_pad, k, mode, None))
                else:
                    for q, s in w:
                        hip.check(L.clv4_threshold_mode(q.ptr, s.ptr, n, n_pad, k, mode, None, None))
                hip.sync()
                return [get(p, n_pad) for p in w]
            one, many = run(False), run(True)
            for j in range(nvec):
                assert same(many[j][0], one[j][0]) and same(many[j][1], vecs[j][1]), (k, nvec, j)
                if 0 < k < n:
                    kept = np.count_nonzero(np.unpackbits(many[j][0][: n // 2]).reshape(-1, 4).any(axis=1))
                    assert kept <= k and (j == 1) <= (kept == k), (k, nvec, j, kept)


# ---------------------------------------------------------------- IHT / GD
def iht_data(hip, oracle, m, n, nvec, seed=5):
    rng = np.random.default_rng(seed + m * 7 + n)
    qP, sP = random_packed(rng, m * n)[0], rng.uniform(0.5, 2.0, size=(m // 64) * (n // 64)).astype(np.float32)
    qT, sT = oracle.m4_transpose(qP, sP, m, n)
    mats = [hip.to_device(v) for v in (qP, sP, qT, sT)]
    ys = [random_packed(rng, m) for _ in range(nvec)]
    return mats, [(hip.to_device(q), hip.to_device(s)) for q, s in ys]


def iht_run(hip, mats, dy, m, n, thr, batch, rng=None, iters=3, stream=None, bufs=None):
    L = hip.lib
    nvec = len(dy)
    lens = dict(x=n, t1=m, t2=m, t3=n)
    v = bufs or {k: pairs(hip, nvec, ln, 0x55) for k, ln in lens.items()}
    x_len, K, mu = n - 5, n // 8, 0.002
    head = [b.ptr for b in mats] + [m, n]
    if batch:
        arrs = {k: (pa([d[0] for d in v[k]]), pa([d[1] for d in v[k]])) for k in v}
        hip.check(L.clm4_iht_batch(*head, nvec, arrs["x"][0], arrs["x"][1], x_len, pa([d[0] for d in dy]), pa([d[1] for d in dy]), arrs["t1"][0],
                                   arrs["t1"][1], arrs["t2"][0], arrs["t2"][1], arrs["t3"][0], arrs["t3"][1], iters, K, mu, thr,
                                   rng.ptr if rng else None, stream))
    else:
        for j in range(nvec):
            hip.check(L.clm4_iht(*head, v["x"][j][0].ptr, v["x"][j][1].ptr, x_len, dy[j][0].ptr, dy[j][1].ptr, v["t1"][j][0].ptr, v["t1"][j][1].ptr,
                                 v["t2"][j][0].ptr, v["t2"][j][1].ptr, v["t3"][j][0].ptr, v["t3"][j][1].ptr, iters, K, mu, thr,
                                 rng.ptr if rng else None, stream))
    return v, lens


def iht_read(v, lens):
    return {k: [get(p, lens[k]) for p in v[k]] for k in v}


def assert_same_vectors(a, b, what=""):
    for k in a:
        for j, (p, q) in enumerate(zip(a[k], b[k])):
            assert same(p[0], q[0]) and same(p[1], q[1]), f"{what} {k} of vector {j}"


@pytest.mark.gpu
@pytest.mark.parametrize("m,n", [(128, 256), (256, 384), (384, 256)])
@pytest.mark.parametrize("nvec", [2, 5, 9])
def test_iht_batch_equals_clm4_iht_per_vector(hip, oracle, m, n, nvec):
    mats, dy = iht_data(hip, oracle, m, n, nvec)
    for thr in (0, 1, 2):
        v1, lens = iht_run(hip, mats, dy, m, n, thr, batch=False)
        hip.sync()
        one = iht_read(v1, lens)
        for force in ("1", None):
            with batch_kernel(force):
                v2, _ = iht_run(hip, mats, dy, m, n, thr, batch=True)
            hip.sync()
            assert_same_vectors(iht_read(v2, lens), one, f"threshold={thr} CLV_MVM_BATCH={force}:")
        assert any(np.any(x[0]) for x in one["x"]), "the loop left every x zero: the comparison shows nothing"


# ---------------------------------------------------------------- with a generator: the sequence of single calls
@pytest.mark.gpu
def test_with_an_rng_the_calls_run_as_the_sequence_of_single_calls(hip, oracle):
    rows, cols, nvec = 128, 256, 3
    S = shape(hip, oracle, rows, cols)
    L = hip.lib
    dx, du = S.dx[:nvec], S.du[:nvec]

    def mvm(batch, st):
        out = pairs(hip, nvec, rows)
        if batch:
            hip.check(L.clm4_mvm_batch(S.dA.ptr, S.dsA.ptr, rows, cols, nvec, pa([d[0] for d in dx]), pa([d[1] for d in dx]), pa([o[0] for o in out]),
                                       pa([o[1] for o in out]), st.ptr, None))
        else:
            for j in range(nvec):
                hip.check(L.clm4_mvm(S.dA.ptr, S.dsA.ptr, rows, cols, dx[j][0].ptr, dx[j][1].ptr, out[j][0].ptr, out[j][1].ptr, st.ptr, None))
        return {"r": out}

    def fused(batch, st):
        t, r = pairs(hip, nvec, rows), pairs(hip, nvec, rows)
        if batch:
            hip.check(L.clm4_mvm_scale_and_add_batch(S.dA.ptr, S.dsA.ptr, rows, cols, nvec, pa([d[0] for d in dx]), pa([d[1] for d in dx]),
                                                     pa([d[0] for d in du]), pa([d[1] for d in du]), 0.37, pa([d[0] for d in t]), pa([d[1] for d in t]),
                                                     pa([d[0] for d in r]), pa([d[1] for d in r]), st.ptr, None))
        else:
            for j in range(nvec):
                hip.check(L.clm4_mvm_scale_and_add(S.dA.ptr, S.dsA.ptr, rows, cols, dx[j][0].ptr, dx[j][1].ptr, du[j][0].ptr, du[j][1].ptr, 0.37,
                                                   t[j][0].ptr, t[j][1].ptr, r[j][0].ptr, r[j][1].ptr, st.ptr, None))
        return {"t": t, "r": r}

    mats, dy = iht_data(hip, oracle, rows, cols, nvec)

    def loop(batch, st):
        return iht_run(hip, mats, dy, rows, cols, 1, batch, rng=st)[0]

    for name, call, ln in (("mvm", mvm, None), ("fused", fused, None), ("iht", loop, dict(x=cols, t1=rows, t2=rows, t3=cols))):
        res = []
        for batch in (False, True):
            st = hip.new_rng(*KEYS)
            v = call(batch, st)
            hip.sync()
            res.append(({k: [get(p, ln[k] if ln else rows) for p in v[k]] for k in v}, hip.rng_get(st)))
        assert_same_vectors(res[1][0], res[0][0], name)
        assert np.array_equal(res[1][1][0], res[0][1][0]) and np.array_equal(res[1][1][1], res[0][1][1]), f"{name}: the XORShift state left behind"
        fresh_keys = hip.rng_get(hip.new_rng(*KEYS))
        assert not np.array_equal(res[1][1][0], fresh_keys[0]), f"{name}: the generator was not used"


# ---------------------------------------------------------------- graph capture
@pytest.mark.gpu
@pytest.mark.parametrize("what", ["clm4_mvm_scale_and_add_batch nvec=5", "clm4_iht_batch nvec=3 FAST"])
def test_the_deterministic_batch_calls_capture_into_a_graph(hip, oracle, what):
    """no pointer table on the device, nothing allocated: captured once (after a warm-up call outside the capture), replayed twice on
    changed inputs, every replay equals the eager call on the same inputs"""
    L = hip.lib
    rt = C.CDLL("libamdhip64.so")
    stream, graph, gexec = C.c_void_p(), C.c_void_p(), C.c_void_p()

    def ok(rc):
        assert rc == 0, f"HIP runtime call failed: {rc}"
    rows, cols = 128, 256
    if what.startswith("clm4_mvm"):
        nvec = 5
        S = shape(hip, oracle, rows, cols)
        dx = pairs(hip, nvec, cols)
        du, t, r = S.du[:nvec], pairs(hip, nvec, rows), pairs(hip, nvec, rows)
        changing = dx

        def enqueue(st, t=t, r=r):
            hip.check(L.clm4_mvm_scale_and_add_batch(S.dA.ptr, S.dsA.ptr, rows, cols, nvec, pa([d[0] for d in dx]), pa([d[1] for d in dx]),
                                                     pa([d[0] for d in du]), pa([d[1] for d in du]), -1.0, pa([d[0] for d in t]), pa([d[1] for d in t]),
                                                     pa([d[0] for d in r]), pa([d[1] for d in r]), None, st))
            return {"t": t, "r": r}
        lens = dict(t=rows, r=rows)

        def eager():
            return enqueue(None, pairs(hip, nvec, rows), pairs(hip, nvec, rows))
    else:
        nvec = 3
        mats, _ = iht_data(hip, oracle, rows, cols, nvec)
        dy = pairs(hip, nvec, rows)
        changing = dy
        lens = dict(x=cols, t1=rows, t2=rows, t3=cols)
        bufs = {k: pairs(hip, nvec, ln, 0x55) for k, ln in lens.items()}

        def enqueue(st):
            return iht_run(hip, mats, dy, rows, cols, 1, True, stream=st, bufs=bufs)[0]

        def eager():
            return iht_run(hip, mats, dy, rows, cols, 1, True)[0]

    def fill(seed):
        for j, (q, s) in enumerate(changing):
            hip.check(L.clv_fill_random_nibbles(q.ptr, q.nbytes, seed + 2 * j, 0, None))
            hip.check(L.clv_fill_random_scales(s.ptr, s.nbytes // 4, seed + 2 * j + 1, 0, None))
        hip.sync()
    with batch_kernel("1"):
        fill(1)
        ok(rt.hipStreamCreate(C.byref(stream)))
        enqueue(stream)                                                     # warm-up outside the capture
        ok(rt.hipStreamSynchronize(stream))
        ok(rt.hipStreamBeginCapture(stream, 0))
        got = enqueue(stream)
        ok(rt.hipStreamEndCapture(stream, C.byref(graph)))
        ok(rt.hipGraphInstantiate(C.byref(gexec), graph, None, None, 0))
        seen = []
        for rep in range(2):
            fill(50 + 10 * rep)
            ok(rt.hipGraphLaunch(gexec, stream))
            ok(rt.hipStreamSynchronize(stream))
            replay = {k: [get(p, lens[k]) for p in got[k]] for k in got}
            want = eager()
            hip.sync()
            assert_same_vectors(replay, {k: [get(p, lens[k]) for p in want[k]] for k in want}, f"replay {rep}:")
            seen.append(replay)
        assert not same(seen[0]["r" if "r" in lens else "t1"][0][0], seen[1]["r" if "r" in lens else "t1"][0][0]), "the replays saw the same inputs"
        ok(rt.hipGraphExecDestroy(gexec))
        ok(rt.hipGraphDestroy(graph))
        ok(rt.hipStreamDestroy(stream))


# ---------------------------------------------------------------- guard bands: the four calls in test_guard_bands' table
GB_ENV = {"CLV_MVM_BATCH": "1"}


def _gb_mvm(rows, cols, nvec, fused=False, with_t=True, in_place=False):
    def build(R):
        orc = R.oracle
        qA, sA = gb.m4(rows * cols + 21, rows, cols)
        regs, want = [("A", "input", qA), ("sA", "input", sA)], {}
        for j in range(nvec):
            qx, sx = gb.v4(cols + 30 + j, cols)
            regs += [(f"x{j}", "input", qx), (f"sx{j}", "input", sx)]
            t = orc.m4_mvm(qA, sA, rows, cols, qx, sx)
            if not fused:
                regs += [(f"r{j}", "output", rows // 2), (f"sr{j}", "output", rows // 16)]
                want.update({f"r{j}": t[0], f"sr{j}": t[1]})
                continue
            qu, su = gb.v4(rows + 50 + j, rows)
            r = orc.v4_scale_and_add(qu, su, *t, -0.5)
            if with_t:
                regs += [(f"t{j}", "output", rows // 2), (f"st{j}", "output", rows // 16)]
                want.update({f"t{j}": t[0], f"st{j}": t[1]})
            if in_place:
                regs += [(f"u{j}", "inout", qu), (f"su{j}", "inout", su)]
                want.update({f"u{j}": r[0], f"su{j}": r[1]})
            else:
                regs += [(f"u{j}", "input", qu), (f"su{j}", "input", su), (f"r{j}", "output", rows // 2), (f"sr{j}", "output", rows // 16)]
                want.update({f"r{j}": r[0], f"sr{j}": r[1]})

        def call(L, p):
            a = lambda name: pa([p[f"{name}{j}"] for j in range(nvec)])  # noqa: E731
            if not fused:
                return L.clm4_mvm_batch(p["A"], p["sA"], rows, cols, nvec, a("x"), a("sx"), a("r"), a("sr"), None, None)
            return L.clm4_mvm_scale_and_add_batch(p["A"], p["sA"], rows, cols, nvec, a("x"), a("sx"), a("u"), a("su"), -0.5, a("t") if with_t else None,
                                                  a("st") if with_t else None, a("u" if in_place else "r"), a("su" if in_place else "sr"), None, None)
        return gb.Case(regs, call, want, env=GB_ENV)
    return build


def _gb_threshold(n_pad, nvec, mode):
    def build(R):
        n, k = n_pad - 37, (n_pad - 37) // 4
        regs, want = [], {}
        for j in range(nvec):
            q, s = gb.threshold_data(4, n_pad, n_pad + 4 + 10 * j)
            regs += [(f"q{j}", "inout", q), (f"s{j}", "input", s)]
            want[f"q{j}"] = gb.threshold_reference(R, 4, q, s, n, k, mode)[0]
        return gb.Case(regs, lambda L, p: L.clv4_threshold_batch(pa([p[f"q{j}"] for j in range(nvec)]), pa([p[f"s{j}"] for j in range(nvec)]), nvec, n,
                                                                 n_pad, k, mode, None), want)
    return build


def _gb_iht(m, n, nvec, thr, iters=3):
    def build(R):
        orc = R.oracle
        x_len, K, mu = n - 5, n // 4, np.float32(0.002)
        qP, sP = gb.m4(m * n + 13, m, n)
        qT, sT = orc.m4_transpose(qP, sP, m, n)
        regs, want = [("Phi", "input", qP), ("sPhi", "input", sP), ("PhiT", "input", qT), ("sPhiT", "input", sT)], {}
        for j in range(nvec):
            y = gb.v4(m + 14 + j, m)
            x = (np.zeros(n // 2, np.uint8), np.ones(n // 64, np.float32))
            t1 = t2 = t3 = None
            for _ in range(iters):
                t1 = orc.m4_mvm(qP, sP, m, n, *x)
                t2 = orc.v4_scale_and_add(*y, *t1, -1.0)
                t3 = orc.m4_mvm(qT, sT, n, m, *t2)
                x = orc.v4_scale_and_add(*x, *t3, float(mu))
                if thr:
                    x = (gb.threshold_reference(R, 4, x[0], x[1], x_len, K, THRESHOLD_REFERENCE if thr == 2 else THRESHOLD_FAST)[0], x[1])
            w = {f"x{j}": x[0], f"sx{j}": x[1], f"t1{j}": t1[0], f"st1{j}": t1[1], f"t2{j}": t2[0], f"st2{j}": t2[1], f"t3{j}": t3[0], f"st3{j}": t3[1]}
            regs += [(f"y{j}", "input", y[0]), (f"sy{j}", "input", y[1])] + [(k, "output", v.nbytes) for k, v in w.items()]
            want.update(w)

        def call(L, p):
            a = lambda name: pa([p[f"{name}{j}"] for j in range(nvec)])  # noqa: E731
            return L.clm4_iht_batch(p["Phi"], p["sPhi"], p["PhiT"], p["sPhiT"], m, n, nvec, a("x"), a("sx"), x_len, a("y"), a("sy"), a("t1"), a("st1"),
                                    a("t2"), a("st2"), a("t3"), a("st3"), iters, K, float(mu), thr, None, None)
        return gb.Case(regs, call, want, env=GB_ENV)
    return build


BATCH_CASES = []
for _r, _c in [(64, 128), (192, 640)]:
    BATCH_CASES.append((f"clm4_mvm_batch {_r}x{_c} nvec=3", _gb_mvm(_r, _c, 3)))
    for _t in (True, False):
        for _ip in (False, True):
            BATCH_CASES.append((f"clm4_mvm_scale_and_add_batch {_r}x{_c} nvec=3 t={_t} in_place={_ip}", _gb_mvm(_r, _c, 3, fused=True, with_t=_t, in_place=_ip)))
BATCH_CASES.append((f"clm4_mvm_batch 64x{CHUNK + 128} nvec=9", _gb_mvm(64, CHUNK + 128, 9)))
for _pad in (128, 384, 131072):
    BATCH_CASES.append((f"clv4_threshold_batch FAST n_pad={_pad} nvec=3", _gb_threshold(_pad, 3, THRESHOLD_FAST)))
BATCH_CASES.append(("clv4_threshold_batch REFERENCE n_pad=384 nvec=3", _gb_threshold(384, 3, THRESHOLD_REFERENCE)))
for _thr in (0, 1, 2):
    BATCH_CASES.append((f"clm4_iht_batch 128x256 nvec=3 threshold={_thr}", _gb_iht(128, 256, 3, _thr)))
for _name, _build in BATCH_CASES:
    if _name not in gb.CASES:                 # the coverage test of test_guard_bands.py reads its table when it runs, after every module is imported
        gb.case(_name)(_build)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, _ in BATCH_CASES])
def test_batch_calls_write_their_outputs_and_nothing_else(hip, refs, name):
    gb.run_case(hip, dict(BATCH_CASES)[name](refs))


@pytest.fixture(scope="module")
def refs(oracle):
    return gb.Refs(oracle, None, None)          # 4-bit cases only: neither the 8-bit nor the half-precision restatement is needed
