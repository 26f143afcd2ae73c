"""Device side of the edge-band tests (test_edge_bands_*.py): the entry points of the three operand pairs by name -- their signatures are
the same per form --, the buffers of one pair at one shape, and one function per form that returns what the call wrote.  Every output
buffer is prefilled with 0x5A; every comparison is on bytes and scale bits (eq)."""
import os

import numpy as np
import pytest

import edge_band_data as D
from edge_band_fixtures import cases, m8, ref  # noqa: F401  (fixtures)
from test_mvm_batch import batch_kernel, pa

KEYS = (4711, 13)
NVECS = (2, 3, 5, 8, 9)                            # NV = 2, 4 and 8 with masked slots, a full group, a remainder group of one
NVECS_RNG = (5, 9)                                 # with a generator the remainder of one runs batched too (NV = 2)


class Abi:
    def __init__(self, pair):
        mvm = {"v4": "clm4_mvm", "mixed": "clm4_mvm_v8", "m8": "clm8_mvm"}[pair]
        iht = {"v4": "clm4_iht", "mixed": "clm4_iht_v8", "m8": "clm8_iht"}[pair]
        self.pair = pair
        self.mvm, self.fused, self.batch, self.fused_batch = mvm, mvm + "_scale_and_add", mvm + "_batch", mvm + "_scale_and_add_batch"
        self.mvm_t, self.fused_t = mvm + "_transposed", mvm + "_transposed_scale_and_add"
        self.batch_t, self.fused_batch_t = mvm + "_transposed_batch", mvm + "_transposed_scale_and_add_batch"
        self.transpose = "clm8_transpose" if pair == "m8" else "clm4_transpose"
        self.scale_and_add = "clv4_scale_and_add" if pair == "v4" else "clv8_scale_and_add"
        self.iht, self.iht_one, self.iht_batch, self.iht_batch_one = iht, iht + "_one_matrix", iht + "_batch", iht + "_batch_one_matrix"
        self.persistent = pair != "m8"               # clm8_iht has no persistent kernel

    def vbytes(self, n):
        return n // 2 if D.VECTOR_BITS[self.pair] == 4 else n

    def mbytes(self, rows, cols):
        return rows * cols // 2 if D.MATRIX_BITS[self.pair] == 4 else rows * cols


def groups(nvec, stochastic=False):
    """batched launches of a forced call: deterministic, a group of ONE vector forwards to the single call; with a generator it does not"""
    return (nvec + 7) // 8 if stochastic else nvec // 8 + (nvec % 8 >= 2)


def eq(a, b):
    return all(np.array_equal(np.ascontiguousarray(p).view(np.uint8), np.ascontiguousarray(q).view(np.uint8)) for p, q in zip(a, b))


def up(hip, v):
    return hip.to_device(np.ascontiguousarray(v[0]).view(np.uint8)), hip.to_device(v[1])


def fresh(hip, abi, count, n):
    """count x (vector bytes, scales), prefilled with 0x5A: a call must write every output itself"""
    out = []
    for _ in range(count):
        q, s = hip.alloc(abi.vbytes(n)), hip.alloc(n // 16)
        hip.check(hip.lib.clv_memset(q.ptr, 0x5A, q.nbytes, None))
        hip.check(hip.lib.clv_memset(s.ptr, 0x5A, s.nbytes, None))
        out.append((q, s))
    return out


def read(abi, p, n):
    return p[0].download(np.uint8, abi.vbytes(n)), p[1].download(np.float32, n // 64)


def copies(hip, abi, src, n):
    """working copies of device vectors (the in-place forms overwrite them)"""
    out = fresh(hip, abi, len(src), n)
    for (wq, ws), (pq, ps) in zip(out, src):
        hip.check(hip.lib.clv_memcpy_d2d(wq.ptr, pq.ptr, abi.vbytes(n), None))
        hip.check(hip.lib.clv_memcpy_d2d(ws.ptr, ps.ptr, n // 16, None))
    return out


def arrays(ps):
    return pa([p[0] for p in ps]), pa([p[1] for p in ps])


class Dev:
    """one pair at one shape on the device: B and the reference's transpose of it, the vectors, the single calls' t per vector"""

    def __init__(self, hip, c):
        self.hip, self.c, self.abi = hip, c, Abi(c.pair)
        self.out, self.in_ = c.out, c.in_
        self.B, self.Bt = up(hip, c.B), up(hip, c.Bt)
        self.x = [up(hip, v) for v in c.x]
        self.x[2] = self.x[0]                                               # the same pointers twice
        self.u = [up(hip, v) for v in c.u]
        t = fresh(hip, self.abi, len(self.x), c.out)
        for x, r in zip(self.x, t):
            self.call_mvm(False, x, r)
        hip.sync()
        self.single = [read(self.abi, r, c.out) for r in t]

    # matrix arguments of a held (B: out x in) or a transposed (B': in x out) call
    def mat(self, transposed):
        return (self.Bt[0].ptr, self.Bt[1].ptr, self.in_, self.out) if transposed else (self.B[0].ptr, self.B[1].ptr, self.out, self.in_)

    def call_mvm(self, transposed, x, r, rng=None):
        fn = getattr(self.hip.lib, self.abi.mvm_t if transposed else self.abi.mvm)
        self.hip.check(fn(*self.mat(transposed), x[0].ptr, x[1].ptr, r[0].ptr, r[1].ptr, rng.ptr if rng else None, None))

    def call_saa(self, u, v, a, r, rng=None):
        fn = getattr(self.hip.lib, self.abi.scale_and_add)
        self.hip.check(fn(u[0].ptr, u[1].ptr, v[0].ptr, v[1].ptr, a, self.out, r[0].ptr, r[1].ptr, rng.ptr if rng else None, None))

    def fused(self, transposed, j, a, with_t=True, in_place=False, rng=None):
        """the single fused call on vector j -> r, t (or None), u afterwards (or None in place)"""
        hip, abi, n = self.hip, self.abi, self.out
        u = copies(hip, abi, [self.u[j]], n)[0]
        t = fresh(hip, abi, 1, n)[0] if with_t else None
        r = u if in_place else fresh(hip, abi, 1, n)[0]
        fn = getattr(hip.lib, abi.fused_t if transposed else abi.fused)
        hip.check(fn(*self.mat(transposed), self.x[j][0].ptr, self.x[j][1].ptr, u[0].ptr, u[1].ptr, a, t[0].ptr if t else None,
                     t[1].ptr if t else None, r[0].ptr, r[1].ptr, rng.ptr if rng else None, None))
        hip.sync()
        return read(abi, r, n), (read(abi, t, n) if t else None), (None if in_place else read(abi, u, n))

    def two_calls(self, transposed, j, a, rng=None):
        """mvm, then scale_and_add, on the device -> r, t"""
        t, r = fresh(self.hip, self.abi, 1, self.out)[0], fresh(self.hip, self.abi, 1, self.out)[0]
        self.call_mvm(transposed, self.x[j], t, rng)
        self.call_saa(self.u[j], t, a, r, rng)
        self.hip.sync()
        return read(self.abi, r, self.out), read(self.abi, t, self.out)

    def batch(self, transposed, nvec, rng=None, force="1"):
        """-> the results per vector, the batched launches the call made"""
        hip, abi = self.hip, self.abi
        out = fresh(hip, abi, nvec, self.out)
        fn = getattr(hip.lib, abi.batch_t if transposed else abi.batch)
        before = hip.lib.clv_mvm_batch_launches()
        with batch_kernel(force):
            hip.check(fn(*self.mat(transposed), nvec, *arrays(self.x[:nvec]), *arrays(out), rng.ptr if rng else None, None))
        hip.sync()
        return [read(abi, o, self.out) for o in out], hip.lib.clv_mvm_batch_launches() - before

    def fused_batch(self, transposed, nvec, a, with_t=True, in_place=False, rng=None, force="1"):
        """-> r, t (or None), u afterwards (or None in place) per vector, the batched launches"""
        hip, abi, n = self.hip, self.abi, self.out
        u = copies(hip, abi, self.u[:nvec], n)
        t = fresh(hip, abi, nvec, n) if with_t else None
        r = u if in_place else fresh(hip, abi, nvec, n)
        fn = getattr(hip.lib, abi.fused_batch_t if transposed else abi.fused_batch)
        ta = arrays(t) if t else (None, None)
        before = hip.lib.clv_mvm_batch_launches()
        with batch_kernel(force):
            hip.check(fn(*self.mat(transposed), nvec, *arrays(self.x[:nvec]), *arrays(u), a, *ta, *arrays(r), rng.ptr if rng else None, None))
        hip.sync()
        return ([read(abi, p, n) for p in r], ([read(abi, p, n) for p in t] if t else None),
                (None if in_place else [read(abi, p, n) for p in u]), hip.lib.clv_mvm_batch_launches() - before)

    def transpose_then_mvm(self, j):
        """clm*_transpose of the matrix under test (B'), then the held-matrix mvm on the result -> t, the transposed matrix' bytes and scales"""
        hip, abi = self.hip, self.abi
        q, s = hip.alloc(abi.mbytes(self.out, self.in_)), hip.alloc((self.out // 64) * (self.in_ // 64) * 4)
        hip.check(getattr(hip.lib, abi.transpose)(self.Bt[0].ptr, self.Bt[1].ptr, self.in_, self.out, q.ptr, s.ptr, None))
        r = fresh(hip, abi, 1, self.out)[0]
        fn = getattr(hip.lib, abi.mvm)
        hip.check(fn(q.ptr, s.ptr, self.out, self.in_, self.x[j][0].ptr, self.x[j][1].ptr, r[0].ptr, r[1].ptr, None, None))
        hip.sync()
        return read(abi, r, self.out), (q.download(np.uint8, q.nbytes), s.download(np.float32, s.nbytes // 4))


@pytest.fixture(scope="module")
def devs(hip, cases):  # noqa: F811
    """devs(pair, out, in_) -> Dev, once per test module"""
    made = {}

    def get(pair, out, in_):
        if (pair, out, in_) not in made:
            made[(pair, out, in_)] = Dev(hip, cases(pair, out, in_))
        return made[(pair, out, in_)]
    return get


def state(hip, st):
    k1, k2 = hip.rng_get(st)
    return np.concatenate([np.asarray(k1, np.uint64), np.asarray(k2, np.uint64)])


def oracle_state(oracle, o):
    return np.concatenate(oracle.rng_keys(o))


# ---------------------------------------------------------------- the loops
class Loop:
    """one pair's IHT / GD problem on the device: Phi, the reference's transpose of it, NVEC_MAX measurements"""

    NAMES = ("x", "t1", "t2", "t3")

    def __init__(self, hip, ref, pair, m, n):
        self.hip, self.abi, self.pair, self.m, self.n = hip, Abi(pair), pair, m, n
        self.host = D.loop_problem(ref, pair, m, n)
        self.Phi, self.PhiT = up(hip, self.host[0]), up(hip, self.host[1])
        self.y = [up(hip, y) for y in self.host[2]]
        self.lens = dict(x=n, t1=m, t2=m, t3=n)

    def bufs(self, nvec):
        return {k: fresh(self.hip, self.abi, nvec, ln) for k, ln in self.lens.items()}

    def get(self, v):
        return {k: [read(self.abi, p, self.lens[k]) for p in v[k]] for k in v}

    def single(self, j, K, thr, one_matrix=False, persistent=None, iterations=D.LOOP_ITERATIONS, mu=D.LOOP_MU):
        """clm*_iht (persistent: CLV_IHT_PERSISTENT = 1 / 0, None = unset) or clm*_iht_one_matrix on measurement j -> the four vectors, the
        persistent launches the call made"""
        hip, L, m, n = self.hip, self.hip.lib, self.m, self.n
        v = self.bufs(1)
        old = os.environ.pop("CLV_IHT_PERSISTENT", None)
        if persistent is not None:
            os.environ["CLV_IHT_PERSISTENT"] = "1" if persistent else "0"
        before = L.clv_iht_persistent_launches()
        try:
            mats = (self.Phi[0].ptr, self.Phi[1].ptr) + (() if one_matrix else (self.PhiT[0].ptr, self.PhiT[1].ptr))
            tail = [p for k in self.NAMES[1:] for p in (v[k][0][0].ptr, v[k][0][1].ptr)]
            fn = getattr(L, self.abi.iht_one if one_matrix else self.abi.iht)
            hip.check(fn(*mats, m, n, v["x"][0][0].ptr, v["x"][0][1].ptr, n, self.y[j][0].ptr, self.y[j][1].ptr, *tail, iterations, K, float(mu), thr,
                         None, None))
            hip.sync()
        finally:
            os.environ.pop("CLV_IHT_PERSISTENT", None)
            if old is not None:
                os.environ["CLV_IHT_PERSISTENT"] = old
        return {k: r[0] for k, r in self.get(v).items()}, L.clv_iht_persistent_launches() - before

    def batched(self, nvec, K, thr, one_matrix=False, force="1", iterations=D.LOOP_ITERATIONS, mu=D.LOOP_MU):
        """clm*_iht_batch or clm*_iht_batch_one_matrix on the first nvec measurements -> the four vectors per measurement, the batched launches"""
        hip, L, m, n = self.hip, self.hip.lib, self.m, self.n
        v = self.bufs(nvec)
        mats = (self.Phi[0].ptr, self.Phi[1].ptr) + (() if one_matrix else (self.PhiT[0].ptr, self.PhiT[1].ptr))
        tail = [p for k in self.NAMES[1:] for p in arrays(v[k])]
        fn = getattr(L, self.abi.iht_batch_one if one_matrix else self.abi.iht_batch)
        before = L.clv_mvm_batch_launches()
        with batch_kernel(force):
            hip.check(fn(*mats, m, n, nvec, *arrays(v["x"]), n, *arrays(self.y[:nvec]), *tail, iterations, K, float(mu), thr, None, None))
        hip.sync()
        return self.get(v), L.clv_mvm_batch_launches() - before


@pytest.fixture(scope="module")
def loops(hip, ref):  # noqa: F811
    """loops(pair, m, n) -> Loop, once per test module"""
    made = {}

    def get(pair, m, n):
        if (pair, m, n) not in made:
            made[(pair, m, n)] = Loop(hip, ref, pair, m, n)
        return made[(pair, m, n)]
    return get
