"""The batched transposed 4-bit mvm on the GPU, rounding disabled: clm4_mvm_transposed_batch and clm4_mvm_transposed_scale_and_add_batch
(k_m4_mvm_t_batch, clover_amd/csrc/mvm_t4_batch.hip) give, BYTE FOR BYTE, what the CPU gives (oracle.m4_transpose, oracle.m4_mvm on the
stored transpose, oracle.v4_scale_and_add) and what the single device calls clm4_mvm_transposed / clm4_mvm_transposed_scale_and_add give
in order.  Data and references: transposed_batch_data.py.

Shapes (rows x cols; C = MVTB_CHUNK, U = MVTB_U(NV), W = MVT_W read from the sources):
  128 x 128, 256 x 128, 128 x 256, 384 x 640     one step; non-square both ways; three steps and ten column tiles
  128 (U + 1) x 128 for each distinct U           one full group of loads plus a tail
  128 x 64 (W + 2), 256 x 64 (2 W + 2)            a masked last workgroup, more than one workgroup
  C - 128, C, C + 128, 2 C + 128 (x 128)          the x re-staging barriers, the loads in flight across them
  C + 128 (lcm U + 1) x 384                       a multiple of neither C nor any U-step, a masked last workgroup
nvec: 1 (forwards), 2, 3 and 5 (masked slots of the 4- and 8-vector instantiations), 8, 9 and 17 (a remainder of one) at the first four
shapes; 2, 3 and 8 (every instantiation) at the other small ones; 3 and 8 at the chunk shapes.  Every case runs with CLV_MVM_BATCH=1; the
first three shapes also with the rule unset and with CLV_MVM_BATCH=0.  The nontemporal instantiation runs once, at 16384 x 32896."""
import numpy as np
import pytest

from test_mvm_batch import batch_kernel, get, pa, pairs
from transposed_batch_data import A_FUSED, CHUNKY, FIRST4, SMALL, W, dev, eq, same, vector

pytestmark = pytest.mark.gpu

NVECS = (1, 2, 3, 5, 8, 9, 17)
MVM_CASES = [(r, c, nv, "1") for r, c in FIRST4 for nv in NVECS] + [(r, c, nv, "1") for r, c in SMALL[4:] for nv in (2, 3, 8)] + \
            [(r, c, nv, "1") for r, c in CHUNKY for nv in (3, 8)] + [(r, c, nv, f) for r, c in FIRST4[:3] for nv in NVECS for f in (None, "0")]
FUSED_CASES = [(r, c, nv, "1") for r, c in SMALL for nv in (2, 5, 9)] + [(r, c, nv, "1") for r, c in CHUNKY for nv in (3, 8)] + \
              [(r, c, nv, f) for r, c in FIRST4[:3] for nv in (1, 3, 9) for f in (None, "0")]
T = 256 << 20


def groups(nvec):
    """batched launches of a forced deterministic call: a group of ONE vector (nvec = 1, the remainder of 9 and 17) forwards to the single call"""
    return nvec // 8 + (nvec % 8 >= 2)


def check_counter(delta, nvec, force):
    if force == "1":
        assert delta == groups(nvec), "forced: one batched launch per group"
    elif force == "0":
        assert delta == 0, "forbidden: every group forwards"
    else:
        assert delta in (0, groups(nvec)), "the rule: whole groups, batched or forwarded"


def mvm_batch(hip, S, nvec, rng=None):
    D = S.D
    out = pairs(hip, nvec, D.cols)
    hip.check(hip.lib.clm4_mvm_transposed_batch(S.dA.ptr, S.dsA.ptr, D.rows, D.cols, nvec, pa([d[0] for d in S.dx[:nvec]]),
                                                pa([d[1] for d in S.dx[:nvec]]), pa([o[0] for o in out]), pa([o[1] for o in out]),
                                                rng.ptr if rng else None, None))
    hip.sync()
    return [get(o, D.cols) for o in out]


@pytest.mark.parametrize("rows,cols,nvec,force", MVM_CASES)
def test_the_batch_equals_the_oracle_and_the_single_calls(hip, oracle, rows, cols, nvec, force):
    S = dev(hip, oracle, rows, cols)
    D = S.D
    before = hip.lib.clv_mvm_batch_launches()
    with batch_kernel(force):
        got = mvm_batch(hip, S, nvec)
    check_counter(hip.lib.clv_mvm_batch_launches() - before, nvec, force)
    for j in range(nvec):
        assert eq(S.single[j], D.t(j)), f"clm4_mvm_transposed itself differs from the oracle, vector {j}"
        assert eq(got[j], D.t(j)), f"vector {j} differs from the oracle"
        assert eq(got[j], S.single[j]), f"vector {j} differs from clm4_mvm_transposed"
        assert not np.any(got[j][0][-32:]) and got[j][1][-1] == 1.0, "the zero column group gives a zero block of scale 1"
    assert np.any(got[0][0])
    if nvec >= 2:
        assert not np.any(got[1][0]) and np.all(got[1][1] == 1.0), "the zero vector: zero nibbles, scales 1.0"
    if nvec >= 3:
        assert eq(got[2], got[0]), "the same x twice"


def single_fused(hip, S, a):
    """clm4_mvm_transposed_scale_and_add per vector, once per shape and factor: (t, r) per vector"""
    key = ("fused", a)
    if key not in S.__dict__:
        L, D = hip.lib, S.D
        n = len(S.dx)
        t, r = pairs(hip, n, D.cols), pairs(hip, n, D.cols)
        for j in range(n):
            hip.check(L.clm4_mvm_transposed_scale_and_add(S.dA.ptr, S.dsA.ptr, D.rows, D.cols, S.dx[j][0].ptr, S.dx[j][1].ptr, S.du[j][0].ptr,
                                                          S.du[j][1].ptr, a, t[j][0].ptr, t[j][1].ptr, r[j][0].ptr, r[j][1].ptr, None, None))
        hip.sync()
        S.__dict__[key] = ([get(p, D.cols) for p in t], [get(p, D.cols) for p in r])
    return S.__dict__[key]


def fused_batch(hip, S, nvec, a, with_t, in_place, rng=None):
    """-> r, t (or None), u afterwards (or None in place)"""
    L, D = hip.lib, S.D
    u = pairs(hip, nvec, D.cols)                                         # working copies of u: the in-place form overwrites them
    for (wq, ws), (pq, ps) in zip(u, S.du):
        hip.check(L.clv_memcpy_d2d(wq.ptr, pq.ptr, D.cols // 2, None))
        hip.check(L.clv_memcpy_d2d(ws.ptr, ps.ptr, D.cols // 16, None))
    t = pairs(hip, nvec, D.cols) if with_t else None
    r = u if in_place else pairs(hip, nvec, D.cols)
    dx = S.dx[:nvec]
    hip.check(L.clm4_mvm_transposed_scale_and_add_batch(
        S.dA.ptr, S.dsA.ptr, D.rows, D.cols, nvec, pa([d[0] for d in dx]), pa([d[1] for d in dx]), pa([d[0] for d in u]), pa([d[1] for d in u]), a,
        pa([d[0] for d in t]) if t else None, pa([d[1] for d in t]) if t else None, pa([d[0] for d in r]), pa([d[1] for d in r]),
        rng.ptr if rng else None, None))
    hip.sync()
    return [get(p, D.cols) for p in r], ([get(p, D.cols) for p in t] if t else None), (None if in_place else [get(p, D.cols) for p in u])


@pytest.mark.parametrize("rows,cols,nvec,force", FUSED_CASES)
def test_the_fused_batch_equals_the_oracle_and_the_single_calls(hip, oracle, rows, cols, nvec, force):
    """with and without t, in place and out of place; a = A_FUSED against the oracle and the single calls, a = -1 (the IHT step's) against
    the single calls"""
    S = dev(hip, oracle, rows, cols)
    D = S.D
    for a in (A_FUSED, -1.0):
        t1, r1 = single_fused(hip, S, a)
        for with_t in (True, False):
            for in_place in (False, True):
                before = hip.lib.clv_mvm_batch_launches()
                with batch_kernel(force):
                    r2, t2, u2 = fused_batch(hip, S, nvec, a, with_t, in_place)
                check_counter(hip.lib.clv_mvm_batch_launches() - before, nvec, force)
                what = f"a={a} t={with_t} in_place={in_place}"
                for j in range(nvec):
                    assert eq(r2[j], r1[j]), f"{what}: r of vector {j} against the single call"
                    if a == A_FUSED:
                        assert eq(r2[j], D.r(j)), f"{what}: r of vector {j} against the oracle"
                    if with_t:
                        assert eq(t2[j], t1[j]) and eq(t2[j], D.t(j)), f"{what}: t of vector {j}"
                    if not in_place:
                        assert eq(u2[j], D.u[j]), f"{what}: u of vector {j} was written"
                assert not same(r2[0][0], D.u[0][0])


def test_the_nontemporal_instantiation(hip, oracle):
    """k_m4_mvm_t_batch<4, ., true, FUSE, false> at 16384 x 32896, one byte row more than the 256 MiB Infinity Cache holds, 514 output
    blocks (the last workgroup half masked), three vectors, plain and fused.  The STORED TRANSPOSE is drawn on the host, so the reference
    is the oracle's mvm on it; the matrix under test is clm4_transpose of it"""
    L = hip.lib
    rows, cols, nvec = 16384, 32896, 3
    assert rows * (cols // 2) > T and (cols // 64) % W
    rng = np.random.default_rng(rows + cols + 3)
    qt = np.frombuffer(rng.bytes(rows * cols // 2), np.uint8).copy()
    qt[(qt >> 4) == 8] ^= 0x80                                              # nibbles in [-7, 7], as a quantiser leaves them
    qt[(qt & 0xF) == 8] ^= 0x08
    At = (qt, rng.uniform(0.5, 2.0, size=(rows // 64) * (cols // 64)).astype(np.float32))
    dA, dsA = hip.alloc(rows * cols // 2), hip.alloc((rows // 64) * (cols // 64) * 4)
    dAt = [hip.to_device(v) for v in At]
    hip.check(L.clm4_transpose(dAt[0].ptr, dAt[1].ptr, cols, rows, dA.ptr, dsA.ptr, None))
    hip.sync()
    del dAt
    xs, us = [vector(rng, rows, zero_block=j) for j in range(nvec)], [vector(rng, cols) for _ in range(nvec)]
    want_t = [oracle.m4_mvm(*At, cols, rows, *x) for x in xs]
    before = L.clv_mvm_batch_launches()
    with batch_kernel("1"):
        got = hip.m4_mvm_transposed_batch(dA, dsA, rows, cols, xs)
        fused = hip.m4_mvm_transposed_scale_and_add_batch(dA, dsA, rows, cols, xs, us, A_FUSED)
    assert L.clv_mvm_batch_launches() - before == 2
    for j in range(nvec):
        assert eq(got[j], want_t[j]), f"plain, vector {j}"
        assert eq(fused[j][0:2], want_t[j]) and eq(fused[j][2:4], oracle.v4_scale_and_add(*us[j], *want_t[j], A_FUSED)), f"fused, vector {j}"
        assert eq(hip.m4_mvm_transposed(dA, dsA, rows, cols, *xs[j]), got[j]), f"the single call, vector {j}"
    assert np.any(want_t[0][0]) and not eq(want_t[0], want_t[1])
