"""The batched transposed mixed mvm (CloverMatrix4 x CloverVector8) on the GPU, rounding disabled: clm4_mvm_v8_transposed_batch and
clm4_mvm_v8_transposed_scale_and_add_batch (k_m4_mvm8_t_batch, clover_amd/csrc/mvm_t8_batch.hip) give, BYTE FOR BYTE, what the CPU gives
(oracle.m4_transpose, oracle.m4_mvm_v8 on the stored transpose, oracle.v8_scale_and_add), what the single device calls clm4_mvm_v8_transposed /
clm4_mvm_v8_transposed_scale_and_add give in order, and what clm4_mvm_v8_batch / clm4_mvm_v8_scale_and_add_batch give on clm4_transpose(A).  Data
and references: mvm_v8_transposed_batch_data.py.

Shapes (rows x cols; C = MVT8B_CHUNK, S = MVT8B_STEP, U = MVT8B_U(NV), W = MVT8B_W read from the sources):
  128 x 128, 256 x 128, 128 x 256, 384 x 640     one round of the walk; non-square both ways (a forgotten transpose, sA[cb][b] read for
                                                  sA[b][cb]); ten column tiles = five workgroups
  S U, 2 S U, S (2 U + 2), 4 S U (x 128)          for the U of every NV: one register set (the tail form of the walk), one and two whole
                                                  rounds, a round and a partial one
  128 x 64 (W + 2), 256 x 64 (2 W + 2)            several workgroups
  C - 128, C, C + 128, 2 C + 128 (x 128)          the x re-staging barriers, the loads in flight across them
  C + 2 S U + 128 x 384                           a multiple of neither C nor the round, three workgroups
nvec: 1 (forwards), 2, 3 and 5 (masked slots of the 4- and 8-vector instantiations), 8, 9 and 17 (a remainder of one), at EVERY shape, plain
and fused, with CLV_MVM_BATCH=1; the small shapes also with the rule unset, the first three also with CLV_MVM_BATCH=0.  The nontemporal
instantiations: test_mvm_v8_transposed_batch_streaming.py."""
import numpy as np
import pytest

from mvm_v8_transposed_batch_data import A_FUSED, CHUNKY, FIRST4, NVECS, SMALL, dev, eq, same
from test_m8_mvm_batch import copies_of, get8, pairs8
from test_mvm_batch import batch_kernel, pa

pytestmark = pytest.mark.gpu

SHAPES = SMALL + CHUNKY
# every shape x nvec on the batched kernel; the small shapes with the measured rule too; the first three also with the kernel forbidden
MVM_CASES = [(r, c, nv, "1") for r, c in SHAPES for nv in NVECS] + [(r, c, nv, None) for r, c in SMALL for nv in NVECS] + \
            [(r, c, nv, "0") for r, c in FIRST4[:3] for nv in NVECS]
FUSED_CASES = MVM_CASES


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
    out = pairs8(hip, nvec, D.cols)
    hip.check(hip.lib.clm4_mvm_v8_transposed_batch(S.dA.ptr, S.dsA.ptr, D.rows, D.cols, nvec, *S.xs(nvec), pa([o[0] for o in out]),
                                                pa([o[1] for o in out]), rng.ptr if rng else None, None))
    hip.sync()
    return [get8(o, D.cols) for o in out]


@pytest.mark.parametrize("rows,cols,nvec,force", MVM_CASES)
def test_the_batch_equals_the_cpu_the_single_calls_and_the_held_batch(hip, oracle, rows, cols, nvec, force):
    S = dev(hip, oracle, rows, cols)
    D = S.D
    before = hip.lib.clv_mvm_batch_launches()
    with batch_kernel(force):
        got = mvm_batch(hip, S, nvec)
    check_counter(hip.lib.clv_mvm_batch_launches() - before, nvec, force)
    for j in range(nvec):
        assert eq(S.single[j], D.t(j)), f"clm4_mvm_v8_transposed itself differs from the CPU, vector {j}"
        assert eq(got[j], D.t(j)), f"vector {j} differs from the CPU"
        assert eq(got[j], S.single[j]), f"vector {j} differs from clm4_mvm_v8_transposed"
        assert eq(got[j], S.held[j]), f"vector {j} differs from clm4_mvm_v8_batch on clm4_transpose(A)"
        assert not np.any(got[j][0][-64:]) and got[j][1][-1] == 1.0, "the zero column group gives a zero block of scale 1"
    assert np.any(got[0][0])
    if nvec >= 2:
        assert not np.any(got[1][0]) and np.all(got[1][1] == 1.0), "the zero vector: zero bytes, scales 1.0"
    if nvec >= 3:
        assert eq(got[2], got[0]), "the same x twice"


def single_fused(hip, S, a):
    """per shape and factor, once: (t, r) per vector of clm4_mvm_v8_transposed_scale_and_add in order, and r of clm4_mvm_v8_scale_and_add_batch on
    clm4_transpose(A)"""
    key = ("fused", a)
    if key not in S.__dict__:
        L, D = hip.lib, S.D
        n = len(S.dx)
        t, r, held = pairs8(hip, n, D.cols), pairs8(hip, n, D.cols), pairs8(hip, n, D.cols)
        for j in range(n):
            hip.check(L.clm4_mvm_v8_transposed_scale_and_add(S.dA.ptr, S.dsA.ptr, D.rows, D.cols, S.dx[j][0].ptr, S.dx[j][1].ptr, S.du[j][0].ptr,
                                                          S.du[j][1].ptr, a, t[j][0].ptr, t[j][1].ptr, r[j][0].ptr, r[j][1].ptr, None, None))
        with batch_kernel("1"):
            hip.check(L.clm4_mvm_v8_scale_and_add_batch(S.dAt[0].ptr, S.dAt[1].ptr, D.cols, D.rows, n, *S.xs(n), pa([d[0] for d in S.du]),
                                                     pa([d[1] for d in S.du]), a, None, None, pa([d[0] for d in held]), pa([d[1] for d in held]),
                                                     None, None))
        hip.sync()
        S.__dict__[key] = ([get8(p, D.cols) for p in t], [get8(p, D.cols) for p in r], [get8(p, D.cols) for p in held])
    return S.__dict__[key]


def fused_batch(hip, S, nvec, a, with_t, in_place, rng=None):
    """-> r, t (or None), u afterwards (or None in place)"""
    L, D = hip.lib, S.D
    u = copies_of(hip, S.du, nvec, D.cols)                               # working copies of u: the in-place form overwrites them
    t = pairs8(hip, nvec, D.cols) if with_t else None
    r = u if in_place else pairs8(hip, nvec, D.cols)
    hip.check(L.clm4_mvm_v8_transposed_scale_and_add_batch(
        S.dA.ptr, S.dsA.ptr, D.rows, D.cols, nvec, *S.xs(nvec), pa([d[0] for d in u]), pa([d[1] for d in u]), a,
        pa([d[0] for d in t]) if t else None, pa([d[1] for d in t]) if t else None, pa([d[0] for d in r]), pa([d[1] for d in r]),
        rng.ptr if rng else None, None))
    hip.sync()
    return [get8(p, D.cols) for p in r], ([get8(p, D.cols) for p in t] if t else None), (None if in_place else [get8(p, D.cols) for p in u])


@pytest.mark.parametrize("rows,cols,nvec,force", FUSED_CASES)
def test_the_fused_batch_equals_the_cpu_the_single_calls_and_the_held_batch(hip, oracle, rows, cols, nvec, force):
    """with and without t, in place and out of place; a = A_FUSED against the CPU, the single calls and the held batch, a = -1 (the IHT
    step's) against the two device references"""
    S = dev(hip, oracle, rows, cols)
    D = S.D
    for a in (A_FUSED, -1.0):
        t1, r1, held = single_fused(hip, S, a)
        for with_t in (True, False):
            for in_place in (False, True):
                before = hip.lib.clv_mvm_batch_launches()
                with batch_kernel(force):
                    r2, t2, u2 = fused_batch(hip, S, nvec, a, with_t, in_place)
                check_counter(hip.lib.clv_mvm_batch_launches() - before, nvec, force)
                what = f"a={a} t={with_t} in_place={in_place}"
                for j in range(nvec):
                    assert eq(r2[j], r1[j]), f"{what}: r of vector {j} against the single call"
                    assert eq(r2[j], held[j]), f"{what}: r of vector {j} against clm4_mvm_v8_scale_and_add_batch on the stored transpose"
                    if a == A_FUSED:
                        assert eq(r2[j], D.r(j)), f"{what}: r of vector {j} against the CPU"
                    if with_t:
                        assert eq(t2[j], t1[j]) and eq(t2[j], D.t(j)), f"{what}: t of vector {j}"
                    if not in_place:
                        assert eq(u2[j], D.u[j]), f"{what}: u of vector {j} was written"
                assert not same(r2[0][0], D.u[0][0])
