"""Every fused, batched and transposed mvm form of the three operand pairs on the band grid of edge_band_data.py: output blocks that are
exactly zero (scale 1.0 from fix_zero_max), blocks whose maximum makes 7 / max or 127 / max infinite (every element 0, the subnormal
maximum as the scale), blocks with k within 8 x of FLT_MAX, scales above 1e30, tiles 2^40 and 2^160 apart in one sum, denormal block
factors; in the fused forms div7 / div127 of whatever scale the mvm produced, times a.  Rounding disabled here; with a generator:
test_edge_bands_rng.py.

The reference is the composition of the pinned single operations (edge_band_data.Ref); test_edge_band_data_cpu.py asserts on it alone that
every band has its category and that no block is non-finite, so nothing is left out here: every output byte and every scale bit is
compared, no tolerance.  The batched calls run with CLV_MVM_BATCH=1 and the launch counter says that the batched kernel ran."""
import numpy as np
import pytest

import edge_band_data as D
from edge_band_gpu import NVECS, cases, devs, eq, fresh, groups, m8, read, ref  # noqa: F401  (cases, devs, m8, ref: fixtures)

pytestmark = pytest.mark.gpu

CASES = [(pair, out, in_) for pair in D.PAIRS for out, in_ in D.shapes_of(pair)]
FORMS = [(with_t, in_place) for with_t in (True, False) for in_place in (False, True)]


def test_the_single_mvm_itself_equals_the_reference(devs):  # noqa: F811
    """what decides between a form and the reference below: the single calls, which the reference fixtures pin on the reference's own code"""
    for pair, out, in_ in CASES:
        S = devs(pair, out, in_)
        for j in range(D.NVEC_MAX):
            assert eq(S.single[j], S.c.t(j)), f"{S.abi.mvm} {out} x {in_}, vector {j}"


@pytest.mark.parametrize("transposed", [False, True], ids=["held", "transposed"])
@pytest.mark.parametrize("pair,out,in_", CASES)
def test_the_single_fused_call(devs, pair, out, in_, transposed):  # noqa: F811
    """*_mvm_scale_and_add and *_mvm_transposed_scale_and_add: t stored and not, in place and not, against the reference and against mvm
    followed by scale_and_add on the device; x itself and x with its kinds rotated by one"""
    S = devs(pair, out, in_)
    c = S.c
    for j in (0, 3):
        for a in D.A_VALUES:
            r2, t2 = S.two_calls(transposed, j, a)
            assert eq(t2, c.t(j)) and eq(r2, c.r(j, a)), f"the two single calls differ from the reference: vector {j}, a={a}"
            for with_t, in_place in FORMS:
                what = f"vector {j} a={a} t={with_t} in_place={in_place}"
                r, t, u = S.fused(transposed, j, a, with_t, in_place)
                assert eq(r, c.r(j, a)), f"{what}: r against the reference"
                assert eq(r, r2), f"{what}: r against mvm + scale_and_add on the device"
                if with_t:
                    assert eq(t, c.t(j)) and eq(t, t2), f"{what}: t"
                if not in_place:
                    assert eq(u, c.u[j]), f"{what}: u was written"


@pytest.mark.parametrize("transposed", [False, True], ids=["held", "transposed"])
@pytest.mark.parametrize("pair,out,in_", CASES)
def test_the_batched_mvm(devs, pair, out, in_, transposed):  # noqa: F811
    """*_mvm_batch and *_mvm_transposed_batch: x, a zero vector, x again (the same pointers), x rotated by 1, 2, ...: different vectors of
    one launch meet different categories in the same block"""
    S = devs(pair, out, in_)
    for nvec in NVECS:
        got, launches = S.batch(transposed, nvec)
        assert launches == groups(nvec), f"nvec={nvec}: forced, one batched launch per group of two or more"
        for j in range(nvec):
            assert eq(got[j], S.c.t(j)), f"nvec={nvec}: vector {j} against the reference"
            assert eq(got[j], S.single[j]), f"nvec={nvec}: vector {j} against the single call"
        assert not np.any(got[1][0]) and np.all(got[1][1] == 1.0), "the zero vector: zero elements, scales 1.0"
        if nvec >= 3:
            assert eq(got[2], got[0]), "the same x twice"
    assert S.batch(transposed, 9, force="0")[1] == 0, "CLV_MVM_BATCH=0: every group forwards"


@pytest.mark.parametrize("transposed", [False, True], ids=["held", "transposed"])
@pytest.mark.parametrize("pair,out,in_", CASES)
def test_the_fused_batch(devs, pair, out, in_, transposed):  # noqa: F811
    """*_mvm_scale_and_add_batch and *_mvm_transposed_scale_and_add_batch, a = -1, 0.37, 2.5: every form at 3 and 9 vectors, one form
    per a at 2, 5 and 8"""
    S = devs(pair, out, in_)
    c = S.c
    for nvec in NVECS:
        for ai, a in enumerate(D.A_VALUES):
            for with_t, in_place in (FORMS if nvec in (3, 9) else [FORMS[(ai + nvec) % 4]]):
                what = f"nvec={nvec} a={a} t={with_t} in_place={in_place}"
                r, t, u, launches = S.fused_batch(transposed, nvec, a, with_t, in_place)
                assert launches == groups(nvec), f"{what}: forced, one batched launch per group of two or more"
                for j in range(nvec):
                    assert eq(r[j], c.r(j, a)), f"{what}: r of vector {j} against the reference"
                    if with_t:
                        assert eq(t[j], c.t(j)) and eq(t[j], S.single[j]), f"{what}: t of vector {j}"
                    if not in_place:
                        assert eq(u[j], c.u[j]), f"{what}: u of vector {j} was written"
    # against the single fused calls on the device, in order
    for j in range(9):
        r1, t1, _ = S.fused(transposed, j, 0.37)
        assert eq(r1, c.r(j, 0.37)) and eq(t1, c.t(j)), f"the single fused call, vector {j}"


@pytest.mark.parametrize("pair,out,in_", CASES)
def test_the_transposed_mvm(hip, devs, pair, out, in_):  # noqa: F811
    """*_mvm_transposed on the transpose of B: against the reference on B, against the held-matrix call on B, and against *_transpose
    followed by *_mvm on the device"""
    S = devs(pair, out, in_)
    t = [None] * D.NVEC_MAX
    outs = fresh(hip, S.abi, D.NVEC_MAX, out)
    for j in range(D.NVEC_MAX):
        S.call_mvm(True, S.x[j], outs[j])
    hip.sync()
    for j in range(D.NVEC_MAX):
        t[j] = read(S.abi, outs[j], out)
        assert eq(t[j], S.c.t(j)), f"vector {j} against the reference"
        assert eq(t[j], S.single[j]), f"vector {j} against the held-matrix call"
    for j in (0, 3):
        t2, B2 = S.transpose_then_mvm(j)
        assert eq(B2, S.c.B), "transposing the matrix under test on the device gives B back"
        assert eq(t[j], t2), f"vector {j} against transpose + mvm on the device"
