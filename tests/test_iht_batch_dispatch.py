"""Which groups of clm4_iht_batch, clm4_iht_v8_batch and clm8_iht_batch run batched under the measured rule (CLV_MVM_BATCH unset), read
from clv_mvm_batch_launches(): a batched group adds two launches per iteration, a group forwarded to the single calls adds none.  The
counter tests of the other files force the batched kernel; the rule of the IHT loops is the part that differs per family:

  4-bit         a single clm4_iht with threshold FAST or none at m, n <= 8192 is of the persistent class: only a full group of 8 runs
                batched.  Threshold REFERENCE: every group of two or more.
  mixed (V8)    where a single clm4_iht_v8 takes the persistent kernel (clm4_iht_v8_persistent_eligible) no group runs batched, except
                with a generator the full group of 8.  At 128 x 256 that function says: eligible with threshold FAST and rounding disabled
                (R1 = R2 = 16, 16 workgroups, two groups of blocks either way); not eligible with REFERENCE (threshold > 1) and not with a
                generator ((m + n) / 64 * 4 = 24 draws per iteration, fewer than 32).  The test checks that reading against
                clv_iht_persistent_launches() of the single calls.
  8-bit matrix  no persistent kernel: every group of two or more.

Shape 128 x 256, 2 iterations, K = 16; nvec = 2 (one small group), 8 (one full group), 10 (a full group and one of two).  In every case x
and t1 .. t3 of every vector equal the single calls' bytes; the single calls run once per family, threshold and rounding for ten vectors
(with a generator the first nvec of them are what nvec single calls produce)."""
import numpy as np
import pytest

import test_m8_mvm_batch as t8
import test_mvm_batch as t4
import test_mvm_v8_batch as tv8
from clover_amd.lib_binding import THRESHOLD_FAST, THRESHOLD_REFERENCE  # noqa: F401
from test_mvm_batch import KEYS, assert_same_vectors, batch_kernel, pa

M, N, ITERS, K, MU, X_LEN, NMAX = 128, 256, 2, 16, 0.002, 251, 10
FAST, REFERENCE = 1, 2                                                  # the loops' `threshold` argument
LENS = dict(x=N, t1=M, t2=M, t3=N)


def _m8_data(hip, oracle, m, n, nvec):
    rng = np.random.default_rng(5 + m * 7 + n)
    Phi = [hip.to_device(v) for v in t8.matrix8(rng, m, n)]
    PhiT = [hip.alloc(m * n), hip.alloc((m // 64) * (n // 64) * 4)]
    hip.check(hip.lib.clm8_transpose(Phi[0].ptr, Phi[1].ptr, m, n, PhiT[0].ptr, PhiT[1].ptr, None))
    return Phi + PhiT, [tuple(hip.to_device(v) for v in t8.v8(rng, m)) for _ in range(nvec)]


FAMILIES = {
    "4-bit": dict(batch="clm4_iht_batch", single="clm4_iht", data=t4.iht_data, pairs=t4.pairs, get=t4.get),
    "v8": dict(batch="clm4_iht_v8_batch", single="clm4_iht_v8", data=tv8.iht_data, pairs=tv8.pairs8, get=tv8.get8),
    "8-bit": dict(batch="clm8_iht_batch", single="clm8_iht", data=_m8_data, pairs=t8.pairs8, get=t8.get8),
}
V8_SINGLE_IS_PERSISTENT = {(FAST, False): True, (FAST, True): False, (REFERENCE, False): False, (REFERENCE, True): False}


def batched_groups(family, thr, gen, nvec):
    groups = [8] * (nvec // 8) + ([nvec % 8] if nvec % 8 else [])
    if family == "4-bit":
        return sum(g >= 2 and (thr == REFERENCE or g == 8) for g in groups)
    if family == "v8":
        return sum(g >= 2 and (not V8_SINGLE_IS_PERSISTENT[(thr, gen)] or (gen and g == 8)) for g in groups)
    return sum(g >= 2 for g in groups)


def test_the_expected_counts_are_the_table_of_the_rule():
    """2 iterations x 2 launches per batched group, nvec = 2 / 8 / 10"""
    for gen in (False, True):
        assert [4 * batched_groups("4-bit", FAST, gen, nv) for nv in (2, 8, 10)] == [0, 4, 4]
        assert [4 * batched_groups("4-bit", REFERENCE, gen, nv) for nv in (2, 8, 10)] == [4, 4, 8]
        for thr in (FAST, REFERENCE):
            assert [4 * batched_groups("8-bit", thr, gen, nv) for nv in (2, 8, 10)] == [4, 4, 8]
    assert [4 * batched_groups("v8", FAST, False, nv) for nv in (2, 8, 10)] == [0, 0, 0]
    assert [4 * batched_groups("v8", FAST, True, nv) for nv in (2, 8, 10)] == [4, 4, 8]
    for gen in (False, True):
        assert [4 * batched_groups("v8", REFERENCE, gen, nv) for nv in (2, 8, 10)] == [4, 4, 8]


def _run(hip, F, mats, dy, thr, batch, rng):
    L = hip.lib
    nvec = len(dy)
    v = {k: F["pairs"](hip, nvec, ln, 0x55) for k, ln in LENS.items()}
    head = [b.ptr for b in mats] + [M, N]
    tail = [ITERS, K, MU, thr, rng.ptr if rng else None, None]
    if batch:
        a = {k: (pa([d[0] for d in v[k]]), pa([d[1] for d in v[k]])) for k in v}
        hip.check(getattr(L, F["batch"])(*head, nvec, *a["x"], X_LEN, pa([d[0] for d in dy]), pa([d[1] for d in dy]), *a["t1"], *a["t2"], *a["t3"], *tail))
    else:
        for j in range(nvec):
            hip.check(getattr(L, F["single"])(*head, *[b.ptr for b in v["x"][j]], X_LEN, dy[j][0].ptr, dy[j][1].ptr, *[b.ptr for b in v["t1"][j]],
                                              *[b.ptr for b in v["t2"][j]], *[b.ptr for b in v["t3"][j]], *tail))
    hip.sync()
    return {k: [F["get"](p, LENS[k]) for p in v[k]] for k in v}


_data, _single = {}, {}


def single_calls(hip, oracle, family, thr, gen):
    """the data of a family and what NMAX single calls leave for (thr, gen), once; with it whether those calls took a persistent kernel"""
    F = FAMILIES[family]
    if family not in _data:
        _data[family] = F["data"](hip, oracle, M, N, NMAX)
    mats, dy = _data[family]
    if (family, thr, gen) not in _single:
        before = hip.lib.clv_iht_persistent_launches()
        with batch_kernel(None):
            one = _run(hip, F, mats, dy, thr, False, hip.new_rng(*KEYS) if gen else None)
        _single[(family, thr, gen)] = (one, hip.lib.clv_iht_persistent_launches() - before)
    return (mats, dy) + _single[(family, thr, gen)]


@pytest.mark.gpu
@pytest.mark.parametrize("nvec", [2, 8, 10])
@pytest.mark.parametrize("gen", [False, True], ids=["rounding disabled", "generator"])
@pytest.mark.parametrize("thr", [FAST, REFERENCE], ids=["FAST", "REFERENCE"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_iht_batch_runs_the_groups_batched_that_the_measured_rule_names(hip, oracle, family, thr, gen, nvec):
    mats, dy, one, persistent = single_calls(hip, oracle, family, thr, gen)
    if family == "v8":
        assert (persistent == NMAX) == V8_SINGLE_IS_PERSISTENT[(thr, gen)] and persistent in (0, NMAX), \
            f"clm4_iht_v8 took the persistent kernel {persistent} times in {NMAX} calls: the docstring reads clm4_iht_v8_persistent_eligible otherwise"
    L = hip.lib
    before = L.clv_mvm_batch_launches()
    with batch_kernel(None):
        got = _run(hip, FAMILIES[family], mats, dy[:nvec], thr, True, hip.new_rng(*KEYS) if gen else None)
    launches = L.clv_mvm_batch_launches() - before
    print(f"{family} threshold={thr} generator={gen} nvec={nvec}: {launches} batched launches")
    assert launches == 2 * ITERS * batched_groups(family, thr, gen, nvec)
    assert_same_vectors(got, {k: one[k][:nvec] for k in one}, f"{family} threshold={thr} generator={gen} nvec={nvec}:")
    assert any(np.any(x[0]) for x in one["x"]), "the loop left every x zero: the comparison shows nothing"
