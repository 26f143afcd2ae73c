"""k_m4_mvm_batch<NV, U, NT, FUSE> (clover_amd/csrc/mvm_batch4.hip) at every group width, with both of its column loops running.

A group of g vectors runs as NV = 2 (g <= 2), 4 (g <= 4) or 8, with U = 8 matrix loads in flight for NV <= 4 and U = 4 for NV = 8; vector
v's epilogue runs on wave v & 3 and, fused, reads its own register of u.  Here g = 2 .. 8, each a single group, at
  (128, 1408)               11 column pairs: one unrolled round of U = 8 (two of U = 4) and three single steps; two row groups
  (128, MVMB_CHUNK + 1408)  the same behind a full chunk: x is staged twice
for the plain and the fused call (t given or not, in place or not, a = -1 and 0.37), EVERY vector against the CPU oracle -- the mvm and
the scaleAndAdd on top of it -- and against the single calls; every vector has its own u, so a result taken from or written to another
vector's slot shows.  The loop call clm4_iht_batch runs groups of 3, 4, 6 and 7 at 1152 x 1408 (9 and 11 column pairs: the unrolled loop
runs in both directions) against clm4_iht per vector.  The nontemporal instantiations (a matrix of 512 MiB) run as groups of 2, 3 and 8,
plain and fused, against the single calls on the same buffers.  CLV_MVM_BATCH=1 throughout: the batched kernel whatever the rule says."""
import numpy as np
import pytest

from test_mvm_batch import CHUNK, assert_same_vectors, batch_kernel, get, iht_data, iht_read, iht_run, pa, pairs, same, shape

ROWS = 128
COLS = [1408, CHUNK + 1408]
NVECS = [2, 3, 4, 5, 6, 7, 8]


def test_the_shapes_run_the_unrolled_loop_and_its_tail():
    for cols in COLS + [1152]:
        npairs = (cols % CHUNK or CHUNK) // 128                # of the last chunk; a full chunk is a multiple of both U
        assert cols % 64 == 0 and npairs >= 8 and npairs % 4 and npairs % 8, cols
    assert (CHUNK // 128) % 8 == 0 and COLS[1] > CHUNK


# ---------------------------------------------------------------- mvm
@pytest.mark.gpu
@pytest.mark.parametrize("nvec", NVECS)
@pytest.mark.parametrize("cols", COLS)
def test_mvm_batch_every_group_width(hip, oracle, cols, nvec):
    S = shape(hip, oracle, ROWS, cols)
    out = pairs(hip, nvec, ROWS)
    with batch_kernel("1"):
        hip.check(hip.lib.clm4_mvm_batch(S.dA.ptr, S.dsA.ptr, ROWS, cols, nvec, pa([d[0] for d in S.dx[:nvec]]), pa([d[1] for d in S.dx[:nvec]]),
                                         pa([o[0] for o in out]), pa([o[1] for o in out]), None, None))
    hip.sync()
    for j in range(nvec):
        r, sr = get(out[j], ROWS)
        assert same(r, S.oracle[j][0]) and same(sr, S.oracle[j][1]), f"vector {j} differs from the oracle"
        assert same(r, S.single[j][0]) and same(sr, S.single[j][1]), f"vector {j} differs from clm4_mvm"
    assert np.any(S.oracle[0][0]) and (nvec < 4 or not same(S.oracle[0][0], S.oracle[3][0])), "the results are non-zero and differ between vectors"


# ---------------------------------------------------------------- the fused form
_fused_oracle = {}


def fused_oracle(oracle, S, j, a):
    key = (S.rows, S.cols, j, a)
    if key not in _fused_oracle:
        _fused_oracle[key] = oracle.v4_scale_and_add(*S.u[j], *S.oracle[j], a)
    return _fused_oracle[key]


def fused_run(hip, S, nvec, a, with_t, in_place, batch):
    """(r, t or None, u after an out-of-place call or None) per vector, of the batch call or of the single calls"""
    L = hip.lib
    rows, cols = S.rows, S.cols
    u = pairs(hip, nvec, rows)                                             # working copies of u: the in-place form overwrites them
    for (wq, ws), (pq, ps) in zip(u, S.du):
        hip.check(L.clv_memcpy_d2d(wq.ptr, pq.ptr, rows // 2, None))
        hip.check(L.clv_memcpy_d2d(ws.ptr, ps.ptr, rows // 16, None))
    t = pairs(hip, nvec, rows) if with_t else None
    r = u if in_place else pairs(hip, nvec, rows)
    dx = S.dx[:nvec]
    if batch:
        with batch_kernel("1"):
            hip.check(L.clm4_mvm_scale_and_add_batch(
                S.dA.ptr, S.dsA.ptr, rows, cols, nvec, pa([d[0] for d in dx]), pa([d[1] for d in dx]), pa([d[0] for d in u]), pa([d[1] for d in u]), a,
                pa([d[0] for d in t]) if t else None, pa([d[1] for d in t]) if t else None, pa([d[0] for d in r]), pa([d[1] for d in r]), None, None))
    else:
        for j in range(nvec):
            hip.check(L.clm4_mvm_scale_and_add(S.dA.ptr, S.dsA.ptr, rows, cols, dx[j][0].ptr, dx[j][1].ptr, u[j][0].ptr, u[j][1].ptr, a,
                                               t[j][0].ptr if t else None, t[j][1].ptr if t else None, r[j][0].ptr, r[j][1].ptr, None, None))
    hip.sync()
    return [get(p, rows) for p in r], ([get(p, rows) for p in t] if t else None), (None if in_place else [get(p, rows) for p in u])


@pytest.mark.gpu
@pytest.mark.parametrize("nvec", NVECS)
@pytest.mark.parametrize("cols", COLS)
def test_fused_batch_every_group_width(hip, oracle, cols, nvec):
    S = shape(hip, oracle, ROWS, cols)
    assert len({S.u[j][0].tobytes() for j in range(nvec)}) == nvec, "every vector has its own u"
    for a in (-1.0, 0.37):
        for with_t in (True, False):
            for in_place in (False, True):
                what = f"a={a} t={with_t} in_place={in_place}"
                r1, t1, _ = fused_run(hip, S, nvec, a, with_t, in_place, batch=False)
                r2, t2, u2 = fused_run(hip, S, nvec, a, with_t, in_place, batch=True)
                for j in range(nvec):
                    want = fused_oracle(oracle, S, j, a)
                    assert same(r2[j][0], want[0]) and same(r2[j][1], want[1]), f"{what}: r of vector {j} against the oracle"
                    assert same(r2[j][0], r1[j][0]) and same(r2[j][1], r1[j][1]), f"{what}: r of vector {j} against the single call"
                    if with_t:
                        assert same(t2[j][0], S.oracle[j][0]) and same(t2[j][1], S.oracle[j][1]), f"{what}: t of vector {j} against the oracle"
                        assert same(t2[j][0], t1[j][0]) and same(t2[j][1], t1[j][1]), f"{what}: t of vector {j} against the single call"
                    if not in_place:
                        assert same(u2[j][0], S.u[j][0]) and same(u2[j][1], S.u[j][1]), f"{what}: u of vector {j} was written"


# ---------------------------------------------------------------- IHT / GD
@pytest.mark.gpu
@pytest.mark.parametrize("nvec", [3, 4, 6, 7])
def test_iht_batch_groups_with_the_unrolled_loop(hip, oracle, nvec):
    m, n = 1152, 1408
    mats, dy = iht_data(hip, oracle, m, n, nvec)
    for thr in (0, 1, 2):
        v1, lens = iht_run(hip, mats, dy, m, n, thr, batch=False)
        hip.sync()
        one = iht_read(v1, lens)
        with batch_kernel("1"):
            v2, _ = iht_run(hip, mats, dy, m, n, thr, batch=True)
        hip.sync()
        assert_same_vectors(iht_read(v2, lens), one, f"nvec={nvec} threshold={thr}:")
        assert any(np.any(x[0]) for x in one["x"]), "the loop left every x zero: the comparison shows nothing"
        assert not same(one["x"][0][0], one["x"][1][0]), "the vectors' iterates differ from each other"


# ---------------------------------------------------------------- the streaming branch
@pytest.mark.gpu
def test_streaming_batch_groups_plain_and_fused(hip):
    """8192 x 131072 = 512 MiB, beyond the 256 MiB rule: k_m4_mvm_batch<2 | 4 | 8, ., true, false | true>.  One matrix, filled on the
    device once; groups of 2, 3 and 8 against clm4_mvm / clm4_mvm_scale_and_add on the same buffers"""
    L = hip.lib
    rows, cols, nmax, a = 8192, 131072, 8, 0.37
    dA, dsA = hip.alloc(rows * cols // 2), hip.alloc((rows // 64) * (cols // 64) * 4)
    hip.check(L.clv_fill_random_nibbles(dA.ptr, dA.nbytes, 21, 0, None))
    hip.check(L.clv_fill_random_scales(dsA.ptr, dsA.nbytes // 4, 22, 0, None))
    dx, du = pairs(hip, nmax, cols), pairs(hip, nmax, rows)
    for j in range(nmax):
        for (q, s), seed in ((dx[j], 300 + j), (du[j], 500 + j)):
            hip.check(L.clv_fill_random_nibbles(q.ptr, q.nbytes, seed, 0, None))
            hip.check(L.clv_fill_random_scales(s.ptr, s.nbytes // 4, seed + 100, 0, None))
    t1, r1 = pairs(hip, nmax, rows), pairs(hip, nmax, rows)
    for j in range(nmax):
        hip.check(L.clm4_mvm_scale_and_add(dA.ptr, dsA.ptr, rows, cols, dx[j][0].ptr, dx[j][1].ptr, du[j][0].ptr, du[j][1].ptr, a, t1[j][0].ptr,
                                           t1[j][1].ptr, r1[j][0].ptr, r1[j][1].ptr, None, None))
    m1 = pairs(hip, nmax, rows)
    for j in range(nmax):
        hip.check(L.clm4_mvm(dA.ptr, dsA.ptr, rows, cols, dx[j][0].ptr, dx[j][1].ptr, m1[j][0].ptr, m1[j][1].ptr, None, None))
    hip.sync()
    t1, r1, m1 = ([get(p, rows) for p in v] for v in (t1, r1, m1))
    for j in range(nmax):
        assert np.any(m1[j][0]) and np.any(r1[j][0]), j
        assert same(t1[j][0], m1[j][0]) and same(t1[j][1], m1[j][1]), j
        assert j == 0 or not same(m1[j][0], m1[0][0]), j
    for g in (2, 3, 8):
        m2, t2, r2 = pairs(hip, g, rows), pairs(hip, g, rows), pairs(hip, g, rows)
        x, sx = pa([d[0] for d in dx[:g]]), pa([d[1] for d in dx[:g]])
        with batch_kernel("1"):
            hip.check(L.clm4_mvm_batch(dA.ptr, dsA.ptr, rows, cols, g, x, sx, pa([d[0] for d in m2]), pa([d[1] for d in m2]), None, None))
            hip.check(L.clm4_mvm_scale_and_add_batch(dA.ptr, dsA.ptr, rows, cols, g, x, sx, pa([d[0] for d in du[:g]]), pa([d[1] for d in du[:g]]), a,
                                                     pa([d[0] for d in t2]), pa([d[1] for d in t2]), pa([d[0] for d in r2]), pa([d[1] for d in r2]),
                                                     None, None))
        hip.sync()
        for j in range(g):
            for name, got, want in (("mvm", m2, m1), ("t", t2, t1), ("r", r2, r1)):
                q, s = get(got[j], rows)
                assert same(q, want[j][0]) and same(s, want[j][1]), (g, name, j)
