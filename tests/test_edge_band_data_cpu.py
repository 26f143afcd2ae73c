"""The band grid of edge_band_data.py on the REFERENCE alone (oracle.m4_mvm / m4_mvm_v8, the CloverMatrix8 restatement, v4_ / v8_scale_and_add):
every band's output block has the property the module's table promises, for every pair, shape and vector of a batch; no block of the
reference is non-finite in dot or scale -- the GPU tests (test_edge_bands_*.py) compare every byte and leave no block out; the fused
results contain a block with k = inf and one of scale above 1e30; the E seeds on record are the ones the search finds; the loops stay
finite and their iterates contain a block of category Z and one of category T once x is no longer zero."""
import numpy as np
import pytest

import edge_band_data as D
from edge_band_fixtures import cases, m8, ref  # noqa: F401  (fixtures)

CASES = [(pair, out, in_) for pair in D.PAIRS for out, in_ in D.shapes_of(pair)]


def blocks(pair, v):
    return D.elements(D.VECTOR_BITS[pair], v[0]).reshape(-1, 64)


@pytest.mark.parametrize("pair,out,in_", CASES)
def test_the_recorded_e_seeds_are_the_ones_the_search_finds(ref, cases, pair, out, in_):  # noqa: F811
    x = D.x_vector(pair, in_)
    rows = [i for i in range(out // 64) if D.BANDS[i % 8] == "E"]
    assert rows and sorted(k[3] for k in D.E_SEEDS if k[:3] == (pair, out, in_)) == rows
    for i in rows:
        assert D.find_e_seed(ref, pair, out, in_, i, x) == D.E_SEEDS[(pair, out, in_, i)]


@pytest.mark.parametrize("pair,out,in_", CASES)
def test_the_operands_are_what_the_table_says(ref, cases, pair, out, in_):  # noqa: F811
    c = cases(pair, out, in_)
    mb, vb = D.MATRIX_BITS[pair], D.VECTOR_BITS[pair]
    B = D.elements(mb, c.B[0].reshape(out, -1)).reshape(out // 64, 64, in_ // 64, 64)
    sB = c.B[1].reshape(out // 64, in_ // 64)
    assert np.isfinite(sB).all() and (sB > 0).all() and np.abs(B).max() == D.STEPS[mb]
    x, sx = blocks(pair, c.x[0]), c.x[0][1]
    assert np.isfinite(sx).all() and (sx > 0).all()
    for b in range(in_ // 64):
        kind = D.X_KINDS[b % 6]
        assert (kind == "zero") == (not x[b].any()), b
        assert {"ord": 0.5 <= sx[b] < 2, "zero": sx[b] == 1.0, "small": sx[b] < 2.0 ** -18, "big": sx[b] >= 2.0 ** 19,
                "sub": 0 < sx[b] < D.FLT_MIN}[kind], (b, kind, sx[b])
        if vb == 8 and kind != "zero":
            assert np.array_equal(x[b][:8], D.CARRY), "the carry image of the int8 split"
    assert not np.any(c.x[1][0]) and np.all(c.x[1][1] == 1.0) and c.x[2] is c.x[0]
    assert [D.X_KINDS[(b + 1) % 6] == "zero" for b in range(in_ // 64)] == [not blk.any() for blk in blocks(pair, c.x[3])], "x rotated by one"
    for i in range(out // 64):
        kind = D.BANDS[i % 8]
        zero_tiles = [not B[i, :, j].any() for j in range(in_ // 64)]
        facing = [D.X_KINDS[j % 6] for j in range(in_ // 64)]
        if kind in ("N", "N2"):
            assert sB[i].max() / sB[i].min() > 2.0 ** 40 and not any(zero_tiles)
        elif kind == "Z":
            assert all(zero_tiles) and np.all(sB[i] == 1.0)
        elif kind == "Zx":
            assert zero_tiles == [f != "zero" for f in facing] and not all(zero_tiles)
        elif kind == "T":
            assert zero_tiles == [f == "big" for f in facing] and np.all(sB[i] < D.FLT_MIN)
        elif kind == "H":
            assert np.all(sB[i] >= 0.5e28) and not any(zero_tiles)
        elif kind == "E":
            assert zero_tiles == [f in ("small", "big", "sub") for f in facing]
        elif kind == "M":
            assert np.all(sB[i][0::2] == np.float32(1e-30)) and np.all(sB[i][1::2] == np.float32(1e20))
            assert not B[i, :32, 1::2].any() and B[i, 32:, 1::2].all() and B[i, :, 0::2].all()
    u, su = blocks(pair, c.u[0]), c.u[0][1]
    kinds = [D.U_KINDS[b % 16] for b in range(out // 64)]
    assert {"ord", "zero", "big", "sub"} <= set(kinds)
    for b, kind in enumerate(kinds):
        assert {"ord": 0.5 <= su[b] < 2, "zero": su[b] == 1.0 and not u[b].any(), "big": su[b] >= 0.5e30, "sub": 0 < su[b] < D.FLT_MIN}[kind]


@pytest.mark.parametrize("pair,out,in_", CASES)
def test_every_band_gives_its_category_and_no_block_is_left_out(ref, cases, pair, out, in_):  # noqa: F811
    c = cases(pair, out, in_)
    steps = np.float32(D.STEPS[D.VECTOR_BITS[pair]])
    lo, hi = D.e_range(pair)
    excluded = 0
    for j in range(D.NVEC_MAX):                                              # every vector of a batch: finite in dot and scale
        d = ref.rowdots(pair, c.B, out, in_, c.x[j])
        excluded += int((~np.isfinite(d.reshape(-1, 64))).any(axis=1).sum()) + int((~np.isfinite(c.t(j)[1])).sum())
    assert excluded == 0, "a block of the reference is non-finite: adjust the band scales, not this cap"
    d = ref.rowdots(pair, c.B, out, in_, c.x[0]).reshape(-1, 64)
    q, s = blocks(pair, c.t(0)), c.t(0)[1]
    for i in range(out // 64):
        kind, m = D.BANDS[i % 8], np.abs(d[i]).max()
        what = f"band {i} ({kind}): maximum {m}, scale {s[i]}"
        with np.errstate(over="ignore"):
            k = steps / m if m else np.float32(0)
        if kind in ("N", "N2"):
            assert q[i].any() and s[i] == m and 2.0 ** -100 < m < 1e30, what
        elif kind in ("Z", "Zx"):
            assert not d[i].any() and not q[i].any() and s[i] == 1.0, what
        elif kind == "T":
            assert d[i].any() and 0 < m < steps / D.FLT_MAX and np.isinf(k), what
            assert not q[i].any() and s[i] == m and s[i] != 1.0, what
            assert D.block_categories(D.VECTOR_BITS[pair], c.t(0))[i] == "T"
        elif kind == "H":
            assert np.isfinite(d[i]).all() and s[i] == m and m > 1e30 and q[i].any(), what
        elif kind == "E":
            assert lo <= m < hi and s[i] == m and np.isfinite(k) and k > D.FLT_MAX / 8 and q[i].any(), what
        elif kind == "M":
            assert d[i][:32].all() and float(np.abs(d[i][:32]).max()) < 2.0 ** -150 * float(m), what
            assert not q[i][:32].any() and q[i][32:].any() and s[i] == m, what
    # different vectors of one launch meet different categories in the same block
    cats = [D.block_categories(D.VECTOR_BITS[pair], c.t(j)) for j in (0, 1, 3)]
    assert any(len({cat[i] for cat in cats}) > 1 for i in range(out // 64))
    assert all(cat == "Z" for cat in cats[1]), "the zero vector"


@pytest.mark.parametrize("pair,out,in_", CASES)
def test_the_fused_results_are_finite_and_hold_k_inf_and_a_huge_block(ref, cases, pair, out, in_):  # noqa: F811
    c = cases(pair, out, in_)
    steps = np.float32(D.STEPS[D.VECTOR_BITS[pair]])
    for a in D.A_VALUES:
        for j in range(D.NVEC_MAX):
            r = c.r(j, a)
            assert np.isfinite(r[1]).all() and (r[1] > 0).all(), (a, j)
        r = c.r(0, a)
        with np.errstate(over="ignore"):
            k = steps / r[1]
        q = blocks(pair, r)
        assert any(np.isinf(k[b]) and not q[b].any() and r[1][b] != 1.0 for b in range(out // 64)), f"a={a}: no block with k = inf"
        assert (r[1] > 1e30).any() and (r[1] == 1.0).any(), f"a={a}: no block of scale above 1e30, or no zero block"
        # sv * a itself never overflows here: where it would, the reference's own scaleAndAdd yields inf (out of contract, common.h div7)
        assert np.isfinite(c.t(0)[1] * np.float32(a)).all()


@pytest.mark.parametrize("pair", D.PAIRS)
@pytest.mark.parametrize("m,n", D.LOOP_SHAPES)
def test_the_loops_stay_finite_and_meet_the_categories(ref, pair, m, n):  # noqa: F811
    Phi, PhiT, ys = D.loop_problem(ref, pair, m, n)
    bits = D.VECTOR_BITS[pair]
    assert np.isfinite(Phi[1]).all() and {"Z", "T"} <= set(D.LOOP_BANDS[m])
    seen = set()
    for K, thr in ((n // 4, 1), (1, 1), (n, 1), (n - 64, 1), (0, 0)):
        for j in range(D.NVEC_MAX):
            final, its = D.loop_reference(ref, pair, Phi, PhiT, ys[j], m, n, K, thr)
            assert len(its) == D.LOOP_ITERATIONS
            for it in its:
                for name, v in it.items():
                    assert np.isfinite(v[1]).all() and (v[1] > 0).all(), (K, thr, j, name)
                cat = D.block_categories(bits, it["x"])
                assert all(cat[b] == "Z" for b in D.LOOP_ZERO_COLUMNS), "the zero columns of Phi leave their blocks of x zero"
            for it in its[1:]:                                               # iteration 1 multiplies x = 0: every block of t1 is Z there
                for v in it.values():
                    seen |= set(D.block_categories(bits, v))
            if thr and 0 < K < n:
                assert np.count_nonzero(D.elements(bits, final["x"][0])) <= K
            assert np.any(final["x"][0])
            if j < 2:                                                        # what test_edge_bands_loops.py compares after two iterations
                assert {"Z", "T"} <= set(D.block_categories(bits, its[1]["t1"])), (K, thr, j)
        # what the first threshold meets, measurement 0: x = mu Phi' y before it
        final, its = D.loop_reference(ref, pair, Phi, PhiT, ys[0], m, n, K, thr)
        pre = its[0]["pre"]
        cat = D.block_categories(bits, pre)
        assert cat[D.LOOP_T_COLUMN] == "T" and 0 < pre[1][D.LOOP_T_COLUMN] < D.FLT_MIN, "a block of x with k = inf and a subnormal scale"
        mags = D.magnitudes(ref, pair, pre, n)[64 * D.LOOP_S_COLUMN:64 * D.LOOP_S_COLUMN + 64]
        assert np.isfinite(np.float32(D.STEPS[bits]) / pre[1][D.LOOP_S_COLUMN]), "the block of subnormal magnitudes has a finite k"
        # (int8: only |q| <= 2 of 127 steps lie below FLT_MIN at the smallest scale with a finite k, so one such element is what to ask for)
        assert int(((mags > 0) & (mags < D.FLT_MIN)).sum()) >= 1 and mags.max() >= D.FLT_MIN, "x holds no non-zero subnormal magnitude"
        if thr and K == n - 64:
            for i, it in enumerate(its):
                tau, ties, nonzero = D.threshold_stats(ref, pair, it["pre"], n, K)
                assert tau == 0.0 and nonzero < K and ties == n - nonzero, (i, tau, ties, nonzero)
                assert ties > 100, f"iteration {i}: the tie group of magnitude 0 holds {ties} elements"
    assert {"Z", "T"} <= seen, "no iterate behind the first has a block of category Z and one of category T"
