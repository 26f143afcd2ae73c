"""The three transposed CloverMatrix8 calls on ONE guard-banded arena each (tests/guarded.py): every output is exact over its declared
range against the CPU (tests/matrix8_restate.c: transpose, then mvm; oracle.v8_scale_and_add; the loop of test_guard_bands.py), the
inputs and every byte outside the contract are unchanged.  384 x 640 and 128 x 384 have 10 and 6 output blocks (5 and 3 workgroups);
the stochastic cases compare the 256-byte state through clv_rng_get.  The cases join the table of test_guard_bands.py, whose coverage
test asks for a case per entry point."""
import numpy as np
import pytest

import test_guard_bands as gb
from clover_amd.lib_binding import THRESHOLD_FAST
from matrix8_helpers import m8  # noqa: F401  (fixture)


def _gb_m8_mvm_t(rows, cols, st=False, fused=False, with_t=True, in_place=False):
    def build(R):
        orc = R.oracle
        qA, sA = gb.m8data(rows * cols + 31, rows, cols)
        At = R.m8.transpose(qA, sA, rows, cols)
        qx, sx = gb.v8(rows + 32, rows)
        o = orc.rng(*gb.KEYS) if st else None
        regs = [("A", "input", qA), ("sA", "input", sA), ("x", "input", qx), ("sx", "input", sx)] + ([("rng", "state", None)] if st else [])
        t = R.m8.mvm(*At, cols, rows, qx, sx, o)
        if not fused:
            regs += [("r", "output", cols), ("sr", "output", cols // 16)]
            return gb.Case(regs, lambda L, p: L.clm8_mvm_transposed(p["A"], p["sA"], rows, cols, p["x"], p["sx"], p["r"], p["sr"], p.get("rng"), None),
                           {"r": t[0], "sr": t[1]}, orng=o)
        qu, su = gb.v8(cols + 33, cols)
        r = orc.v8_scale_and_add(qu, su, *t, -0.5, o)
        want = {}
        if with_t:
            regs += [("t", "output", cols), ("st", "output", cols // 16)]
            want.update(t=t[0], st=t[1])
        if in_place:
            regs += [("u", "inout", qu), ("su", "inout", su)]
            want.update(u=r[0], su=r[1])
        else:
            regs += [("u", "input", qu), ("su", "input", su), ("r", "output", cols), ("sr", "output", cols // 16)]
            want.update(r=r[0], sr=r[1])
        return gb.Case(regs, lambda L, p: L.clm8_mvm_transposed_scale_and_add(p["A"], p["sA"], rows, cols, p["x"], p["sx"], p["u"], p["su"], -0.5,
                                                                              p.get("t"), p.get("st"), p["u" if in_place else "r"],
                                                                              p["su" if in_place else "sr"], p.get("rng"), None), want, orng=o)
    return build


def _gb_m8_iht_one(m, n, thr, st, iters=3):
    def build(R):
        orc = R.oracle
        x_len, K, mu = n - 5, n // 4, np.float32(0.0002)
        qP, sP = gb.m8data(m * n + 13, m, n)
        qT, sT = R.m8.transpose(qP, sP, m, n)
        y = gb.v8(m + 14, m)
        o = orc.rng(*gb.KEYS) if st else None
        x = (np.zeros(n, np.int8), np.ones(n // 64, np.float32))      # x.clear()
        t1 = t2 = t3 = None
        for _ in range(iters):
            t1 = R.m8.mvm(qP, sP, m, n, *x, o)
            t2 = orc.v8_scale_and_add(*y, *t1, -1.0, o)
            t3 = R.m8.mvm(qT, sT, n, m, *t2, o)
            x = orc.v8_scale_and_add(*x, *t3, float(mu), o)
            if thr:
                x = (gb.threshold_reference(R, 8, x[0], x[1], x_len, K, THRESHOLD_FAST)[0], x[1])
        want = dict(x=x[0], sx=x[1], t1=t1[0], st1=t1[1], t2=t2[0], st2=t2[1], t3=t3[0], st3=t3[1])
        regs = [("Phi", "input", qP), ("sPhi", "input", sP), ("y", "input", y[0]), ("sy", "input", y[1])] + ([("rng", "state", None)] if st else [])
        regs += [(k, "output", v.nbytes) for k, v in want.items()]
        return gb.Case(regs, lambda L, p: L.clm8_iht_one_matrix(p["Phi"], p["sPhi"], m, n, p["x"], p["sx"], x_len, p["y"], p["sy"], p["t1"], p["st1"],
                                                                p["t2"], p["st2"], p["t3"], p["st3"], iters, K, float(mu), thr, p.get("rng"), None),
                       want, orng=o)
    return build


M8T_CASES = []
for _st in (False, True):
    _how = "stochastic" if _st else "rounding disabled"
    M8T_CASES.append((f"clm8_mvm_transposed 384x640 {_how}", _gb_m8_mvm_t(384, 640, _st)))
    M8T_CASES.append((f"clm8_mvm_transposed_scale_and_add 384x640 {_how}", _gb_m8_mvm_t(384, 640, _st, fused=True)))
    M8T_CASES.append((f"clm8_mvm_transposed_scale_and_add 128x384 t=False in place {_how}",
                      _gb_m8_mvm_t(128, 384, _st, fused=True, with_t=False, in_place=True)))
    M8T_CASES.append((f"clm8_iht_one_matrix 128x256 threshold=1 {_how}", _gb_m8_iht_one(128, 256, 1, _st)))
M8T_CASES.append(("clm8_mvm_transposed 128x128 rounding disabled", _gb_m8_mvm_t(128, 128)))
M8T_CASES.append(("clm8_iht_one_matrix 256x128 threshold=0 rounding disabled", _gb_m8_iht_one(256, 128, 0, False)))
for _name, _build in M8T_CASES:
    if _name not in gb.CASES:                 # the coverage test of test_guard_bands.py reads its table when it runs, after every module is imported
        gb.case(_name)(_build)


@pytest.fixture(scope="module")
def refs(oracle, m8):  # noqa: F811
    return gb.Refs(oracle, m8, None)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, _ in M8T_CASES])
def test_transposed_8_bit_calls_write_their_outputs_and_nothing_else(hip, refs, name):
    gb.run_case(hip, dict(M8T_CASES)[name](refs))
