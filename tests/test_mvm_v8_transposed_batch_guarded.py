"""The four batched transposed mixed calls, CloverMatrix4 x CloverVector8, (include/clover_hip_batch_t_v8.h) on ONE guard-banded arena each (tests/guarded.py): every output is
exact over its declared range against the CPU (oracle.m4_transpose, then oracle.m4_mvm_v8; oracle.v8_scale_and_add; the CPU loop for the
IHT call), the inputs and every byte outside the contract are unchanged.  Every case runs the batched kernel (CLV_MVM_BATCH=1, checked
through the launch counter).  The cases stay in a table of this file -- the table of test_guard_bands.py is the one of SIGNATURES -- with
the same coverage rule: a case per name of SIGNATURES_BATCH_T_V8."""
import numpy as np
import pytest

import test_guard_bands as gb
from clover_amd.lib_binding import SIGNATURES_BATCH_T_V8, THRESHOLD_FAST, THRESHOLD_REFERENCE
from mvm_v8_transposed_batch_data import C_, W
from test_mvm_batch import pa

GB_ENV = {"CLV_MVM_BATCH": "1"}


def _burnt(orc, draws):
    o = orc.rng(*gb.KEYS)
    for _ in range(draws):
        orc.rng_draw(o)
    return o


def _gb_mvm(rows, cols, nvec, st, fused=False, with_t=True, in_place=False, at=False):
    """at: clm4_mvm_v8_transposed_batch_at -- deterministic: the positions are ignored; stochastic: windows at 3 + j (2 G + 1), the state moved
    by 5.  x has rows elements, everything else cols"""
    def build(R):
        orc = R.oracle
        G = cols // 64
        base, stride, commit = (3, 2 * G + 1, 5) if st else (1 << 60, 1 << 60, 1 << 60)
        qA, sA = gb.m4(rows * cols + 91, rows, cols)
        At = orc.m4_transpose(qA, sA, rows, cols)
        regs, want = [("A", "input", qA), ("sA", "input", sA)] + ([("rng", "state", None)] if st else []), {}
        o = orc.rng(*gb.KEYS) if st and not at else None
        for j in range(nvec):
            qx, sx = gb.v8(rows + 30 + j, rows)
            regs += [(f"x{j}", "input", qx), (f"sx{j}", "input", sx)]
            t = orc.m4_mvm_v8(*At, cols, rows, qx, sx, _burnt(orc, base + j * stride) if st and at else o)
            if not fused:
                regs += [(f"r{j}", "output", cols), (f"sr{j}", "output", cols // 16)]
                want.update({f"r{j}": t[0], f"sr{j}": t[1]})
                continue
            qu, su = gb.v8(cols + 50 + j, cols)
            r = orc.v8_scale_and_add(qu, su, *t, -0.5, o)
            if with_t:
                regs += [(f"t{j}", "output", cols), (f"st{j}", "output", cols // 16)]
                want.update({f"t{j}": t[0], f"st{j}": t[1]})
            if in_place:
                regs += [(f"u{j}", "inout", qu), (f"su{j}", "inout", su)]
                want.update({f"u{j}": r[0], f"su{j}": r[1]})
            else:
                regs += [(f"u{j}", "input", qu), (f"su{j}", "input", su), (f"r{j}", "output", cols), (f"sr{j}", "output", cols // 16)]
                want.update({f"r{j}": r[0], f"sr{j}": r[1]})
        if st and at:
            o = _burnt(orc, commit)

        def call(L, p):
            a = lambda name: pa([p[f"{name}{j}"] for j in range(nvec)])  # noqa: E731
            before = L.clv_mvm_batch_launches()
            if at:
                rc = L.clm4_mvm_v8_transposed_batch_at(p["A"], p["sA"], rows, cols, nvec, a("x"), a("sx"), a("r"), a("sr"), p.get("rng"), base, stride,
                                                    commit, None)
            elif not fused:
                rc = L.clm4_mvm_v8_transposed_batch(p["A"], p["sA"], rows, cols, nvec, a("x"), a("sx"), a("r"), a("sr"), p.get("rng"), None)
            else:
                rc = L.clm4_mvm_v8_transposed_scale_and_add_batch(p["A"], p["sA"], rows, cols, nvec, a("x"), a("sx"), a("u"), a("su"), -0.5,
                                                               a("t") if with_t else None, a("st") if with_t else None, a("u" if in_place else "r"),
                                                               a("su" if in_place else "sr"), p.get("rng"), None)
            # without a generator a remainder group of one vector is forwarded to the single call
            want_launches = (nvec + 7) // 8 if st else nvec // 8 + (nvec % 8 >= 2)
            assert L.clv_mvm_batch_launches() - before == want_launches, "the call did not take the batched kernel"
            return rc
        return gb.Case(regs, call, want, orng=o, env=GB_ENV)
    return build


def _gb_iht(m, n, nvec, thr, st, iters=3):
    """the CPU loop per vector, vector after vector on ONE generator: the order of the single calls.  The arena holds Phi only"""
    def build(R):
        orc = R.oracle
        x_len, K, mu = n - 5, n // 4, np.float32(0.002)
        qP, sP = gb.m4(m * n + 17, m, n)
        qT, sT = orc.m4_transpose(qP, sP, m, n)
        regs, want = [("Phi", "input", qP), ("sPhi", "input", sP)] + ([("rng", "state", None)] if st else []), {}
        o = orc.rng(*gb.KEYS) if st else None
        for j in range(nvec):
            y = gb.v8(m + 18 + j, m)
            x = (np.zeros(n, np.int8), np.ones(n // 64, np.float32))
            t1 = t2 = t3 = None
            for _ in range(iters):
                t1 = orc.m4_mvm_v8(qP, sP, m, n, *x, o)
                t2 = orc.v8_scale_and_add(*y, *t1, -1.0, o)
                t3 = orc.m4_mvm_v8(qT, sT, n, m, *t2, o)
                x = orc.v8_scale_and_add(*x, *t3, float(mu), o)
                if thr:
                    x = (gb.threshold_reference(R, 8, x[0], x[1], x_len, K, THRESHOLD_REFERENCE if thr == 2 else THRESHOLD_FAST)[0], x[1])
            w = {f"x{j}": x[0], f"sx{j}": x[1], f"t1{j}": t1[0], f"st1{j}": t1[1], f"t2{j}": t2[0], f"st2{j}": t2[1], f"t3{j}": t3[0], f"st3{j}": t3[1]}
            regs += [(f"y{j}", "input", y[0]), (f"sy{j}", "input", y[1])] + [(k, "output", v.nbytes) for k, v in w.items()]
            want.update(w)

        def call(L, p):
            a = lambda name: pa([p[f"{name}{j}"] for j in range(nvec)])  # noqa: E731
            before = L.clv_mvm_batch_launches()
            rc = L.clm4_iht_v8_batch_one_matrix(p["Phi"], p["sPhi"], m, n, nvec, a("x"), a("sx"), x_len, a("y"), a("sy"), a("t1"), a("st1"), a("t2"),
                                             a("st2"), a("t3"), a("st3"), iters, K, float(mu), thr, p.get("rng"), None)
            assert L.clv_mvm_batch_launches() - before == 2 * iters, "the call did not take the batched loop"
            return rc
        return gb.Case(regs, call, want, orng=o, env=GB_ENV)
    return build


WIDE = 64 * (W + 2)                           # two workgroups: each may store only the blocks it owns
CASES = []
for _st in (False, True):
    _how = "stochastic" if _st else "rounding disabled"
    CASES.append((f"clm4_mvm_v8_transposed_batch 256x{WIDE} nvec=3 {_how}", _gb_mvm(256, WIDE, 3, _st)))
    CASES.append((f"clm4_mvm_v8_transposed_batch_at 256x{WIDE} nvec=3 {_how}", _gb_mvm(256, WIDE, 3, _st, at=True)))
    CASES.append((f"clm4_mvm_v8_transposed_scale_and_add_batch 256x{WIDE} nvec=3 {_how}", _gb_mvm(256, WIDE, 3, _st, fused=True)))
    CASES.append((f"clm4_mvm_v8_transposed_scale_and_add_batch 128x128 nvec=5 t=False in_place=True {_how}",
                  _gb_mvm(128, 128, 5, _st, fused=True, with_t=False, in_place=True)))
    CASES.append((f"clm4_iht_v8_batch_one_matrix 128x256 nvec=3 threshold=1 {_how}", _gb_iht(128, 256, 3, 1, _st)))
CASES.append((f"clm4_mvm_v8_transposed_batch {C_ + 128}x128 nvec=9 rounding disabled", _gb_mvm(C_ + 128, 128, 9, False)))
CASES.append((f"clm4_mvm_v8_transposed_batch_at {C_ + 128}x128 nvec=9 stochastic", _gb_mvm(C_ + 128, 128, 9, True, at=True)))
CASES.append((f"clm4_iht_v8_batch_one_matrix 256x{WIDE} nvec=3 threshold=0 rounding disabled", _gb_iht(256, WIDE, 3, 0, False)))


def test_every_entry_point_of_the_table_has_a_case():
    assert {name.split()[0] for name, _ in CASES} == set(SIGNATURES_BATCH_T_V8)
    assert not {name for name, _ in CASES} & set(gb.CASES), "these cases stay out of the table that is pinned to SIGNATURES"


@pytest.fixture(scope="module")
def refs(oracle):
    return gb.Refs(oracle, None, None)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_the_batched_transposed_mixed_calls_write_their_outputs_and_nothing_else(hip, refs, name):
    gb.run_case(hip, dict(CASES)[name](refs))
