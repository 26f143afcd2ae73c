"""The five calls of include/clover_hip_m8_f32.h on ONE guard-banded arena each (tests/guarded.py): every output is exact over its declared
range against the CPU references (m8.mvm_f32 on m8.transpose, rf.scale_and_add, the composed loop of
tests/m8_f32_helpers.py), the inputs and every byte outside the contract are unchanged.  The calls take no workspace.  The cases stay in a
table of this file -- the table of test_guard_bands.py is the one of SIGNATURES -- with the same coverage rule: a case per name of
SIGNATURES_M8_F32.  u, t and r2 start a few bytes behind a 256-byte boundary in some cases: they need only their element alignment."""
import pytest

import test_guard_bands as gb
from clover_amd.lib_binding import SIGNATURES_M8_F32
from fp32_helpers import rf  # noqa: F401  (fixture)
from m8_f32_helpers import COLS, loop_problem, loop_reference, problem
from matrix8_helpers import m8  # noqa: F401  (fixture)

A = -0.5


def _gb_mvt(rows, cols, shift=0):
    def build(R):
        qA, sA, x = problem(rows, cols, seed=3)[:3]
        qT, sT = R.m8.transpose(qA, sA, rows, cols)
        want = R.m8.mvm_f32(qT, sT, cols, rows, x)
        regs = [("A", "input", qA), ("sA", "input", sA), ("x", "input", x), ("r", "output", want.nbytes, shift)]
        return gb.Case(regs, lambda L, p: L.clm8_mvm_f32_transposed(p["A"], p["sA"], rows, cols, p["x"], p["r"], None), {"r": want})
    return build


def _gb_fused(rows, cols, transposed, with_t=True, in_place=False, shift=0):
    def build(R):
        qA, sA, xr, xc, ur, uc = problem(rows, cols, seed=4)
        if transposed:
            qT, sT = R.m8.transpose(qA, sA, rows, cols)
            x, u, d = xr, uc, R.m8.mvm_f32(qT, sT, cols, rows, xr)
        else:
            x, u, d = xc, ur, R.m8.mvm_f32(qA, sA, rows, cols, xc)
        r2 = R.rf.scale_and_add(u, d, A)
        regs, want = [("A", "input", qA), ("sA", "input", sA), ("x", "input", x)], {}
        if with_t:
            regs.append(("t", "output", d.nbytes, shift))
            want["t"] = d
        if in_place:
            regs.append(("u", "inout", u, shift))
            want["u"] = r2
        else:
            regs += [("u", "input", u, shift), ("r2", "output", d.nbytes, shift)]
            want["r2"] = r2
        fn = "clm8_mvm_f32_transposed_scale_and_add" if transposed else "clm8_mvm_f32_scale_and_add"
        return gb.Case(regs, lambda L, p: getattr(L, fn)(p["A"], p["sA"], rows, cols, p["x"], p["u"], A, p["t"] if with_t else None,
                                                         p["u" if in_place else "r2"], None), want)
    return build


def _gb_iht(m, n, thr, one_matrix, iters=2):
    def build(R):
        x_len, K = n - 64, n // 8
        qPhi, sPhi, y, mu = loop_problem(R.m8, m, n, False)
        qT, sT = R.m8.transpose(qPhi, sPhi, m, n)
        want = loop_reference(R.m8, R.rf, qPhi, sPhi, m, n, y, iters, K, mu, thr, x_len, lambda t2: R.m8.mvm_f32(qT, sT, n, m, t2))
        regs = [("Phi", "input", qPhi), ("sPhi", "input", sPhi)] + ([] if one_matrix else [("PhiT", "input", qT), ("sPhiT", "input", sT)])
        regs += [("y", "input", y)] + [(k, "output", v.nbytes) for k, v in want.items()]

        def call(L, p):
            tail = (m, n, p["x"], x_len, p["y"], p["t1"], p["t2"], p["t3"], iters, K, float(mu), thr, None)
            if one_matrix:
                return L.clm8_iht_f32_one_matrix(p["Phi"], p["sPhi"], *tail)
            return L.clm8_iht_f32(p["Phi"], p["sPhi"], p["PhiT"], p["sPhiT"], *tail)
        return gb.Case(regs, call, want)
    return build


WIDE = COLS + 128        # two workgroups (strips are 128 columns: every strip is whole)
CASES = [
    ("clm8_mvm_f32_transposed 128x128", _gb_mvt(128, 128)),
    (f"clm8_mvm_f32_transposed 384x{WIDE} shift=4", _gb_mvt(384, WIDE, shift=4)),
    (f"clm8_mvm_f32_transposed_scale_and_add 256x{WIDE} shift=4", _gb_fused(256, WIDE, True, shift=4)),
    ("clm8_mvm_f32_transposed_scale_and_add 128x128 t=False in_place=True", _gb_fused(128, 128, True, with_t=False, in_place=True)),
    (f"clm8_mvm_f32_transposed_scale_and_add 128x{WIDE} in_place=True shift=8", _gb_fused(128, WIDE, True, in_place=True, shift=8)),
    ("clm8_mvm_f32_scale_and_add 192x256 shift=4", _gb_fused(192, 256, False, shift=4)),
    ("clm8_mvm_f32_scale_and_add 128x128 t=False in_place=True", _gb_fused(128, 128, False, with_t=False, in_place=True)),
    ("clm8_mvm_f32_scale_and_add 128x384 in_place=True shift=12", _gb_fused(128, 384, False, in_place=True, shift=12)),
    ("clm8_iht_f32 128x256 threshold=1", _gb_iht(128, 256, 1, False)),
    ("clm8_iht_f32 256x128 threshold=0", _gb_iht(256, 128, 0, False)),
    ("clm8_iht_f32 128x256 threshold=2", _gb_iht(128, 256, 2, False)),
    ("clm8_iht_f32_one_matrix 128x256 threshold=1", _gb_iht(128, 256, 1, True)),
    ("clm8_iht_f32_one_matrix 256x128 threshold=0", _gb_iht(256, 128, 0, True)),
    ("clm8_iht_f32_one_matrix 128x256 threshold=2", _gb_iht(128, 256, 2, True)),
]


def test_every_entry_point_of_the_table_has_a_case():
    assert {name.split()[0] for name, _ in CASES} == set(SIGNATURES_M8_F32)
    assert not {name for name, _ in CASES} & set(gb.CASES), "these cases stay out of the table that is pinned to SIGNATURES"


class Refs:
    def __init__(self, m8, rf):  # noqa: F811
        self.m8, self.rf = m8, rf


@pytest.fixture(scope="module")
def refs(m8, rf):  # noqa: F811
    return Refs(m8, rf)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_the_fp32_vector_calls_of_the_8_bit_matrix_write_their_outputs_and_nothing_else(hip, refs, name):
    gb.run_case(hip, dict(CASES)[name](refs))
