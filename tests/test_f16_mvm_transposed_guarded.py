"""The four transposed half-precision calls (include/clover_hip_f16_t.h) on ONE guard-banded arena each (tests/guarded.py): every output is
exact over its declared range against the CPU restatement (tests/half16_t_restate.c: the column walk; half16_restate.c: scale_and_add, the
threshold, the CPU loop for the IHT call), the inputs and every byte outside the contract are unchanged.  The cases stay in a table of this
file -- the table of test_guard_bands.py is the one of SIGNATURES -- with the same coverage rule: a case per name of SIGNATURES_F16_T.
u, t and r start a few bytes behind a 256-byte boundary in some cases: they need only their element alignment."""
import numpy as np
import pytest

import test_guard_bands as gb
from clover_amd.lib_binding import SIGNATURES_F16_T, THRESHOLD_FAST, THRESHOLD_REFERENCE
from f16_batch_helpers import _scaled_matrix
from f16_transposed_data import COLS, matrix, vector_cols, vector_rows, vector_rows_f32
from f16_transposed_helpers import rt  # noqa: F401  (fixture)


def _gb_mvt(rows, cols, f32=False, shift=0):
    def build(R):
        rng = np.random.default_rng(rows * 31 + cols)
        A = matrix(rng, rows, cols)
        if f32:
            x = vector_rows_f32(rng, rows)
            want = R.rh.mvm_f32_transposed(A, rows, cols, x)
        else:
            x = vector_rows(rng, rows)
            want = R.rh.mvm_transposed(A, rows, cols, x)
        regs = [("A", "input", A), ("x", "input", x), ("r", "output", want.nbytes, shift)]
        fn = "clm_f16_mvm_f32_transposed" if f32 else "clm_f16_mvm_transposed"
        return gb.Case(regs, lambda L, p: getattr(L, fn)(p["A"], rows, cols, p["x"], p["r"], None), {"r": want})
    return build


def _gb_fused(rows, cols, with_t=True, in_place=False, shift=0):
    def build(R):
        rng = np.random.default_rng(rows * 37 + cols)
        A, x, u = matrix(rng, rows, cols), vector_rows(rng, rows), vector_cols(rng, cols)
        t, r = R.rh.mvm_transposed_scale_and_add(A, rows, cols, x, u, np.float32(-0.5))
        regs, want = [("A", "input", A), ("x", "input", x)], {}
        if with_t:
            regs.append(("t", "output", 2 * cols, shift))
            want["t"] = t
        if in_place:
            regs.append(("u", "inout", u, shift))
            want["u"] = r
        else:
            regs += [("u", "input", u, shift), ("r", "output", 2 * cols, shift)]
            want["r"] = r
        return gb.Case(regs, lambda L, p: L.clm_f16_mvm_transposed_scale_and_add(p["A"], rows, cols, p["x"], p["u"], -0.5, p["t"] if with_t else None,
                                                                                 p["u" if in_place else "r"], None), want)
    return build


def _gb_iht(m, n, thr, iters=2):
    def build(R):
        x_len, K, mu = n - 5, n // 4, np.float32(0.5)
        Phi = R.rh.quantize(_scaled_matrix(m * n + 51, m, n)).ravel()
        y = gb.v16(m + 52, m)
        x = np.zeros(n, np.uint16)
        t1 = t2 = t3 = None
        for _ in range(iters):
            t1 = R.rh.mvm(Phi, m, n, x)
            t2 = R.rh.scale_and_add(y, t1, np.float32(-1.0))
            t3 = R.rh.mvm_transposed(Phi, m, n, t2)
            x = R.rh.scale_and_add(x, t3, mu)
            if thr:
                x = gb.threshold_reference(R, 16, x, None, x_len, K, THRESHOLD_REFERENCE if thr == 2 else THRESHOLD_FAST)[0]
        want = {"x": x, "t1": t1, "t2": t2, "t3": t3}
        assert not any(np.any(v & 0x7C00 == 0x7C00) for v in want.values())
        regs = [("Phi", "input", Phi), ("y", "input", y)] + [(k, "output", v.nbytes) for k, v in want.items()]
        return gb.Case(regs, lambda L, p: L.clm_f16_iht_one_matrix(p["Phi"], m, n, p["x"], x_len, p["y"], p["t1"], p["t2"], p["t3"], iters, K,
                                                                   float(mu), thr, None), want)
    return build


WIDE = COLS + 128        # two workgroups, the last one partial where a strip is wider than 128 columns
CASES = [
    ("clm_f16_mvm_transposed 128x128", _gb_mvt(128, 128)),
    (f"clm_f16_mvm_transposed 256x{WIDE} shift=2", _gb_mvt(256, WIDE, shift=2)),
    ("clm_f16_mvm_f32_transposed 128x256", _gb_mvt(128, 256, f32=True)),
    (f"clm_f16_mvm_f32_transposed 384x{WIDE} shift=4", _gb_mvt(384, WIDE, f32=True, shift=4)),
    (f"clm_f16_mvm_transposed_scale_and_add 256x{WIDE} shift=2", _gb_fused(256, WIDE, shift=2)),
    ("clm_f16_mvm_transposed_scale_and_add 128x128 t=False in_place=True", _gb_fused(128, 128, with_t=False, in_place=True)),
    (f"clm_f16_mvm_transposed_scale_and_add 128x{WIDE} in_place=True shift=6", _gb_fused(128, WIDE, in_place=True, shift=6)),
    ("clm_f16_iht_one_matrix 128x256 threshold=1", _gb_iht(128, 256, 1)),
    ("clm_f16_iht_one_matrix 256x128 threshold=0", _gb_iht(256, 128, 0)),
    ("clm_f16_iht_one_matrix 128x256 threshold=2", _gb_iht(128, 256, 2)),
]


def test_every_entry_point_of_the_table_has_a_case():
    assert {name.split()[0] for name, _ in CASES} == set(SIGNATURES_F16_T)
    assert not {name for name, _ in CASES} & set(gb.CASES), "these cases stay out of the table that is pinned to SIGNATURES"


@pytest.fixture(scope="module")
def refs(rt):  # noqa: F811
    return gb.Refs(None, None, rt)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_the_transposed_half_precision_calls_write_their_outputs_and_nothing_else(hip, refs, name):
    gb.run_case(hip, dict(CASES)[name](refs))
