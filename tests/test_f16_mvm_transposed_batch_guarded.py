"""The three batched transposed half-precision calls (include/clover_hip_batch_f16_t.h) on ONE guard-banded arena each (tests/guarded.py):
every output is exact over its declared range against the CPU restatement (tests/half16_t_restate.c: the column walk; half16_restate.c:
scale_and_add, the threshold, the CPU loop for the IHT call), the inputs and every byte outside the contract are unchanged.  Every case
runs the batched kernel (CLV_MVM_BATCH=1, checked through the launch counter); partly filled groups (3 and 5 vectors) and a remainder
group of one are among them.  The cases stay in a table of this file -- the table of test_guard_bands.py is the one of SIGNATURES --
with the same coverage rule: a case per name of SIGNATURES_BATCH_F16_T.  u, t and r start a few bytes behind a 256-byte boundary in
some cases: they need only their element alignment."""
import numpy as np
import pytest

import test_guard_bands as gb
from clover_amd.lib_binding import SIGNATURES_BATCH_F16_T, THRESHOLD_FAST, THRESHOLD_REFERENCE
from f16_batch_helpers import _scaled_matrix, pa
from f16_transposed_batch_data import WIDTHS
from f16_transposed_data import matrix, vector_cols, vector_rows
from f16_transposed_helpers import rt  # noqa: F401  (fixture)

GB_ENV = {"CLV_MVM_BATCH": "1"}


def _gb_mvm(rows, cols, nvec, fused=False, with_t=True, in_place=False, shift=0):
    def build(R):
        rng = np.random.default_rng(rows * 41 + cols + nvec)
        A = matrix(rng, rows, cols)
        regs, want = [("A", "input", A)], {}
        for j in range(nvec):
            x = vector_rows(rng, rows)
            regs.append((f"x{j}", "input", x))
            if not fused:
                regs.append((f"r{j}", "output", 2 * cols, shift))
                want[f"r{j}"] = R.rh.mvm_transposed(A, rows, cols, x)
                continue
            u = vector_cols(rng, cols)
            t, r = R.rh.mvm_transposed_scale_and_add(A, rows, cols, x, u, np.float32(-0.5))
            if with_t:
                regs.append((f"t{j}", "output", 2 * cols, shift))
                want[f"t{j}"] = t
            if in_place:
                regs.append((f"u{j}", "inout", u, shift))
                want[f"u{j}"] = r
            else:
                regs += [(f"u{j}", "input", u, shift), (f"r{j}", "output", 2 * cols, shift)]
                want[f"r{j}"] = r

        def call(L, p):
            a = lambda name: pa([p[f"{name}{j}"] for j in range(nvec)])  # noqa: E731
            before = L.clv_mvm_batch_launches()
            if not fused:
                rc = L.clm_f16_mvm_transposed_batch(p["A"], rows, cols, nvec, a("x"), a("r"), None)
            else:
                rc = L.clm_f16_mvm_transposed_scale_and_add_batch(p["A"], rows, cols, nvec, a("x"), a("u"), -0.5, a("t") if with_t else None,
                                                                  a("u" if in_place else "r"), None)
            assert L.clv_mvm_batch_launches() - before == (nvec + 7) // 8, "the call did not take the batched kernel"
            return rc
        return gb.Case(regs, call, want, env=GB_ENV)
    return build


def _gb_iht(m, n, nvec, thr, iters=2):
    def build(R):
        x_len, K, mu = n - 5, n // 4, np.float32(0.5)
        Phi = R.rh.quantize(_scaled_matrix(m * n + 51, m, n)).ravel()
        regs, want = [("Phi", "input", Phi)], {}
        for j in range(nvec):
            y = gb.v16(m + 52 + j, m)
            x = np.zeros(n, np.uint16)
            t1 = t2 = t3 = None
            for _ in range(iters):
                t1 = R.rh.mvm(Phi, m, n, x)
                t2 = R.rh.scale_and_add(y, t1, np.float32(-1.0))
                t3 = R.rh.mvm_transposed(Phi, m, n, t2)
                x = R.rh.scale_and_add(x, t3, mu)
                if thr:
                    x = gb.threshold_reference(R, 16, x, None, x_len, K, THRESHOLD_REFERENCE if thr == 2 else THRESHOLD_FAST)[0]
            w = {f"x{j}": x, f"t1{j}": t1, f"t2{j}": t2, f"t3{j}": t3}
            assert not any(np.any(v & 0x7C00 == 0x7C00) for v in w.values())
            regs += [(f"y{j}", "input", y)] + [(k, "output", v.nbytes) for k, v in w.items()]
            want.update(w)

        def call(L, p):
            a = lambda name: pa([p[f"{name}{j}"] for j in range(nvec)])  # noqa: E731
            before = L.clv_mvm_batch_launches()
            rc = L.clm_f16_iht_batch_one_matrix(p["Phi"], m, n, nvec, a("x"), x_len, a("y"), a("t1"), a("t2"), a("t3"), iters, K, float(mu), thr, None)
            assert L.clv_mvm_batch_launches() - before == 2 * iters * ((nvec + 7) // 8), "the call did not take the batched loop"
            return rc
        return gb.Case(regs, call, want, env=GB_ENV)
    return build


WIDE = max(WIDTHS) + 128        # two workgroups or more at every strip width, the last one partial where a strip is wider than 128 columns
CASES = [
    (f"clm_f16_mvm_transposed_batch 256x{WIDE} nvec=3 shift=2", _gb_mvm(256, WIDE, 3, shift=2)),
    ("clm_f16_mvm_transposed_batch 384x128 nvec=9", _gb_mvm(384, 128, 9)),                       # a remainder group of one
    (f"clm_f16_mvm_transposed_scale_and_add_batch 256x{WIDE} nvec=3 shift=2", _gb_mvm(256, WIDE, 3, fused=True, shift=2)),
    ("clm_f16_mvm_transposed_scale_and_add_batch 128x128 nvec=5 t=False in_place=True", _gb_mvm(128, 128, 5, fused=True, with_t=False, in_place=True)),
    (f"clm_f16_mvm_transposed_scale_and_add_batch 128x{WIDE} nvec=2 in_place=True shift=6", _gb_mvm(128, WIDE, 2, fused=True, in_place=True, shift=6)),
    ("clm_f16_iht_batch_one_matrix 128x256 nvec=3 threshold=1", _gb_iht(128, 256, 3, 1)),
    ("clm_f16_iht_batch_one_matrix 256x128 nvec=9 threshold=0", _gb_iht(256, 128, 9, 0)),
    ("clm_f16_iht_batch_one_matrix 128x256 nvec=5 threshold=2", _gb_iht(128, 256, 5, 2)),
]


def test_every_entry_point_of_the_table_has_a_case():
    assert {name.split()[0] for name, _ in CASES} == set(SIGNATURES_BATCH_F16_T)
    assert not {name for name, _ in CASES} & set(gb.CASES), "these cases stay out of the table that is pinned to SIGNATURES"


@pytest.fixture(scope="module")
def refs(rt):  # noqa: F811
    return gb.Refs(None, None, rt)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_the_batched_transposed_half_precision_calls_write_their_outputs_and_nothing_else(hip, refs, name):
    gb.run_case(hip, dict(CASES)[name](refs))
