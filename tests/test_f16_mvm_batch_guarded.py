"""The four batched half-precision calls (include/clover_hip_batch_f16.h) on ONE guard-banded arena each (tests/guarded.py): every output is
exact over its declared range against the CPU restatement (tests/half16_restate.c: mvm, scale_and_add, the threshold; the CPU loop for
the IHT call), the inputs and every byte outside the contract are unchanged.  The mvm and IHT cases run the batched kernel
(CLV_MVM_BATCH=1, checked through the launch counter).  The cases stay in a table of this file -- the table of test_guard_bands.py is the
one of SIGNATURES -- with the same coverage rule: a case per name of SIGNATURES_BATCH_F16."""
import numpy as np
import pytest

import test_guard_bands as gb
from clover_amd.lib_binding import SIGNATURES_BATCH_F16, THRESHOLD_FAST, THRESHOLD_REFERENCE
from f16_batch_helpers import _scaled_matrix, pa
from half16_helpers import rh  # noqa: F401

GB_ENV = {"CLV_MVM_BATCH": "1"}


def _gb_mvm(rows, cols, nvec, fused=False, with_t=True, in_place=False, shift=0):
    """shift: u, t and r start that many bytes behind a 256-byte boundary (they need only their element alignment)"""
    def build(R):
        A = gb.v16(rows * cols + 61, rows * cols)
        regs, want = [("A", "input", A)], {}
        for j in range(nvec):
            x = gb.v16(cols + 62 + j, cols)
            t = R.rh.mvm(A, rows, cols, x)
            regs.append((f"x{j}", "input", x))
            if not fused:
                regs.append((f"r{j}", "output", 2 * rows, shift))
                want[f"r{j}"] = t
                continue
            u = gb.v16(rows + 80 + j, rows)
            r = R.rh.scale_and_add(u, t, np.float32(-0.5))
            if with_t:
                regs.append((f"t{j}", "output", 2 * rows, shift))
                want[f"t{j}"] = t
            if in_place:
                regs.append((f"u{j}", "inout", u, shift))
                want[f"u{j}"] = r
            else:
                regs += [(f"u{j}", "input", u, shift), (f"r{j}", "output", 2 * rows, shift)]
                want[f"r{j}"] = r

        def call(L, p):
            a = lambda name: pa([p[f"{name}{j}"] for j in range(nvec)])  # noqa: E731
            before = L.clv_mvm_batch_launches()
            if not fused:
                rc = L.clm_f16_mvm_batch(p["A"], rows, cols, nvec, a("x"), a("r"), None)
            else:
                rc = L.clm_f16_mvm_scale_and_add_batch(p["A"], rows, cols, nvec, a("x"), a("u"), -0.5, a("t") if with_t else None,
                                                       a("u" if in_place else "r"), None)
            assert L.clv_mvm_batch_launches() - before == (nvec + 7) // 8, "the call did not take the batched kernel"
            return rc
        return gb.Case(regs, call, want, env=GB_ENV)
    return build


def _gb_threshold(n_pad, n, nvec, mode):
    def build(R):
        k = n // 4
        regs, want = [], {}
        for j in range(nvec):
            h = gb.threshold_data(16, n_pad, n_pad + 7 + j)[0]
            regs.append((f"h{j}", "inout", h))
            want[f"h{j}"] = gb.threshold_reference(R, 16, h, None, n, k, mode)[0]
        return gb.Case(regs, lambda L, p: L.clv_f16_threshold_batch(pa([p[f"h{j}"] for j in range(nvec)]), nvec, n, n_pad, k, mode, None), want)
    return build


def _gb_iht(m, n, nvec, thr, iters=2):
    def build(R):
        x_len, K, mu = n - 5, n // 4, np.float32(0.5)
        Phi = R.rh.quantize(_scaled_matrix(m * n + 51, m, n)).ravel()
        PhiT = R.rh.transpose(Phi, m, n)
        regs, want = [("Phi", "input", Phi), ("PhiT", "input", PhiT)], {}
        for j in range(nvec):
            y = gb.v16(m + 52 + j, m)
            x = np.zeros(n, np.uint16)
            t1 = t2 = t3 = None
            for _ in range(iters):
                t1 = R.rh.mvm(Phi, m, n, x)
                t2 = R.rh.scale_and_add(y, t1, np.float32(-1.0))
                t3 = R.rh.mvm(PhiT, n, m, t2)
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
            rc = L.clm_f16_iht_batch(p["Phi"], p["PhiT"], m, n, nvec, a("x"), x_len, a("y"), a("t1"), a("t2"), a("t3"), iters, K, float(mu), thr, None)
            assert L.clv_mvm_batch_launches() - before == 2 * iters * ((nvec + 7) // 8), "the call did not take the batched loop"
            return rc
        return gb.Case(regs, call, want, env=GB_ENV)
    return build


CASES = [
    ("clm_f16_mvm_batch 100x256 nvec=3", _gb_mvm(100, 256, 3, shift=2)),                       # ragged rows: two workgroups, a tail
    ("clm_f16_mvm_batch 40x640 nvec=9", _gb_mvm(40, 640, 9)),                                  # a second chunk of x; a remainder group
    ("clm_f16_mvm_scale_and_add_batch 100x256 nvec=3", _gb_mvm(100, 256, 3, fused=True, shift=2)),
    ("clm_f16_mvm_scale_and_add_batch 64x128 nvec=5 t=False in_place=True", _gb_mvm(64, 128, 5, fused=True, with_t=False, in_place=True)),
    ("clm_f16_mvm_scale_and_add_batch 100x256 nvec=2 in_place=True", _gb_mvm(100, 256, 2, fused=True, in_place=True, shift=2)),
    ("clv_f16_threshold_batch FAST n_pad=256 n=200 nvec=3", _gb_threshold(256, 200, 3, THRESHOLD_FAST)),
    ("clv_f16_threshold_batch FAST n_pad=2048 n=2011 nvec=65", _gb_threshold(2048, 2011, 65, THRESHOLD_FAST)),
    ("clv_f16_threshold_batch REFERENCE n_pad=256 n=200 nvec=3", _gb_threshold(256, 200, 3, THRESHOLD_REFERENCE)),
    ("clm_f16_iht_batch 128x256 nvec=3 threshold=1", _gb_iht(128, 256, 3, 1)),
    ("clm_f16_iht_batch 256x128 nvec=9 threshold=0", _gb_iht(256, 128, 9, 0)),
    ("clm_f16_iht_batch 128x256 nvec=2 threshold=2", _gb_iht(128, 256, 2, 2)),
]


def test_every_entry_point_of_the_table_has_a_case():
    assert {name.split()[0] for name, _ in CASES} == set(SIGNATURES_BATCH_F16)
    assert not {name for name, _ in CASES} & set(gb.CASES), "these cases stay out of the table that is pinned to SIGNATURES"


@pytest.fixture(scope="module")
def refs(rh):  # noqa: F811
    return gb.Refs(None, None, rh)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_the_batched_half_precision_calls_write_their_outputs_and_nothing_else(hip, refs, name):
    gb.run_case(hip, dict(CASES)[name](refs))
