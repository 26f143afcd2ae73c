#!/usr/bin/env python3
"""Launches the single-vector mvm and the batched mvm (2, 4, 8 vectors, the batched kernel) at 65536^2 three times each, for a counters-only
rocprofv3 pass:  rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_BUSY_CYCLES GRBM_GUI_ACTIVE -d DIR --output-format csv -- python
tools/mvm_batch_pmc.py;  python tools/pmc_summary.py DIR k_m4_mvm.  Read SQ_ACTIVE_INST_VALU / SQ_BUSY_CYCLES as a RELATIVE measure between the
launches of one pass; the instruction count per vector = SQ_INSTS_VALU of the batched launch / its vectors against the single launch's."""
import ctypes as C
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from clover_amd.lib_binding import CloverHip  # noqa: E402

hip = CloverHip()
lib = hip.lib
n = int(os.environ.get("MVMB_N", "65536"))
A, sA = hip.alloc(n * n // 2), hip.alloc((n // 64) ** 2 * 4)
hip.check(lib.clv_fill_random_nibbles(A.ptr, A.nbytes, 1, 0, None))
hip.check(lib.clv_fill_random_scales(sA.ptr, sA.nbytes // 4, 2, 0, None))
xs, rs = [], []
for j in range(8):
    x, sx, r, sr = hip.alloc(n // 2), hip.alloc(n // 16), hip.alloc(n // 2), hip.alloc(n // 16)
    hip.check(lib.clv_fill_random_nibbles(x.ptr, x.nbytes, 10 + j, 0, None))
    hip.check(lib.clv_fill_random_scales(sx.ptr, sx.nbytes // 4, 30 + j, 0, None))
    xs.append((x, sx))
    rs.append((r, sr))
arr = lambda bufs, i, g: (C.c_void_p * g)(*[b[i].ptr for b in bufs[:g]])  # noqa: E731
os.environ["CLV_MVM_BATCH"] = "1"
for _ in range(3):
    hip.check(lib.clm4_mvm(A.ptr, sA.ptr, n, n, xs[0][0].ptr, xs[0][1].ptr, rs[0][0].ptr, rs[0][1].ptr, None, None))
    for g in (2, 4, 8):
        hip.check(lib.clm4_mvm_batch(A.ptr, sA.ptr, n, n, g, arr(xs, 0, g), arr(xs, 1, g), arr(rs, 0, g), arr(rs, 1, g), None, None))
hip.sync()
print("mvm batch pmc probe done")
