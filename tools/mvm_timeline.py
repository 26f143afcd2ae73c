#!/usr/bin/env python3
"""Launch timeline of the single-round streaming mvm (GPU box, probe build; not part of the product).

The stamped instantiations of k_m4_mvm64<8, nt> (the parent of the single-round shapes) and of k_m4_mvm_cu<G, K> let lane 0 of every wave
write the device wall clock (s_memrealtime, 100 MHz: 10 ns per tick) at five points: kernel entry, after the staging barrier, after its
first matrix step has been consumed, after its last step, before exit -- plus, once, its HW_ID and XCC_ID registers, from which this
driver tells the CUs apart.  Each kernel and shape runs three unstamped warm-up calls, then ONE stamped call.  Per phase the report holds
the earliest, median and latest wave over the chip (µs after the first wave's entry), then the spread of the last-step stamps inside a
CU (largest - smallest among the CU's waves: median and largest over the CUs) and between CUs (largest - smallest of the CUs' medians).
The stamped kernels are measured only with the stamps; no other timing comes from them.

    python tools/mvm_timeline.py [--out profiles/mvm_launch_timeline.txt] [--k 0,4,16]
"""
import argparse
import ctypes as C
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from clover_amd.build import build_probe_library  # noqa: E402
from clover_amd.lib_binding import CloverHip  # noqa: E402

PHASES = ["entry", "staged (after the barrier)", "first step consumed", "last step consumed", "before exit"]
TICK_US = 0.01


def summarize(st, label, out):
    """st: (waves, 8) uint64 -- five stamps, HW_ID, XCC_ID, unused"""
    st = st[st[:, 0] != 0]                                  # waves that never ran (none at the shapes below) left their words zero
    t0 = st[:, 0].min()
    rel = (st[:, :5].astype(np.int64) - np.int64(t0)) * TICK_US
    cu = ((st[:, 6] & 0xF) << 8) | ((st[:, 5] >> 8) & 0xFF)         # XCC_ID[3:0], HW_ID: SE_ID[15:13] SH_ID[12] CU_ID[11:8]
    keys = np.unique(cu)
    out.append(f"== {label}: {st.shape[0]} waves on {keys.size} CUs ({st.shape[0] / keys.size:.1f} waves per CU); "
               f"first entry to last exit {rel[:, 4].max():.2f} us")
    out.append(f"   {'phase':<28}{'earliest':>10}{'median':>10}{'latest':>10}   (us after the first wave's entry)")
    for p, name in enumerate(PHASES):
        out.append(f"   {name:<28}{rel[:, p].min():>10.2f}{np.median(rel[:, p]):>10.2f}{rel[:, p].max():>10.2f}")
    per_wave = rel[:, 1:] - rel[:, :-1]
    out.append("   per wave, median us: entry->staged %.2f, staged->first %.2f, first->last %.2f, last->exit %.2f"
               % tuple(np.median(per_wave[:, k]) for k in range(4)))
    last = rel[:, 3]
    inside = np.array([last[cu == k].max() - last[cu == k].min() for k in keys])
    med = np.array([np.median(last[cu == k]) for k in keys])
    out.append(f"   last-step spread inside a CU: median {np.median(inside):.2f} us, largest {inside.max():.2f} us; "
               f"between CUs (medians): {med.max() - med.min():.2f} us")
    out.append(f"   idle tail: the median wave finishes its last step {rel[:, 4].max() - np.median(last):.2f} us before the last exit")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "mvm_launch_timeline.txt"))
    ap.add_argument("--k", default="0,4,16", help="lockstep distances of k_m4_mvm_cu to stamp")
    args = ap.parse_args()
    hip = CloverHip(path=build_probe_library(), allow_probe=True)
    lib = hip.lib
    vp, u64 = C.c_void_p, C.c_uint64
    lib.clvx_mvm_variant.argtypes = [C.c_int, vp, vp, u64, u64, vp, vp, vp, vp, vp]
    lib.clvx_mvm_cu.argtypes = [C.c_int, vp, vp, u64, u64, vp, vp, vp, vp, vp, vp]
    lib.clvx_mvm64_stamped.argtypes = [vp, vp, u64, u64, vp, vp, vp, vp, vp, vp]
    cus = hip.device_info()["compute_units"]
    big = hip.alloc(2 << 30)
    hip.check(lib.clv_fill_random_nibbles(big.ptr, big.nbytes, 1, 0, None))
    out = [f"mvm launch timeline, {hip.device_info()['name']}, {cus} CUs; one stamped call per section after three unstamped warm-up calls"]
    for rows, cols in ((65536, 65536), (49152, 65536), (32768, 32768)):
        groups = rows // 64
        sA = hip.alloc(groups * (cols // 64) * 4)
        x, sx = hip.alloc(cols // 2), hip.alloc(cols // 16)
        r, sr = hip.alloc(rows // 2), hip.alloc(rows // 16)
        hip.check(lib.clv_fill_random_scales(sA.ptr, sA.nbytes // 4, 2, 0, None))
        hip.check(lib.clv_fill_random_nibbles(x.ptr, x.nbytes, 3, 0, None))
        hip.check(lib.clv_fill_random_scales(sx.ptr, sx.nbytes // 4, 4, 0, None))
        stamps = hip.alloc((groups + 4) * 4 * 8 * 8)
        runs = [("k_m4_mvm64<8, nt> (parent)", lambda: lib.clvx_mvm_variant(0, big.ptr, sA.ptr, rows, cols, x.ptr, sx.ptr, r.ptr, sr.ptr, None),
                 lambda: lib.clvx_mvm64_stamped(big.ptr, sA.ptr, rows, cols, x.ptr, sx.ptr, r.ptr, sr.ptr, stamps.ptr, None))]
        if 2 * cus < groups <= 4 * cus:
            for k in (int(v) for v in args.k.split(",")):
                runs.append((f"k_m4_mvm_cu<{-(-groups // cus)}, K = {k}>",
                             lambda k=k: lib.clvx_mvm_cu(k, big.ptr, sA.ptr, rows, cols, x.ptr, sx.ptr, r.ptr, sr.ptr, None, None),
                             lambda k=k: lib.clvx_mvm_cu(k, big.ptr, sA.ptr, rows, cols, x.ptr, sx.ptr, r.ptr, sr.ptr, stamps.ptr, None)))
        for label, plain, stamped in runs:
            for _ in range(3):
                hip.check(plain())
            hip.check(lib.clv_memset(stamps.ptr, 0, stamps.nbytes, None))
            hip.sync()
            hip.check(stamped())
            hip.sync()
            summarize(stamps.download(np.uint64).reshape(-1, 8), f"{rows} x {cols}, {label}", out)
    text = "\n".join(out) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
