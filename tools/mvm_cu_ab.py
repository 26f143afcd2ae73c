#!/usr/bin/env python3
"""clm4_mvm as it dispatches, in two builds of the library, on the shapes around k_m4_mvm_cu's rule (GPU box; not part of the product).

    python tools/mvm_cu_ab.py --libs parent=/path/libclover_hip.so new=/path/libclover_hip.so [--rounds 5] [--out FILE]

Every round starts one fresh process per build, the builds alternating; a process fills one buffer and times clm4_mvm back to back with
HIP events on 65536^2 (C3) and 49152 x 65536 (the shapes k_m4_mvm_cu takes), and on 32768^2, 131072 x 65536 and the C5 whole launch
2^20 x 2^16, whose dispatch is the same in both builds.  Per shape and build: median, smallest and largest round; the "spread" of a
build is largest - smallest."""
import argparse
import ctypes as C
import json
import subprocess
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

SHAPES = [(65536, 65536, 50), (49152, 65536, 50), (32768, 32768, 100), (131072, 65536, 30), (1 << 20, 1 << 16, 6)]


def child(path):
    from clover_amd.lib_binding import CloverHip
    hip = CloverHip(path=path)
    lib = hip.lib
    rows_max, cols_max = max(s[0] for s in SHAPES), max(s[1] for s in SHAPES)
    A = hip.alloc(rows_max * cols_max // 2)
    sA = hip.alloc((rows_max // 64) * (cols_max // 64) * 4)
    x, sx = hip.alloc(cols_max // 2), hip.alloc(cols_max // 16)
    r, sr = hip.alloc(rows_max // 2), hip.alloc(rows_max // 16)
    hip.check(lib.clv_fill_random_nibbles(A.ptr, A.nbytes, 1, 0, None))
    hip.check(lib.clv_fill_random_scales(sA.ptr, sA.nbytes // 4, 2, 0, None))
    hip.check(lib.clv_fill_random_nibbles(x.ptr, x.nbytes, 3, 0, None))
    hip.check(lib.clv_fill_random_scales(sx.ptr, sx.nbytes // 4, 4, 0, None))
    a, b = C.c_void_p(), C.c_void_p()
    hip.check(lib.clv_event_create(C.byref(a)))
    hip.check(lib.clv_event_create(C.byref(b)))
    res = {}
    for rows, cols, calls in SHAPES:
        def fn():
            hip.check(lib.clm4_mvm(A.ptr, sA.ptr, rows, cols, x.ptr, sx.ptr, r.ptr, sr.ptr, None, None))
        for _ in range(3):
            fn()
        hip.sync()
        hip.check(lib.clv_event_record(a, None))
        for _ in range(calls):
            fn()
        hip.check(lib.clv_event_record(b, None))
        hip.check(lib.clv_event_sync(b))
        ms = C.c_float()
        hip.check(lib.clv_event_elapsed_ms(a, b, C.byref(ms)))
        res[f"{rows}x{cols}"] = ms.value / calls
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs=2, metavar="NAME=PATH")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    libs = [v.split("=", 1) for v in args.libs]
    ts = {name: {} for name, _ in libs}
    for _ in range(args.rounds):
        for name, path in libs:
            p = subprocess.run([sys.executable, __file__, "--child", path], capture_output=True, text=True, timeout=300)
            if p.returncode != 0:                 # nothing more is started on the GPU after a failure
                raise SystemExit(f"{name}: exit {p.returncode}\n{p.stdout}\n{p.stderr}")
            for k, v in json.loads(p.stdout.strip().splitlines()[-1]).items():
                ts[name].setdefault(k, []).append(v)
    lines = [f"clm4_mvm, ms per call (HIP events, back to back), {args.rounds} rounds, one fresh process per build and round, builds alternating",
             f"{'shape':<18}{'build':<8}{'median':>9}{'min':>9}{'max':>9}{'spread':>9}"]
    for k in ts[libs[0][0]]:
        for name, _ in libs:
            t = sorted(ts[name][k])
            lines.append(f"{k:<18}{name:<8}{t[len(t) // 2]:>9.4f}{t[0]:>9.4f}{t[-1]:>9.4f}{t[-1] - t[0]:>9.4f}")
    text = "\n".join(lines) + "\n"
    if args.out:
        Path(args.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
