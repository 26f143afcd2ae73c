#!/usr/bin/env python3
"""bench.py -- headline benchmark: CloverMatrix4::mvm (int4 GEMV + re-quantise) on MI355X.

    python bench.py --gpus N --steps K --warmup W

One "step" = one mvm of a (N * rows_per_gpu) x cols 4-bit matrix with a 4-bit vector.  Each rank owns a
contiguous row shard (a multiple of 64 rows) resident in HBM; N > 1 adds one RCCL all-gather of the packed
result (nibbles + scales) per step -- the only exchange the path has; it runs on RCCL's stream and
overlaps the next step's kernel (two result buffers), every step's gather is complete inside the timed region.  Weak scaling: the
per-GPU shard is fixed (default 65536 x 65536 = BASELINE.json configs[2], "C3"); --rows-per-gpu 131072
at N=8 is exactly configs[4] ("C5", 2^20 x 2^16).

Prints ONE JSON line on rank 0 with the headline figures and `roofline` (HBM, algorithmic bytes / HIP-event
kernel time of the sampled timed steps).  A plain run does only that: set up, warm up, time the K steps, write
--dump-outputs, print.  Everything else the benchmark measures or checks runs behind --full: the cold figures, the
`c5` object, the product's own multi-GPU loops, the gathered-result checks, at N=1 the `gemm` and `extras`
objects, and `cpu_baseline` (the AVX2+OpenMP restatement of the reference on the host cores, bounded sample).
Inputs are synthetic and generated on the device before the timed region.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

HBM_PEAK_GBS = 8000.0     # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s is the measured copy ceiling


def pmc_traffic(rows: int, cols: int):
    """HBM bytes per launch from the committed rocprofv3 --pmc passes (profiles/rNN_mvm_c3_pmc.json); PMC cannot
    be collected inside a timed run, so the latest committed measurement of the same kernel + shape is reported."""
    best = None
    for f in sorted((ROOT / "profiles").glob("r*_mvm_c3_pmc.json")):
        try:
            d = json.loads(f.read_text())["mvm_c3"]
            if d["rows"] == rows and d["cols"] == cols:
                best = (round(d["traffic_bytes_per_launch"]), f.name)
        except (OSError, KeyError, ValueError):
            continue
    return best


def mvm_bytes(rows: int, cols: int) -> int:
    """Algorithmic bytes of one mvm: every operand incl. scales counted once."""
    return rows * cols // 2 + 4 * (rows // 64) * (cols // 64) + (cols // 2 + cols // 16) + (rows // 2 + rows // 16)


SIDE_STEPS = 20                      # timed steps of every side measurement (cold pass, c5, product loops): min(--steps, this)
DUMP_LIMIT_BYTES = 64 << 20          # --dump-outputs: total size of the written arrays


def write_outputs(out_dir: str, arrays: dict) -> None:
    """--dump-outputs: each array as out_dir/<name>.npy (float32 or float64 only), all of them within DUMP_LIMIT_BYTES."""
    import numpy as np
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_LIMIT_BYTES, f"--dump-outputs: {total} B exceeds {DUMP_LIMIT_BYTES} B"
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(out_dir, f"{name}.npy"), np.ascontiguousarray(a))


def decode_v4(nib, scales) -> dict:
    """A packed CloverVector4 (32 bytes of nibbles per 64-element block, high nibble first, + one fp32 scale per block) as the
    caller receives it: the restored values (nibble * (scale / 7), the reference's restore order), the nibbles and the scales."""
    import numpy as np
    b = np.asarray(nib, dtype=np.uint8)
    q = np.empty(2 * b.size, dtype=np.int8)
    q[0::2] = ((b >> 4) ^ 8).astype(np.int8) - 8
    q[1::2] = ((b & 15) ^ 8).astype(np.int8) - 8
    s = np.asarray(scales, dtype=np.float32)
    vals = (q.astype(np.float32).reshape(-1, 64) * (s / np.float32(7.0))[:, None]).reshape(-1)
    return {"values": vals, "nibbles": q.astype(np.float32), "scales": s}


# ----------------------------------------------------------------------------------------------------
# CPU baseline leg (runs in a child process so OpenMP binding env vars take effect)
# ----------------------------------------------------------------------------------------------------
def cpu_baseline_child(path: str) -> None:
    """Everything sequential is timed FIRST and the thread counts then go up: OMP_WAIT_POLICY=active keeps the idle threads of an earlier,
    larger team spinning, and under a cgroup cpu quota (16 cpus on the driver's boxes) those spinners get the whole process throttled --
    round 3's first run measured the one-core quantize at 2 GB/s after a 256-thread team had run (18 GB/s before one)."""
    try:
        runnable = len(os.sched_getaffinity(0))   # cpus this process may run on -- read BEFORE the OpenMP runtime binds the main thread
    except AttributeError:
        runnable = os.cpu_count() or 1
    import numpy as np

    from oracle.binding import FastOracle          # test/bench infrastructure: the timed CPU port
    with np.load(path) as z:
        d = {k: z[k] for k in z.files}            # materialise once (NpzFile re-reads the zip on every access)
    rows, cols = int(d["rows"]), int(d["cols"])
    F = FastOracle()
    F.set_kernel("maddubs")                       # the reference's instruction mix (CloverVector4.h:1136-1180)
    cores = os.cpu_count() or 1
    out = (np.zeros(rows // 2, np.uint8), np.zeros(rows // 64, np.float32))
    counts = [t for t in sorted({1, min(16, cores), min(64, cores), max(1, cores // 2), cores}) if t <= rows // 64]
    vec_counts = [t for t in counts if t in (1, min(16, cores), min(64, cores))]

    def med_time(fn, reps, seconds, min_reps=3):
        fn()                                       # warm-up (and first touch of the outputs)
        ts, t_end = [], time.perf_counter() + seconds
        while len(ts) < reps and (len(ts) < min_reps or time.perf_counter() < t_end):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return sorted(ts)[len(ts) // 2], min(ts), max(ts), len(ts)

    # the vectors of BASELINE configs[1] ("quantize + dot ... vs AVX2 host"): n = 2^24 (configs[1]'s size: 18.9 / 76.5 MB, inside this host's
    # L3 -- the reference's 4-core box was DRAM-bound there) and n = 2^30 (DRAM for everyone); sources are integers in [-10, 10] like the
    # reference's setRandomInteger(10) data (01_measure.h:797).  Bytes as 01_measure.h:644, 717, 804: dot 1.125 n, quantize 4.5625 n.
    vecs, vec = {}, {}
    try:
        base = (np.arange(1 << 20, dtype=np.int64) * 2654435761 % 21 - 10).astype(np.float32)
        for logn in (24, 30):
            n = 1 << logn
            xs = np.empty(n, np.float32)
            xs.reshape(-1, 1 << 20)[:] = base
            vecs[logn] = {"x": xs, "q1": np.empty(n // 2, np.uint8), "s1": np.empty(n // 64, np.float32),
                          "q2": np.empty(n // 2, np.uint8), "s2": np.empty(n // 64, np.float32)}
            vec[f"n2^{logn}"] = {"n": n}
    except MemoryError as e:
        vec["failed"] = f"MemoryError: {e}"

    best, tried, match, by_threads = None, {}, None, {}
    for threads in counts:
        F.set_threads(threads)
        qA = F.first_touch_copy(d["qA"], rows)          # NUMA placement for this thread count (threads are bound: OMP_PROC_BIND)
        med, mn, mx, runs = med_time(lambda: F.m4_mvm(qA, d["sA"], rows, cols, d["qx"], d["sx"], out=out), 15, 4.0)
        tried[threads] = round(med * 1e3, 3)
        by_threads[threads] = {"s": med, "ms": round(med * 1e3, 3), "ms_min": round(mn * 1e3, 3), "ms_max": round(mx * 1e3, 3), "runs": runs}
        if best is None or med < best[0]:
            best = (med, threads, mn, mx, runs)
        if match is None:
            match = bool(np.array_equal(out[0], d["r"]) and np.array_equal(out[1].view(np.uint32), d["sr"].view(np.uint32)))
        del qA
        if threads not in vec_counts:
            continue
        for logn, v in vecs.items():
            n, ent = 1 << logn, vec[f"n2^{logn}"]
            reps, secs = (9, 1.0) if logn == 24 else (3, 2.0)
            name = "sequential" if threads == 1 else "all_cores"
            tq, _, _, rq = med_time(lambda: F.v4_quantize_into(v["x"], v["q1"], v["s1"]), reps, secs, 2)
            if threads == 1:
                F.v4_quantize_into(v["x"][::-1].copy() if logn == 24 else v["x"], v["q2"], v["s2"])
                td, _, _, rd = med_time(lambda: F.v4_dot(v["q1"], v["s1"], v["q2"], v["s2"]), reps, secs, 2)
                order = "the reference's dot: 2 x 8 sequential fma chains (bit-exact order)"
            else:
                td, _, _, rd = med_time(lambda: F.v4_dot_parallel(v["q1"], v["s1"], v["q2"], v["s2"]), reps, secs, 2)
                order = "dot_parallel: block pairs split over threads + reduction (tolerance-only, as in the reference)"
            for key, t_, r_, nb, extra in ((f"quantize_{name}", tq, rq, 4.5625 * n, {}), (f"dot_{name}", td, rd, 1.125 * n, {"order": order})):
                cand = {"value": round(nb / t_ / 1e9, 2), "unit": "GB/s", "threads": threads, "ms": round(t_ * 1e3, 3), "runs": r_, **extra}
                if key not in ent or cand["value"] > ent[key]["value"]:
                    ent[key] = cand
    dot = None
    if "dot_sequential" in vec.get("n2^24", {}):
        dot = {"n": 1 << 24, "seconds": vec["n2^24"]["dot_sequential"]["ms"] / 1e3}
    print(json.dumps({"seconds": best[0], "threads": best[1], "min_s": best[2], "max_s": best[3], "runs": best[4], "median_ms_by_threads": tried, "by_threads": by_threads,
                      "runnable_cpus": runnable, "gpu_result_matches_cpu": match, "dot": dot, "vector_ops": vec}))


def run_cpu_baseline(hip, A, sA, x, sx, r, sr, rows_total: int, cols: int, sample_rows: int) -> dict:
    import numpy as np
    sample_rows = min(sample_rows, rows_total)
    hb = cols // 64
    data = {
        "rows": sample_rows, "cols": cols,
        "qA": A[: sample_rows * cols // 2].cpu().numpy(), "sA": sA[: (sample_rows // 64) * hb].cpu().numpy(),
        "qx": x.cpu().numpy(), "sx": sx.cpu().numpy(),
        "r": r[: sample_rows // 2].cpu().numpy(), "sr": sr[: sample_rows // 64].cpu().numpy(),
    }
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "sample.npz")
        np.savez(path, **data)
        env = dict(os.environ, OMP_PROC_BIND="true", OMP_WAIT_POLICY="active")
        env.pop("OMP_NUM_THREADS", None)
        out = subprocess.run([sys.executable, __file__, "--cpu-baseline-child", path], env=env, check=True,
                             capture_output=True, text=True, timeout=600).stdout
    res = json.loads(out.strip().splitlines()[-1])
    nbytes = mvm_bytes(sample_rows, cols)
    quota = "no cgroup cpu quota"
    try:
        mx, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if mx != "max":
            quota = f"cgroup cpu quota {int(mx) / int(period):g} cpus (short bursts run wider)"
    except (OSError, ValueError):
        pass
    cpu_model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                cpu_model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    # the cgroup quota is what the process may use ON AVERAGE; a team wider than it runs in bursts and gets throttled (ms_max).  Both are
    # reported: the best thread count overall (`value`) and the widest team that stays inside the quota (`within_quota`)
    quota_cpus = None
    try:
        mxq, period = open("/sys/fs/cgroup/cpu.max").read().split()
        quota_cpus = None if mxq == "max" else int(mxq) / int(period)
    except (OSError, ValueError):
        pass
    bt = {int(k): v for k, v in (res.get("by_threads") or {}).items()}
    for v in bt.values():
        v["GB/s"] = round(nbytes / v.pop("s") / 1e9, 3)
    inside = [t for t in bt if quota_cpus is None or t <= quota_cpus]
    within = None
    if inside:
        tq = min(inside, key=lambda t: bt[t]["ms"])
        within = {"threads": tq, **bt[tq], "note": "best team no wider than the cgroup cpu quota" if quota_cpus else "no quota: same as value"}
    # `value`: under a cgroup cpu quota the SUSTAINED figure -- the best team no wider than the quota (stable to 1 % over the rounds: 97-98 GB/s with
    # 16 threads) -- because a wider team only runs in bursts until the quota throttles it: its median moved 136 -> 462 -> 297 -> 169 -> 279 GB/s
    # from run to run.  The best burst stays beside it (`burst_best`); without a quota the two are the same team.
    best_any = {"value": round(nbytes / res["seconds"] / 1e9, 3), "threads": res["threads"], "ms": round(res["seconds"] * 1e3, 3),
                "ms_min": round(res["min_s"] * 1e3, 3), "ms_max": round(res["max_s"] * 1e3, 3),
                "note": "best median over all team sizes; wider than the quota = short bursts, not sustainable"}
    head = within if (within and quota_cpus) else None
    return {
        "value": head["GB/s"] if head else best_any["value"], "unit": "GB/s", "cores": head["threads"] if head else res["threads"], "kind": "port",
        "value_is": ("best team within the cgroup cpu quota (sustained)" if head else "best team (no cpu quota)"), "burst_best": best_any,
        "within_quota": within, "quota_cpus": quota_cpus, "by_threads": {str(k): v for k, v in sorted(bt.items())},
        "sample": f"mvm of {'ALL' if sample_rows == rows_total else 'the first'} {sample_rows} rows x {cols} cols of the same matrix ({nbytes} B), median of <=15 runs, "
                  f"AVX2+OpenMP restatement with the reference's vpmaddubsw instruction mix (oracle/clover4_fast.c, bound threads, NUMA "
                  f"first-touch placement, teams of 1/16/64/half/all threads) on {cpu_model}, {os.cpu_count()} cpus, "
                  f"{res.get('runnable_cpus')} runnable by this process, {quota}",
        "ms": head["ms"] if head else round(res["seconds"] * 1e3, 3), "ms_min": head["ms_min"] if head else round(res["min_s"] * 1e3, 3),
        "ms_max": head["ms_max"] if head else round(res["max_s"] * 1e3, 3), "runs": head["runs"] if head else res["runs"],
        "threads_used": head["threads"] if head else res["threads"], "runnable_cpus": res.get("runnable_cpus"), "cgroup": quota,
        "median_ms_by_threads": res.get("median_ms_by_threads"), "gpu_result_matches_cpu": res["gpu_result_matches_cpu"],
        **({"dot": {"value": round(1.125 * res["dot"]["n"] / res["dot"]["seconds"] / 1e9, 3), "unit": "GB/s", "cores": 1,
                    "sample": f"CloverVector4::dot order (sequential, as the reference's dot), n = {res['dot']['n']}, median"}}
           if res.get("dot") else {}),
        "vector_ops": {**(res.get("vector_ops") or {}),
                       "what": "BASELINE configs[1] on the host: CloverVector4 quantize (rounding disabled) and dot, sequential = the reference's "
                               "quantize / dot on one core, all_cores = quantize_parallel / dot_parallel's split, the better of 16 and 64 bound "
                               "threads; bytes as 01_measure.h:644, 717, 804 (dot 1.125 n, quantize 4.5625 n); the reference published "
                               "7.7 / 18.8 GB/s (quantize, 1 / 4 threads) and 15.0 / 24.4 GB/s (dot) at n = 2^24 on its 4-core box "
                               "(performance.txt:78, 109, 171, 202)"},
    }


# ----------------------------------------------------------------------------------------------------
def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=500,
                    help=f"timed steps of the headline (ms_per_step = their wall time / K); the cold pass in front of them and the side "
                         f"measurements of --full -- the c5 object, the product's loops -- time min(K, {SIDE_STEPS}) steps each, so that K alone "
                         f"sets the run's length")
    ap.add_argument("--warmup", type=int, default=None, help="untimed steps before the timed ones (default 20; 80 for --workload gemm: the matrix "
                                                               "pipe's clocks settle after about 50 calls)")
    ap.add_argument("--rows-per-gpu", type=int, default=65536)
    ap.add_argument("--preset", choices=("c3", "c5-weak", "c5-strong"), default=None,
                    help="default (no preset): the headline is c3 -- 65536 x 65536 per GPU, weak scaling (BASELINE configs[2] at N=1) -- and with "
                         "--full the SAME line carries a `c5` object timed right behind it: BASELINE configs[4], the 2^20 x 2^16 matrix row-sharded "
                         "over the N GPUs (2^20 / N rows each, CloverMatrix4.h:1700-1705's split).  c3 / c5-weak (131072 x 65536 per GPU = configs[4] "
                         "at N=8) / c5-strong (configs[4] split over the N GPUs as the headline): one configuration, no c5 object")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beside the headline, on the same line: ms_per_step_cold (the cold pass runs in every run, as the "
                         "start of the warm-up; --full reports it), the c5 object, the product's "
                         "own multi-GPU loops (one_process, gemm_sharded), for N > 1 the blocking gather time and the check of the gathered result, "
                         "for N = 1 the gemm and extras objects, and the CPU baseline; the --no-* options below leave parts out.  Off by default: "
                         "a plain run sets up, warms up, times the K steps, writes --dump-outputs and prints the line")
    ap.add_argument("--no-c5", action="store_true", help="leave the c5 object out of a --full run without --preset")
    ap.add_argument("--cols", type=int, default=65536)
    ap.add_argument("--cpu-sample-rows", type=int, default=65536,
                    help="rows of the matrix the CPU baseline of --full multiplies (default: all 65536 rows of C3 = 2 GiB of nibbles: beyond the "
                         "2 x 256 MB of L3 of the host, so the number is a DRAM number like the reference's)")
    ap.add_argument("--workload", choices=("mvm", "gemm"), default="mvm",
                    help="mvm (default): the headline GEMV of BASELINE configs[2]; gemm: configs[3], one GPU, its own JSON line")
    ap.add_argument("--gemm-size", type=int, default=8192)
    ap.add_argument("--mode", choices=("ranks", "one-process"), default="ranks",
                    help="how N > 1 GPUs are driven.  ranks (default): one process per GPU under torch.distributed (backend nccl = RCCL); when "
                         "no launcher set WORLD_SIZE, bench.py starts torch.distributed.run itself.  one-process: this process drives all N "
                         "devices through the C ABI's clm4_sharded_* loop calls (RCCL all-gather on a second stream per device)")
    ap.add_argument("--event-every", type=int, default=0,
                    help="HIP event pair around every Nth timed step; the kernel average (roofline) comes from the sampled steps.  Default 0 = "
                         "auto: steps // 8 clamped to [1, 8].  An event pair puts two barrier packets into the queue, which keeps a launch from "
                         "overlapping its predecessor's drain: with a pair around EVERY step the timed loop ran 0.336 ms per step, with none "
                         "0.3285 ms -- less than the 0.3307 ms the events themselves report for the kernel (rocprofv3: 0.3278)")
    ap.add_argument("--settle-ms", type=float, default=60.0,
                    help="untimed launches of the same step for this many milliseconds BEFORE the W warm-up steps: after an idle period the chip "
                         "needs ~20-30 ms of work to reach its steady clocks (the driver's --warmup 5 is 1.6 ms: the 20 timed steps behind it ran "
                         "0.349 ms per step against 0.330 in steady state).  Reported in the JSON; 0 switches it off")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="leave the CPU baseline out of a --full run")
    ap.add_argument("--no-extras", action="store_true", help="leave the gemm and extras objects out of a --full run")
    ap.add_argument("--no-one-process", action="store_true",
                    help="leave out of a --full run the `one_process` and `gemm_sharded` objects (the product's clm4_sharded_* loops over the "
                         "same N devices, driven by rank 0 behind the ranks' timed regions)")
    ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                    help="after the timed steps, write what the timed path computed in its last step to DIR/<name>.npy (float32 / float64, "
                         f"at most {DUMP_LIMIT_BYTES >> 20} MB in all; a fixed, seeded sample of a larger output).  The inputs are seeded: the "
                         "same arguments give the same inputs on every run, so two builds can be compared output for output")
    ap.add_argument("--cpu-baseline-child", type=str, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--gemm-probe-child", type=str, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--product-loops-child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.dump_outputs and args.mode == "one-process":
        raise SystemExit("bench.py --dump-outputs: supported for the mvm path in --mode ranks and for --workload gemm")
    if args.warmup is None:
        args.warmup = 80 if args.workload == "gemm" else 20
    if args.event_every <= 0:
        args.event_every = max(1, min(8, args.steps // 8))
    if args.product_loops_child:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        return product_loops_child(args, args.product_loops_child)
    if args.gemm_probe_child:
        return gemm_probe_child(args.gemm_probe_child, args.gemm_size)
    if args.workload == "gemm":
        return gemm_main(args)

    if args.cpu_baseline_child:
        cpu_baseline_child(args.cpu_baseline_child)
        return

    # the host driver of these boxes only supports dmabuf IPC: without this RCCL's cross-process buffer sharing fails with
    # `hipIpcGetMemHandle: invalid argument`.  The environment exports it already; keep it even when a launcher drops it.
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

    import numpy as np
    import torch
    import torch.distributed as dist

    from clover_amd.lib_binding import DOT_EXACT, DOT_FAST, CloverHip
    from clover_amd.sharding import gather_packed, gather_packed_async, packed_bytes, partition_rows, unpack_gathered

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    launched = "WORLD_SIZE" in os.environ              # torch.distributed.run (the driver's, or our own below) set the rank env
    if not launched and (args.gpus > 1 or args.mode == "one-process"):
        need = 1 if os.environ.get("CLOVER_BENCH_DEBUG_ONE_GPU") == "1" else args.gpus
        have = torch.cuda.device_count()
        if have < need:
            raise SystemExit(f"bench.py --gpus {args.gpus}: this box shows {have} GPU(s) (torch.cuda.device_count()), {need} needed "
                             f"-- a device-count problem, not a launcher problem: bench.py starts its own ranks")
        if args.mode == "one-process":
            return one_process_main(args, torch, CloverHip)
        return self_launch(args)
    if launched and args.mode == "one-process":
        raise SystemExit("bench.py --mode one-process drives all GPUs from ONE process: run it without torch.distributed.run")
    if world != args.gpus:
        args.gpus = world
    # CLOVER_BENCH_DEBUG_ONE_GPU=1: rehearsal of the N>1 control flow on a box with ONE GPU -- every rank uses device 0 and the
    # exchange goes through gloo and the host.  Never a measurement: the output says so.
    debug_one_gpu = world > 1 and os.environ.get("CLOVER_BENCH_DEBUG_ONE_GPU") == "1"
    # CLOVER_BENCH_FORCE_DIST=1 (under a launcher, any world size incl. 1): take the N > 1 code path -- process groups, RCCL sub-group,
    # per-step all-gather -- even with one rank, so that the very calls an 8-GPU run makes execute on a one-GPU box (tests)
    dist_on = world > 1 or (launched and os.environ.get("CLOVER_BENCH_FORCE_DIST") == "1")
    dev_index = 0 if debug_one_gpu else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    red_dev = torch.device("cpu")                    # control plane (timing maxima, flags, barriers): always gloo on the host
    data_group, data_backend, nccl_error = None, "gloo", None
    if dist_on:
        # one node, rendezvous on 127.0.0.1: keep gloo on the loopback interface (a container hostname that does not resolve would
        # otherwise stop it before the first collective)
        if os.environ.get("MASTER_ADDR", "127.0.0.1") in ("127.0.0.1", "localhost"):
            os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
        # gloo announces its connections with printf ("[Gloo] Rank 0 is connected to 1 peer ranks ...") on STDOUT, where the contract wants
        # exactly one JSON line: file descriptor 1 points at stderr while the groups are built
        sys.stdout.flush()
        saved_fd = os.dup(1)
        os.dup2(2, 1)
        try:
            dist.init_process_group("gloo")
            dist.barrier()
        finally:
            sys.stdout.flush()
            os.dup2(saved_fd, 1)
            os.close(saved_fd)
        if not debug_one_gpu:
            # data plane: an RCCL (backend "nccl") group for the per-step all-gather.  If it cannot be built or its first collective
            # fails on ANY rank, every rank falls back to gloo through the host for the 72 KiB exchange -- slower, reported as such, but
            # a scaling run still produces its line (the ranks agree on the outcome over the gloo group)
            ok = 1
            try:
                data_group = dist.new_group(backend="nccl")
                probe = torch.ones(1, dtype=torch.float32, device=dev)
                dist.all_reduce(probe, group=data_group)
                torch.cuda.synchronize()
                ok = int(float(probe.item()) == float(world))
            except Exception as e:                       # noqa: BLE001 -- whatever RCCL raises, the answer is the fallback
                ok, nccl_error = 0, f"{type(e).__name__}: {e}"[:300]
            flag = torch.tensor([ok], dtype=torch.int32)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            if int(flag.item()) == 1:
                data_backend = "nccl"
            else:
                data_group = None
    # tests: CLOVER_BENCH_FORCE_GLOO_FALLBACK=1 takes the "RCCL group could not be built" branch on purpose, so that the degraded line an
    # 8-GPU run would print after an RCCL failure is seen (and asserted) before it ever matters
    if dist_on and not debug_one_gpu and os.environ.get("CLOVER_BENCH_FORCE_GLOO_FALLBACK") == "1":
        data_group, data_backend, nccl_error = None, "gloo", "forced by CLOVER_BENCH_FORCE_GLOO_FALLBACK=1 (test)"
    host_exchange = dist_on and data_backend == "gloo"       # the packed result travels through host memory
    degraded = host_exchange                                  # every timed step then carries a device->host copy + a gloo all-gather

    hip = CloverHip(device=dev_index)                # raises if libclover_hip.so is missing: no fallback
    lib = hip.lib
    stream = torch.cuda.current_stream().cuda_stream
    seed = 0xC10FE4
    cols = args.cols
    assert cols % 128 == 0
    hb = cols // 64

    scaling = "weak"
    preset = args.preset or "c3"
    if preset == "c5-weak":
        args.rows_per_gpu = 131072
    elif preset == "c5-strong":
        assert (1 << 20) % (64 * world) == 0
        args.rows_per_gpu, scaling = (1 << 20) // world, "strong"

    x = torch.empty(cols // 2, dtype=torch.uint8, device=dev)
    sx = torch.empty(hb, dtype=torch.float32, device=dev)
    hip.check(lib.clv_fill_random_nibbles(x.data_ptr(), x.numel(), seed + 2, 0, stream))
    hip.check(lib.clv_fill_random_scales(sx.data_ptr(), sx.numel(), seed + 3, 0, stream))

    def time_config(rows: int, cold_first: bool, steps: int) -> dict:
        """One row-sharded mvm configuration: this rank's `rows` rows of a (rows * world) x cols matrix, generated in HBM, then
        [cold_first: W warm-up + min(K, SIDE_STEPS) timed steps straight away], the clock settle, W warm-up steps and the K = `steps`
        timed steps.  Both timed regions are bracketed by barrier + synchronize, their wall time is the max over ranks."""
        assert rows % 64 == 0
        rows_total = rows * world
        # ---- synthetic operands, resident in HBM (quantised domain: nibbles U[-7,7], scales U[0.5,2)) ----
        A = torch.empty(rows * cols // 2, dtype=torch.uint8, device=dev)
        sA = torch.empty((rows // 64) * hb, dtype=torch.float32, device=dev)
        hip.check(lib.clv_fill_random_nibbles(A.data_ptr(), A.numel(), seed, rank * rows * cols // 2, stream))
        hip.check(lib.clv_fill_random_scales(sA.data_ptr(), sA.numel(), seed + 1, rank * (rows // 64) * hb, stream))
        # packed result of this rank: [rows/2 nibble bytes | rows/64 fp32 scales]; gathered as one buffer
        assert partition_rows(rows_total, world, rank) == (rank * rows, rows)     # equal contiguous shards
        # two result buffers: while the gather of step i is in flight on RCCL's stream, step i+1 writes the other one
        res_bufs = [torch.empty(packed_bytes(rows), dtype=torch.uint8, device=dev) for _ in range(2)]
        res = res_bufs[0]
        pending = [None, None]
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]

        def step(i: int | None, n: int) -> None:
            buf = res_bufs[n & 1]
            if pending[n & 1] is not None:            # the gather that last read this buffer must be done before it is overwritten
                pending[n & 1].wait()
                pending[n & 1] = None
            timed = i is not None and i % args.event_every == 0
            if timed:
                ev[i][0].record()
            hip.check(lib.clm4_mvm(A.data_ptr(), sA.data_ptr(), rows, cols, x.data_ptr(), sx.data_ptr(), buf.data_ptr(),
                                   buf.data_ptr() + rows // 2, None, stream))
            if timed:
                ev[i][1].record()
            if dist_on:                               # RCCL all-gather of [nibbles | scales] from every rank, overlapping the next step
                pending[n & 1] = gather_packed_async(buf.cpu() if host_exchange else buf, rows_total, group=data_group)

        def drain() -> None:                          # every gather has landed (the stream waits; synchronize() follows)
            for j in (0, 1):
                if pending[j] is not None:
                    pending[j].wait()
                    pending[j] = None

        def timed_region(k: int) -> tuple[float, float]:
            """W untimed + k timed steps -> (wall seconds of the k steps, max over ranks; kernel ms from the sampled event pairs, this rank)"""
            for w_ in range(args.warmup):
                step(None, w_)
            drain()
            torch.cuda.synchronize()
            if dist_on:
                dist.barrier()
            t0 = time.perf_counter()
            for i in range(k):
                step(i, i)
            drain()
            torch.cuda.synchronize()
            if dist_on:
                dist.barrier()
            el = time.perf_counter() - t0
            t = torch.tensor([el], dtype=torch.float64, device=red_dev)
            if dist_on:
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
            km = [a.elapsed_time(b) for i, (a, b) in enumerate(ev[:k]) if i % args.event_every == 0]
            return float(t.item()), sum(km) / len(km)

        torch.cuda.synchronize()
        cold_steps = min(steps, SIDE_STEPS)
        cold = timed_region(cold_steps) if cold_first else None
        # clock settle (untimed, reported): the same step, back to back, until --settle-ms of work have been issued
        # (a launch COUNT derived from the shape, not a wall-clock loop: with N > 1 every step carries a collective, so all ranks must issue
        #  the same number of them)
        settle_launches = 0
        if args.settle_ms > 0:
            est_ms = mvm_bytes(rows, cols) / 6.0e12 * 1e3                      # one launch at ~6 TB/s
            settle_target = min(256, max(8, int(args.settle_ms / est_ms + 7) // 8 * 8))        # small test shapes: capped
            while settle_launches < settle_target:
                for _ in range(8):
                    step(None, settle_launches)
                    settle_launches += 1
                drain()
                torch.cuda.synchronize()
        elapsed, kern_mine = timed_region(steps)
        kt = torch.tensor([kern_mine], dtype=torch.float64, device=red_dev)
        if dist_on:
            dist.all_reduce(kt, op=dist.ReduceOp.MAX)
        r = {"rows": rows, "rows_total": rows_total, "elapsed": elapsed, "kern_avg_ms": float(kt.item()), "kern_samples": len(range(0, steps, args.event_every)),
             "settle_launches": settle_launches, "cold": cold, "cold_steps": cold_steps, "per_rank_kernel_ms": None, "gather_us": None, "gather_ok": None,
             "A": A, "sA": sA, "res": res, "last": res_bufs[(steps - 1) & 1]}
        if dist_on:
            pr = [torch.zeros(1, dtype=torch.float64, device=red_dev) for _ in range(world)]
            dist.all_gather(pr, torch.tensor([kern_mine], dtype=torch.float64, device=red_dev))
            r["per_rank_kernel_ms"] = [round(float(v.item()), 5) for v in pr]
        if dist_on and args.full:
            # the exchange alone, outside the timed region: K blocking all-gathers of the packed result
            reps = 50
            dist.barrier()
            torch.cuda.synchronize()
            g0 = time.perf_counter()
            for _ in range(reps):
                gather_packed(res.cpu() if host_exchange else res, rows_total, group=data_group)
            torch.cuda.synchronize()
            gt = torch.tensor([(time.perf_counter() - g0) / reps * 1e6], dtype=torch.float64, device=red_dev)
            dist.all_reduce(gt, op=dist.ReduceOp.MAX)
            r["gather_us"] = round(float(gt.item()), 1)
            # outside the timed region: every rank finds its own shard, bit for bit, at its place in the gathered vector
            g = gather_packed(res.cpu() if host_exchange else res, rows_total, group=data_group)
            nib, sc = unpack_gathered(g, rows_total, world)
            mine = res.cpu() if host_exchange else res
            ok = bool(torch.equal(nib[rank * rows // 2: (rank + 1) * rows // 2], mine[: rows // 2])) and \
                bool(torch.equal(sc[rank * rows // 64: (rank + 1) * rows // 64], mine[rows // 2:].view(torch.float32)))
            okt = torch.tensor([1 if ok else 0], dtype=torch.int32, device=red_dev)
            dist.all_reduce(okt, op=dist.ReduceOp.MIN)
            r["gather_ok"] = bool(okt.item())
        return r

    rows = args.rows_per_gpu
    # the cold pass runs in every run: its W + min(K, SIDE_STEPS) steps (about 10 ms at C3) are the start of the warm-up that the settled
    # steps have always been timed behind; only --full reports them (ms_per_step_cold)
    head = time_config(rows, cold_first=True, steps=args.steps)
    rows_total = head["rows_total"]
    if args.dump_outputs:
        # the result vector of the last timed step as the caller receives it: with N > 1 the all-gathered whole (untimed, every rank takes part)
        last = head.pop("last")
        if dist_on:
            nib, sc = unpack_gathered(gather_packed(last.cpu() if host_exchange else last, rows_total, group=data_group), rows_total, world)
        else:
            nib, sc = last[: rows // 2], last[rows // 2:].view(torch.float32)
        if rank == 0:
            nib, sc = nib.cpu().numpy(), sc.cpu().numpy()
            blocks = rows_total // 64
            keep = blocks if blocks * (64 * 8 + 4) <= DUMP_LIMIT_BYTES // 2 else (DUMP_LIMIT_BYTES // 2) // (64 * 8 + 4 + 8)
            dump = {}
            if keep < blocks:                                    # a fixed, seeded sample of whole 64-row blocks
                idx = np.sort(np.random.default_rng(0xD0).choice(blocks, keep, replace=False))
                nib = nib.reshape(blocks, 32)[idx].reshape(-1)
                sc = sc[idx]
                dump["mvm_result_block_index"] = idx.astype(np.float64)
            dump.update({f"mvm_result_{k}": v for k, v in decode_v4(nib, sc).items()})
            write_outputs(args.dump_outputs, dump)
    head.pop("last", None)
    rccl_ranks = (dist.get_world_size(data_group) if data_backend == "nccl" else 0) if dist_on else None

    # BASELINE configs[4] in the same line: the 2^20 x 2^16 matrix row-sharded over the N ranks (2^20 / N rows each: strong scaling; 32 GiB
    # fit one GPU, so N = 1 carries it too).  Only when no --preset was asked for: the presets time one configuration each.
    c5 = None
    c5_total = int(os.environ.get("CLOVER_BENCH_C5_ROWS", str(1 << 20)))       # tests shrink it; the object says so
    if args.full and args.preset is None and not args.no_c5:
        if c5_total % (64 * world) != 0:
            c5 = {"skipped": f"{c5_total} rows do not split into {world} equal shards of whole 64-row blocks"}
        else:
            head_A, head_sA, head_res = head.pop("A"), head.pop("sA"), head.pop("res")
            keep_for_cpu = rank == 0 and not args.no_cpu_baseline
            if not keep_for_cpu:
                del head_A, head_sA
            torch.cuda.empty_cache()
            c5_steps = min(args.steps, SIDE_STEPS)
            c5r = time_config(c5_total // world, cold_first=False, steps=c5_steps)
            c5r.pop("A"), c5r.pop("sA"), c5r.pop("res"), c5r.pop("last")
            torch.cuda.empty_cache()
            if keep_for_cpu:
                head["A"], head["sA"] = head_A, head_sA
            head["res"] = head_res
            b_tot, b_gpu = mvm_bytes(c5_total, cols), mvm_bytes(c5_total // world, cols)
            ms5 = c5r["elapsed"] / c5_steps * 1e3
            ach5 = b_gpu / (c5r["kern_avg_ms"] * 1e-3) / 1e9
            c5 = {
                "workload": f"CloverMatrix4::mvm {c5_total}x{cols} int4 row-sharded {world} way(s), {c5_total // world} rows per GPU"
                            + (" = BASELINE configs[4]" if (c5_total, cols) == (1 << 20, 65536) else " (NOT configs[4]: shrunk by CLOVER_BENCH_C5_ROWS / --cols)"),
                "scaling": "strong", "n_gpus": world, "rows_per_gpu": c5_total // world, "cols": cols, "steps": c5_steps, "warmup": args.warmup,
                "settle_launches": c5r["settle_launches"],
                "ms_per_step": round(ms5, 5), "value": round(b_tot / (ms5 * 1e-3) / 1e9, 2), "unit": "GB/s",
                "frac": round(b_tot / (ms5 * 1e-3) / 1e9 / (world * HBM_PEAK_GBS), 4), "frac_of": f"{world} x {HBM_PEAK_GBS:g} GB/s",
                "algorithmic_bytes_per_step": b_tot, "algorithmic_bytes_per_launch": b_gpu,
                "kernel_avg_ms": round(c5r["kern_avg_ms"], 5), "kernel_frac": round(ach5 / HBM_PEAK_GBS, 4),
                "kernel_only_aggregate_GBs": round(world * ach5, 2),
                "per_rank_kernel_ms": c5r["per_rank_kernel_ms"], "gather_us_blocking": c5r["gather_us"],
                "gather_bytes_per_rank": packed_bytes(c5_total // world), "gathered_result_verified": c5r["gather_ok"],
                **({"backend": data_backend, "rccl_ranks": rccl_ranks} if dist_on else {}),
                **({"degraded": True} if degraded else {}),
            }

    if rank != 0:
        dist.barrier()                                           # pairs with rank 0's barrier in front of its one-process loops
        dist.destroy_process_group()
        return

    elapsed, kern_avg_ms, settle_launches = head["elapsed"], head["kern_avg_ms"], head["settle_launches"]
    per_rank_kernel_ms, gather_us, gather_ok = head["per_rank_kernel_ms"], head["gather_us"], head["gather_ok"]
    ms_per_step = elapsed / args.steps * 1e3
    cold = head["cold"] if args.full else None
    ms_cold = cold[0] / head["cold_steps"] * 1e3 if cold else None
    bytes_total = mvm_bytes(rows_total, cols)
    bytes_gpu = mvm_bytes(rows, cols)
    value = bytes_total / (ms_per_step * 1e-3) / 1e9
    achieved = bytes_gpu / (kern_avg_ms * 1e-3) / 1e9

    out = {
        "metric": "int4 GEMV (CloverMatrix4::mvm) effective GB/s, algorithmic operand bytes / time",
        "value": round(value, 2), "unit": "GB/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 5),
        # --full: the first min(K, SIDE_STEPS) steps, measured FIRST, behind nothing but the data fill and the W warm-up steps (no clock settle)
        **({"ms_per_step_cold": round(ms_cold, 5), "value_cold": round(bytes_total / (ms_cold * 1e-3) / 1e9, 2)} if cold else {}),
        "higher_is_better": True, "scaling": scaling, "vs_baseline": None,
        "dtype": "int4", "data": "synthetic",
        # degraded: the RCCL group could not be used and every timed step carried a device->host copy + a gloo all-gather: `value` is NOT
        # a scaling number then; the kernel-only aggregate is what the GPUs did
        **({"degraded": True, "degraded_why": ("CLOVER_BENCH_DEBUG_ONE_GPU rehearsal" if debug_one_gpu else
                                                 f"RCCL unavailable ({nccl_error or 'the RCCL group failed on another rank'}): exchange through gloo and host memory"),
            "value_kernel_only": round(world * achieved, 2)} if degraded else {}),
        "config": {
            "workload": f"CloverMatrix4::mvm {rows_total}x{cols} int4 ({rows}x{cols} per GPU; preset {preset}: BASELINE "
                        f"{'configs[2] per GPU' if preset == 'c3' else 'configs[4]' + (' at N=8' if preset == 'c5-weak' else '')}), "
                        f"x and result CloverVector4, STOCHASTIC_ROUNDING_DISABLED, bit-exact reference order",
            "rows_per_gpu": rows, "cols": cols, "parallelism": f"row-shard x{world}" + (" + all-gather of every step's packed result, overlapped with the next step" if dist_on else ""),
            "settle_launches": settle_launches, "settle_ms": args.settle_ms,
            **({**({"gathered_result_verified": gather_ok} if args.full else {}), "rccl_ranks": rccl_ranks, "backend": data_backend,
                **({"nccl_fallback_reason": nccl_error or "the RCCL group failed on another rank"} if host_exchange and not debug_one_gpu else {}),
                "per_rank_kernel_ms": per_rank_kernel_ms, **({"gather_us_blocking": gather_us} if args.full else {}),
                "gather_bytes_per_rank": packed_bytes(rows)} if dist_on else {}),
            **({"mode": "ranks", "launcher": os.environ.get("CLOVER_BENCH_LAUNCHER", "external torch.distributed.run")} if dist_on else {}),
            **({"DEBUG": "CLOVER_BENCH_DEBUG_ONE_GPU rehearsal: all ranks on one GPU, gloo through the host -- not a measurement"} if debug_one_gpu else {}),
            "gflops": round(2.0 * rows_total * cols / (ms_per_step * 1e-3) / 1e9, 1),
            "algorithmic_bytes_per_step": bytes_total,
            "clock_settle": f"{settle_launches} untimed launches of the same step ({args.settle_ms:g} ms) before the {args.warmup} warm-up steps "
                            "(steady clocks need 20-30 ms of work after idle); the K timed steps and their barriers are unchanged"
                            + (f"; ms_per_step_cold = the first min(K, {SIDE_STEPS}) = {head['cold_steps']} of the same steps, measured before any of that"
                               if cold else ""),
            "arithmetic": "int4 x int4 products summed exactly per 32-bit word (v_dot8_i32_i4), fp32 per-block scale + fma chains in reference order",
        },
        "roofline": {
            "bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": None,
            "kernel": "k_m4_mvm64", "kernel_avg_ms": round(kern_avg_ms, 5), "algorithmic_bytes_per_launch": bytes_gpu,
            **({"kernel_avg_ms_cold": round(cold[1], 5)} if cold else {}),
            "kernel_avg_of": f"HIP event pairs around every {args.event_every}. timed step ({head['kern_samples']} launches) on the launch stream",
        },
    }
    if c5 is not None:
        out["c5"] = c5

    tr = pmc_traffic(rows, cols)
    if tr:
        out["roofline"]["traffic"] = tr[0]
        out["roofline"]["traffic_source"] = f"profiles/{tr[1]} (FETCH_SIZE x1024 x2 gfx950 correction + WRITE_SIZE x1024, per launch)"

    # --full: the product's own multi-GPU loops, timed by the same command: rank 0 -- the other ranks have left their timed regions
    # and are idle or gone -- drives all N devices through the C ABI: `one_process` = clm4_sharded_mvm_enqueue over the same shards (c3
    # headline + c5), `gemm_sharded` = configs[3] split by rows of A with the C row panels all-gathered
    if dist_on:
        dist.barrier()                                           # every rank is past its last kernel and collective
        dist.destroy_process_group()                             # torch's RCCL communicators are gone before the product builds its own
    if args.full and not args.no_one_process:
        if world == 1 or debug_one_gpu or torch.cuda.device_count() >= world:
            torch.cuda.empty_cache()
            out.update(run_product_loops(args, world))
        else:                                                    # a launcher that shows every rank its own device only
            why = {"skipped": f"rank 0 sees {torch.cuda.device_count()} device(s), the one-process loops need all {world}"}
            out.update({"one_process": why, "gemm_sharded": dict(why)})

    # side measurements first, while the chip is warm from the timed loop (the matrix pipe's clocks need ~50 calls to settle after an idle
    # period, and the CPU baseline below leaves the GPU idle for half a minute: round 3 measured the GEMM 5 % slower behind it)
    if args.full and world == 1 and not args.no_extras:
        for key, fn in (("gemm", gemm_object), ("extras", extras)):      # side measurements must never cost the headline line
            try:
                out[key] = fn(hip, torch, dev, stream)
            except Exception as e:
                out[key] = {"failed": f"{type(e).__name__}: {e}"}

    if args.full and not args.no_cpu_baseline:                    # rank 0's own shard (the whole C3 matrix by default), at every N
        try:
            res = head["res"]
            out["cpu_baseline"] = run_cpu_baseline(hip, head["A"], head["sA"], x, sx, res[: rows // 2], res[rows // 2:].view(torch.float32),
                                                   rows_total, cols, args.cpu_sample_rows)
        except Exception as e:                                   # the baseline must never kill the GPU number
            out["cpu_baseline"] = {"value": None, "unit": "GB/s", "cores": 0, "kind": "port", "sample": f"failed: {e}"}

    # dot in the reference's order is a dependent-fma chain: say so next to the host core's time for the same order, so that nobody reads
    # the GPU figure as a win (for n >= 2^20 the bandwidth-bound orders -- CLV_DOT_FAST / dot_parallel -- are the ones to use)
    try:
        de = out["extras"]["footnote_cache_resident_n2^24"]["dot_exact"]
        host = out["cpu_baseline"]["vector_ops"]["n2^24"]["dot_sequential"]
        de["host_one_core_ms_same_order"] = host["ms"]
        de["verdict"] = (f"{de['ms']:.3f} ms on the GPU vs {host['ms']:.3f} ms on one host core for the same bit-exact order: not a speed-up "
                         "(floor 0.30 ms = 131072 dependent fmas); n >= 2^20 should use CLV_DOT_FAST / dot_parallel()")
    except (KeyError, TypeError):
        pass
    print(json.dumps(out))


def self_launch(args) -> None:
    """`python bench.py --gpus N` with N > 1 and no launcher: start the ranks ourselves, exactly as the driver's launcher would
    (`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py <same flags>`),
    pass rank 0's JSON line through on stdout and return the launcher's exit code."""
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"),
               CLOVER_BENCH_LAUNCHER="bench.py self-launch (torch.distributed.run re-exec)")
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(Path(__file__).resolve()), *sys.argv[1:]]
    sys.stdout.flush()
    raise SystemExit(subprocess.run(cmd, env=env).returncode)


def one_process_main(args, torch, CloverHip) -> None:
    """`--mode one-process`: the line of one_process_measure on its own."""
    print(json.dumps(one_process_measure(args, torch, CloverHip(device=0), args.gpus)))


def one_process_measure(args, torch, hip, n: int) -> dict:
    """N GPUs driven by THIS process through the C ABI (clm4_sharded_create / _set_x / _loop_begin / _mvm_enqueue / _sync): the product's
    own multi-GPU path, timed as it would run inside an application loop.  A step = every shard's kernel on its device's compute stream +
    one grouped in-place ncclAllGather pair on its exchange stream (overlapping the next step's kernel); no host synchronisation inside
    the timed region.  CLOVER_BENCH_DEBUG_ONE_GPU=1 lists device 0 N times (exchanges become copies): a rehearsal, not a measurement.
    Without --preset the result also carries the `c5` object (BASELINE configs[4] split N ways), as in ranks mode.  Returns the JSON
    object: printed as the line by --mode one-process, merged as `one_process` into the line of a ranks run (rank 0, after the ranks'
    timed regions -- the other ranks are idle by then)."""
    import ctypes as C

    import numpy as np
    debug = os.environ.get("CLOVER_BENCH_DEBUG_ONE_GPU") == "1"
    lib = hip.lib
    hip.check(lib.clv_set_device(0))
    scaling = "weak"
    preset = args.preset or "c3"
    if preset == "c5-weak":
        args.rows_per_gpu = 131072
    elif preset == "c5-strong":
        assert (1 << 20) % (64 * n) == 0
        args.rows_per_gpu, scaling = (1 << 20) // n, "strong"
    cols = args.cols
    x = torch.empty(cols // 2, dtype=torch.uint8, device="cuda:0")
    sx = torch.empty(cols // 64, dtype=torch.float32, device="cuda:0")
    hip.check(lib.clv_fill_random_nibbles(x.data_ptr(), x.numel(), 0xC10FE4 + 2, 0, None))
    hip.check(lib.clv_fill_random_scales(sx.data_ptr(), sx.numel(), 0xC10FE4 + 3, 0, None))
    torch.cuda.synchronize()

    def time_config(rows: int, steps: int) -> dict:
        rows_total = rows * n
        devs = (C.c_int * n)(*([0] * n if debug else range(n)))
        ctx = C.c_void_p()
        hip.check(lib.clm4_sharded_create(C.byref(ctx), n, devs, rows_total, cols))
        try:
            hip.check(lib.clm4_sharded_fill_random(ctx, 0xC10FE4))
            hip.check(lib.clm4_sharded_set_x(ctx, x.data_ptr(), sx.data_ptr(), 0))
            hip.check(lib.clm4_sharded_loop_begin(ctx, steps))
            settle = 0
            if args.settle_ms > 0:                        # clock settle, as in ranks mode (untimed)
                settle_target = min(256, max(8, int(args.settle_ms / (mvm_bytes(rows, cols) / 6.0e12 * 1e3) + 7) // 8 * 8))
                while settle < settle_target:
                    for _ in range(8):
                        hip.check(lib.clm4_sharded_mvm_enqueue(ctx, settle, 0))
                        settle += 1
                    hip.check(lib.clm4_sharded_sync(ctx))
            for w_ in range(args.warmup):
                hip.check(lib.clm4_sharded_mvm_enqueue(ctx, w_, 0))
            hip.check(lib.clm4_sharded_sync(ctx))
            t0 = time.perf_counter()
            sampled = list(range(0, steps, args.event_every))       # event triples around every Nth step only (see --event-every)
            for i in range(steps):
                hip.check(lib.clm4_sharded_mvm_enqueue(ctx, i, 1 if i % args.event_every == 0 else 0))
            hip.check(lib.clm4_sharded_sync(ctx))
            elapsed = time.perf_counter() - t0
            per_k, per_g = [], []
            km, gm = C.c_float(), C.c_float()
            for d in range(n):
                ks, gs = 0.0, 0.0
                for i in sampled:
                    hip.check(lib.clm4_sharded_step_timing(ctx, d, i, C.byref(km), C.byref(gm)))
                    ks += km.value
                    gs += gm.value
                per_k.append(ks / len(sampled))
                per_g.append(gs / len(sampled))
            ranks, equal = C.c_int(), C.c_int()
            hip.check(lib.clm4_sharded_comm_info(ctx, C.byref(ranks), C.byref(equal)))
            full = []
            if args.full:
                # every device holds the full result, and it equals the unsharded call's (n * 72 KiB: compared on the host)
                last = (steps - 1) & 1
                for d in range(n):
                    rp, sp = C.c_void_p(), C.c_void_p()
                    hip.check(lib.clm4_sharded_result_buf(ctx, d, last, C.byref(rp), C.byref(sp)))
                    rr = np.empty(rows_total // 2, np.uint8)
                    ss = np.empty(rows_total // 64, np.float32)
                    hip.check(lib.clv_set_device(0 if debug else d))
                    hip.check(lib.clv_memcpy_d2h(rr.ctypes.data, rp, rr.nbytes, None))
                    hip.check(lib.clv_memcpy_d2h(ss.ctypes.data, sp, ss.nbytes, None))
                    hip.check(lib.clv_device_sync())
                    full.append((rr, ss))
                hip.check(lib.clv_set_device(0))
        finally:
            lib.clm4_sharded_destroy(ctx)
        base = {"rows": rows, "rows_total": rows_total, "elapsed": elapsed, "per_k": per_k, "per_g": per_g, "rccl_ranks": ranks.value,
                "settle_launches": settle}
        if not args.full:
            return base
        same = all(np.array_equal(full[0][0], f[0]) and np.array_equal(full[0][1].view(np.uint32), f[1].view(np.uint32)) for f in full[1:])
        # shard 0's rows against a plain clm4_mvm of the same (regenerated) rows on device 0 (after the context released its memory)
        A0 = torch.empty(rows * cols // 2, dtype=torch.uint8, device="cuda:0")
        sA0 = torch.empty((rows // 64) * (cols // 64), dtype=torch.float32, device="cuda:0")
        r0 = torch.empty(rows // 2, dtype=torch.uint8, device="cuda:0")
        sr0 = torch.empty(rows // 64, dtype=torch.float32, device="cuda:0")
        hip.check(lib.clv_fill_random_nibbles(A0.data_ptr(), A0.numel(), 0xC10FE4, 0, None))
        hip.check(lib.clv_fill_random_scales(sA0.data_ptr(), sA0.numel(), 0xC10FE4 + 1, 0, None))
        hip.check(lib.clm4_mvm(A0.data_ptr(), sA0.data_ptr(), rows, cols, x.data_ptr(), sx.data_ptr(), r0.data_ptr(), sr0.data_ptr(), None, None))
        torch.cuda.synchronize()
        ok0 = bool(np.array_equal(r0.cpu().numpy(), full[0][0][: rows // 2]) and
                   np.array_equal(sr0.cpu().numpy().view(np.uint32), full[0][1][: rows // 64].view(np.uint32)))
        del A0, sA0, r0, sr0
        torch.cuda.empty_cache()
        return {**base, "verified": bool(same and ok0)}

    rows = args.rows_per_gpu
    h = time_config(rows, args.steps)
    rows_total = h["rows_total"]
    backend = lambda r: "rccl (dlopen, ncclCommInitAll)" if r["rccl_ranks"] else "device copies"       # noqa: E731
    ms_per_step = h["elapsed"] / args.steps * 1e3
    kern_avg_ms = max(h["per_k"])
    bytes_total, bytes_gpu = mvm_bytes(rows_total, cols), mvm_bytes(rows, cols)
    achieved = bytes_gpu / (kern_avg_ms * 1e-3) / 1e9
    degraded = debug or (n > 1 and not h["rccl_ranks"])
    out = {
        "metric": "int4 GEMV (CloverMatrix4::mvm) effective GB/s, algorithmic operand bytes / time",
        "value": round(bytes_total / (ms_per_step * 1e-3) / 1e9, 2), "unit": "GB/s", "n_gpus": n, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 5), "higher_is_better": True, "scaling": scaling, "vs_baseline": None, "dtype": "int4",
        "data": "synthetic",
        **({"degraded": True, "degraded_why": "CLOVER_BENCH_DEBUG_ONE_GPU rehearsal" if debug else "no RCCL communicator: exchanges are device copies",
            "value_kernel_only": round(n * achieved, 2)} if degraded else {}),
        "config": {
            "workload": f"CloverMatrix4::mvm {rows_total}x{cols} int4 ({rows}x{cols} per GPU; preset {preset}), x and result CloverVector4, "
                        "STOCHASTIC_ROUNDING_DISABLED, bit-exact reference order",
            "rows_per_gpu": rows, "cols": cols, "mode": "one-process",
            "parallelism": f"row-shard x{n}, one process drives all devices (clm4_sharded_mvm_enqueue): grouped in-place ncclAllGather pair per "
                           "step on a second stream per device, overlapped with the next step's kernel",
            "settle_launches": h["settle_launches"], "settle_ms": args.settle_ms,
            **({"gathered_result_verified": h["verified"]} if args.full else {}), "rccl_ranks": h["rccl_ranks"], "backend": backend(h),
            "per_rank_kernel_ms": [round(v, 5) for v in h["per_k"]], "gather_ms_behind_kernel": [round(v, 5) for v in h["per_g"]],
            "gather_bytes_per_rank": rows // 2 + rows // 16,
            **({"DEBUG": "CLOVER_BENCH_DEBUG_ONE_GPU rehearsal: all shards on device 0, exchanges are copies -- not a measurement"} if debug else {}),
            "gflops": round(2.0 * rows_total * cols / (ms_per_step * 1e-3) / 1e9, 1), "algorithmic_bytes_per_step": bytes_total,
        },
        "roofline": {"bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                     "traffic": None, "kernel": "k_m4_mvm64", "kernel_avg_ms": round(kern_avg_ms, 5), "algorithmic_bytes_per_launch": bytes_gpu},
    }
    c5_total = int(os.environ.get("CLOVER_BENCH_C5_ROWS", str(1 << 20)))
    if args.full and args.preset is None and not args.no_c5:
        if c5_total % (64 * n) != 0:
            out["c5"] = {"skipped": f"{c5_total} rows do not split into {n} equal shards of whole 64-row blocks"}
        else:
            c5_steps = min(args.steps, SIDE_STEPS)
            c = time_config(c5_total // n, c5_steps)
            ms5, k5 = c["elapsed"] / c5_steps * 1e3, max(c["per_k"])
            b_tot, b_gpu = mvm_bytes(c5_total, cols), mvm_bytes(c5_total // n, cols)
            ach5 = b_gpu / (k5 * 1e-3) / 1e9
            out["c5"] = {
                "workload": f"CloverMatrix4::mvm {c5_total}x{cols} int4 row-sharded {n} way(s), {c5_total // n} rows per GPU"
                            + (" = BASELINE configs[4]" if (c5_total, cols) == (1 << 20, 65536) else " (NOT configs[4]: shrunk by CLOVER_BENCH_C5_ROWS / --cols)"),
                "scaling": "strong", "n_gpus": n, "rows_per_gpu": c5_total // n, "cols": cols, "steps": c5_steps, "warmup": args.warmup,
                "settle_launches": c["settle_launches"], "mode": "one-process",
                "ms_per_step": round(ms5, 5), "value": round(b_tot / (ms5 * 1e-3) / 1e9, 2), "unit": "GB/s",
                "frac": round(b_tot / (ms5 * 1e-3) / 1e9 / (n * HBM_PEAK_GBS), 4), "frac_of": f"{n} x {HBM_PEAK_GBS:g} GB/s",
                "algorithmic_bytes_per_step": b_tot, "algorithmic_bytes_per_launch": b_gpu,
                "kernel_avg_ms": round(k5, 5), "kernel_frac": round(ach5 / HBM_PEAK_GBS, 4), "kernel_only_aggregate_GBs": round(n * ach5, 2),
                "per_rank_kernel_ms": [round(v, 5) for v in c["per_k"]], "gather_ms_behind_kernel": [round(v, 5) for v in c["per_g"]],
                "gather_bytes_per_rank": packed_bytes_of(c5_total // n), "gathered_result_verified": c["verified"],
                "backend": backend(c), "rccl_ranks": c["rccl_ranks"],
                **({"degraded": True} if degraded else {}),
            }
    tr = pmc_traffic(rows, cols)
    if tr:
        out["roofline"]["traffic"] = tr[0]
        out["roofline"]["traffic_source"] = f"profiles/{tr[1]}"
    return out


def product_loops_child(args, n: int) -> None:
    """`--product-loops-child N` (started by run_product_loops): both product loops over N devices in a process of their own"""
    import torch

    from clover_amd.lib_binding import CloverHip
    hip = CloverHip(device=0)
    res = {}
    for key, fn in (("one_process", one_process_object), ("gemm_sharded", gemm_sharded_measure)):
        try:
            res[key] = fn(args, torch, hip, n)
        except Exception as e:                                   # noqa: BLE001
            res[key] = {"failed": f"{type(e).__name__}: {e}"[:400]}
        torch.cuda.empty_cache()
    print(json.dumps(res))


def run_product_loops(args, n: int) -> dict:
    """The product's own loops over the same N devices (`one_process`, `gemm_sharded`) in a CHILD process with a time limit: a side
    measurement -- RCCL through dlopen, ncclCommInitAll over N devices, paths no one-GPU box can rehearse with more than one rank --
    must never cost the headline line, whether it raises, crashes or hangs."""
    cmd = [sys.executable, str(Path(__file__).resolve()), "--product-loops-child", str(n), "--full", "--gpus", str(n), "--steps", str(min(args.steps, SIDE_STEPS)), "--warmup", str(args.warmup),
           "--rows-per-gpu", str(args.rows_per_gpu), "--cols", str(args.cols), "--settle-ms", str(args.settle_ms), "--event-every", str(args.event_every),
           "--gemm-size", str(args.gemm_size), *(["--preset", args.preset] if args.preset else []), *(["--no-c5"] if args.no_c5 else [])]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "GROUP_RANK", "ROLE_RANK",
                                                               "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID", "OMP_NUM_THREADS")}
    try:
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=420)      # ~15 s of work at N = 8; a hang must not eat the run
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not lines:
            raise RuntimeError(f"child exit code {p.returncode}: {p.stderr.strip()[-300:]}")
        return json.loads(lines[-1])
    except Exception as e:                                       # noqa: BLE001
        why = {"failed": f"{type(e).__name__}: {e}"[:500]}
        return {"one_process": why, "gemm_sharded": dict(why)}


def one_process_object(args, torch, hip, n: int) -> dict:
    """one_process_measure as an object of the ranks line: the step time of the product's own loop beside the ranks' (torch.distributed)"""
    o = one_process_measure(args, torch, hip, n)
    cfg = o["config"]
    return {
        "what": "the same shards through the product's own loop: ONE process drives the N devices (clm4_sharded_create / _set_x / _loop_begin / "
                "_mvm_enqueue / _sync), RCCL through dlopen, grouped in-place ncclAllGather pair per step on a second stream per device",
        "workload": cfg["workload"], "n_gpus": o["n_gpus"], "steps": o["steps"], "warmup": o["warmup"], "settle_launches": cfg["settle_launches"],
        "ms_per_step": o["ms_per_step"], "value": o["value"], "unit": o["unit"],
        "frac": round(o["value"] / (n * HBM_PEAK_GBS), 4), "frac_of": f"{n} x {HBM_PEAK_GBS:g} GB/s",
        "kernel_avg_ms": o["roofline"]["kernel_avg_ms"], "kernel_frac": o["roofline"]["frac"],
        "per_rank_kernel_ms": cfg["per_rank_kernel_ms"], "gather_ms_behind_kernel": cfg["gather_ms_behind_kernel"],
        "gather_bytes_per_rank": cfg["gather_bytes_per_rank"], "gathered_result_verified": cfg["gathered_result_verified"],
        "rccl_ranks": cfg["rccl_ranks"], "backend": cfg["backend"],
        **({"degraded": True, "degraded_why": o["degraded_why"], "value_kernel_only": o["value_kernel_only"]} if o.get("degraded") else {}),
        **({"c5": o["c5"]} if "c5" in o else {}),
    }


def gemm_sharded_measure(args, torch, hip, n: int) -> dict:
    """BASELINE configs[3] (CloverMatrix4 GEMM G^3, G = 8192) split by rows of A over the N GPUs -- mvm_parallel's row split
    (CloverMatrix4.h:1700-1705) applied to C = A * B^T: G / N rows of A per device (multiples of 128), B replicated, and the fp32 C ROW
    PANELS ALL-GATHERED over RCCL on each device's exchange stream, through the product's own loop (clm4_sharded_gemm_begin /
    _enqueue / _sync) driven by this one process.  A step = every device's clm4_gemm (FP6 re-code + MFMA kernel) + one in-place
    ncclAllGather of the panel it produced; the gather of step i overlaps the kernel of step i + 1 (two C buffers).  Strong scaling: the
    exchange moves (N-1)/N of the 4 G^2 bytes of C into every device, so beyond N = 1 the step is exchange-bound -- both figures are
    reported: `value` (whole step) and `kernel_only_aggregate_TOPs`.  The gathered C of the first and the last device are compared
    with the unsharded clm4_gemm, bit for bit."""
    import ctypes as C

    import numpy as np
    debug = os.environ.get("CLOVER_BENCH_DEBUG_ONE_GPU") == "1"
    lib = hip.lib
    G = int(os.environ.get("CLOVER_BENCH_GEMM_SIZE", str(args.gemm_size)))
    if G % (128 * n) != 0:
        return {"skipped": f"{G} rows of A do not split into {n} equal shards of whole 128-row units"}
    steps, warm = 60, 80
    hip.check(lib.clv_set_device(0))
    B = torch.empty(G * G // 2, dtype=torch.uint8, device="cuda:0")
    sB = torch.empty((G // 64) ** 2, dtype=torch.float32, device="cuda:0")
    hip.check(lib.clv_fill_random_nibbles(B.data_ptr(), B.numel(), 22, 0, None))
    hip.check(lib.clv_fill_random_scales(sB.data_ptr(), sB.numel(), 24, 0, None))
    torch.cuda.synchronize()
    devs = (C.c_int * n)(*([0] * n if debug else range(n)))
    ctx = C.c_void_p()
    hip.check(lib.clm4_sharded_create(C.byref(ctx), n, devs, G, G))
    try:
        hip.check(lib.clm4_sharded_fill_random(ctx, 21))                      # A: nibbles seed 21, tile scales seed 22 (= 21 + 1)
        hip.check(lib.clm4_sharded_gemm_begin(ctx, B.data_ptr(), sB.data_ptr(), G, 0, steps))
        for w_ in range(warm):                                                # the matrix pipe's clocks settle after ~50 calls
            hip.check(lib.clm4_sharded_gemm_enqueue(ctx, w_, 0))
        hip.check(lib.clm4_sharded_sync(ctx))
        t0 = time.perf_counter()
        sampled = list(range(0, steps, 6))                                    # event triples around every 6th step
        for i in range(steps):
            hip.check(lib.clm4_sharded_gemm_enqueue(ctx, i, 1 if i % 6 == 0 else 0))
        hip.check(lib.clm4_sharded_sync(ctx))
        elapsed = time.perf_counter() - t0
        per_k, per_g = [], []
        km, gm = C.c_float(), C.c_float()
        for d in range(n):
            ks = gs = 0.0
            for i in sampled:
                hip.check(lib.clm4_sharded_step_timing(ctx, d, i, C.byref(km), C.byref(gm)))
                ks += km.value
                gs += gm.value
            per_k.append(ks / len(sampled))
            per_g.append(gs / len(sampled))
        ranks, equal = C.c_int(), C.c_int()
        hip.check(lib.clm4_sharded_comm_info(ctx, C.byref(ranks), C.byref(equal)))
        full = []
        for d in sorted({0, n - 1}):
            cp = C.c_void_p()
            hip.check(lib.clm4_sharded_gemm_full(ctx, d, (steps - 1) & 1, C.byref(cp)))
            host = np.empty(G * G, np.float32)
            hip.check(lib.clv_set_device(0 if debug else d))
            hip.check(lib.clv_memcpy_d2h(host.ctypes.data, cp, host.nbytes, None))
            hip.check(lib.clv_device_sync())
            full.append(host)
        hip.check(lib.clv_set_device(0))
        # the other two exchange modes of the loop (round 6): panels to device 0 only / no exchange, C stays row-sharded like A
        modes = {}
        for mname, mode in (("gather_root", 1), ("sharded", 2)):
            msteps = 30
            hip.check(lib.clm4_sharded_gemm_begin_mode(ctx, B.data_ptr(), sB.data_ptr(), G, 0, steps, mode))
            for w_ in range(10):
                hip.check(lib.clm4_sharded_gemm_enqueue(ctx, w_, 0))
            hip.check(lib.clm4_sharded_sync(ctx))
            t0 = time.perf_counter()
            for i in range(msteps):
                hip.check(lib.clm4_sharded_gemm_enqueue(ctx, i, 0))
            hip.check(lib.clm4_sharded_sync(ctx))
            mel = time.perf_counter() - t0
            held = {}
            for d in sorted({0, n - 1}):
                cp = C.c_void_p()
                hip.check(lib.clm4_sharded_gemm_full(ctx, d, (msteps - 1) & 1, C.byref(cp)))
                host = np.empty(G * G, np.float32)
                hip.check(lib.clv_set_device(0 if debug else d))
                hip.check(lib.clv_memcpy_d2h(host.ctypes.data, cp, host.nbytes, None))
                hip.check(lib.clv_device_sync())
                held[d] = host
            hip.check(lib.clv_set_device(0))
            modes[mname] = {"ms": mel / msteps * 1e3, "held": held}
    finally:
        lib.clm4_sharded_destroy(ctx)
        hip.check(lib.clv_set_device(0))
    # the unsharded product of the same (regenerated) operands on device 0
    A0 = torch.empty(G * G // 2, dtype=torch.uint8, device="cuda:0")
    sA0 = torch.empty((G // 64) ** 2, dtype=torch.float32, device="cuda:0")
    C0 = torch.empty(G * G, dtype=torch.float32, device="cuda:0")
    hip.check(lib.clv_fill_random_nibbles(A0.data_ptr(), A0.numel(), 21, 0, None))
    hip.check(lib.clv_fill_random_scales(sA0.data_ptr(), sA0.numel(), 22, 0, None))
    hip.check(lib.clm4_gemm(A0.data_ptr(), sA0.data_ptr(), G, G, B.data_ptr(), sB.data_ptr(), G, C0.data_ptr(), None))
    torch.cuda.synchronize()
    ref = C0.cpu().numpy().view(np.uint32)
    verified = all(np.array_equal(f.view(np.uint32), ref) for f in full)
    rows_per = G // n
    mode_out = {}
    for mname, mres in modes.items():
        oks = []
        for d, host in mres["held"].items():
            h = host.view(np.uint32)
            if mname == "gather_root" and d == 0:
                oks.append(bool(np.array_equal(h, ref)))                                         # the root holds the whole C
            else:
                oks.append(bool(np.array_equal(h[d * rows_per * G:(d + 1) * rows_per * G], ref[d * rows_per * G:(d + 1) * rows_per * G])))      # its own panel
        mtops = 2.0 * G ** 3 / mres["ms"] / 1e9
        mode_out[mname] = {"ms_per_step": round(mres["ms"], 5), "value": round(mtops, 1), "unit": "TOP/s", "frac": round(mtops / (n * FP6_PEAK_TOPS), 4),
                           "bytes_received": ({"root": (n - 1) * rows_per * G * 4, "others": 0} if mname == "gather_root" else 0), "verified": all(oks)}
    del A0, sA0, C0, B, sB
    torch.cuda.empty_cache()
    ops = 2.0 * G ** 3
    ms = elapsed / steps * 1e3
    kmax = max(per_k)
    tops, ktops = ops / ms / 1e9, ops / kmax / 1e9
    degraded = debug or (n > 1 and not ranks.value)
    return {
        "workload": f"CloverMatrix4::gemm {G}x{G}x{G} int4 x int4 -> fp32" + (" (BASELINE configs[3])" if G == 8192 else " (NOT configs[3]: shrunk)")
                    + f", rows of A split {n} way(s): {G // n} rows per GPU, B replicated, fp32 C row panels all-gathered",
        "scaling": "strong", "n_gpus": n, "rows_per_gpu": G // n, "steps": steps, "warmup": warm, "mode": "one-process (clm4_sharded_gemm_begin / _enqueue)",
        "ms_per_step": round(ms, 5), "value": round(tops, 1), "unit": "TOP/s",
        "frac": round(tops / (n * FP6_PEAK_TOPS), 4), "frac_of": f"{n} x {FP6_PEAK_TOPS:g} TOP/s (dense FP6 MFMA, the pipe the kernel runs on)",
        "per_rank_kernel_ms": [round(v, 5) for v in per_k], "kernel_only_aggregate_TOPs": round(ktops, 1),
        "kernel_only_frac": round(ktops / (n * FP6_PEAK_TOPS), 4),
        "gather_ms_behind_kernel": [round(v, 5) for v in per_g],
        "gather_bytes_received_per_rank": (n - 1) * (G // n) * G * 4, "c_panel_bytes": (G // n) * G * 4,
        "exchange": ("device copies (same-device rehearsal)" if debug else "ncclAllGather of the fp32 panels, in place, one per device and step"
                     if ranks.value and equal.value else "none (one shard)" if n == 1 and not ranks.value else "per-owner ncclBroadcast"),
        "rccl_ranks": ranks.value, "gathered_c_verified": bool(verified),
        "other_exchange_modes": {**mode_out, "note": "clm4_sharded_gemm_begin_mode: gather_root = panels to device 0 only (grouped ncclSend / ncclRecv), "
                                 "sharded = no exchange, C stays row-sharded like A; the headline figures above are the all-gather of SURVEY 8(e)"},
        "verified_how": "the whole C held by the first and the last device after the last step == clm4_gemm of the unsharded operands, all bits",
        **({"degraded": True} if degraded else {}),
    }


def packed_bytes_of(rows: int) -> int:
    return rows // 2 + rows // 16


def gemm_main(args) -> None:
    """BASELINE configs[3]: CloverMatrix4::gemm G x G x G (default 8192) on one GPU.  A step = one clm4_gemm call (the FP6 re-coding
    pass + the MFMA kernel); the bound is the dense FP6 peak of the pipe the kernel uses (10 POP/s), the int8 figure is quoted beside."""
    import torch

    from clover_amd.lib_binding import CloverHip
    if int(os.environ.get("WORLD_SIZE", "1")) != 1 or args.gpus != 1:
        raise SystemExit("bench.py --workload gemm measures one GPU (row shards of C are independent: clm4_sharded_gemm)")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    hip = CloverHip(device=0)
    lib = hip.lib
    stream = torch.cuda.current_stream().cuda_stream
    G = args.gemm_size
    assert G % 128 == 0
    A = torch.empty(G * G // 2, dtype=torch.uint8, device=dev)
    B = torch.empty(G * G // 2, dtype=torch.uint8, device=dev)
    sA = torch.empty((G // 64) ** 2, dtype=torch.float32, device=dev)
    sB = torch.empty((G // 64) ** 2, dtype=torch.float32, device=dev)
    Cm = torch.empty(G * G, dtype=torch.float32, device=dev)
    for t, sd in ((A, 21), (B, 22)):
        hip.check(lib.clv_fill_random_nibbles(t.data_ptr(), t.numel(), sd, 0, stream))
    for t, sd in ((sA, 23), (sB, 24)):
        hip.check(lib.clv_fill_random_scales(t.data_ptr(), t.numel(), sd, 0, stream))

    def step():
        hip.check(lib.clm4_gemm(A.data_ptr(), sA.data_ptr(), G, G, B.data_ptr(), sB.data_ptr(), G, Cm.data_ptr(), stream))

    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        ev[i][0].record()
        step()
        ev[i][1].record()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    ms = elapsed / args.steps * 1e3
    call_ms = sum(a.elapsed_time(b) for a, b in ev) / len(ev)
    if args.dump_outputs:
        # C of the last timed call (fp32, G x G): whole when it fits, else a fixed, seeded sample of its elements with their flat indices
        import numpy as np
        keep = G * G if G * G * 4 <= DUMP_LIMIT_BYTES else 1 << 20
        if keep < G * G:
            idx = np.sort(np.random.default_rng(0xD1).choice(G * G, keep, replace=False))
            c = Cm[torch.from_numpy(idx).to(dev)].cpu().numpy()
            write_outputs(args.dump_outputs, {"gemm_C_index": idx.astype(np.float64), "gemm_C": c})
        else:
            write_outputs(args.dump_outputs, {"gemm_C": Cm.cpu().numpy()})
    ops = 2.0 * G ** 3
    tops = ops / (ms * 1e-3) / 1e12
    ach = ops / (call_ms * 1e-3) / 1e12
    print(json.dumps({
        "metric": "int4 GEMM (CloverMatrix4 x CloverMatrix4^T -> fp32) TOP/s, 2 M N K / time", "value": round(tops, 1), "unit": "TOP/s",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 5), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "int4", "data": "synthetic",
        "config": {"workload": f"CloverMatrix4::gemm {G}x{G}x{G} int4 (BASELINE configs[3]), bit-exact against the build-defined "
                               "semantics (one fma chain over the 64-element K-blocks per element)", "M": G, "N": G, "K": G,
                   "parallelism": "1 GPU"},
        "roofline": {"bound": "mfma", "achieved": round(ach, 1), "peak": FP6_PEAK_TOPS, "unit": "TOP/s", "frac": round(ach / FP6_PEAK_TOPS, 4),
                     "traffic": None, "kernel": "k_m4_to_fp6 + k_m4_gemm_fp6_t256 (one clm4_gemm call)", "kernel_avg_ms": round(call_ms, 5),
                     "frac_of_int8_peak": round(ach / INT8_PEAK_TOPS, 4),
                     "peak_note": "10 POP/s = dense FP6 block-scaled MFMA, the pipe the kernel runs on; 5 POP/s = dense int8 MFMA, the pipe "
                                  "BASELINE names; counters in profiles/"},
    }))


def _timeit(torch, fn, reps, warm=3):
    """mean ms per call of `reps` calls after `warm` untimed ones.  Matrix-pipe kernels need a long warm-up: the first ~50 GEMM calls
    (about 25 ms of work) run 10-20 % slower than the steady state the clocks settle at (profiles/r02_gemm_warmup_series.txt)."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


FP6_PEAK_TOPS = 10000.0     # dense FP6/FP4 block-scaled MFMA (MI355X_MICROARCH.md): the pipe the GEMM kernel runs on
INT8_PEAK_TOPS = 5000.0     # dense int8 MFMA: the pipe BASELINE's wording names


def gemm_probe_child(spec: str, G: int) -> None:
    """One timing of the 8192^3 GEMM in a process of its own (the kernel switches CLV_GEMM_KERNEL / CLV_GEMM_LOOP are read once per process).
    spec = "<library>:<call>", library = product | probe (tools/_build/libclover_hip_probe.so: the loop's timing-only variants), call =
    gemm | prepared | i32_prepared.  No torch: ctypes + the library only.  Prints {"ms": mean of 100 calls after 80 untimed ones}."""
    import ctypes as C

    from clover_amd.build import probe_library_path
    from clover_amd.lib_binding import CloverHip
    which, call = spec.split(":")
    hip = CloverHip(path=probe_library_path() if which == "probe" else None, device=0, allow_probe=which == "probe")
    lib = hip.lib
    A, B = hip.alloc(G * G // 2), hip.alloc(G * G // 2)
    sA, sB = hip.alloc((G // 64) ** 2 * 4), hip.alloc((G // 64) ** 2 * 4)
    Cc = hip.alloc(G * G * 4)
    for t, sd in ((A, 21), (B, 22)):
        hip.check(lib.clv_fill_random_nibbles(t.ptr, t.nbytes, sd, 0, None))
    for t, sd in ((sA, 23), (sB, 24)):
        hip.check(lib.clv_fill_random_scales(t.ptr, t.nbytes // 4, sd, 0, None))
    opA, opB = C.c_void_p(), C.c_void_p()
    if call != "gemm":
        hip.check(lib.clm4_gemm_prepare(A.ptr, G, G, C.byref(opA), None))
        hip.check(lib.clm4_gemm_prepare(B.ptr, G, G, C.byref(opB), None))
    fn = {"gemm": lambda: lib.clm4_gemm(A.ptr, sA.ptr, G, G, B.ptr, sB.ptr, G, Cc.ptr, None),
          "prepared": lambda: lib.clm4_gemm_prepared(opA, None, sA.ptr, G, G, opB, None, sB.ptr, G, Cc.ptr, None),
          "i32_prepared": lambda: lib.clm4_gemm_i32_prepared(opA, None, G, G, opB, None, G, 0, G // 64, Cc.ptr, None)}[call]
    for _ in range(80):
        hip.check(fn())
    hip.sync()
    a, b = C.c_void_p(), C.c_void_p()
    hip.check(lib.clv_event_create(C.byref(a)))
    hip.check(lib.clv_event_create(C.byref(b)))
    hip.check(lib.clv_event_record(a, None))
    for _ in range(100):
        hip.check(fn())
    hip.check(lib.clv_event_record(b, None))
    hip.check(lib.clv_event_sync(b))
    ms = C.c_float()
    hip.check(lib.clv_event_elapsed_ms(a, b, C.byref(ms)))
    print(json.dumps({"ms": ms.value / 100}))


def gemm_probe(spec: str, G: int, env_extra: dict) -> float | None:
    env = dict(os.environ, **env_extra)
    for k in ("CLV_GEMM_LOOP", "CLV_GEMM_KERNEL", "CLV_GEMM_TILE"):
        if k not in env_extra:
            env.pop(k, None)
    try:
        out = subprocess.run([sys.executable, __file__, "--gemm-probe-child", spec, "--gemm-size", str(G)], env=env, check=True, capture_output=True,
                             text=True, timeout=300).stdout
        return float(json.loads(out.strip().splitlines()[-1])["ms"])
    except Exception:
        return None


def gemm_pmc(G: int):
    """matrix-pipe busy share and memory traffic of the GEMM kernel from the latest committed rocprofv3 --pmc passes (profiles/rNN_gemm_pmc.json,
    written by tools/gemm_pmc_json.py on the GPU box: counters cannot be collected inside a timed run)"""
    best = None
    for f in sorted((ROOT / "profiles").glob("r*_gemm_pmc.json")):
        try:
            d = json.loads(f.read_text())
            if d["G"] == G:
                best = (d, f.name)
        except (OSError, KeyError, ValueError):
            continue
    return best


def smi_power_clock():
    """socket power (W) and shader clock (MHz) right now, from rocm-smi; None where the tool or a field is missing"""
    try:
        out = subprocess.run(["rocm-smi", "--showpower", "--showclocks", "--json"], capture_output=True, text=True, timeout=20).stdout
        card = next(iter(json.loads(out).values()))
        power = next((float(v) for k, v in card.items() if "power" in k.lower() and "socket" in k.lower()), None)
        if power is None:
            power = next((float(v) for k, v in card.items() if "power" in k.lower() and str(v).replace(".", "", 1).isdigit()), None)
        sclk = next((v for k, v in card.items() if k.lower().startswith("sclk")), None)
        mhz = float("".join(ch for ch in str(sclk).split("Mhz")[0].split("(")[-1] if ch.isdigit() or ch == ".")) if sclk else None
        return {"socket_power_W": power, "sclk_MHz": mhz}
    except Exception:
        return None


def gemm_object(hip, torch, dev, stream, G: int = 8192) -> dict:
    """BASELINE configs[3]: CloverMatrix4::gemm 8192^3.  One clm4_gemm call = the FP6 re-coding pass over both operands + the matrix
    kernel; timed with HIP events on the launch stream.  Normalised to the FP6 dense peak (the pipe in use); the int8 figure beside."""
    import ctypes as C
    lib = hip.lib
    gA = torch.empty(G * G // 2, dtype=torch.uint8, device=dev)
    gB = torch.empty(G * G // 2, dtype=torch.uint8, device=dev)
    gsA = torch.empty((G // 64) ** 2, dtype=torch.float32, device=dev)
    gsB = torch.empty((G // 64) ** 2, dtype=torch.float32, device=dev)
    gC = torch.empty(G * G, dtype=torch.float32, device=dev)
    for t, sd in ((gA, 21), (gB, 22)):
        hip.check(lib.clv_fill_random_nibbles(t.data_ptr(), t.numel(), sd, 0, stream))
    for t, sd in ((gsA, 23), (gsB, 24)):
        hip.check(lib.clv_fill_random_scales(t.data_ptr(), t.numel(), sd, 0, stream))
    ops = 2.0 * G ** 3
    g_ms = _timeit(torch, lambda: hip.check(lib.clm4_gemm(gA.data_ptr(), gsA.data_ptr(), G, G, gB.data_ptr(), gsB.data_ptr(), G, gC.data_ptr(), stream)), 100, warm=80)
    opA, opB = C.c_void_p(), C.c_void_p()
    hip.check(lib.clm4_gemm_prepare(gA.data_ptr(), G, G, C.byref(opA), stream))
    hip.check(lib.clm4_gemm_prepare(gB.data_ptr(), G, G, C.byref(opB), stream))
    p_ms = _timeit(torch, lambda: hip.check(lib.clm4_gemm_prepared(opA, None, gsA.data_ptr(), G, G, opB, None, gsB.data_ptr(), G, gC.data_ptr(), stream)), 100, warm=40)
    ip_ms = _timeit(torch, lambda: hip.check(lib.clm4_gemm_i32_prepared(opA, None, G, G, opB, None, G, 0, G // 64, gC.data_ptr(), stream)), 100, warm=40)
    # power and clock while the prepared GEMM runs back to back: 4000 calls are enqueued (about 1.5 s of work), sampled 0.5 s in
    power = None
    try:
        for _ in range(4000):
            hip.check(lib.clm4_gemm_prepared(opA, None, gsA.data_ptr(), G, G, opB, None, gsB.data_ptr(), G, gC.data_ptr(), stream))
        time.sleep(0.5)
        power = smi_power_clock()
        torch.cuda.synchronize()
    except Exception:
        torch.cuda.synchronize()
    hip.check(lib.clm4_gemm_release(opA))
    hip.check(lib.clm4_gemm_release(opB))
    i_ms = _timeit(torch, lambda: hip.check(lib.clm4_gemm_i32(gA.data_ptr(), G, G, gB.data_ptr(), G, 0, G // 64, gC.data_ptr(), stream)), 100, warm=40)
    tops = ops / g_ms / 1e9
    # the ceiling, measured on THIS box: the same main loop with parts left out (bench-only probe library, separate processes), and the
    # int8-MFMA kernel (the pipe BASELINE's wording names) for comparison
    full_p = gemm_probe("probe:prepared", G, {})
    arith = gemm_probe("probe:prepared", G, {"CLV_GEMM_LOOP": "v9"})
    nofold = gemm_probe("probe:prepared", G, {"CLV_GEMM_LOOP": "v5"})
    mfma_only = gemm_probe("probe:i32_prepared", G, {"CLV_GEMM_LOOP": "v9"})
    i8_ms = gemm_probe("product:gemm", G, {"CLV_GEMM_KERNEL": "i8"})
    ceiling = {
        "full_loop_ms": full_p, "mfma_plus_fold_only_ms": arith, "no_fold_ms": nofold, "mfma_only_ms": mfma_only,
        "frac_if_only_arithmetic": round(ops / arith / 1e9 / FP6_PEAK_TOPS, 4) if arith else None,
        "power_and_clock_during_prepared_gemm": power,
        "what": "k_m4_gemm_fp6_t256 on prepared operands through tools/_build/libclover_hip_probe.so (bench-only build of the same kernel with "
                "CLV_GEMM_LOOP=vN variants: v9 = nothing but the wave's MFMAs and the per-K-block fp32 fold -- no staging, fragment reads, "
                "barrier, store or pointer arithmetic; v5 = the whole loop without the fold; int32 v9 = the MFMAs alone).  The definition's "
                "one fp32 fma per element and K-block runs on the VALU, which on a CDNA4 SIMD issues BESIDE an MFMA for only 2-5 instructions "
                "per 32-cycle MFMA (tools/mfma_fold_probe.hip, profiles/r02_mfma_fold_probe.txt: MFMA 14.5 ns + 8 packed fmas 15.8 ns = 30.9 ns "
                "together): mfma_plus_fold_only_ms is the floor of ANY schedule of this definition on this box, frac_if_only_arithmetic the "
                "roofline fraction it would give",
    }
    pmc = gemm_pmc(G)
    return {
        "ceiling": ceiling,
        "int8_mfma_kernel": {"ms": i8_ms, "TOP/s": round(ops / i8_ms / 1e9, 1) if i8_ms else None,
                             "frac_of_int8_peak": round(ops / i8_ms / 1e9 / INT8_PEAK_TOPS, 4) if i8_ms else None,
                             "note": "k_m4_gemm_mfma (v_mfma_i32_16x16x64_i8, CLV_GEMM_KERNEL=i8), one clm4_gemm call, own process"},
        "workload": f"CloverMatrix4::gemm {G}x{G}x{G} int4 x int4 -> fp32 (BASELINE configs[3]), both operands re-coded inside the call, "
                    "bit-exact against the build-defined semantics (one fma chain over the 64-element K-blocks per element)",
        "ms": round(g_ms, 4), "value": round(tops, 1), "unit": "TOP/s",
        "roofline": {"bound": "mfma", "achieved": round(tops, 1), "peak": FP6_PEAK_TOPS, "unit": "TOP/s", "frac": round(tops / FP6_PEAK_TOPS, 4),
                     "traffic": pmc[0].get("traffic_bytes_per_call") if pmc else None,
                     **({"traffic_source": f"profiles/{pmc[1]}: " + pmc[0].get("traffic_how", ""),
                         "mfma_busy_pct": pmc[0].get("mfma_busy_pct"), "mfma_busy_how": pmc[0].get("mfma_busy_how"),
                         "l2_hit_pct": pmc[0].get("l2_hit_pct"), "algorithmic_bytes_per_call": pmc[0].get("algorithmic_bytes_per_call")} if pmc else {}),
                     "kernel": "k_m4_to_fp6 + k_m4_gemm_fp6_t256 (one clm4_gemm call)", "kernel_avg_ms": round(g_ms, 4),
                     "frac_of_int8_peak": round(tops / INT8_PEAK_TOPS, 4),
                     "peak_note": "10 POP/s = dense FP6 block-scaled MFMA, the pipe the kernel runs on (nibbles are exact E2M3 values); "
                                  "5 POP/s = dense int8 MFMA, the pipe BASELINE names"},
        "prepared_operands": {"ms": round(p_ms, 4), "TOP/s": round(ops / p_ms / 1e9, 1), "frac_of_fp6_peak": round(ops / p_ms / 1e9 / FP6_PEAK_TOPS, 4),
                              "note": "clm4_gemm_prepared: both FP6 images made once outside the timed region (weights-style reuse)"},
        "int32_unscaled": {"ms": round(i_ms, 4), "TOP/s": round(ops / i_ms / 1e9, 1), "frac_of_fp6_peak": round(ops / i_ms / 1e9 / FP6_PEAK_TOPS, 4),
                           "note": "clm4_gemm_i32 over all K-blocks: the exact int4 x int4 -> int32 contraction (no scales), accumulated inside "
                                   "the matrix pipe; time includes the re-coding pass",
                           "prepared_operands": {"ms": round(ip_ms, 4), "TOP/s": round(ops / ip_ms / 1e9, 1),
                                                 "frac_of_fp6_peak": round(ops / ip_ms / 1e9 / FP6_PEAK_TOPS, 4)}},
        "timing": "mean of 100 calls after 40-80 untimed ones (steady-state clocks), HIP events on the launch stream",
        "note": "CLV_GEMM_LOOP=hipcc runs the compiler-scheduled main loop, CLV_GEMM_KERNEL=i8 the int8-MFMA kernel (A/B runs)",
    }


def hbm_resident(hip, torch, dev, stream) -> dict:
    """BASELINE configs[1]'s operations at a footprint that cannot live in the 256 MiB Infinity Cache: n = 2^30 (fp32 source 4 GiB,
    a quantized vector 576 MiB).  Algorithmic bytes per call as in SURVEY 8(d); HIP events on the launch stream."""
    from clover_amd.lib_binding import DOT_FAST
    lib = hip.lib
    n = 1 << 30
    xs = torch.empty(n, dtype=torch.float32, device=dev)
    hip.check(lib.clv_fill_random_ints_f32(xs.data_ptr(), n, 10, 11, 0, stream))
    qa = torch.empty(n // 2, dtype=torch.uint8, device=dev)
    qb = torch.empty(n // 2, dtype=torch.uint8, device=dev)
    sa = torch.empty(n // 64, dtype=torch.float32, device=dev)
    sb = torch.empty(n // 64, dtype=torch.float32, device=dev)
    o = torch.empty(2, dtype=torch.float32, device=dev)
    rng_state = hip.new_rng(5, 6)
    q_ms = _timeit(torch, lambda: hip.check(lib.clv4_quantize(xs.data_ptr(), n, qa.data_ptr(), sa.data_ptr(), None, stream)), 10)
    qs_ms = _timeit(torch, lambda: hip.check(lib.clv4_quantize(xs.data_ptr(), n, qb.data_ptr(), sb.data_ptr(), rng_state.ptr, stream)), 10)
    f_ms = _timeit(torch, lambda: hip.check(lib.clv4_dot(qa.data_ptr(), sa.data_ptr(), qb.data_ptr(), sb.data_ptr(), n, DOT_FAST, o.data_ptr(), None, stream)), 10)
    sa_ms = _timeit(torch, lambda: hip.check(lib.clv4_scale_and_add(qa.data_ptr(), sa.data_ptr(), qb.data_ptr(), sb.data_ptr(), 0.5, n, qb.data_ptr(), sb.data_ptr(), None, stream)), 10)
    r_ms = _timeit(torch, lambda: hip.check(lib.clv4_restore(qa.data_ptr(), sa.data_ptr(), n, xs.data_ptr(), stream)), 10)

    def obj(nbytes, ms, what):
        gbs = nbytes / ms / 1e6
        return {"ms": round(ms, 4), "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4),
                "algorithmic_bytes": int(nbytes), "what": what}
    return {
        "n": n,
        "quantize": obj(4.5625 * n, q_ms, "CloverVector4::quantize, rounding disabled (4 B in, 0.5625 B out per element)"),
        "quantize_stochastic": obj(4.5625 * n, qs_ms, "the same with the XORShift stream (the reference's default build)"),
        "dot_fast": obj(1.125 * n, f_ms, "CloverVector4::dot, exact integer block sums, fp32 tree order (dot_parallel's role)"),
        "scale_and_add": obj(3 * 0.5625 * n, sa_ms, "CloverVector4::scaleAndAdd in place (two vectors in, one out)"),
        "restore": obj(4.5625 * n, r_ms, "CloverVector4::restore (0.5625 B in, 4 B out per element)"),
    }


def iht_through_headers() -> dict:
    """tools/iht_dropin.cpp: Q_IHT of include/CloverIHT.h on container objects (the reference's caller, 01_measure.h:923-946), N = 8192, in
    both container builds (page-tracked mirrors / -DCLOVER_HIP_EXPLICIT_SYNC) and both settings of the exactness switch; compiled here
    with g++ against the in-tree library (a few seconds), run as child processes"""
    from clover_amd.build import hip_library_path
    lib = hip_library_path()
    outd = ROOT / "tools" / "_build"
    outd.mkdir(parents=True, exist_ok=True)
    res = {}
    for key, flags in (("page_tracked", []), ("explicit_sync", ["-DCLOVER_HIP_EXPLICIT_SYNC"])):
        exe = outd / f"iht_dropin_{key}"
        try:
            subprocess.run(["g++", "-std=c++11", "-O2", "-DCLOVER_STOCHASTIC_ROUNDING_DISABLED=1", *flags, f"-I{ROOT / 'include'}", str(ROOT / "tools" / "iht_dropin.cpp"),
                            "-o", str(exe), f"-L{lib.parent}", "-lclover_hip", f"-Wl,-rpath,{lib.parent}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"],
                           check=True, capture_output=True, text=True, timeout=300)
            out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=300).stdout
            res[key] = json.loads(out.strip().splitlines()[-1])
        except Exception as e:                                    # noqa: BLE001
            res[key] = {"failed": f"{type(e).__name__}: {e}"[:300]}
    res["what"] = ("us per iteration of Q_IHT(Phi, PhiT, x, y, t1, t2, t3, iterations, K, mu) through include/CloverIHT.h with CloverMatrix4 / "
                   "CloverVector4 (fast, reference_bits) and CloverVector8 (_v8) objects, wall clock incl. reading x back; fast_generic_five_calls = the "
                   "reference's five-call template unchanged; reference_bits = the default build of the headers (threshold = the reference's heap walk)")
    return res


INFINITY_CACHE_BYTES = 256 << 20


def published_sizes(hip, torch, dev, stream) -> dict:
    """The sizes the REFERENCE publishes for this path (doc/results/performance.txt: mvm 8192^2 / 32768^2 at :357, 369, 438, 450; dot
    n = 2^24 / 2^26 / 2^29 at :171-176, 202-207), plus 16384^2 and C3, each measured two ways and labelled:
      warm = the same operands again and again (what fits stays in the 8 x 4 MiB of L2 / the 256 MiB Infinity Cache),
      cold = a rotation over distinct operands whose total footprint exceeds the Infinity Cache (every call streams from HBM).
    An operand set that exceeds the cache by itself is HBM-resident either way.  HIP events on the launch stream, mean over the calls."""
    from clover_amd.lib_binding import DOT_FAST
    lib = hip.lib
    pool = torch.empty(2 << 30, dtype=torch.uint8, device=dev)                 # nibbles of every matrix / vector below
    spool = torch.empty(1 << 24, dtype=torch.float32, device=dev)              # their scales (64 MiB)
    hip.check(lib.clv_fill_random_nibbles(pool.data_ptr(), pool.numel(), 71, 0, stream))
    hip.check(lib.clv_fill_random_scales(spool.data_ptr(), spool.numel(), 72, 0, stream))
    x = torch.empty(65536 // 2, dtype=torch.uint8, device=dev)
    sx = torch.empty(65536 // 64, dtype=torch.float32, device=dev)
    r = torch.empty(65536 // 2, dtype=torch.uint8, device=dev)
    sr = torch.empty(65536 // 64, dtype=torch.float32, device=dev)
    o = torch.empty(1, dtype=torch.float32, device=dev)
    hip.check(lib.clv_fill_random_nibbles(x.data_ptr(), x.numel(), 73, 0, stream))
    hip.check(lib.clv_fill_random_scales(sx.data_ptr(), sx.numel(), 74, 0, stream))
    ref_mvm = {8192: (8533.23, 23250.02, "performance.txt:357, 438"), 16384: (8214.25, 21316.01, "performance.txt:361, 442"),
               32768: (8193.62, 21409.47, "performance.txt:369, 450")}
    ref_dot = {24: (15031.08, 24385.78, "performance.txt:171, 202"), 26: (14169.39, 21045.92, "performance.txt:173, 204"),
               29: (14340.13, 21040.33, "performance.txt:176, 207")}

    def entry(nbytes, ms, footprint, rotation):
        gbs = nbytes / ms / 1e6
        return {"ms": round(ms, 5), "GB/s": round(gbs, 1), "frac_of_8TBs": round(gbs / HBM_PEAK_GBS, 4),
                "resident": ("HBM" if footprint > INFINITY_CACHE_BYTES else "cache") + f" ({footprint >> 20} MiB touched" + (f", {rotation}" if rotation else "") + ")"}

    def rotate(fn_of_k, count):                  # one call per operand set, round-robin
        state = [0]

        def fn():
            fn_of_k(state[0] % count)
            state[0] += 1
        return fn

    sweep = []
    for S in (8192, 16384, 32768, 65536):
        mat, nsc = S * S // 2, (S // 64) ** 2
        nmat = max(1, min(pool.numel() // mat, max(2, -(-(3 * INFINITY_CACHE_BYTES) // mat))))     # >= 768 MiB of distinct matrices where the pool allows
        nb = mvm_bytes(S, S)

        def call(k, S=S, mat=mat, nsc=nsc):
            hip.check(lib.clm4_mvm(pool.data_ptr() + k * mat, spool.data_ptr() + 4 * k * nsc, S, S, x.data_ptr(), sx.data_ptr(), r.data_ptr(), sr.data_ptr(), None, stream))
        reps = max(20, min(400, int(40e-3 / (nb / 5e12))))                      # about 40 ms of work per timing
        warm = _timeit(torch, lambda: call(0), reps, warm=max(3, reps // 10))
        row = {"size": f"{S}x{S}", "algorithmic_bytes": nb, "workgroups": S // 64, "warm": entry(nb, warm, mat, None)}
        if nmat > 1:
            reps_c = -(-reps // nmat) * nmat
            cold = _timeit(torch, rotate(call, nmat), reps_c, warm=nmat)
            row["cold"] = entry(nb, cold, nmat * mat, f"{nmat} distinct matrices round-robin")
        else:
            row["cold"] = dict(row["warm"], note="one matrix exceeds the Infinity Cache by itself: warm == cold")
        if S in ref_mvm:
            row["reference_published_MiBs"] = {"sequential": ref_mvm[S][0], "4_threads": ref_mvm[S][1], "source": ref_mvm[S][2],
                                               "hardware": "Xeon E3-1285L v3, 4 cores, 25.6 GB/s DRAM"}
        sweep.append(row)

    dots = []
    for logn in (24, 26, 29):
        n = 1 << logn
        pair, spair = n, 2 * (n // 64)                                          # bytes of nibbles / floats of scales per operand pair
        npairs = max(1, min(pool.numel() // pair, spool.numel() // spair, max(2, -(-(3 * INFINITY_CACHE_BYTES) // (pair * 9 // 8)))))
        nb = 1.125 * n

        def call(k, n=n, pair=pair, spair=spair):
            qa, sa = pool.data_ptr() + k * pair, spool.data_ptr() + 4 * k * spair
            hip.check(lib.clv4_dot(qa, sa, qa + n // 2, sa + 4 * (n // 64), n, DOT_FAST, o.data_ptr(), None, stream))
        reps = max(20, min(400, int(40e-3 / (nb / 5e12))))
        warm = _timeit(torch, lambda: call(0), reps, warm=max(3, reps // 10))
        row = {"n": n, "algorithmic_bytes": int(nb), "warm": entry(nb, warm, int(nb), None)}
        if npairs > 1:
            cold = _timeit(torch, rotate(call, npairs), -(-reps // npairs) * npairs, warm=npairs)
            row["cold"] = entry(nb, cold, int(npairs * nb), f"{npairs} distinct operand pairs round-robin")
        else:
            row["cold"] = dict(row["warm"], note="one operand pair exceeds the Infinity Cache by itself: warm == cold")
        row["reference_published_MiBs"] = {"sequential": ref_dot[logn][0], "4_threads": ref_dot[logn][1], "source": ref_dot[logn][2],
                                           "hardware": "Xeon E3-1285L v3, 4 cores, 25.6 GB/s DRAM"}
        dots.append(row)
    return {"what": published_sizes.__doc__.split("\n\n")[0].replace("\n    ", " "),
            "mvm_sweep": sweep, "dot_fast": dots}


def extras(hip, torch, dev, stream) -> dict:
    """Secondary numbers of the same path.  `hbm_resident`: configs[1]'s operations at n = 2^30, each with its own achieved / peak /
    frac.  The n = 2^24 figures of configs[1] itself fit the 256 MiB Infinity Cache: cache-resident rates, kept as a footnote."""
    from clover_amd.lib_binding import DOT_EXACT, DOT_FAST
    lib = hip.lib
    hbm = hbm_resident(hip, torch, dev, stream)
    n = 1 << 24
    xs = torch.empty(n, dtype=torch.float32, device=dev)
    ys = torch.empty(n, dtype=torch.float32, device=dev)
    hip.check(lib.clv_fill_random_ints_f32(xs.data_ptr(), n, 10, 11, 0, stream))
    hip.check(lib.clv_fill_random_ints_f32(ys.data_ptr(), n, 10, 12, 0, stream))
    qa = torch.empty(n // 2, dtype=torch.uint8, device=dev)
    qb = torch.empty(n // 2, dtype=torch.uint8, device=dev)
    sa = torch.empty(n // 64, dtype=torch.float32, device=dev)
    sb = torch.empty(n // 64, dtype=torch.float32, device=dev)
    o = torch.empty(2, dtype=torch.float32, device=dev)

    def timeit(fn, reps):
        return _timeit(torch, fn, reps)

    q_ms = timeit(lambda: hip.check(lib.clv4_quantize(xs.data_ptr(), n, qa.data_ptr(), sa.data_ptr(), None, stream)), 50)
    hip.check(lib.clv4_quantize(ys.data_ptr(), n, qb.data_ptr(), sb.data_ptr(), None, stream))
    f_ms = timeit(lambda: hip.check(lib.clv4_dot(qa.data_ptr(), sa.data_ptr(), qb.data_ptr(), sb.data_ptr(), n, DOT_FAST, o.data_ptr(), None, stream)), 50)
    e_ms = timeit(lambda: hip.check(lib.clv4_dot(qa.data_ptr(), sa.data_ptr(), qb.data_ptr(), sb.data_ptr(), n, DOT_EXACT, o.data_ptr() + 4, None, stream)), 5)
    vals = o.cpu().numpy()
    # the caller loop: one quantized IHT iteration, N = 8192 (m x 2m, K = 25 % of m), HBM-resident
    m, nn = 4096, 8192
    Phi = torch.empty(m * nn // 2, dtype=torch.uint8, device=dev)
    PhiT = torch.empty(m * nn // 2, dtype=torch.uint8, device=dev)
    sPhi = torch.empty((m // 64) * (nn // 64), dtype=torch.float32, device=dev)
    sPhiT = torch.empty((m // 64) * (nn // 64), dtype=torch.float32, device=dev)
    hip.check(lib.clv_fill_random_nibbles(Phi.data_ptr(), Phi.numel(), 31, 0, stream))
    hip.check(lib.clv_fill_random_scales(sPhi.data_ptr(), sPhi.numel(), 32, 0, stream))
    hip.check(lib.clm4_transpose(Phi.data_ptr(), sPhi.data_ptr(), m, nn, PhiT.data_ptr(), sPhiT.data_ptr(), stream))

    def vec(n_, sd):
        qv_ = torch.empty(n_ // 2, dtype=torch.uint8, device=dev)
        sv_ = torch.empty(n_ // 64, dtype=torch.float32, device=dev)
        hip.check(lib.clv_fill_random_nibbles(qv_.data_ptr(), qv_.numel(), sd, 0, stream))
        hip.check(lib.clv_fill_random_scales(sv_.data_ptr(), sv_.numel(), sd + 1, 0, stream))
        return qv_, sv_
    (xq, xs_), (yq, ys_), (t1q, t1s), (t2q, t2s), (t3q, t3s) = vec(nn, 41), vec(m, 43), vec(m, 45), vec(m, 47), vec(nn, 49)

    def iht_iter():
        hip.check(lib.clm4_mvm(Phi.data_ptr(), sPhi.data_ptr(), m, nn, xq.data_ptr(), xs_.data_ptr(), t1q.data_ptr(), t1s.data_ptr(), None, stream))
        hip.check(lib.clv4_scale_and_add(yq.data_ptr(), ys_.data_ptr(), t1q.data_ptr(), t1s.data_ptr(), -1.0, m, t2q.data_ptr(), t2s.data_ptr(), None, stream))
        hip.check(lib.clm4_mvm(PhiT.data_ptr(), sPhiT.data_ptr(), nn, m, t2q.data_ptr(), t2s.data_ptr(), t3q.data_ptr(), t3s.data_ptr(), None, stream))
        hip.check(lib.clv4_scale_and_add(xq.data_ptr(), xs_.data_ptr(), t3q.data_ptr(), t3s.data_ptr(), 1e-3, nn, xq.data_ptr(), xs_.data_ptr(), None, stream))
        hip.check(lib.clv4_threshold(xq.data_ptr(), xs_.data_ptr(), nn, nn, m // 4, None, stream))
    i_ms = timeit(iht_iter, 100)
    # the reference's default build rounds stochastically: same loop, every re-quantisation drawing from one XORShift stream
    rng_state = hip.new_rng(5, 6)

    def iht_iter_st():
        rs = rng_state.ptr
        hip.check(lib.clm4_mvm(Phi.data_ptr(), sPhi.data_ptr(), m, nn, xq.data_ptr(), xs_.data_ptr(), t1q.data_ptr(), t1s.data_ptr(), rs, stream))
        hip.check(lib.clv4_scale_and_add(yq.data_ptr(), ys_.data_ptr(), t1q.data_ptr(), t1s.data_ptr(), -1.0, m, t2q.data_ptr(), t2s.data_ptr(), rs, stream))
        hip.check(lib.clm4_mvm(PhiT.data_ptr(), sPhiT.data_ptr(), nn, m, t2q.data_ptr(), t2s.data_ptr(), t3q.data_ptr(), t3s.data_ptr(), rs, stream))
        hip.check(lib.clv4_scale_and_add(xq.data_ptr(), xs_.data_ptr(), t3q.data_ptr(), t3s.data_ptr(), 1e-3, nn, xq.data_ptr(), xs_.data_ptr(), rs, stream))
        hip.check(lib.clv4_threshold(xq.data_ptr(), xs_.data_ptr(), nn, nn, m // 4, None, stream))
    s_ms = timeit(iht_iter_st, 100)
    # the same loop as ONE C call (clm4_iht enqueues all iterations from C++)
    import ctypes as C
    side = C.c_void_p()
    hip.check(lib.clv_stream_create(C.byref(side)))

    def iht_call(K=m // 4, iters=100, rs=None):
        hip.check(lib.clm4_iht(Phi.data_ptr(), sPhi.data_ptr(), PhiT.data_ptr(), sPhiT.data_ptr(), m, nn, xq.data_ptr(), xs_.data_ptr(), nn,
                               yq.data_ptr(), ys_.data_ptr(), t1q.data_ptr(), t1s.data_ptr(), t2q.data_ptr(), t2s.data_ptr(),
                               t3q.data_ptr(), t3s.data_ptr(), iters, K, 1e-3, 1, rs, side))
        hip.check(lib.clv_stream_sync(side))

    def iht_time(K, persistent, rs=None):
        # per-iteration time of ONE call with many iterations, by difference of two call lengths (the per-call cost -- a memset, the
        # launch, the matrix slices' way into LDS -- drops out); CLV_IHT_PERSISTENT is read per call (iht_persist.hip)
        os.environ["CLV_IHT_PERSISTENT"] = "1" if persistent else "0"
        try:
            iht_call(K, 100, rs)
            best = {}
            for iters in (100, 1100):
                best[iters] = 1e9
                for _ in range(3):
                    t0 = time.perf_counter()
                    iht_call(K, iters, rs)
                    best[iters] = min(best[iters], time.perf_counter() - t0)
            return (best[1100] - best[100]) / 1000 * 1e3, best[100] * 1e3
        finally:
            os.environ.pop("CLV_IHT_PERSISTENT", None)
    g_ms, g_call100_ms = iht_time(m // 4, True)                          # K = 1024: the figure of rounds 3-5
    g25_ms, _ = iht_time(nn // 4, True)                                  # K = 25 % of N = 2048: the reference's table (00_test.cpp:702, 750)
    gl_ms, gl_call100_ms = iht_time(m // 4, False)                       # the launch-per-step loop (iht4.hip): three launches per iteration
    gl25_ms, _ = iht_time(nn // 4, False)
    gst_ms, _ = iht_time(nn // 4, True, rng_state.ptr)                   # every re-quantisation drawing from one XORShift stream, same kernel
    glst_ms, _ = iht_time(nn // 4, False, rng_state.ptr)
    hip.check(lib.clv_stream_destroy(side))
    # the reference's published "4-bit" IHT: CloverMatrix4 with CloverVector8 vectors (02_bit04.cpp:140), whole loop from C++
    def vec8(n_, sd):
        qv_ = torch.empty(n_, dtype=torch.uint8, device=dev)
        sv_ = torch.empty(n_ // 64, dtype=torch.float32, device=dev)
        hip.check(lib.clv_fill_random_nibbles(qv_.data_ptr(), qv_.numel(), sd, 0, stream))
        hip.check(lib.clv_fill_random_scales(sv_.data_ptr(), sv_.numel(), sd + 1, 0, stream))
        return qv_, sv_
    (x8q, x8s), (y8q, y8s), (a8q, a8s), (b8q, b8s), (c8q, c8s) = vec8(nn, 61), vec8(m, 63), vec8(m, 65), vec8(m, 67), vec8(nn, 69)
    side8 = C.c_void_p()
    hip.check(lib.clv_stream_create(C.byref(side8)))

    def iht8_call(K=m // 4, iters=100, rs=None):
        hip.check(lib.clm4_iht_v8(Phi.data_ptr(), sPhi.data_ptr(), PhiT.data_ptr(), sPhiT.data_ptr(), m, nn, x8q.data_ptr(), x8s.data_ptr(), nn,
                                  y8q.data_ptr(), y8s.data_ptr(), a8q.data_ptr(), a8s.data_ptr(), b8q.data_ptr(), b8s.data_ptr(),
                                  c8q.data_ptr(), c8s.data_ptr(), iters, K, 1e-3, 1, rs, side8))
        hip.check(lib.clv_stream_sync(side8))

    def iht8_time(K, persistent, rs=None):                            # as iht_time: by difference of two call lengths
        os.environ["CLV_IHT_PERSISTENT"] = "1" if persistent else "0"
        try:
            iht8_call(K, 100, rs)
            best = {}
            for iters in (100, 1100):
                best[iters] = 1e9
                for _ in range(3):
                    t0 = time.perf_counter()
                    iht8_call(K, iters, rs)
                    best[iters] = min(best[iters], time.perf_counter() - t0)
            return (best[1100] - best[100]) / 1000 * 1e3
        finally:
            os.environ.pop("CLV_IHT_PERSISTENT", None)
    launches0 = lib.clv_iht_persistent_launches()
    g8_ms = iht8_time(m // 4, True)
    g8_25_ms = iht8_time(nn // 4, True)
    g8st_ms = iht8_time(nn // 4, True, rng_state.ptr)
    g8_persistent_calls = lib.clv_iht_persistent_launches() - launches0      # 21 if every one of these calls ran as one launch
    g8l_ms = iht8_time(nn // 4, False)
    g8lst_ms = iht8_time(nn // 4, False, rng_state.ptr)
    hip.check(lib.clv_stream_destroy(side8))
    iht8_bytes = 2 * (m * nn // 2 + 4 * (m // 64) * (nn // 64)) + (2 * nn + 3 * m) * 17 // 16
    iht_bytes = 2 * (m * nn // 2 + 4 * (m // 64) * (nn // 64)) + (2 * nn + 3 * m) * 9 // 16
    iht = {"ms_per_iteration": round(i_ms, 5), "GB/s": round(iht_bytes / i_ms / 1e6, 1),
           "ms_per_iteration_stochastic": round(s_ms, 5), "GB/s_stochastic": round(iht_bytes / s_ms / 1e6, 1),
           "ms_per_iteration_clm4_iht": round(g_ms, 5), "GB/s_clm4_iht": round(iht_bytes / g_ms / 1e6, 1),
           "clm4_iht": {"path": "one persistent launch, Phi and PhiT resident in LDS (iht_persist.hip)",
                        "us_per_iteration_K1024": round(g_ms * 1e3, 2), "us_per_iteration_K2048_reference_ratio": round(g25_ms * 1e3, 2),
                        "ms_per_call_100_iterations": round(g_call100_ms, 4), "us_per_iteration_stochastic_K2048": round(gst_ms * 1e3, 2),
                        "launch_per_step_loop": {"us_per_iteration_K1024": round(gl_ms * 1e3, 2), "us_per_iteration_K2048": round(gl25_ms * 1e3, 2),
                                                 "us_per_iteration_stochastic_K2048": round(glst_ms * 1e3, 2),
                                                 "ms_per_call_100_iterations": round(gl_call100_ms, 4)},
                        "method": "difference of a 1100- and a 100-iteration call, best of 3 each"},
           "ms_per_iteration_clm4_iht_v8": round(g8_ms, 5), "GB/s_clm4_iht_v8": round(iht8_bytes / g8_ms / 1e6, 1),
           "clm4_iht_v8": {"path": "one persistent launch (k_iht8_persist<ST>, iht_persist.hip)", "calls_that_ran_persistent_of_21": int(g8_persistent_calls),
                           "us_per_iteration_K1024": round(g8_ms * 1e3, 2), "us_per_iteration_K2048_reference_ratio": round(g8_25_ms * 1e3, 2),
                           "us_per_iteration_stochastic_K2048": round(g8st_ms * 1e3, 2),
                           "launch_per_step_loop": {"us_per_iteration_K2048": round(g8l_ms * 1e3, 2),
                                                    "us_per_iteration_stochastic_K2048": round(g8lst_ms * 1e3, 2)},
                           "method": "difference of a 1100- and a 100-iteration call, best of 3 each"},
           "note": "Q_IHT step sequence (mvm, scaleAndAdd, mvm^T, scaleAndAdd, threshold) at N=8192 (4096x8192), bytes counted like "
                   "01_measure.h:1117-1125; _v8 = the published configuration (4-bit matrix, 8-bit vectors); reference published "
                   "19.5 GB/s with 4 threads (performance.txt:581)"}
    iht["through_headers"] = iht_through_headers()
    try:
        iht["header_overhead_vs_clm4_iht"] = round(iht["through_headers"]["page_tracked"]["us_per_iteration"]["fast"] / (g_ms * 1e3), 3)
    except (KeyError, TypeError):
        pass
    del xs, ys, qa, qb, sa, sb
    torch.cuda.empty_cache()
    try:
        published = published_sizes(hip, torch, dev, stream)
    except Exception as e:                                          # noqa: BLE001
        published = {"failed": f"{type(e).__name__}: {e}"[:300]}
    return {
        "hbm_resident_n2^30": hbm,
        "published_sizes": published,
        "iht_iteration_N8192": iht,
        "footnote_cache_resident_n2^24": {
            "note": "BASELINE configs[1] sizes: the operands (76.5 MB / 18.9 MB) fit the 256 MiB Infinity Cache -- cache-resident, "
                    "launch-bound rates, NOT HBM-roofline claims (those are hbm_resident_n2^30 above)",
            "quantize": {"ms": round(q_ms, 5), "GB/s": round(4.5625 * n / q_ms / 1e6, 1)},
            "dot_fast": {"ms": round(f_ms, 5), "GB/s": round(1.125 * n / f_ms / 1e6, 1), "GFLOP/s": round(2 * n / f_ms / 1e6, 1)},
            "dot_exact": {"ms": round(e_ms, 5), "GB/s": round(1.125 * n / e_ms / 1e6, 1),
                          "note": "the reference's 16 sequential fma chains (131072 dependent fmas each at this n): latency-bound by definition"},
            "dot_fast_minus_exact_rel": float(abs(vals[0] - vals[1]) / max(abs(vals[1]), 1e-30)),
        },
    }


if __name__ == "__main__":
    main()
