#!/usr/bin/env python3
"""Per-kernel achieved bandwidth at HBM-resident sizes (operands >> 256 MiB Infinity Cache), printed as JSON.

Algorithmic bytes per element follow SURVEY 8(d): quantize/restore 4.5625, dot 1.125, scaleAndAdd 1.6875,
threshold 1.125 (nibbles + scales read and written once each), transpose 2 x (1/2 + 4/4096), matrix quantize 4.5625;
CloverMatrix8 (m8_*): quantize 4 + 1 + 4/4096, transpose 2 x (1 + 4/4096), mvm 1 + 4/4096 per matrix element;
CloverVector16 / CloverMatrix16 (f16_*): 2 bytes per element and no scales -- quantize / restore 4 + 2, scaleAndAdd 2 + 2 + 2, dot 2 + 2,
threshold 2 + 2 (read once, written once), matrix quantize 4 + 2, transpose 2 + 2, mvm 2 per matrix element + x + r;
CloverVector32 / CloverMatrix32 (f32_*): 4 bytes per element -- scaleAndAdd 4 + 4 + 4, dot 4 + 4, threshold 4 + 4, transpose 4 + 4, mvm 4 per
matrix element + x + r (+ u, t, r2 for the fused form).

The GEMM rows with 8-bit operands (m8_gemm_*, m4_gemm_m8_*, and their yardstick m4_gemm_i8_*: clm4_gemm on the int8-MFMA kernel of gemm4.hip)
are compute rows: ms, TOP/s = 2 M N K / time, and the fraction of the 5 POP/s dense int8 matrix peak (half the FP6 peak DESIGN.md 6 quotes).
They run first, and a run that asks for nothing else (KB_ONLY naming only GEMM rows) ends after them."""
import ctypes as C
import json
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from clover_amd.lib_binding import DOT_EXACT, DOT_FAST, CloverHip  # noqa: E402

hip = CloverHip(path=os.environ.get("CLV_LIB"))      # CLV_LIB: another build of the library, for same-box A/B runs
lib = hip.lib
vp = C.c_void_p


def timeit(fn, reps=10, rounds=5, warm=2):
    for _ in range(warm):
        fn()
    hip.sync()
    a, b = vp(), vp()
    hip.check(lib.clv_event_create(C.byref(a)))
    hip.check(lib.clv_event_create(C.byref(b)))
    ts = []
    for _ in range(rounds):
        hip.check(lib.clv_event_record(a, None))
        for _ in range(reps):
            fn()
        hip.check(lib.clv_event_record(b, None))
        hip.check(lib.clv_event_sync(b))
        ms = C.c_float()
        hip.check(lib.clv_event_elapsed_ms(a, b, C.byref(ms)))
        ts.append(ms.value / reps)
    return sorted(ts)[len(ts) // 2]


res = {}


ONLY = os.environ.get("KB_ONLY")      # substring filter, or several separated by commas: KB_ONLY=scale_and_add python tools/kernel_bench.py


def selected(name):
    return not ONLY or any(o in name for o in ONLY.split(","))


def rec(name, nbytes, fn, extra=None, reps=10):
    if not selected(name):
        return
    ms = timeit(fn, reps=reps)
    res[name] = {"ms": round(ms, 5), "GB/s": round(nbytes / ms / 1e6, 1), "frac_of_8TBs": round(nbytes / ms / 1e6 / 8000.0, 4)}
    if extra:
        res[name].update(extra)


# ---- GEMM with 8-bit operands on the int8 matrix cores (gemm8.hip): compute rows
INT8_PEAK_OPS = 5.0e15
GEMM_ROWS = ("m8_gemm_4096^3", "m8_gemm_8192^3", "m4_gemm_m8_8192^3", "m4_gemm_i8_8192^3")


def rec_gemm(name, G, fn):
    ms = timeit(fn, reps=50)
    ops = 2.0 * G ** 3
    res[name] = {"ms": round(ms, 5), "TOP/s": round(ops / ms / 1e9, 1), "frac_of_int8_peak": round(ops / (ms * 1e-3) / INT8_PEAK_OPS, 4)}


def gemm_operands(G, nibbles):
    """(values, tile scales) of a G x G operand: random bytes (nibbles in [-7, 7], so no byte is -128) and random scales"""
    q, s = hip.alloc(G * G // 2 if nibbles else G * G), hip.alloc(4 * (G // 64) ** 2)
    hip.check(lib.clv_fill_random_nibbles(q.ptr, q.nbytes, 71 + nibbles, 0, None))
    hip.check(lib.clv_fill_random_scales(s.ptr, (G // 64) ** 2, 73, 0, None))
    return q, s


def yardstick_i8():
    """clm4_gemm under CLV_GEMM_KERNEL=i8: the library reads that switch once per process, so the row runs in a child process of its own"""
    import subprocess
    env = dict(os.environ, CLV_GEMM_KERNEL="i8", KB_ONLY="m4_gemm_i8_8192^3", KB_GEMM_CHILD="1")
    out = subprocess.run([sys.executable, str(Path(__file__).resolve())], env=env, check=True, capture_output=True, text=True, timeout=600).stdout
    return json.loads(out)["m4_gemm_i8_8192^3"]


if any(selected(r) for r in GEMM_ROWS):
    if os.environ.get("KB_GEMM_CHILD"):
        G = 8192
        (a4, sa4), (b4, sb4), c = gemm_operands(G, True), gemm_operands(G, True), hip.alloc(4 * G * G)
        rec_gemm("m4_gemm_i8_8192^3", G, lambda: hip.check(lib.clm4_gemm(a4.ptr, sa4.ptr, G, G, b4.ptr, sb4.ptr, G, c.ptr, None)))
        print(json.dumps(res))
        sys.exit(0)
    # the yardstick before and after the new rows: the same box, the same minutes
    runs = [yardstick_i8()] if selected("m4_gemm_i8_8192^3") else []
    for G in (4096, 8192):
        (a8, sa8), (b8, sb8), c = gemm_operands(G, False), gemm_operands(G, False), hip.alloc(4 * G * G)
        if selected(f"m8_gemm_{G}^3"):
            rec_gemm(f"m8_gemm_{G}^3", G, lambda: hip.check(lib.clm8_gemm(a8.ptr, sa8.ptr, G, G, b8.ptr, sb8.ptr, G, c.ptr, None)))
        if G == 8192 and selected("m4_gemm_m8_8192^3"):
            a4, sa4 = gemm_operands(G, True)
            rec_gemm("m4_gemm_m8_8192^3", G, lambda: hip.check(lib.clm4_gemm_m8(a4.ptr, sa4.ptr, G, G, b8.ptr, sb8.ptr, G, c.ptr, None)))
            del a4, sa4
        del a8, sa8, b8, sb8, c
    if runs:
        runs.append(yardstick_i8())
        res["m4_gemm_i8_8192^3"] = dict(min(runs, key=lambda r: r["ms"]), ms_before_and_after=[r["ms"] for r in runs],
                                        note="clm4_gemm under CLV_GEMM_KERNEL=i8 (k_m4_gemm_mfma), in a child process before and after the rows "
                                             "above; the faster of the two runs")
    if ONLY and all(any(o in r for r in GEMM_ROWS) for o in ONLY.split(",")):
        print(json.dumps(res, indent=1))
        sys.exit(0)


# ---- several vectors with one CloverMatrix4 (mvm_batch4.hip): every row pairs the batch call, on the batched kernel (CLV_MVM_BATCH=1),
# with the same vectors issued as single calls in the same session.  A run that names only these rows (KB_ONLY=mvm_batch,mvm_saa_batch,
# iht_batch) ends after them.  The *_st_* rows are the same pairs with a generator (stochastic rounding): the batch call on the stochastic
# batched kernel against the g single stochastic calls, same session, same vectors, one state (KB_ONLY=_st_ runs only them).
BATCH_ROWS = ("mvm_batch2_32768^2", "mvm_batch4_32768^2", "mvm_batch8_32768^2", "mvm_batch2_65536^2", "mvm_batch4_65536^2", "mvm_batch8_65536^2",
              "mvm_saa_batch2_8192x4096", "mvm_saa_batch4_8192x4096", "mvm_saa_batch8_8192x4096", "iht_batch8_N8192")
IHT_SHAPE_ROWS = BATCH_ROWS[6:] + tuple(r.replace("batch2_", "batch2_st_").replace("batch4_", "batch4_st_").replace("batch8_", "batch8_st_") for r in BATCH_ROWS[6:])
BATCH_ROWS = BATCH_ROWS + tuple(r.replace("batch2_", "batch2_st_").replace("batch4_", "batch4_st_").replace("batch8_", "batch8_st_") for r in BATCH_ROWS)


def rounds_of(fn, reps=10, rounds=5, warm=2):
    """the five round values of timeit (ms per call), not only their median"""
    for _ in range(warm):
        fn()
    hip.sync()
    a, b = vp(), vp()
    hip.check(lib.clv_event_create(C.byref(a)))
    hip.check(lib.clv_event_create(C.byref(b)))
    ts = []
    for _ in range(rounds):
        hip.check(lib.clv_event_record(a, None))
        for _ in range(reps):
            fn()
        hip.check(lib.clv_event_record(b, None))
        hip.check(lib.clv_event_sync(b))
        ms = C.c_float()
        hip.check(lib.clv_event_elapsed_ms(a, b, C.byref(ms)))
        ts.append(ms.value / reps)
    return sorted(ts)


def rec_pair(name, nbytes_single, g, single, batch, reps=10, per=1, alias=None):
    """single: the g single calls; batch: the one batch call.  per: divides both (iterations of a loop call); alias: a second name KB_ONLY
    may select the row by"""
    if not (selected(name) or (alias and selected(alias))):
        return
    os.environ.pop("CLV_MVM_BATCH", None)
    one = [t / per for t in rounds_of(single, reps=reps)]
    os.environ["CLV_MVM_BATCH"] = "1"
    try:
        many = [t / per for t in rounds_of(batch, reps=reps)]
    finally:
        os.environ.pop("CLV_MVM_BATCH", None)
    o, m, spread = one[len(one) // 2], many[len(many) // 2], one[-1] - one[0]
    res[name] = {"vectors": g, "batch_ms": round(m, 5), "single_calls_ms": round(o, 5), "single_calls_rounds_ms": [round(t, 5) for t in one],
                 "batch_rounds_ms": [round(t, 5) for t in many], "single_calls_spread_ms": round(spread, 5), "speedup": round(o / m, 3),
                 "batch_faster_by_more_than_the_spread": bool(o - m > spread),
                 "GB/s_per_vector_batch": round(g * nbytes_single / m / 1e6, 1), "GB/s_single_calls": round(g * nbytes_single / o / 1e6, 1)}


def ptrs(bufs):
    return (vp * len(bufs))(*[b.ptr for b in bufs])


def vec_set(count, n, seed):
    out = []
    for j in range(count):
        q, s = hip.alloc(n // 2), hip.alloc(n // 16)
        hip.check(lib.clv_fill_random_nibbles(q.ptr, q.nbytes, seed + 2 * j, 0, None))
        hip.check(lib.clv_fill_random_scales(s.ptr, s.nbytes // 4, seed + 2 * j + 1, 0, None))
        out.append((q, s))
    return out


if any(selected(r) for r in BATCH_ROWS):
    for nb in (32768, 65536):
        if not any(selected(f"mvm_batch{g}_{t}{nb}^2") for g in (2, 4, 8) for t in ("", "st_")):
            continue
        bA, bsA = hip.alloc(nb * nb // 2), hip.alloc((nb // 64) ** 2 * 4)
        hip.check(lib.clv_fill_random_nibbles(bA.ptr, bA.nbytes, 41, 0, None))
        hip.check(lib.clv_fill_random_scales(bsA.ptr, bsA.nbytes // 4, 42, 0, None))
        bx, br = vec_set(8, nb, 300), vec_set(8, nb, 400)
        one_b = nb * nb // 2 + 4 * (nb // 64) ** 2 + 2 * (nb // 2 + nb // 16)
        for g in (2, 4, 8):
            ax, asx, ar, asr = ptrs([v[0] for v in bx[:g]]), ptrs([v[1] for v in bx[:g]]), ptrs([v[0] for v in br[:g]]), ptrs([v[1] for v in br[:g]])

            def singles(g=g):
                for j in range(g):
                    hip.check(lib.clm4_mvm(bA.ptr, bsA.ptr, nb, nb, bx[j][0].ptr, bx[j][1].ptr, br[j][0].ptr, br[j][1].ptr, None, None))
            rec_pair(f"mvm_batch{g}_{nb}^2", one_b, g, singles,
                     lambda g=g, a=(ax, asx, ar, asr): hip.check(lib.clm4_mvm_batch(bA.ptr, bsA.ptr, nb, nb, g, a[0], a[1], a[2], a[3], None, None)),
                     reps=10 if nb == 32768 else 4)
            st = hip.new_rng(1, 2)

            def singles_st(g=g, st=st):
                for j in range(g):
                    hip.check(lib.clm4_mvm(bA.ptr, bsA.ptr, nb, nb, bx[j][0].ptr, bx[j][1].ptr, br[j][0].ptr, br[j][1].ptr, st.ptr, None))
            rec_pair(f"mvm_batch{g}_st_{nb}^2", one_b, g, singles_st,
                     lambda g=g, a=(ax, asx, ar, asr), st=st: hip.check(lib.clm4_mvm_batch(bA.ptr, bsA.ptr, nb, nb, g, a[0], a[1], a[2], a[3], st.ptr, None)),
                     reps=10 if nb == 32768 else 4)
        del bA, bsA, bx, br
    # the IHT shape (N = 8192: Phi 4096 x 8192, cache-resident): the x += mu Phi' t2 step for 8 signals, and the whole loop
    im, inn, ig, iters = 4096, 8192, 8, 20
    if any(selected(r) for r in IHT_SHAPE_ROWS):
        P, sP, PT, sPT = hip.alloc(im * inn // 2), hip.alloc(4 * (im // 64) * (inn // 64)), hip.alloc(im * inn // 2), hip.alloc(4 * (im // 64) * (inn // 64))
        hip.check(lib.clv_fill_random_nibbles(P.ptr, P.nbytes, 51, 0, None))
        hip.check(lib.clv_fill_random_scales(sP.ptr, sP.nbytes // 4, 52, 0, None))
        hip.check(lib.clm4_transpose(P.ptr, sP.ptr, im, inn, PT.ptr, sPT.ptr, None))
        vy, vx, vt1, vt2, vt3 = vec_set(ig, im, 500), vec_set(ig, inn, 600), vec_set(ig, im, 700), vec_set(ig, im, 800), vec_set(ig, inn, 900)
        A = {k: (ptrs([p[0] for p in v]), ptrs([p[1] for p in v])) for k, v in dict(y=vy, x=vx, t1=vt1, t2=vt2, t3=vt3).items()}
        vr = vec_set(ig, inn, 1000)
        Ar = (ptrs([p[0] for p in vr]), ptrs([p[1] for p in vr]))
        saa_b = im * inn // 2 + 4 * (im // 64) * (inn // 64) + (im // 2 + im // 16) + 3 * (inn // 2 + inn // 16)

        for sg in (2, 4, 8):
            def saa_singles(sg=sg):
                for j in range(sg):
                    hip.check(lib.clm4_mvm_scale_and_add(PT.ptr, sPT.ptr, inn, im, vt2[j][0].ptr, vt2[j][1].ptr, vx[j][0].ptr, vx[j][1].ptr, 0.002,
                                                         vt3[j][0].ptr, vt3[j][1].ptr, vr[j][0].ptr, vr[j][1].ptr, None, None))
            rec_pair(f"mvm_saa_batch{sg}_8192x4096", saa_b, sg, saa_singles,
                     lambda sg=sg: hip.check(lib.clm4_mvm_scale_and_add_batch(PT.ptr, sPT.ptr, inn, im, sg, A["t2"][0], A["t2"][1], A["x"][0], A["x"][1], 0.002,
                                                                              A["t3"][0], A["t3"][1], Ar[0], Ar[1], None, None)), reps=20)
            st = hip.new_rng(1, 2)

            def saa_singles_st(sg=sg, st=st):
                for j in range(sg):
                    hip.check(lib.clm4_mvm_scale_and_add(PT.ptr, sPT.ptr, inn, im, vt2[j][0].ptr, vt2[j][1].ptr, vx[j][0].ptr, vx[j][1].ptr, 0.002,
                                                         vt3[j][0].ptr, vt3[j][1].ptr, vr[j][0].ptr, vr[j][1].ptr, st.ptr, None))
            rec_pair(f"mvm_saa_batch{sg}_st_8192x4096", saa_b, sg, saa_singles_st,
                     lambda sg=sg, st=st: hip.check(lib.clm4_mvm_scale_and_add_batch(PT.ptr, sPT.ptr, inn, im, sg, A["t2"][0], A["t2"][1], A["x"][0], A["x"][1],
                                                                                     0.002, A["t3"][0], A["t3"][1], Ar[0], Ar[1], st.ptr, None)), reps=20)

        def iht_singles():
            for j in range(ig):
                hip.check(lib.clm4_iht(P.ptr, sP.ptr, PT.ptr, sPT.ptr, im, inn, vx[j][0].ptr, vx[j][1].ptr, inn, vy[j][0].ptr, vy[j][1].ptr,
                                       vt1[j][0].ptr, vt1[j][1].ptr, vt2[j][0].ptr, vt2[j][1].ptr, vt3[j][0].ptr, vt3[j][1].ptr, iters, im // 4, 0.002, 1,
                                       None, None))
        rec_pair("iht_batch8_N8192", 2 * (im * inn // 2), ig, iht_singles,
                 lambda: hip.check(lib.clm4_iht_batch(P.ptr, sP.ptr, PT.ptr, sPT.ptr, im, inn, ig, A["x"][0], A["x"][1], inn, A["y"][0], A["y"][1],
                                                      A["t1"][0], A["t1"][1], A["t2"][0], A["t2"][1], A["t3"][0], A["t3"][1], iters, im // 4, 0.002, 1,
                                                      None, None)), reps=2, per=iters)
        if "iht_batch8_N8192" in res:
            res["iht_batch8_N8192"]["note"] = (f"ms per iteration for all 8 signals, calls of {iters} iterations, K = m / 4, FAST threshold; the single calls are "
                                               "8 x clm4_iht as the library runs it (the persistent kernel at this size)")
        ist = hip.new_rng(1, 2)

        def iht_singles_st():
            for j in range(ig):
                hip.check(lib.clm4_iht(P.ptr, sP.ptr, PT.ptr, sPT.ptr, im, inn, vx[j][0].ptr, vx[j][1].ptr, inn, vy[j][0].ptr, vy[j][1].ptr,
                                       vt1[j][0].ptr, vt1[j][1].ptr, vt2[j][0].ptr, vt2[j][1].ptr, vt3[j][0].ptr, vt3[j][1].ptr, iters, im // 4, 0.002, 1,
                                       ist.ptr, None))
        rec_pair("iht_batch8_st_N8192", 2 * (im * inn // 2), ig, iht_singles_st,
                 lambda: hip.check(lib.clm4_iht_batch(P.ptr, sP.ptr, PT.ptr, sPT.ptr, im, inn, ig, A["x"][0], A["x"][1], inn, A["y"][0], A["y"][1],
                                                      A["t1"][0], A["t1"][1], A["t2"][0], A["t2"][1], A["t3"][0], A["t3"][1], iters, im // 4, 0.002, 1,
                                                      ist.ptr, None)), reps=2, per=iters)
        if "iht_batch8_st_N8192" in res:
            res["iht_batch8_st_N8192"]["note"] = (f"ms per iteration for all 8 signals, calls of {iters} iterations, K = m / 4, FAST threshold, one generator; the "
                                                  "single calls are 8 x clm4_iht with that generator as the library runs it (the stochastic persistent kernel)")
        del P, sP, PT, sPT, vy, vx, vt1, vt2, vt3, vr
    if ONLY and all(any(o in r for r in BATCH_ROWS) for o in ONLY.split(",")):
        print(json.dumps(res, indent=1))
        sys.exit(0)


# ---- several CloverVector8 with one CloverMatrix4 (mvm_batch8.hip): the rows above for the configuration the reference publishes as "4-bit".
# Every row pairs the batch call under CLV_MVM_BATCH=1 with the same vectors issued as single calls in the same session; the *_st_* twins
# run with a generator.  A run that names only these rows (KB_ONLY=mvm_v8,iht_v8) ends after them.
V8_BATCH_ROWS = tuple(f"mvm_v8_batch{g}_{t}{nb}^2" for nb in (32768, 65536) for g in (2, 4, 8) for t in ("", "st_")) + \
    tuple(f"mvm_v8_saa_batch{g}_{t}8192x4096" for g in (2, 4, 8) for t in ("", "st_")) + ("iht_v8_batch8_N8192", "iht_v8_batch8_st_N8192")


def vec8_set(count, n, seed):
    """count x (n int8 in [-127, 127], n / 64 scales): fp32 integers quantised to CloverVector8 on the device"""
    out, f = [], hip.alloc(4 * n)
    for j in range(count):
        q, s = hip.alloc(n), hip.alloc(n // 16)
        hip.check(lib.clv_fill_random_ints_f32(f.ptr, n, 100, seed + j, 0, None))
        hip.check(lib.clv8_quantize(f.ptr, n, q.ptr, s.ptr, None, None))
        out.append((q, s))
    hip.sync()
    return out


if any(selected(r) for r in V8_BATCH_ROWS):
    for nb in (32768, 65536):
        if not any(selected(f"mvm_v8_batch{g}_{t}{nb}^2") for g in (2, 4, 8) for t in ("", "st_")):
            continue
        bA, bsA = hip.alloc(nb * nb // 2), hip.alloc((nb // 64) ** 2 * 4)
        hip.check(lib.clv_fill_random_nibbles(bA.ptr, bA.nbytes, 41, 0, None))
        hip.check(lib.clv_fill_random_scales(bsA.ptr, bsA.nbytes // 4, 42, 0, None))
        bx, br = vec8_set(8, nb, 300), vec8_set(8, nb, 400)
        one_b = nb * nb // 2 + 4 * (nb // 64) ** 2 + 2 * (nb + nb // 16)
        for g in (2, 4, 8):
            ax, asx, ar, asr = ptrs([v[0] for v in bx[:g]]), ptrs([v[1] for v in bx[:g]]), ptrs([v[0] for v in br[:g]]), ptrs([v[1] for v in br[:g]])
            for tag, st in (("", None), ("st_", hip.new_rng(1, 2))):
                sp = st.ptr if st else None

                def singles(g=g, sp=sp):
                    for j in range(g):
                        hip.check(lib.clm4_mvm_v8(bA.ptr, bsA.ptr, nb, nb, bx[j][0].ptr, bx[j][1].ptr, br[j][0].ptr, br[j][1].ptr, sp, None))
                rec_pair(f"mvm_v8_batch{g}_{tag}{nb}^2", one_b, g, singles,
                         lambda g=g, a=(ax, asx, ar, asr), sp=sp: hip.check(lib.clm4_mvm_v8_batch(bA.ptr, bsA.ptr, nb, nb, g, a[0], a[1], a[2], a[3], sp, None)),
                         reps=10 if nb == 32768 else 4)
        del bA, bsA, bx, br
    # the IHT shape (N = 8192: Phi 4096 x 8192, cache-resident): the x += mu Phi' t2 step for 2, 4 and 8 signals, and the whole loop for 8
    im, inn, ig, iters = 4096, 8192, 8, 20
    if any(selected(r) for r in V8_BATCH_ROWS[12:]):
        P, sP, PT, sPT = hip.alloc(im * inn // 2), hip.alloc(4 * (im // 64) * (inn // 64)), hip.alloc(im * inn // 2), hip.alloc(4 * (im // 64) * (inn // 64))
        hip.check(lib.clv_fill_random_nibbles(P.ptr, P.nbytes, 51, 0, None))
        hip.check(lib.clv_fill_random_scales(sP.ptr, sP.nbytes // 4, 52, 0, None))
        hip.check(lib.clm4_transpose(P.ptr, sP.ptr, im, inn, PT.ptr, sPT.ptr, None))
        vy, vx, vt1, vt2, vt3, vr = (vec8_set(ig, n, seed) for n, seed in ((im, 500), (inn, 600), (im, 700), (im, 800), (inn, 900), (inn, 1000)))
        A = {k: (ptrs([p[0] for p in v]), ptrs([p[1] for p in v])) for k, v in dict(y=vy, x=vx, t1=vt1, t2=vt2, t3=vt3, r=vr).items()}
        saa_b = im * inn // 2 + 4 * (im // 64) * (inn // 64) + (im + im // 16) + 3 * (inn + inn // 16)
        for tag, st in (("", None), ("st_", hip.new_rng(1, 2))):
            sp = st.ptr if st else None
            for sg in (2, 4, 8):
                def saa_singles(sg=sg, sp=sp):
                    for j in range(sg):
                        hip.check(lib.clm4_mvm_v8_scale_and_add(PT.ptr, sPT.ptr, inn, im, vt2[j][0].ptr, vt2[j][1].ptr, vx[j][0].ptr, vx[j][1].ptr, 0.002,
                                                                vt3[j][0].ptr, vt3[j][1].ptr, vr[j][0].ptr, vr[j][1].ptr, sp, None))
                rec_pair(f"mvm_v8_saa_batch{sg}_{tag}8192x4096", saa_b, sg, saa_singles,
                         lambda sg=sg, sp=sp: hip.check(lib.clm4_mvm_v8_scale_and_add_batch(PT.ptr, sPT.ptr, inn, im, sg, A["t2"][0], A["t2"][1], A["x"][0],
                                                                                            A["x"][1], 0.002, A["t3"][0], A["t3"][1], A["r"][0], A["r"][1],
                                                                                            sp, None)), reps=20)

            def iht_singles(sp=sp):
                for j in range(ig):
                    hip.check(lib.clm4_iht_v8(P.ptr, sP.ptr, PT.ptr, sPT.ptr, im, inn, vx[j][0].ptr, vx[j][1].ptr, inn, vy[j][0].ptr, vy[j][1].ptr,
                                              vt1[j][0].ptr, vt1[j][1].ptr, vt2[j][0].ptr, vt2[j][1].ptr, vt3[j][0].ptr, vt3[j][1].ptr, iters, im // 4, 0.002,
                                              1, sp, None))
            name = f"iht_v8_batch8_{tag}N8192"
            before = lib.clv_iht_persistent_launches()
            rec_pair(name, 2 * (im * inn // 2), ig, iht_singles,
                     lambda sp=sp: hip.check(lib.clm4_iht_v8_batch(P.ptr, sP.ptr, PT.ptr, sPT.ptr, im, inn, ig, A["x"][0], A["x"][1], inn, A["y"][0], A["y"][1],
                                                                   A["t1"][0], A["t1"][1], A["t2"][0], A["t2"][1], A["t3"][0], A["t3"][1], iters, im // 4,
                                                                   0.002, 1, sp, None)), reps=2, per=iters)
            if name in res:
                res[name]["single_calls_took_the_persistent_kernel"] = bool(lib.clv_iht_persistent_launches() > before)
                res[name]["note"] = (f"ms per iteration for all 8 signals, calls of {iters} iterations, K = m / 4, FAST threshold" +
                                     (", one generator" if st else "") + "; the single calls are 8 x clm4_iht_v8 as the library runs it")
        del P, sP, PT, sPT, vy, vx, vt1, vt2, vt3, vr
    if ONLY and all(any(o in r for r in V8_BATCH_ROWS) for o in ONLY.split(",")):
        print(json.dumps(res, indent=1))
        sys.exit(0)


# ---- several CloverVector8 with one CloverMatrix8 (matrix8_batch.hip): the pure 8-bit path.  Every row pairs the batch call under
# CLV_MVM_BATCH=1 with the same vectors issued as single calls (clm8_mvm, clm8_mvm_scale_and_add, clm8_iht) in the same session; the *_st_*
# twins run with a generator.  The fused rows run at 8192 x 4096 (32 MiB: cache-resident) and at 65536^2 (4 GiB: streamed).
# KB_ONLY=m8_mvm_batch,m8_iht_batch selects all of them (the m8_mvm_saa_batch rows answer to m8_mvm_batch too) and the run ends after them.
M8_BATCH_ROWS = tuple(f"m8_mvm_batch{g}_{t}{nb}^2" for nb in (32768, 65536) for g in (2, 4, 8) for t in ("", "st_")) + \
    tuple(f"m8_mvm_saa_batch{g}_{t}{shape}" for shape in ("8192x4096", "65536^2") for g in (2, 4, 8) for t in ("", "st_")) + \
    ("m8_iht_batch8_N8192", "m8_iht_batch8_st_N8192")


def m8_selected(name):
    return selected(name) or selected(name.replace("_saa", ""))


def m8_matrix(rows, cols, seed):
    q, s = hip.alloc(rows * cols), hip.alloc(4 * (rows // 64) * (cols // 64))
    hip.check(lib.clv_fill_random_nibbles(q.ptr, q.nbytes, seed, 0, None))
    hip.check(lib.clv_fill_random_scales(s.ptr, s.nbytes // 4, seed + 1, 0, None))
    return q, s


if any(m8_selected(r) for r in M8_BATCH_ROWS):
    for nb in (32768, 65536):
        if not any(m8_selected(r) for r in M8_BATCH_ROWS if r.endswith(f"_{nb}^2")):
            continue
        bA, bsA = m8_matrix(nb, nb, 41)
        bx, br, bu, bt = vec8_set(8, nb, 300), vec8_set(8, nb, 400), vec8_set(8, nb, 500), vec8_set(8, nb, 600)
        one_b = nb * nb + 4 * (nb // 64) ** 2 + 2 * (nb + nb // 16)
        for g in (2, 4, 8):
            ax, asx, ar, asr = ptrs([v[0] for v in bx[:g]]), ptrs([v[1] for v in bx[:g]]), ptrs([v[0] for v in br[:g]]), ptrs([v[1] for v in br[:g]])
            au, asu, at, ast = ptrs([v[0] for v in bu[:g]]), ptrs([v[1] for v in bu[:g]]), ptrs([v[0] for v in bt[:g]]), ptrs([v[1] for v in bt[:g]])
            for tag, st in (("", None), ("st_", hip.new_rng(1, 2))):
                sp = st.ptr if st else None

                def singles(g=g, sp=sp):
                    for j in range(g):
                        hip.check(lib.clm8_mvm(bA.ptr, bsA.ptr, nb, nb, bx[j][0].ptr, bx[j][1].ptr, br[j][0].ptr, br[j][1].ptr, sp, None))
                rec_pair(f"m8_mvm_batch{g}_{tag}{nb}^2", one_b, g, singles,
                         lambda g=g, a=(ax, asx, ar, asr), sp=sp: hip.check(lib.clm8_mvm_batch(bA.ptr, bsA.ptr, nb, nb, g, a[0], a[1], a[2], a[3], sp, None)),
                         reps=10 if nb == 32768 else 4)
                if nb != 65536:
                    continue

                def saa_singles(g=g, sp=sp):
                    for j in range(g):
                        hip.check(lib.clm8_mvm_scale_and_add(bA.ptr, bsA.ptr, nb, nb, bx[j][0].ptr, bx[j][1].ptr, bu[j][0].ptr, bu[j][1].ptr, 0.002,
                                                             bt[j][0].ptr, bt[j][1].ptr, br[j][0].ptr, br[j][1].ptr, sp, None))
                name = f"m8_mvm_saa_batch{g}_{tag}{nb}^2"
                rec_pair(name, one_b + 3 * (nb + nb // 16), g, saa_singles,
                         lambda g=g, a=(ax, asx, au, asu, at, ast, ar, asr), sp=sp: hip.check(lib.clm8_mvm_scale_and_add_batch(
                             bA.ptr, bsA.ptr, nb, nb, g, a[0], a[1], a[2], a[3], 0.002, a[4], a[5], a[6], a[7], sp, None)),
                         reps=4, alias=name.replace("_saa", ""))
        del bA, bsA, bx, br, bu, bt
    # the IHT shape (N = 8192: Phi 4096 x 8192, 32 MiB, cache-resident): the x += mu Phi' t2 step for 2, 4 and 8 signals, and the whole loop for 8
    im, inn, ig, iters = 4096, 8192, 8, 20
    if any(m8_selected(r) for r in M8_BATCH_ROWS if r.endswith("8192x4096") or r.endswith("N8192")):
        (P, sP), PT, sPT = m8_matrix(im, inn, 51), hip.alloc(im * inn), hip.alloc(4 * (im // 64) * (inn // 64))
        hip.check(lib.clm8_transpose(P.ptr, sP.ptr, im, inn, PT.ptr, sPT.ptr, None))
        vy, vx, vt1, vt2, vt3, vr = (vec8_set(ig, n, seed) for n, seed in ((im, 500), (inn, 600), (im, 700), (im, 800), (inn, 900), (inn, 1000)))
        A = {k: (ptrs([p[0] for p in v]), ptrs([p[1] for p in v])) for k, v in dict(y=vy, x=vx, t1=vt1, t2=vt2, t3=vt3, r=vr).items()}
        saa_b = im * inn + 4 * (im // 64) * (inn // 64) + (im + im // 16) + 3 * (inn + inn // 16)
        for tag, st in (("", None), ("st_", hip.new_rng(1, 2))):
            sp = st.ptr if st else None
            for sg in (2, 4, 8):
                def saa_singles(sg=sg, sp=sp):
                    for j in range(sg):
                        hip.check(lib.clm8_mvm_scale_and_add(PT.ptr, sPT.ptr, inn, im, vt2[j][0].ptr, vt2[j][1].ptr, vx[j][0].ptr, vx[j][1].ptr, 0.002,
                                                             vt3[j][0].ptr, vt3[j][1].ptr, vr[j][0].ptr, vr[j][1].ptr, sp, None))
                name = f"m8_mvm_saa_batch{sg}_{tag}8192x4096"
                rec_pair(name, saa_b, sg, saa_singles,
                         lambda sg=sg, sp=sp: hip.check(lib.clm8_mvm_scale_and_add_batch(PT.ptr, sPT.ptr, inn, im, sg, A["t2"][0], A["t2"][1], A["x"][0],
                                                                                         A["x"][1], 0.002, A["t3"][0], A["t3"][1], A["r"][0], A["r"][1],
                                                                                         sp, None)), reps=20, alias=name.replace("_saa", ""))

            def iht_singles(sp=sp):
                for j in range(ig):
                    hip.check(lib.clm8_iht(P.ptr, sP.ptr, PT.ptr, sPT.ptr, im, inn, vx[j][0].ptr, vx[j][1].ptr, inn, vy[j][0].ptr, vy[j][1].ptr,
                                           vt1[j][0].ptr, vt1[j][1].ptr, vt2[j][0].ptr, vt2[j][1].ptr, vt3[j][0].ptr, vt3[j][1].ptr, iters, im // 4, 0.002,
                                           1, sp, None))
            name = f"m8_iht_batch8_{tag}N8192"
            rec_pair(name, 2 * im * inn, ig, iht_singles,
                     lambda sp=sp: hip.check(lib.clm8_iht_batch(P.ptr, sP.ptr, PT.ptr, sPT.ptr, im, inn, ig, A["x"][0], A["x"][1], inn, A["y"][0], A["y"][1],
                                                                A["t1"][0], A["t1"][1], A["t2"][0], A["t2"][1], A["t3"][0], A["t3"][1], iters, im // 4,
                                                                0.002, 1, sp, None)), reps=2, per=iters)
            if name in res:
                res[name]["note"] = (f"ms per iteration for all 8 signals, calls of {iters} iterations, K = m / 4, FAST threshold" +
                                     (", one generator" if st else "") + "; the single calls are 8 x clm8_iht (three launches per iteration each)")
        del P, sP, PT, sPT, vy, vx, vt1, vt2, vt3, vr
    if ONLY and all(any(o in r or o in r.replace("_saa", "") for r in M8_BATCH_ROWS) for o in ONLY.split(",")):
        print(json.dumps(res, indent=1))
        sys.exit(0)


# ---- A' x straight from A (mvm_t4.hip).  Per size three rows from ONE session, the same matrix and the same vectors, their rounds ALTERNATED
# (a round of each in turn, so a drift of the box hits all three alike): m4_mvm_transposed_N (one clm4_mvm_transposed), m4_transpose_then_mvm_N
# (clm4_transpose + clm4_mvm on the result: the only other way to A' x from A) and m4_mvm_held_transpose_N (clm4_mvm on an A' that is already
# there: what holding the second matrix buys).  iht_one_matrix_*: clm4_iht_one_matrix against clm4_iht, ms per iteration.
# KB_ONLY=mvm_transposed,transpose_then_mvm,held_transpose,iht_one_matrix selects them and the run ends after them.
MVT_SIZES = (8192, 32768, 65536)
MVT_ROWS = tuple(f"{k}_{nb}" for nb in MVT_SIZES for k in ("m4_mvm_transposed", "m4_transpose_then_mvm", "m4_mvm_held_transpose")) + \
    ("iht_one_matrix_N8192", "iht_one_matrix_gd_32768^2")


def alternated(fns, reps, rounds=5, warm=2):
    """per function the sorted round values (ms per call); round i of every function before round i + 1 of any"""
    for fn in fns:
        for _ in range(warm):
            fn()
    hip.sync()
    a, b = vp(), vp()
    hip.check(lib.clv_event_create(C.byref(a)))
    hip.check(lib.clv_event_create(C.byref(b)))
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            hip.check(lib.clv_event_record(a, None))
            for _ in range(reps):
                fn()
            hip.check(lib.clv_event_record(b, None))
            hip.check(lib.clv_event_sync(b))
            ms = C.c_float()
            hip.check(lib.clv_event_elapsed_ms(a, b, C.byref(ms)))
            ts[i].append(ms.value / reps)
    return [sorted(t) for t in ts]


if any(selected(r) for r in MVT_ROWS):
    for nb in MVT_SIZES:
        if not any(selected(r) for r in MVT_ROWS if r.endswith(f"_{nb}")):
            continue
        tA, tsA, tAt, tsAt = hip.alloc(nb * nb // 2), hip.alloc(4 * (nb // 64) ** 2), hip.alloc(nb * nb // 2), hip.alloc(4 * (nb // 64) ** 2)
        hip.check(lib.clv_fill_random_nibbles(tA.ptr, tA.nbytes, 61, 0, None))
        hip.check(lib.clv_fill_random_scales(tsA.ptr, tsA.nbytes // 4, 62, 0, None))
        (tx, tsx), (tr, tsr) = vec_set(1, nb, 310)[0], vec_set(1, nb, 320)[0]
        hip.check(lib.clm4_transpose(tA.ptr, tsA.ptr, nb, nb, tAt.ptr, tsAt.ptr, None))

        def direct():
            hip.check(lib.clm4_mvm_transposed(tA.ptr, tsA.ptr, nb, nb, tx.ptr, tsx.ptr, tr.ptr, tsr.ptr, None, None))

        def pair():
            hip.check(lib.clm4_transpose(tA.ptr, tsA.ptr, nb, nb, tAt.ptr, tsAt.ptr, None))
            hip.check(lib.clm4_mvm(tAt.ptr, tsAt.ptr, nb, nb, tx.ptr, tsx.ptr, tr.ptr, tsr.ptr, None, None))

        def held():
            hip.check(lib.clm4_mvm(tAt.ptr, tsAt.ptr, nb, nb, tx.ptr, tsx.ptr, tr.ptr, tsr.ptr, None, None))
        d, p, h = alternated((direct, pair, held), reps=20 if nb == 8192 else 10 if nb == 32768 else 4)
        one_b = nb * nb // 2 + 4 * (nb // 64) ** 2 + 2 * (nb // 2 + nb // 16)
        md, mp, mh = d[len(d) // 2], p[len(p) // 2], h[len(h) // 2]
        for name, t, m, nbytes in ((f"m4_mvm_transposed_{nb}", d, md, one_b), (f"m4_transpose_then_mvm_{nb}", p, mp, 3 * one_b),
                                   (f"m4_mvm_held_transpose_{nb}", h, mh, one_b)):
            res[name] = {"ms": round(m, 5), "rounds_ms": [round(v, 5) for v in t], "spread_ms": round(t[-1] - t[0], 5),
                         "GB/s": round(nbytes / m / 1e6, 1), "frac_of_8TBs": round(nbytes / m / 1e6 / 8000.0, 4)}
        res[f"m4_mvm_transposed_{nb}"].update({
            "speedup_over_transpose_then_mvm": round(mp / md, 3), "faster_than_the_pair_by_more_than_its_spread": bool(mp - md > p[-1] - p[0]),
            "ratio_to_mvm_on_a_held_transpose": round(md / mh, 3), "within_the_spread_of_the_held_transpose_call": bool(abs(md - mh) <= h[-1] - h[0])})
        del tA, tsA, tAt, tsAt
    for name, im, inn, thr, iters in (("iht_one_matrix_N8192", 4096, 8192, 1, 20), ("iht_one_matrix_gd_32768^2", 32768, 32768, 0, 4)):
        if not selected(name):
            continue
        P, sP, PT, sPT = hip.alloc(im * inn // 2), hip.alloc(4 * (im // 64) * (inn // 64)), hip.alloc(im * inn // 2), hip.alloc(4 * (im // 64) * (inn // 64))
        hip.check(lib.clv_fill_random_nibbles(P.ptr, P.nbytes, 63, 0, None))
        hip.check(lib.clv_fill_random_scales(sP.ptr, sP.nbytes // 4, 64, 0, None))
        hip.check(lib.clm4_transpose(P.ptr, sP.ptr, im, inn, PT.ptr, sPT.ptr, None))
        (vy, vx, vt1, vt2, vt3) = (vec_set(1, n, seed)[0] for n, seed in ((im, 500), (inn, 600), (im, 700), (im, 800), (inn, 900)))
        tail = (vx[0].ptr, vx[1].ptr, inn, vy[0].ptr, vy[1].ptr, vt1[0].ptr, vt1[1].ptr, vt2[0].ptr, vt2[1].ptr, vt3[0].ptr, vt3[1].ptr, iters, im // 4,
                0.002, thr, None, None)

        def two():
            hip.check(lib.clm4_iht(P.ptr, sP.ptr, PT.ptr, sPT.ptr, im, inn, *tail))

        def two_loop():
            os.environ["CLV_IHT_PERSISTENT"] = "0"
            try:
                hip.check(lib.clm4_iht(P.ptr, sP.ptr, PT.ptr, sPT.ptr, im, inn, *tail))
            finally:
                os.environ.pop("CLV_IHT_PERSISTENT", None)

        def one():
            hip.check(lib.clm4_iht_one_matrix(P.ptr, sP.ptr, im, inn, *tail))
        t2, tl, t1 = ([v / iters for v in t] for t in alternated((two, two_loop, one), reps=2))
        res[name] = {"one_matrix_ms_per_iteration": round(t1[len(t1) // 2], 5), "clm4_iht_ms_per_iteration": round(t2[len(t2) // 2], 5),
                     "clm4_iht_launch_per_step_ms_per_iteration": round(tl[len(tl) // 2], 5),
                     "one_matrix_rounds_ms": [round(v, 5) for v in t1], "clm4_iht_rounds_ms": [round(v, 5) for v in t2],
                     "clm4_iht_launch_per_step_rounds_ms": [round(v, 5) for v in tl],
                     "note": f"calls of {iters} iterations, K = m / 4, threshold = {thr}; clm4_iht as it dispatches by itself, and with CLV_IHT_PERSISTENT=0"}
        del P, sP, PT, sPT
    if ONLY and all(any(o in r for r in MVT_ROWS) for o in ONLY.split(",")):
        print(json.dumps(res, indent=1))
        sys.exit(0)


# ---- A' x for several vectors straight from A (mvm_t4_batch.hip).  Per row three calls from ONE session on the same matrix and vectors, their
# rounds ALTERNATED: the batch call on the batched kernel (CLV_MVM_BATCH=1), the same vectors as g single clm4_mvm_transposed
# (clm4_mvm_transposed_scale_and_add) calls -- unchanged by this kernel, so this is what a caller paid before it -- and clm4_mvm_batch
# (clm4_mvm_scale_and_add_batch) on a held A': what not holding the second matrix costs.  The *_st_* twins run with a generator.
# m4_iht_batch_one_matrix_N8192: clm4_iht_batch_one_matrix against 8 x clm4_iht_one_matrix and clm4_iht_batch, ms per iteration for 8 signals.
# KB_ONLY=transposed_batch,transposed_saa_batch,iht_batch_one_matrix selects them and the run ends after them.
MVTB_ROWS = tuple(f"m4_mvm_transposed_batch{g}_{t}{nb}" for nb in (32768, 65536) for g in (2, 4, 8) for t in ("", "st_")) + \
    tuple(f"m4_mvm_transposed_saa_batch{g}_{t}{shape}" for shape in ("8192x4096", "65536^2") for g in (2, 4, 8) for t in ("", "st_")) + \
    ("m4_iht_batch_one_matrix_N8192", "m4_iht_batch_one_matrix_st_N8192")


def forced_batch(fn):
    def run():
        os.environ["CLV_MVM_BATCH"] = "1"
        try:
            fn()
        finally:
            os.environ.pop("CLV_MVM_BATCH", None)
    return run


def rec_three(name, g, singles, batch, held, reps, per=1):
    """singles, batch, held: see above; per divides all three (iterations of a loop call)"""
    if not selected(name):
        return
    os.environ.pop("CLV_MVM_BATCH", None)
    one, many, hold = ([t / per for t in ts] for ts in alternated((singles, forced_batch(batch), forced_batch(held)), reps=reps))
    o, m, h = one[len(one) // 2], many[len(many) // 2], hold[len(hold) // 2]
    spread = (one[-1] - one[0]) + (many[-1] - many[0])
    res[name] = {"vectors": g, "batch_ms": round(m, 5), "single_calls_ms": round(o, 5), "batch_on_a_held_transpose_ms": round(h, 5),
                 "batch_rounds_ms": [round(t, 5) for t in many], "single_calls_rounds_ms": [round(t, 5) for t in one],
                 "batch_on_a_held_transpose_rounds_ms": [round(t, 5) for t in hold], "spread_of_both_ms": round(spread, 5),
                 "speedup_over_single_calls": round(o / m, 3), "batch_faster_by_more_than_the_spread_of_both": bool(o - m > spread),
                 "ratio_to_batch_on_a_held_transpose": round(m / h, 3)}


if any(selected(r) for r in MVTB_ROWS):
    def mvtb_rows(tag, rows, cols, reps):
        """the plain rows (tag = the size) or the fused ones (tag = the shape's name) of one matrix of rows x cols"""
        fusedf = not tag.isdigit()
        stem = "m4_mvm_transposed_saa_batch" if fusedf else "m4_mvm_transposed_batch"
        if not any(selected(f"{stem}{g}_{t}{tag}") for g in (2, 4, 8) for t in ("", "st_")):
            return
        tA, tsA, tAt, tsAt = (hip.alloc(rows * cols // 2), hip.alloc(4 * (rows // 64) * (cols // 64)), hip.alloc(rows * cols // 2),
                              hip.alloc(4 * (rows // 64) * (cols // 64)))
        hip.check(lib.clv_fill_random_nibbles(tA.ptr, tA.nbytes, 65, 0, None))
        hip.check(lib.clv_fill_random_scales(tsA.ptr, tsA.nbytes // 4, 66, 0, None))
        hip.check(lib.clm4_transpose(tA.ptr, tsA.ptr, rows, cols, tAt.ptr, tsAt.ptr, None))
        vx, vu, vt, vr = vec_set(8, rows, 330), vec_set(8, cols, 340), vec_set(8, cols, 350), vec_set(8, cols, 360)
        for g in (2, 4, 8):
            a = {k: (ptrs([p[0] for p in v[:g]]), ptrs([p[1] for p in v[:g]])) for k, v in dict(x=vx, u=vu, t=vt, r=vr).items()}
            for t, st in (("", None), ("st_", hip.new_rng(1, 2))):
                sp = st.ptr if st else None
                if fusedf:
                    def singles(g=g, sp=sp):
                        for j in range(g):
                            hip.check(lib.clm4_mvm_transposed_scale_and_add(tA.ptr, tsA.ptr, rows, cols, vx[j][0].ptr, vx[j][1].ptr, vu[j][0].ptr,
                                                                            vu[j][1].ptr, 0.002, vt[j][0].ptr, vt[j][1].ptr, vr[j][0].ptr, vr[j][1].ptr, sp, None))

                    def batch(g=g, a=a, sp=sp):
                        hip.check(lib.clm4_mvm_transposed_scale_and_add_batch(tA.ptr, tsA.ptr, rows, cols, g, a["x"][0], a["x"][1], a["u"][0], a["u"][1],
                                                                              0.002, a["t"][0], a["t"][1], a["r"][0], a["r"][1], sp, None))

                    def held(g=g, a=a, sp=sp):
                        hip.check(lib.clm4_mvm_scale_and_add_batch(tAt.ptr, tsAt.ptr, cols, rows, g, a["x"][0], a["x"][1], a["u"][0], a["u"][1], 0.002,
                                                                   a["t"][0], a["t"][1], a["r"][0], a["r"][1], sp, None))
                else:
                    def singles(g=g, sp=sp):
                        for j in range(g):
                            hip.check(lib.clm4_mvm_transposed(tA.ptr, tsA.ptr, rows, cols, vx[j][0].ptr, vx[j][1].ptr, vr[j][0].ptr, vr[j][1].ptr, sp, None))

                    def batch(g=g, a=a, sp=sp):
                        hip.check(lib.clm4_mvm_transposed_batch(tA.ptr, tsA.ptr, rows, cols, g, a["x"][0], a["x"][1], a["r"][0], a["r"][1], sp, None))

                    def held(g=g, a=a, sp=sp):
                        hip.check(lib.clm4_mvm_batch(tAt.ptr, tsAt.ptr, cols, rows, g, a["x"][0], a["x"][1], a["r"][0], a["r"][1], sp, None))
                rec_three(f"{stem}{g}_{t}{tag}", g, singles, batch, held, reps)
        del tA, tsA, tAt, tsAt

    mvtb_rows("32768", 32768, 32768, 10)
    mvtb_rows("65536", 65536, 65536, 4)
    mvtb_rows("8192x4096", 4096, 8192, 20)          # the IHT shape's step 2: Phi is 4096 x 8192, t3 = Phi' t2
    mvtb_rows("65536^2", 65536, 65536, 4)
    im, inn, ig, iters = 4096, 8192, 8, 20
    if selected("m4_iht_batch_one_matrix_N8192") or selected("m4_iht_batch_one_matrix_st_N8192"):
        P, sP, PT, sPT = hip.alloc(im * inn // 2), hip.alloc(4 * (im // 64) * (inn // 64)), hip.alloc(im * inn // 2), hip.alloc(4 * (im // 64) * (inn // 64))
        hip.check(lib.clv_fill_random_nibbles(P.ptr, P.nbytes, 67, 0, None))
        hip.check(lib.clv_fill_random_scales(sP.ptr, sP.nbytes // 4, 68, 0, None))
        hip.check(lib.clm4_transpose(P.ptr, sP.ptr, im, inn, PT.ptr, sPT.ptr, None))
        vy, vx, vt1, vt2, vt3 = vec_set(ig, im, 500), vec_set(ig, inn, 600), vec_set(ig, im, 700), vec_set(ig, im, 800), vec_set(ig, inn, 900)
        A = {k: (ptrs([p[0] for p in v]), ptrs([p[1] for p in v])) for k, v in dict(y=vy, x=vx, t1=vt1, t2=vt2, t3=vt3).items()}
        for t, st in (("", None), ("st_", hip.new_rng(1, 2))):
            sp = st.ptr if st else None
            tail = (im, inn, ig, A["x"][0], A["x"][1], inn, A["y"][0], A["y"][1], A["t1"][0], A["t1"][1], A["t2"][0], A["t2"][1], A["t3"][0], A["t3"][1],
                    iters, im // 4, 0.002, 1, sp, None)

            def singles(sp=sp):
                for j in range(ig):
                    hip.check(lib.clm4_iht_one_matrix(P.ptr, sP.ptr, im, inn, vx[j][0].ptr, vx[j][1].ptr, inn, vy[j][0].ptr, vy[j][1].ptr, vt1[j][0].ptr,
                                                      vt1[j][1].ptr, vt2[j][0].ptr, vt2[j][1].ptr, vt3[j][0].ptr, vt3[j][1].ptr, iters, im // 4, 0.002, 1, sp,
                                                      None))
            name = f"m4_iht_batch_one_matrix_{t}N8192"
            rec_three(name, ig, singles, lambda tail=tail: hip.check(lib.clm4_iht_batch_one_matrix(P.ptr, sP.ptr, *tail)),
                      lambda tail=tail: hip.check(lib.clm4_iht_batch(P.ptr, sP.ptr, PT.ptr, sPT.ptr, *tail)), reps=2, per=iters)
            if name in res:
                res[name]["note"] = (f"ms per iteration for all 8 signals, calls of {iters} iterations, K = m / 4, FAST threshold; the single calls are "
                                     "8 x clm4_iht_one_matrix, the held-transpose column is clm4_iht_batch under CLV_MVM_BATCH=1")
        del P, sP, PT, sPT, vy, vx, vt1, vt2, vt3
    if ONLY and all(any(o in r for r in MVTB_ROWS) for o in ONLY.split(",")):
        print(json.dumps(res, indent=1))
        sys.exit(0)


# ---- A' x for several CloverVector8 straight from a CloverMatrix8 (matrix8_t_batch.hip): the rows of the block above for the pure 8-bit
# pair.  Per row the calls come from ONE session on the same matrix and vectors, their rounds ALTERNATED: the batch call on the batched kernel
# (CLV_MVM_BATCH=1), the same vectors as g single clm8_mvm_transposed (clm8_mvm_transposed_scale_and_add) calls, clm8_mvm_batch
# (clm8_mvm_scale_and_add_batch) on a held A' and, in the plain rows, clm8_transpose + clm8_mvm_batch.  The *_st_* twins run with a generator.
# m8_iht_batch_one_matrix_N8192: clm8_iht_batch_one_matrix against 8 x clm8_iht_one_matrix and clm8_iht_batch, ms per iteration for 8 signals.
# KB_ONLY=m8_mvm_transposed_batch,m8_mvm_transposed_saa_batch,m8_iht_batch_one_matrix selects them and the run ends after them.
M8TB_ROWS = tuple(f"m8_mvm_transposed_batch{g}_{t}{nb}" for nb in (32768, 65536) for g in (2, 4, 8) for t in ("", "st_")) + \
    tuple(f"m8_mvm_transposed_saa_batch{g}_{t}{shape}" for shape in ("8192x4096", "65536^2") for g in (2, 4, 8) for t in ("", "st_")) + \
    ("m8_iht_batch_one_matrix_N8192", "m8_iht_batch_one_matrix_st_N8192")

if any(selected(r) for r in M8TB_ROWS):
    def rec_m8tb(name, g, singles, batch, held, reps, per=1, pair=None):
        """rec_three with, where pair is given, a fourth alternated call: the transpose followed by the held batch"""
        if not selected(name):
            return
        os.environ.pop("CLV_MVM_BATCH", None)
        fns = (singles, forced_batch(batch), forced_batch(held)) + ((forced_batch(pair),) if pair else ())
        ts = [[t / per for t in r] for r in alternated(fns, reps=reps)]
        one, many, hold = ts[:3]
        o, m, h = one[len(one) // 2], many[len(many) // 2], hold[len(hold) // 2]
        spread = (one[-1] - one[0]) + (many[-1] - many[0])
        res[name] = {"vectors": g, "batch_ms": round(m, 5), "single_calls_ms": round(o, 5), "batch_on_a_held_transpose_ms": round(h, 5),
                     "batch_rounds_ms": [round(t, 5) for t in many], "single_calls_rounds_ms": [round(t, 5) for t in one],
                     "batch_on_a_held_transpose_rounds_ms": [round(t, 5) for t in hold], "spread_of_both_ms": round(spread, 5),
                     "speedup_over_single_calls": round(o / m, 3), "batch_faster_by_more_than_the_spread_of_both": bool(o - m > spread),
                     "ratio_to_batch_on_a_held_transpose": round(m / h, 3)}
        if pair:
            p = ts[3]
            res[name].update({"transpose_then_batch_ms": round(p[len(p) // 2], 5), "transpose_then_batch_rounds_ms": [round(t, 5) for t in p]})

    def m8tb_rows(tag, rows, cols, reps):
        """the plain rows (tag = the size) or the fused ones (tag = the shape's name) of one matrix of rows x cols"""
        fusedf = not tag.isdigit()
        stem = "m8_mvm_transposed_saa_batch" if fusedf else "m8_mvm_transposed_batch"
        if not any(selected(f"{stem}{g}_{t}{tag}") for g in (2, 4, 8) for t in ("", "st_")):
            return
        (tA, tsA), tAt, tsAt = m8_matrix(rows, cols, 65), hip.alloc(rows * cols), hip.alloc(4 * (rows // 64) * (cols // 64))
        hip.check(lib.clm8_transpose(tA.ptr, tsA.ptr, rows, cols, tAt.ptr, tsAt.ptr, None))
        vx, vu, vt, vr = vec8_set(8, rows, 330), vec8_set(8, cols, 340), vec8_set(8, cols, 350), vec8_set(8, cols, 360)
        for g in (2, 4, 8):
            a = {k: (ptrs([p[0] for p in v[:g]]), ptrs([p[1] for p in v[:g]])) for k, v in dict(x=vx, u=vu, t=vt, r=vr).items()}
            for t, st in (("", None), ("st_", hip.new_rng(1, 2))):
                sp = st.ptr if st else None
                pair = None
                if fusedf:
                    def singles(g=g, sp=sp):
                        for j in range(g):
                            hip.check(lib.clm8_mvm_transposed_scale_and_add(tA.ptr, tsA.ptr, rows, cols, vx[j][0].ptr, vx[j][1].ptr, vu[j][0].ptr,
                                                                            vu[j][1].ptr, 0.002, vt[j][0].ptr, vt[j][1].ptr, vr[j][0].ptr, vr[j][1].ptr, sp, None))

                    def batch(g=g, a=a, sp=sp):
                        hip.check(lib.clm8_mvm_transposed_scale_and_add_batch(tA.ptr, tsA.ptr, rows, cols, g, a["x"][0], a["x"][1], a["u"][0], a["u"][1],
                                                                              0.002, a["t"][0], a["t"][1], a["r"][0], a["r"][1], sp, None))

                    def held(g=g, a=a, sp=sp):
                        hip.check(lib.clm8_mvm_scale_and_add_batch(tAt.ptr, tsAt.ptr, cols, rows, g, a["x"][0], a["x"][1], a["u"][0], a["u"][1], 0.002,
                                                                   a["t"][0], a["t"][1], a["r"][0], a["r"][1], sp, None))
                else:
                    def singles(g=g, sp=sp):
                        for j in range(g):
                            hip.check(lib.clm8_mvm_transposed(tA.ptr, tsA.ptr, rows, cols, vx[j][0].ptr, vx[j][1].ptr, vr[j][0].ptr, vr[j][1].ptr, sp, None))

                    def batch(g=g, a=a, sp=sp):
                        hip.check(lib.clm8_mvm_transposed_batch(tA.ptr, tsA.ptr, rows, cols, g, a["x"][0], a["x"][1], a["r"][0], a["r"][1], sp, None))

                    def held(g=g, a=a, sp=sp):
                        hip.check(lib.clm8_mvm_batch(tAt.ptr, tsAt.ptr, cols, rows, g, a["x"][0], a["x"][1], a["r"][0], a["r"][1], sp, None))

                    def pair(held=held):
                        hip.check(lib.clm8_transpose(tA.ptr, tsA.ptr, rows, cols, tAt.ptr, tsAt.ptr, None))
                        held()
                rec_m8tb(f"{stem}{g}_{t}{tag}", g, singles, batch, held, reps, pair=pair)
        del tA, tsA, tAt, tsAt

    m8tb_rows("32768", 32768, 32768, 10)
    m8tb_rows("65536", 65536, 65536, 4)
    m8tb_rows("8192x4096", 4096, 8192, 20)          # the IHT shape's step 2: Phi is 4096 x 8192, t3 = Phi' t2
    m8tb_rows("65536^2", 65536, 65536, 4)
    im, inn, ig, iters = 4096, 8192, 8, 20
    if selected("m8_iht_batch_one_matrix_N8192") or selected("m8_iht_batch_one_matrix_st_N8192"):
        (P, sP), PT, sPT = m8_matrix(im, inn, 67), hip.alloc(im * inn), hip.alloc(4 * (im // 64) * (inn // 64))
        hip.check(lib.clm8_transpose(P.ptr, sP.ptr, im, inn, PT.ptr, sPT.ptr, None))
        vy, vx, vt1, vt2, vt3 = vec8_set(ig, im, 500), vec8_set(ig, inn, 600), vec8_set(ig, im, 700), vec8_set(ig, im, 800), vec8_set(ig, inn, 900)
        A = {k: (ptrs([p[0] for p in v]), ptrs([p[1] for p in v])) for k, v in dict(y=vy, x=vx, t1=vt1, t2=vt2, t3=vt3).items()}
        for t, st in (("", None), ("st_", hip.new_rng(1, 2))):
            sp = st.ptr if st else None
            tail = (im, inn, ig, A["x"][0], A["x"][1], inn, A["y"][0], A["y"][1], A["t1"][0], A["t1"][1], A["t2"][0], A["t2"][1], A["t3"][0], A["t3"][1],
                    iters, im // 4, 0.002, 1, sp, None)

            def singles(sp=sp):
                for j in range(ig):
                    hip.check(lib.clm8_iht_one_matrix(P.ptr, sP.ptr, im, inn, vx[j][0].ptr, vx[j][1].ptr, inn, vy[j][0].ptr, vy[j][1].ptr, vt1[j][0].ptr,
                                                      vt1[j][1].ptr, vt2[j][0].ptr, vt2[j][1].ptr, vt3[j][0].ptr, vt3[j][1].ptr, iters, im // 4, 0.002, 1, sp,
                                                      None))
            name = f"m8_iht_batch_one_matrix_{t}N8192"
            rec_m8tb(name, ig, singles, lambda tail=tail: hip.check(lib.clm8_iht_batch_one_matrix(P.ptr, sP.ptr, *tail)),
                     lambda tail=tail: hip.check(lib.clm8_iht_batch(P.ptr, sP.ptr, PT.ptr, sPT.ptr, *tail)), reps=2, per=iters)
            if name in res:
                res[name]["note"] = (f"ms per iteration for all 8 signals, calls of {iters} iterations, K = m / 4, FAST threshold; the single calls are "
                                     "8 x clm8_iht_one_matrix, the held-transpose column is clm8_iht_batch under CLV_MVM_BATCH=1")
        del P, sP, PT, sPT, vy, vx, vt1, vt2, vt3
    if ONLY and all(any(o in r for r in M8TB_ROWS) for o in ONLY.split(",")):
        print(json.dumps(res, indent=1))
        sys.exit(0)


# ---- A' x for CloverVector8 straight from A (mvm_t8.hip): the three rows per size of the block above with clm4_mvm_v8_transposed, clm4_transpose +
# clm4_mvm_v8 and clm4_mvm_v8 on a held A', rounds alternated in one session; iht_v8_one_matrix_*: clm4_iht_v8_one_matrix against clm4_iht_v8.
# KB_ONLY=mvm_v8_transposed,transpose_then_mvm_v8,mvm_v8_held_transpose,iht_v8_one_matrix selects them and the run ends after them.
MVT8_ROWS = tuple(f"{k}_{nb}" for nb in MVT_SIZES for k in ("m4_mvm_v8_transposed", "m4_transpose_then_mvm_v8", "m4_mvm_v8_held_transpose")) + \
    ("iht_v8_one_matrix_N8192", "iht_v8_one_matrix_gd_32768^2")

if any(selected(r) for r in MVT8_ROWS):
    for nb in MVT_SIZES:
        if not any(selected(r) for r in MVT8_ROWS if r.endswith(f"_{nb}")):
            continue
        tA, tsA, tAt, tsAt = hip.alloc(nb * nb // 2), hip.alloc(4 * (nb // 64) ** 2), hip.alloc(nb * nb // 2), hip.alloc(4 * (nb // 64) ** 2)
        hip.check(lib.clv_fill_random_nibbles(tA.ptr, tA.nbytes, 61, 0, None))
        hip.check(lib.clv_fill_random_scales(tsA.ptr, tsA.nbytes // 4, 62, 0, None))
        (tx, tsx), (tr, tsr) = vec8_set(1, nb, 310)[0], vec8_set(1, nb, 320)[0]
        hip.check(lib.clm4_transpose(tA.ptr, tsA.ptr, nb, nb, tAt.ptr, tsAt.ptr, None))

        def direct8():
            hip.check(lib.clm4_mvm_v8_transposed(tA.ptr, tsA.ptr, nb, nb, tx.ptr, tsx.ptr, tr.ptr, tsr.ptr, None, None))

        def pair8():
            hip.check(lib.clm4_transpose(tA.ptr, tsA.ptr, nb, nb, tAt.ptr, tsAt.ptr, None))
            hip.check(lib.clm4_mvm_v8(tAt.ptr, tsAt.ptr, nb, nb, tx.ptr, tsx.ptr, tr.ptr, tsr.ptr, None, None))

        def held8():
            hip.check(lib.clm4_mvm_v8(tAt.ptr, tsAt.ptr, nb, nb, tx.ptr, tsx.ptr, tr.ptr, tsr.ptr, None, None))
        d, p, h = alternated((direct8, pair8, held8), reps=20 if nb == 8192 else 10 if nb == 32768 else 4)
        mat_b = nb * nb // 2 + 4 * (nb // 64) ** 2
        one_b = mat_b + 2 * (nb + nb // 16)
        md, mp, mh = d[len(d) // 2], p[len(p) // 2], h[len(h) // 2]
        for name, t, m, nbytes in ((f"m4_mvm_v8_transposed_{nb}", d, md, one_b), (f"m4_transpose_then_mvm_v8_{nb}", p, mp, 2 * mat_b + one_b),
                                   (f"m4_mvm_v8_held_transpose_{nb}", h, mh, one_b)):
            res[name] = {"ms": round(m, 5), "rounds_ms": [round(v, 5) for v in t], "spread_ms": round(t[-1] - t[0], 5),
                         "GB/s": round(nbytes / m / 1e6, 1), "frac_of_8TBs": round(nbytes / m / 1e6 / 8000.0, 4)}
        res[f"m4_mvm_v8_transposed_{nb}"].update({
            "speedup_over_transpose_then_mvm_v8": round(mp / md, 3), "faster_than_the_pair_by_more_than_its_spread": bool(mp - md > p[-1] - p[0]),
            "ratio_to_mvm_v8_on_a_held_transpose": round(md / mh, 3), "within_the_spread_of_the_held_transpose_call": bool(abs(md - mh) <= h[-1] - h[0])})
        del tA, tsA, tAt, tsAt
    for name, im, inn, thr, iters in (("iht_v8_one_matrix_N8192", 4096, 8192, 1, 20), ("iht_v8_one_matrix_gd_32768^2", 32768, 32768, 0, 4)):
        if not selected(name):
            continue
        P, sP, PT, sPT = hip.alloc(im * inn // 2), hip.alloc(4 * (im // 64) * (inn // 64)), hip.alloc(im * inn // 2), hip.alloc(4 * (im // 64) * (inn // 64))
        hip.check(lib.clv_fill_random_nibbles(P.ptr, P.nbytes, 63, 0, None))
        hip.check(lib.clv_fill_random_scales(sP.ptr, sP.nbytes // 4, 64, 0, None))
        hip.check(lib.clm4_transpose(P.ptr, sP.ptr, im, inn, PT.ptr, sPT.ptr, None))
        (vy, vx, vt1, vt2, vt3) = (vec8_set(1, n, seed)[0] for n, seed in ((im, 500), (inn, 600), (im, 700), (im, 800), (inn, 900)))
        tail = (vx[0].ptr, vx[1].ptr, inn, vy[0].ptr, vy[1].ptr, vt1[0].ptr, vt1[1].ptr, vt2[0].ptr, vt2[1].ptr, vt3[0].ptr, vt3[1].ptr, iters, im // 4,
                0.002, thr, None, None)

        def two8():
            hip.check(lib.clm4_iht_v8(P.ptr, sP.ptr, PT.ptr, sPT.ptr, im, inn, *tail))

        def two8_loop():
            os.environ["CLV_IHT_PERSISTENT"] = "0"
            try:
                hip.check(lib.clm4_iht_v8(P.ptr, sP.ptr, PT.ptr, sPT.ptr, im, inn, *tail))
            finally:
                os.environ.pop("CLV_IHT_PERSISTENT", None)

        def one8():
            hip.check(lib.clm4_iht_v8_one_matrix(P.ptr, sP.ptr, im, inn, *tail))
        t2, tl, t1 = ([v / iters for v in t] for t in alternated((two8, two8_loop, one8), reps=2))
        res[name] = {"one_matrix_ms_per_iteration": round(t1[len(t1) // 2], 5), "clm4_iht_v8_ms_per_iteration": round(t2[len(t2) // 2], 5),
                     "clm4_iht_v8_launch_per_step_ms_per_iteration": round(tl[len(tl) // 2], 5),
                     "one_matrix_rounds_ms": [round(v, 5) for v in t1], "clm4_iht_v8_rounds_ms": [round(v, 5) for v in t2],
                     "clm4_iht_v8_launch_per_step_rounds_ms": [round(v, 5) for v in tl],
                     "note": f"calls of {iters} iterations, K = m / 4, threshold = {thr}; clm4_iht_v8 as it dispatches by itself, and with CLV_IHT_PERSISTENT=0"}
        del P, sP, PT, sPT
    if ONLY and all(any(o in r for r in MVT8_ROWS) for o in ONLY.split(",")):
        print(json.dumps(res, indent=1))
        sys.exit(0)


# ---- A' x for several CloverVector8 straight from a CloverMatrix4 (mvm_t8_batch.hip): the rows of the MVTB_ROWS / M8TB_ROWS blocks for the
# mixed pair.  Per row three calls from ONE session on the same matrix and vectors, their rounds ALTERNATED (rec_three): the batch call on
# the batched kernel (CLV_MVM_BATCH=1), the same vectors as g single clm4_mvm_v8_transposed (clm4_mvm_v8_transposed_scale_and_add) calls, and
# clm4_mvm_v8_batch (clm4_mvm_v8_scale_and_add_batch) on a held A'.  The *_st_* twins run with a generator.
# m4_iht_v8_batch_one_matrix_N8192: clm4_iht_v8_batch_one_matrix against 8 x clm4_iht_v8_one_matrix and clm4_iht_v8_batch, ms per iteration
# for 8 signals.  KB_ONLY=m4_mvm_v8_transposed_batch,m4_mvm_v8_transposed_saa_batch,m4_iht_v8_batch_one_matrix selects them and the run
# ends after them.
MVT8B_ROWS = tuple(f"m4_mvm_v8_transposed_batch{g}_{t}{nb}" for nb in (32768, 65536) for g in (2, 4, 8) for t in ("", "st_")) + \
    tuple(f"m4_mvm_v8_transposed_saa_batch{g}_{t}{shape}" for shape in ("8192x4096", "65536^2") for g in (2, 4, 8) for t in ("", "st_")) + \
    ("m4_iht_v8_batch_one_matrix_N8192", "m4_iht_v8_batch_one_matrix_st_N8192")

if any(selected(r) for r in MVT8B_ROWS):
    def mvt8b_rows(tag, rows, cols, reps):
        """the plain rows (tag = the size) or the fused ones (tag = the shape's name) of one matrix of rows x cols"""
        fusedf = not tag.isdigit()
        stem = "m4_mvm_v8_transposed_saa_batch" if fusedf else "m4_mvm_v8_transposed_batch"
        if not any(selected(f"{stem}{g}_{t}{tag}") for g in (2, 4, 8) for t in ("", "st_")):
            return
        tA, tsA, tAt, tsAt = (hip.alloc(rows * cols // 2), hip.alloc(4 * (rows // 64) * (cols // 64)), hip.alloc(rows * cols // 2),
                              hip.alloc(4 * (rows // 64) * (cols // 64)))
        hip.check(lib.clv_fill_random_nibbles(tA.ptr, tA.nbytes, 65, 0, None))
        hip.check(lib.clv_fill_random_scales(tsA.ptr, tsA.nbytes // 4, 66, 0, None))
        hip.check(lib.clm4_transpose(tA.ptr, tsA.ptr, rows, cols, tAt.ptr, tsAt.ptr, None))
        vx, vu, vt, vr = vec8_set(8, rows, 330), vec8_set(8, cols, 340), vec8_set(8, cols, 350), vec8_set(8, cols, 360)
        for g in (2, 4, 8):
            a = {k: (ptrs([p[0] for p in v[:g]]), ptrs([p[1] for p in v[:g]])) for k, v in dict(x=vx, u=vu, t=vt, r=vr).items()}
            for t, st in (("", None), ("st_", hip.new_rng(1, 2))):
                sp = st.ptr if st else None
                if fusedf:
                    def singles(g=g, sp=sp):
                        for j in range(g):
                            hip.check(lib.clm4_mvm_v8_transposed_scale_and_add(tA.ptr, tsA.ptr, rows, cols, vx[j][0].ptr, vx[j][1].ptr, vu[j][0].ptr,
                                                                               vu[j][1].ptr, 0.002, vt[j][0].ptr, vt[j][1].ptr, vr[j][0].ptr, vr[j][1].ptr, sp,
                                                                               None))

                    def batch(g=g, a=a, sp=sp):
                        hip.check(lib.clm4_mvm_v8_transposed_scale_and_add_batch(tA.ptr, tsA.ptr, rows, cols, g, a["x"][0], a["x"][1], a["u"][0], a["u"][1],
                                                                                 0.002, a["t"][0], a["t"][1], a["r"][0], a["r"][1], sp, None))

                    def held(g=g, a=a, sp=sp):
                        hip.check(lib.clm4_mvm_v8_scale_and_add_batch(tAt.ptr, tsAt.ptr, cols, rows, g, a["x"][0], a["x"][1], a["u"][0], a["u"][1], 0.002,
                                                                      a["t"][0], a["t"][1], a["r"][0], a["r"][1], sp, None))
                else:
                    def singles(g=g, sp=sp):
                        for j in range(g):
                            hip.check(lib.clm4_mvm_v8_transposed(tA.ptr, tsA.ptr, rows, cols, vx[j][0].ptr, vx[j][1].ptr, vr[j][0].ptr, vr[j][1].ptr, sp, None))

                    def batch(g=g, a=a, sp=sp):
                        hip.check(lib.clm4_mvm_v8_transposed_batch(tA.ptr, tsA.ptr, rows, cols, g, a["x"][0], a["x"][1], a["r"][0], a["r"][1], sp, None))

                    def held(g=g, a=a, sp=sp):
                        hip.check(lib.clm4_mvm_v8_batch(tAt.ptr, tsAt.ptr, cols, rows, g, a["x"][0], a["x"][1], a["r"][0], a["r"][1], sp, None))
                rec_three(f"{stem}{g}_{t}{tag}", g, singles, batch, held, reps)
        del tA, tsA, tAt, tsAt

    mvt8b_rows("32768", 32768, 32768, 10)
    mvt8b_rows("65536", 65536, 65536, 4)
    mvt8b_rows("8192x4096", 4096, 8192, 20)         # the IHT shape's step 2: Phi is 4096 x 8192, t3 = Phi' t2
    mvt8b_rows("65536^2", 65536, 65536, 4)
    im, inn, ig, iters = 4096, 8192, 8, 20
    if selected("m4_iht_v8_batch_one_matrix_N8192") or selected("m4_iht_v8_batch_one_matrix_st_N8192"):
        P, sP, PT, sPT = hip.alloc(im * inn // 2), hip.alloc(4 * (im // 64) * (inn // 64)), hip.alloc(im * inn // 2), hip.alloc(4 * (im // 64) * (inn // 64))
        hip.check(lib.clv_fill_random_nibbles(P.ptr, P.nbytes, 67, 0, None))
        hip.check(lib.clv_fill_random_scales(sP.ptr, sP.nbytes // 4, 68, 0, None))
        hip.check(lib.clm4_transpose(P.ptr, sP.ptr, im, inn, PT.ptr, sPT.ptr, None))
        vy, vx, vt1, vt2, vt3 = vec8_set(ig, im, 500), vec8_set(ig, inn, 600), vec8_set(ig, im, 700), vec8_set(ig, im, 800), vec8_set(ig, inn, 900)
        A = {k: (ptrs([p[0] for p in v]), ptrs([p[1] for p in v])) for k, v in dict(y=vy, x=vx, t1=vt1, t2=vt2, t3=vt3).items()}
        for t, st in (("", None), ("st_", hip.new_rng(1, 2))):
            sp = st.ptr if st else None
            tail = (im, inn, ig, A["x"][0], A["x"][1], inn, A["y"][0], A["y"][1], A["t1"][0], A["t1"][1], A["t2"][0], A["t2"][1], A["t3"][0], A["t3"][1],
                    iters, im // 4, 0.002, 1, sp, None)

            def singles(sp=sp):
                for j in range(ig):
                    hip.check(lib.clm4_iht_v8_one_matrix(P.ptr, sP.ptr, im, inn, vx[j][0].ptr, vx[j][1].ptr, inn, vy[j][0].ptr, vy[j][1].ptr, vt1[j][0].ptr,
                                                         vt1[j][1].ptr, vt2[j][0].ptr, vt2[j][1].ptr, vt3[j][0].ptr, vt3[j][1].ptr, iters, im // 4, 0.002, 1,
                                                         sp, None))
            name = f"m4_iht_v8_batch_one_matrix_{t}N8192"
            rec_three(name, ig, singles, lambda tail=tail: hip.check(lib.clm4_iht_v8_batch_one_matrix(P.ptr, sP.ptr, *tail)),
                      lambda tail=tail: hip.check(lib.clm4_iht_v8_batch(P.ptr, sP.ptr, PT.ptr, sPT.ptr, *tail)), reps=2, per=iters)
            if name in res:
                res[name]["note"] = (f"ms per iteration for all 8 signals, calls of {iters} iterations, K = m / 4, FAST threshold; the single calls are "
                                     "8 x clm4_iht_v8_one_matrix, the held-transpose column is clm4_iht_v8_batch under CLV_MVM_BATCH=1")
        del P, sP, PT, sPT, vy, vx, vt1, vt2, vt3
    if ONLY and all(any(o in r for r in MVT8B_ROWS) for o in ONLY.split(",")):
        print(json.dumps(res, indent=1))
        sys.exit(0)


# ---- A' x for a CloverMatrix8 straight from A (matrix8_t.hip): the three rows per size of the two blocks above with clm8_mvm_transposed,
# clm8_transpose + clm8_mvm and clm8_mvm on a held A', rounds alternated in one session; m8_iht_one_matrix_*: clm8_iht_one_matrix against clm8_iht
# (launch per step either way: no persistent kernel at this width).
# KB_ONLY=m8_mvm_transposed,m8_transpose_then_mvm,m8_mvm_held_transpose,m8_iht_one_matrix selects them and the run ends after them.
M8T_ROWS = tuple(f"{k}_{nb}" for nb in MVT_SIZES for k in ("m8_mvm_transposed", "m8_transpose_then_mvm", "m8_mvm_held_transpose")) + \
    ("m8_iht_one_matrix_N8192", "m8_iht_one_matrix_gd_32768^2")

if any(selected(r) for r in M8T_ROWS):
    for nb in MVT_SIZES:
        if not any(selected(r) for r in M8T_ROWS if r.endswith(f"_{nb}")):
            continue
        (tA, tsA), tAt, tsAt = m8_matrix(nb, nb, 61), hip.alloc(nb * nb), hip.alloc(4 * (nb // 64) ** 2)
        (tx, tsx), (tr, tsr) = vec8_set(1, nb, 310)[0], vec8_set(1, nb, 320)[0]
        hip.check(lib.clm8_transpose(tA.ptr, tsA.ptr, nb, nb, tAt.ptr, tsAt.ptr, None))

        def direct_m8():
            hip.check(lib.clm8_mvm_transposed(tA.ptr, tsA.ptr, nb, nb, tx.ptr, tsx.ptr, tr.ptr, tsr.ptr, None, None))

        def pair_m8():
            hip.check(lib.clm8_transpose(tA.ptr, tsA.ptr, nb, nb, tAt.ptr, tsAt.ptr, None))
            hip.check(lib.clm8_mvm(tAt.ptr, tsAt.ptr, nb, nb, tx.ptr, tsx.ptr, tr.ptr, tsr.ptr, None, None))

        def held_m8():
            hip.check(lib.clm8_mvm(tAt.ptr, tsAt.ptr, nb, nb, tx.ptr, tsx.ptr, tr.ptr, tsr.ptr, None, None))
        d, p, h = alternated((direct_m8, pair_m8, held_m8), reps=20 if nb == 8192 else 10 if nb == 32768 else 4)
        mat_b = nb * nb + 4 * (nb // 64) ** 2
        one_b = mat_b + 2 * (nb + nb // 16)
        md, mp, mh = d[len(d) // 2], p[len(p) // 2], h[len(h) // 2]
        for name, t, m, nbytes in ((f"m8_mvm_transposed_{nb}", d, md, one_b), (f"m8_transpose_then_mvm_{nb}", p, mp, 2 * mat_b + one_b),
                                   (f"m8_mvm_held_transpose_{nb}", h, mh, one_b)):
            res[name] = {"ms": round(m, 5), "rounds_ms": [round(v, 5) for v in t], "spread_ms": round(t[-1] - t[0], 5),
                         "GB/s": round(nbytes / m / 1e6, 1), "frac_of_8TBs": round(nbytes / m / 1e6 / 8000.0, 4)}
        res[f"m8_mvm_transposed_{nb}"].update({
            "speedup_over_transpose_then_mvm": round(mp / md, 3), "faster_than_the_pair_by_more_than_its_spread": bool(mp - md > p[-1] - p[0]),
            "ratio_to_mvm_on_a_held_transpose": round(md / mh, 3), "within_the_spread_of_the_held_transpose_call": bool(abs(md - mh) <= h[-1] - h[0])})
        del tA, tsA, tAt, tsAt
    for name, im, inn, thr, iters in (("m8_iht_one_matrix_N8192", 4096, 8192, 1, 20), ("m8_iht_one_matrix_gd_32768^2", 32768, 32768, 0, 4)):
        if not selected(name):
            continue
        (P, sP), PT, sPT = m8_matrix(im, inn, 63), hip.alloc(im * inn), hip.alloc(4 * (im // 64) * (inn // 64))
        hip.check(lib.clm8_transpose(P.ptr, sP.ptr, im, inn, PT.ptr, sPT.ptr, None))
        (vy, vx, vt1, vt2, vt3) = (vec8_set(1, n, seed)[0] for n, seed in ((im, 500), (inn, 600), (im, 700), (im, 800), (inn, 900)))
        tail = (vx[0].ptr, vx[1].ptr, inn, vy[0].ptr, vy[1].ptr, vt1[0].ptr, vt1[1].ptr, vt2[0].ptr, vt2[1].ptr, vt3[0].ptr, vt3[1].ptr, iters, im // 4,
                0.002, thr, None, None)

        def two_m8():
            hip.check(lib.clm8_iht(P.ptr, sP.ptr, PT.ptr, sPT.ptr, im, inn, *tail))

        def one_m8():
            hip.check(lib.clm8_iht_one_matrix(P.ptr, sP.ptr, im, inn, *tail))
        t2, t1 = ([v / iters for v in t] for t in alternated((two_m8, one_m8), reps=2))
        m2, m1 = t2[len(t2) // 2], t1[len(t1) // 2]
        res[name] = {"one_matrix_ms_per_iteration": round(m1, 5), "clm8_iht_ms_per_iteration": round(m2, 5),
                     "one_matrix_rounds_ms": [round(v, 5) for v in t1], "clm8_iht_rounds_ms": [round(v, 5) for v in t2],
                     "ratio_to_clm8_iht": round(m1 / m2, 3), "within_the_spread_of_clm8_iht": bool(abs(m1 - m2) <= t2[-1] - t2[0]),
                     "note": f"calls of {iters} iterations, K = m / 4, threshold = {thr}; both loops are launch per step"}
        del P, sP, PT, sPT
    if ONLY and all(any(o in r for r in M8T_ROWS) for o in ONLY.split(",")):
        print(json.dumps(res, indent=1))
        sys.exit(0)


SLAB = 1 << 28


def f16_fill(dst, count, seed):
    """count f16 values = quantized random fp32 integers in [-10, 10], through a 1 GiB fp32 slab"""
    src = hip.alloc(4 * min(SLAB, count))
    for o in range(0, count, SLAB):
        c = min(SLAB, count - o)
        hip.check(lib.clv_fill_random_ints_f32(src.ptr, c, 10, seed, o, None))
        hip.check(lib.clv_f16_quantize(src.ptr, c, dst.ptr + 2 * o, None))
    hip.sync()


# ---- A' x for a CloverMatrix16 straight from A (half16_t.hip): the three rows per size of the blocks above with clm_f16_mvm_transposed,
# clm_f16_transpose + clm_f16_mvm and clm_f16_mvm on a held A', rounds alternated in one session; f16_iht_one_matrix_N8192:
# clm_f16_iht_one_matrix against clm_f16_iht (the loop of f16_iht_loop_N8192: 4096 x 8192, FAST threshold, launch per step either way).
# KB_ONLY=f16_mvm_transposed,f16_transpose_then_mvm,f16_mvm_held_transpose,f16_iht_one_matrix selects them and the run ends after them.
F16T_ROWS = tuple(f"{k}_{nb}" for nb in MVT_SIZES for k in ("f16_mvm_transposed", "f16_transpose_then_mvm", "f16_mvm_held_transpose")) + \
    ("f16_iht_one_matrix_N8192",)

if any(selected(r) for r in F16T_ROWS):
    for nb in MVT_SIZES:
        if not any(selected(r) for r in F16T_ROWS if r.endswith(f"_{nb}")):
            continue
        hA, hAt = hip.alloc(2 * nb * nb), hip.alloc(2 * nb * nb)
        f16_fill(hA, nb * nb, 64)
        hx, hr = hip.alloc(2 * nb), hip.alloc(2 * nb)
        f16_fill(hx, nb, 311)
        hip.check(lib.clm_f16_transpose(hA.ptr, nb, nb, hAt.ptr, None))

        def direct_f16():
            hip.check(lib.clm_f16_mvm_transposed(hA.ptr, nb, nb, hx.ptr, hr.ptr, None))

        def pair_f16():
            hip.check(lib.clm_f16_transpose(hA.ptr, nb, nb, hAt.ptr, None))
            hip.check(lib.clm_f16_mvm(hAt.ptr, nb, nb, hx.ptr, hr.ptr, None))

        def held_f16():
            hip.check(lib.clm_f16_mvm(hAt.ptr, nb, nb, hx.ptr, hr.ptr, None))
        d, p, h = alternated((direct_f16, pair_f16, held_f16), reps=20 if nb == 8192 else 10 if nb == 32768 else 4)
        mat_b = 2 * nb * nb
        one_b = mat_b + 4 * nb
        md, mp, mh = d[len(d) // 2], p[len(p) // 2], h[len(h) // 2]
        for name, t, m, nbytes in ((f"f16_mvm_transposed_{nb}", d, md, one_b), (f"f16_transpose_then_mvm_{nb}", p, mp, 2 * mat_b + one_b),
                                   (f"f16_mvm_held_transpose_{nb}", h, mh, one_b)):
            res[name] = {"ms": round(m, 5), "rounds_ms": [round(v, 5) for v in t], "spread_ms": round(t[-1] - t[0], 5),
                         "GB/s": round(nbytes / m / 1e6, 1), "frac_of_8TBs": round(nbytes / m / 1e6 / 8000.0, 4)}
        res[f"f16_mvm_transposed_{nb}"].update({
            "speedup_over_transpose_then_mvm": round(mp / md, 3), "faster_than_the_pair_by_more_than_its_spread": bool(mp - md > p[-1] - p[0]),
            "ratio_to_mvm_on_a_held_transpose": round(md / mh, 3), "within_the_spread_of_the_held_transpose_call": bool(abs(md - mh) <= h[-1] - h[0])})
        del hA, hAt, hx, hr
    if selected("f16_iht_one_matrix_N8192"):
        im, inn, iters = 4096, 8192, 20
        P, PT = hip.alloc(2 * im * inn), hip.alloc(2 * im * inn)
        f16_fill(P, im * inn, 65)
        hip.check(lib.clm_f16_transpose(P.ptr, im, inn, PT.ptr, None))
        vy, vx, vt1, vt2, vt3 = (hip.alloc(2 * n) for n in (im, inn, im, im, inn))
        f16_fill(vy, im, 501)
        tail = (vx.ptr, inn, vy.ptr, vt1.ptr, vt2.ptr, vt3.ptr, iters, im // 4, 2.0 ** -24, 1, None)

        def two_f16():
            hip.check(lib.clm_f16_iht(P.ptr, PT.ptr, im, inn, *tail))

        def one_f16():
            hip.check(lib.clm_f16_iht_one_matrix(P.ptr, im, inn, *tail))
        t2, t1 = ([v / iters for v in t] for t in alternated((two_f16, one_f16), reps=2))
        m2, m1 = t2[len(t2) // 2], t1[len(t1) // 2]
        res["f16_iht_one_matrix_N8192"] = {
            "one_matrix_ms_per_iteration": round(m1, 5), "clm_f16_iht_ms_per_iteration": round(m2, 5),
            "one_matrix_rounds_ms": [round(v, 5) for v in t1], "clm_f16_iht_rounds_ms": [round(v, 5) for v in t2],
            "ratio_to_clm_f16_iht": round(m1 / m2, 3), "within_the_spread_of_clm_f16_iht": bool(abs(m1 - m2) <= t2[-1] - t2[0]),
            "note": f"calls of {iters} iterations, 4096 x 8192, K = m / 4, FAST threshold; both loops are launch per step"}
        del P, PT
    if ONLY and all(any(o in r for r in F16T_ROWS) for o in ONLY.split(",")):
        print(json.dumps(res, indent=1))
        sys.exit(0)


# ---- CloverMatrix4 on fp32 vectors (mvm_f32.hip, mvm_f32_t.hip; clover_hip_m4_f32.h).  Per row the calls of ONE session on the same matrix
# and vectors, their rounds ALTERNATED.  mvm_f32_transposed_<n>^2: clm4_mvm_f32_transposed beside (a) clm4_transpose + clm4_mvm_f32 and
# (b) clm4_mvm_f32 on a held A'.  mvm_f32_scale_and_add_<n>^2 / mvm_f32_transposed_scale_and_add_<n>^2: the fused call beside the two calls it
# replaces.  m4_f32_iht_loop_N8192 (Phi 4096 x 8192, FAST): clm4_iht_f32 and clm4_iht_f32_one_matrix beside the five calls issued one by one
# (three launches: clm4_mvm_f32, clv_f32_scale_and_add twice and the threshold are four calls, the products two more), ms per iteration.
# 8192^2 is cache-resident (32 MiB of nibbles): no share of the HBM peak is claimed for it.
# KB_ONLY=mvm_f32_transposed,mvm_f32_scale_and_add,m4_f32_iht_loop selects them and the run ends after them.
M4F32_ROWS = tuple(f"{k}_{nb}^2" for nb in MVT_SIZES for k in ("mvm_f32_transposed", "mvm_f32_transpose_then_mvm", "mvm_f32_held_transpose",
                                                                "mvm_f32_scale_and_add", "mvm_f32_transposed_scale_and_add")) + ("m4_f32_iht_loop_N8192",)


def summary(t, nbytes, hbm):
    m = t[len(t) // 2]
    out = {"ms": round(m, 5), "rounds_ms": [round(v, 5) for v in t], "spread_ms": round(t[-1] - t[0], 5), "GB/s": round(nbytes / m / 1e6, 1)}
    if hbm:
        out["frac_of_8TBs"] = round(nbytes / m / 1e6 / 8000.0, 4)
    else:
        out["note"] = "cache-resident: the matrix fits the 256 MiB Infinity Cache, GB/s is no share of the HBM peak"
    return out


if any(selected(r) for r in M4F32_ROWS):
    for nb in MVT_SIZES:
        if not any(selected(r) for r in M4F32_ROWS if r.endswith(f"_{nb}^2")):
            continue
        fA, fsA, fAt, fsAt = hip.alloc(nb * nb // 2), hip.alloc(4 * (nb // 64) ** 2), hip.alloc(nb * nb // 2), hip.alloc(4 * (nb // 64) ** 2)
        hip.check(lib.clv_fill_random_nibbles(fA.ptr, fA.nbytes, 81, 0, None))
        hip.check(lib.clv_fill_random_scales(fsA.ptr, fsA.nbytes // 4, 82, 0, None))
        fx, fu, ft, fr = (hip.alloc(4 * nb) for _ in range(4))
        hip.check(lib.clv_fill_random_ints_f32(fx.ptr, nb, 10, 83, 0, None))
        hip.check(lib.clv_fill_random_ints_f32(fu.ptr, nb, 10, 84, 0, None))
        hip.check(lib.clm4_transpose(fA.ptr, fsA.ptr, nb, nb, fAt.ptr, fsAt.ptr, None))
        reps = 20 if nb == 8192 else 10 if nb == 32768 else 4
        hbm = nb > 8192
        mat_b = nb * nb // 2 + 4 * (nb // 64) ** 2
        one_b = mat_b + 8 * nb

        def direct_f32():
            hip.check(lib.clm4_mvm_f32_transposed(fA.ptr, fsA.ptr, nb, nb, fx.ptr, fr.ptr, None))

        def pair_f32():
            hip.check(lib.clm4_transpose(fA.ptr, fsA.ptr, nb, nb, fAt.ptr, fsAt.ptr, None))
            hip.check(lib.clm4_mvm_f32(fAt.ptr, fsAt.ptr, nb, nb, fx.ptr, fr.ptr, None))

        def held_f32():
            hip.check(lib.clm4_mvm_f32(fAt.ptr, fsAt.ptr, nb, nb, fx.ptr, fr.ptr, None))
        if any(selected(f"{k}_{nb}^2") for k in ("mvm_f32_transposed", "mvm_f32_transpose_then_mvm", "mvm_f32_held_transpose")):
            d, p, h = alternated((direct_f32, pair_f32, held_f32), reps=reps)
            md, mp, mh = d[len(d) // 2], p[len(p) // 2], h[len(h) // 2]
            res[f"mvm_f32_transposed_{nb}^2"] = summary(d, one_b, hbm)
            res[f"mvm_f32_transpose_then_mvm_{nb}^2"] = summary(p, 3 * mat_b + 8 * nb, hbm)
            res[f"mvm_f32_held_transpose_{nb}^2"] = summary(h, one_b, hbm)
            res[f"mvm_f32_transposed_{nb}^2"].update({
                "speedup_over_transpose_then_mvm": round(mp / md, 3), "faster_than_the_pair_by_more_than_its_spread": bool(mp - md > p[-1] - p[0]),
                "ratio_to_mvm_on_a_held_transpose": round(md / mh, 3), "within_the_spread_of_the_held_transpose_call": bool(abs(md - mh) <= h[-1] - h[0])})
        for name, fused_fn, plain_fn, mat in (("mvm_f32_scale_and_add", lib.clm4_mvm_f32_scale_and_add, lib.clm4_mvm_f32, (fA, fsA)),
                                              ("mvm_f32_transposed_scale_and_add", lib.clm4_mvm_f32_transposed_scale_and_add,
                                               lib.clm4_mvm_f32_transposed, (fA, fsA))):
            if not selected(f"{name}_{nb}^2"):
                continue

            def fused_call(fused_fn=fused_fn, mat=mat):
                hip.check(fused_fn(mat[0].ptr, mat[1].ptr, nb, nb, fx.ptr, fu.ptr, 0.37, ft.ptr, fr.ptr, None))

            def two_calls(plain_fn=plain_fn, mat=mat):
                hip.check(plain_fn(mat[0].ptr, mat[1].ptr, nb, nb, fx.ptr, ft.ptr, None))
                hip.check(lib.clv_f32_scale_and_add(fu.ptr, ft.ptr, 0.37, nb, fr.ptr, None))
            f, t2 = alternated((fused_call, two_calls), reps=reps)
            mf, m2 = f[len(f) // 2], t2[len(t2) // 2]
            res[f"{name}_{nb}^2"] = summary(f, mat_b + 16 * nb, hbm)
            res[f"{name}_{nb}^2"].update({"two_calls_ms": round(m2, 5), "two_calls_rounds_ms": [round(v, 5) for v in t2],
                                          "two_calls_spread_ms": round(t2[-1] - t2[0], 5), "ratio_to_the_two_calls": round(mf / m2, 3),
                                          "not_slower_than_the_two_calls_by_more_than_their_spread": bool(mf - m2 <= t2[-1] - t2[0])})
        del fA, fsA, fAt, fsAt
    if selected("m4_f32_iht_loop_N8192"):
        im, inn, iters = 4096, 8192, 20
        P, sP, PT, sPT = hip.alloc(im * inn // 2), hip.alloc(4 * (im // 64) * (inn // 64)), hip.alloc(im * inn // 2), hip.alloc(4 * (im // 64) * (inn // 64))
        hip.check(lib.clv_fill_random_nibbles(P.ptr, P.nbytes, 85, 0, None))
        hip.check(lib.clv_fill_random_scales(sP.ptr, sP.nbytes // 4, 86, 0, None))
        hip.check(lib.clm4_transpose(P.ptr, sP.ptr, im, inn, PT.ptr, sPT.ptr, None))
        vy, vx, vt1, vt2, vt3 = (hip.alloc(4 * n) for n in (im, inn, im, im, inn))
        hip.check(lib.clv_fill_random_ints_f32(vy.ptr, im, 10, 87, 0, None))
        K, mu = im // 4, 2.0 ** -24
        tail = (im, inn, vx.ptr, inn, vy.ptr, vt1.ptr, vt2.ptr, vt3.ptr, iters, K, mu, 1, None)

        def two_m():
            hip.check(lib.clm4_iht_f32(P.ptr, sP.ptr, PT.ptr, sPT.ptr, *tail))

        def one_m():
            hip.check(lib.clm4_iht_f32_one_matrix(P.ptr, sP.ptr, *tail))

        def five_calls():
            hip.check(lib.clv_memset(vx.ptr, 0, 4 * inn, None))
            for _ in range(iters):
                hip.check(lib.clm4_mvm_f32(P.ptr, sP.ptr, im, inn, vx.ptr, vt1.ptr, None))
                hip.check(lib.clv_f32_scale_and_add(vy.ptr, vt1.ptr, -1.0, im, vt2.ptr, None))
                hip.check(lib.clm4_mvm_f32(PT.ptr, sPT.ptr, inn, im, vt2.ptr, vt3.ptr, None))
                hip.check(lib.clv_f32_scale_and_add(vx.ptr, vt3.ptr, mu, inn, vx.ptr, None))
                hip.check(lib.clv_f32_threshold_mode(vx.ptr, inn, inn, K, 0, None, None))      # 0 = CLV_THRESHOLD_FAST
        t2m, t1m, t5 = ([v / iters for v in t] for t in alternated((two_m, one_m, five_calls), reps=2))
        m2m, m1m, m5 = t2m[len(t2m) // 2], t1m[len(t1m) // 2], t5[len(t5) // 2]
        res["m4_f32_iht_loop_N8192"] = {
            "clm4_iht_f32_ms_per_iteration": round(m2m, 5), "clm4_iht_f32_one_matrix_ms_per_iteration": round(m1m, 5),
            "five_calls_ms_per_iteration": round(m5, 5), "clm4_iht_f32_rounds_ms": [round(v, 5) for v in t2m],
            "clm4_iht_f32_one_matrix_rounds_ms": [round(v, 5) for v in t1m], "five_calls_rounds_ms": [round(v, 5) for v in t5],
            "two_matrices_over_five_calls": round(m2m / m5, 3), "one_matrix_over_two_matrices": round(m1m / m2m, 3),
            "note": f"calls of {iters} iterations, Phi 4096 x 8192 (16 MiB of nibbles: cache-resident), K = m / 4, FAST threshold; the five calls "
                    "are issued from Python one by one on the same buffers, all on the device"}
        del P, sP, PT, sPT
    if ONLY and all(any(o in r for r in M4F32_ROWS) for o in ONLY.split(",")):
        print(json.dumps(res, indent=1))
        sys.exit(0)


# ---- CloverMatrix8 on fp32 vectors (matrix8.hip, matrix8_f32_t.hip; clover_hip_m8_f32.h): the rows of the block above at one byte per
# element.  m8_mvm_f32_transposed_<n>^2: clm8_mvm_f32_transposed beside (a) clm8_transpose + clm8_mvm_f32 and (b) clm8_mvm_f32 on a held A'
# (65536^2 holds 8 GiB: the matrix and its transpose).  m8_mvm_f32_scale_and_add_<n>^2 / m8_mvm_f32_transposed_scale_and_add_<n>^2: the
# fused call beside the two calls it replaces.  m8_f32_iht_loop_N8192 (Phi 4096 x 8192, FAST): clm8_iht_f32 and clm8_iht_f32_one_matrix
# beside the five calls issued one by one, the baseline's threshold in the FAST mode too; ms per iteration.  8192^2 is cache-resident
# (64 MiB): no share of the HBM peak is claimed for it.
# KB_ONLY=m8_mvm_f32_,m8_f32_iht_loop selects them and the run ends after them.
M8F32_ROWS = tuple(f"{k}_{nb}^2" for nb in MVT_SIZES for k in ("m8_mvm_f32_transposed", "m8_mvm_f32_transpose_then_mvm", "m8_mvm_f32_held_transpose",
                                                                "m8_mvm_f32_scale_and_add", "m8_mvm_f32_transposed_scale_and_add")) + ("m8_f32_iht_loop_N8192",)

if any(selected(r) for r in M8F32_ROWS):
    for nb in MVT_SIZES:
        if not any(selected(r) for r in M8F32_ROWS if r.endswith(f"_{nb}^2")):
            continue
        fA, fsA, fAt, fsAt = hip.alloc(nb * nb), hip.alloc(4 * (nb // 64) ** 2), hip.alloc(nb * nb), hip.alloc(4 * (nb // 64) ** 2)
        hip.check(lib.clv_fill_random_nibbles(fA.ptr, fA.nbytes, 91, 0, None))           # random bytes: every value of an int8
        hip.check(lib.clv_fill_random_scales(fsA.ptr, fsA.nbytes // 4, 92, 0, None))
        fx, fu, ft, fr = (hip.alloc(4 * nb) for _ in range(4))
        hip.check(lib.clv_fill_random_ints_f32(fx.ptr, nb, 10, 93, 0, None))
        hip.check(lib.clv_fill_random_ints_f32(fu.ptr, nb, 10, 94, 0, None))
        hip.check(lib.clm8_transpose(fA.ptr, fsA.ptr, nb, nb, fAt.ptr, fsAt.ptr, None))
        reps = 20 if nb == 8192 else 10 if nb == 32768 else 4
        hbm = nb > 8192
        mat_b = nb * nb + 4 * (nb // 64) ** 2
        one_b = mat_b + 8 * nb

        def direct_m8():
            hip.check(lib.clm8_mvm_f32_transposed(fA.ptr, fsA.ptr, nb, nb, fx.ptr, fr.ptr, None))

        def pair_m8():
            hip.check(lib.clm8_transpose(fA.ptr, fsA.ptr, nb, nb, fAt.ptr, fsAt.ptr, None))
            hip.check(lib.clm8_mvm_f32(fAt.ptr, fsAt.ptr, nb, nb, fx.ptr, fr.ptr, None))

        def held_m8():
            hip.check(lib.clm8_mvm_f32(fAt.ptr, fsAt.ptr, nb, nb, fx.ptr, fr.ptr, None))
        if any(selected(f"{k}_{nb}^2") for k in ("m8_mvm_f32_transposed", "m8_mvm_f32_transpose_then_mvm", "m8_mvm_f32_held_transpose")):
            d, p, h = alternated((direct_m8, pair_m8, held_m8), reps=reps)
            md, mp, mh = d[len(d) // 2], p[len(p) // 2], h[len(h) // 2]
            res[f"m8_mvm_f32_transposed_{nb}^2"] = summary(d, one_b, hbm)
            res[f"m8_mvm_f32_transpose_then_mvm_{nb}^2"] = summary(p, 3 * mat_b + 8 * nb, hbm)
            res[f"m8_mvm_f32_held_transpose_{nb}^2"] = summary(h, one_b, hbm)
            res[f"m8_mvm_f32_transposed_{nb}^2"].update({
                "speedup_over_transpose_then_mvm": round(mp / md, 3), "faster_than_the_pair_by_more_than_its_spread": bool(mp - md > p[-1] - p[0]),
                "ratio_to_mvm_on_a_held_transpose": round(md / mh, 3), "within_the_spread_of_the_held_transpose_call": bool(abs(md - mh) <= h[-1] - h[0])})
        for name, fused_fn, plain_fn in (("m8_mvm_f32_scale_and_add", lib.clm8_mvm_f32_scale_and_add, lib.clm8_mvm_f32),
                                         ("m8_mvm_f32_transposed_scale_and_add", lib.clm8_mvm_f32_transposed_scale_and_add, lib.clm8_mvm_f32_transposed)):
            if not selected(f"{name}_{nb}^2"):
                continue

            def fused_call(fused_fn=fused_fn):
                hip.check(fused_fn(fA.ptr, fsA.ptr, nb, nb, fx.ptr, fu.ptr, 0.37, ft.ptr, fr.ptr, None))

            def two_calls(plain_fn=plain_fn):
                hip.check(plain_fn(fA.ptr, fsA.ptr, nb, nb, fx.ptr, ft.ptr, None))
                hip.check(lib.clv_f32_scale_and_add(fu.ptr, ft.ptr, 0.37, nb, fr.ptr, None))
            f, t2 = alternated((fused_call, two_calls), reps=reps)
            mf, m2 = f[len(f) // 2], t2[len(t2) // 2]
            res[f"{name}_{nb}^2"] = summary(f, mat_b + 16 * nb, hbm)
            res[f"{name}_{nb}^2"].update({"two_calls_ms": round(m2, 5), "two_calls_rounds_ms": [round(v, 5) for v in t2],
                                          "two_calls_spread_ms": round(t2[-1] - t2[0], 5), "ratio_to_the_two_calls": round(mf / m2, 3),
                                          "not_slower_than_the_two_calls_by_more_than_their_spread": bool(mf - m2 <= t2[-1] - t2[0])})
        del fA, fsA, fAt, fsAt
    if selected("m8_f32_iht_loop_N8192"):
        im, inn, iters = 4096, 8192, 20
        P, sP, PT, sPT = hip.alloc(im * inn), hip.alloc(4 * (im // 64) * (inn // 64)), hip.alloc(im * inn), hip.alloc(4 * (im // 64) * (inn // 64))
        hip.check(lib.clv_fill_random_nibbles(P.ptr, P.nbytes, 95, 0, None))
        hip.check(lib.clv_fill_random_scales(sP.ptr, sP.nbytes // 4, 96, 0, None))
        hip.check(lib.clm8_transpose(P.ptr, sP.ptr, im, inn, PT.ptr, sPT.ptr, None))
        vy, vx, vt1, vt2, vt3 = (hip.alloc(4 * n) for n in (im, inn, im, im, inn))
        hip.check(lib.clv_fill_random_ints_f32(vy.ptr, im, 10, 97, 0, None))
        K, mu = im // 4, 2.0 ** -24
        tail = (im, inn, vx.ptr, inn, vy.ptr, vt1.ptr, vt2.ptr, vt3.ptr, iters, K, mu, 1, None)

        def two_m8():
            hip.check(lib.clm8_iht_f32(P.ptr, sP.ptr, PT.ptr, sPT.ptr, *tail))

        def one_m8():
            hip.check(lib.clm8_iht_f32_one_matrix(P.ptr, sP.ptr, *tail))

        def five_calls_m8():
            hip.check(lib.clv_memset(vx.ptr, 0, 4 * inn, None))
            for _ in range(iters):
                hip.check(lib.clm8_mvm_f32(P.ptr, sP.ptr, im, inn, vx.ptr, vt1.ptr, None))
                hip.check(lib.clv_f32_scale_and_add(vy.ptr, vt1.ptr, -1.0, im, vt2.ptr, None))
                hip.check(lib.clm8_mvm_f32(PT.ptr, sPT.ptr, inn, im, vt2.ptr, vt3.ptr, None))
                hip.check(lib.clv_f32_scale_and_add(vx.ptr, vt3.ptr, mu, inn, vx.ptr, None))
                hip.check(lib.clv_f32_threshold_mode(vx.ptr, inn, inn, K, 0, None, None))      # 0 = CLV_THRESHOLD_FAST, as the loops' threshold = 1
        t2m, t1m, t5 = ([v / iters for v in t] for t in alternated((two_m8, one_m8, five_calls_m8), reps=2))
        m2m, m1m, m5 = t2m[len(t2m) // 2], t1m[len(t1m) // 2], t5[len(t5) // 2]
        res["m8_f32_iht_loop_N8192"] = {
            "clm8_iht_f32_ms_per_iteration": round(m2m, 5), "clm8_iht_f32_one_matrix_ms_per_iteration": round(m1m, 5),
            "five_calls_ms_per_iteration": round(m5, 5), "clm8_iht_f32_rounds_ms": [round(v, 5) for v in t2m],
            "clm8_iht_f32_one_matrix_rounds_ms": [round(v, 5) for v in t1m], "five_calls_rounds_ms": [round(v, 5) for v in t5],
            "two_matrices_over_five_calls": round(m2m / m5, 3), "one_matrix_over_two_matrices": round(m1m / m2m, 3),
            "note": f"calls of {iters} iterations, Phi 4096 x 8192 (32 MiB of bytes: cache-resident), K = m / 4, FAST threshold on both sides; the "
                    "five calls are issued from Python one by one on the same buffers, all on the device"}
        del P, sP, PT, sPT
    if ONLY and all(any(o in r for r in M8F32_ROWS) for o in ONLY.split(",")):
        print(json.dumps(res, indent=1))
        sys.exit(0)


# ---- vector ops at n = 2^30 (4 GiB fp32 source, 512 MiB + 64 MiB quantized) and n = 2^24
for logn in (24, 30):
    n = 1 << logn
    x = hip.alloc(4 * n)
    hip.check(lib.clv_fill_random_ints_f32(x.ptr, n, 10, 5, 0, None))
    q, s = hip.alloc(n // 2), hip.alloc(n // 16)
    q2, s2 = hip.alloc(n // 2), hip.alloc(n // 16)
    q3, s3 = hip.alloc(n // 2), hip.alloc(n // 16)
    out = hip.alloc(8)
    rng = hip.new_rng(1, 2)
    hip.check(lib.clv4_quantize(x.ptr, n, q.ptr, s.ptr, None, None))         # operands exist even when KB_ONLY skips the timed calls
    hip.check(lib.clv4_quantize(x.ptr, n, q2.ptr, s2.ptr, None, None))
    rec(f"quantize_n2^{logn}", 4.5625 * n, lambda: hip.check(lib.clv4_quantize(x.ptr, n, q.ptr, s.ptr, None, None)))
    rec(f"quantize_stochastic_n2^{logn}", 4.5625 * n, lambda: hip.check(lib.clv4_quantize(x.ptr, n, q2.ptr, s2.ptr, rng.ptr, None)))
    rec(f"dot_fast_n2^{logn}", 1.125 * n, lambda: hip.check(lib.clv4_dot(q.ptr, s.ptr, q2.ptr, s2.ptr, n, DOT_FAST, out.ptr, None, None)))
    rec(f"scale_and_add_n2^{logn}", 1.6875 * n, lambda: hip.check(lib.clv4_scale_and_add(q.ptr, s.ptr, q2.ptr, s2.ptr, 0.5, n, q3.ptr, s3.ptr, None, None)))
    rec(f"scale_and_add_stochastic_n2^{logn}", 1.6875 * n, lambda: hip.check(lib.clv4_scale_and_add(q.ptr, s.ptr, q2.ptr, s2.ptr, 0.5, n, q3.ptr, s3.ptr, rng.ptr, None)))
    q8 = hip.alloc(n)
    rec(f"v8_quantize_n2^{logn}", 5.0625 * n, lambda: hip.check(lib.clv8_quantize(x.ptr, n, q8.ptr, s3.ptr, None, None)))
    rec(f"v8_quantize_stochastic_n2^{logn}", 5.0625 * n, lambda: hip.check(lib.clv8_quantize(x.ptr, n, q8.ptr, s3.ptr, rng.ptr, None)))
    rec(f"restore_n2^{logn}", 4.5625 * n, lambda: hip.check(lib.clv4_restore(q.ptr, s.ptr, n, x.ptr, None)))
    if logn == 24:
        k = n // 4
        hip.check(lib.clv_memcpy_d2d(q3.ptr, q.ptr, n // 2, None))
        thr_note = ("three launches (round 6): the pass over the nibbles builds per-block magnitude tables and radix level 0, one persistent launch "
                    "runs levels 1-2 and the tie prefixes over the tables, one pass applies on bit planes (threshold4_large, threshold4.hip); bytes = "
                    "nibbles + scales read and written once each (1.125 n; rounds 3-5 counted five passes here), time = calls back to back on one "
                    "stream incl. launch gaps (kernel time alone: profiles/r06_threshold_three_launch.txt)")
        rec(f"threshold_k25pct_n2^{logn}", 1.125 * n, lambda: hip.check(lib.clv4_threshold(q3.ptr, s.ptr, n, n, k, None, None)), reps=3,
            extra={"note": thr_note})
        nb = 1 << 28
        qb, sb = hip.alloc(nb // 2), hip.alloc(nb // 16)
        hip.check(lib.clv_fill_random_nibbles(qb.ptr, qb.nbytes, 7, 0, None))
        hip.check(lib.clv_fill_random_scales(sb.ptr, nb // 64, 8, 0, None))
        rec("threshold_k25pct_n2^28", 1.125 * nb, lambda: hip.check(lib.clv4_threshold(qb.ptr, sb.ptr, nb, nb, nb // 4, None, None)), reps=3,
            extra={"note": thr_note + "; the vector is thresholded in place, so every call after the first finds it already thresholded (same passes, same time)"})
        del qb, sb
        rec(f"dot_exact_n2^{logn}", 1.125 * n, lambda: hip.check(lib.clv4_dot(q.ptr, s.ptr, q2.ptr, s2.ptr, n, DOT_EXACT, out.ptr, None, None)), reps=2)
    q8b = hip.alloc(n)
    hip.check(lib.clv8_quantize(x.ptr, n, q8.ptr, s3.ptr, None, None))
    hip.check(lib.clv8_quantize(x.ptr, n, q8b.ptr, s2.ptr, None, None))
    rec(f"v8_dot_fast_n2^{logn}", 2.125 * n, lambda: hip.check(lib.clv8_dot(q8.ptr, s3.ptr, q8b.ptr, s2.ptr, n, DOT_FAST, out.ptr, None, None)))
    if logn == 24:
        rec(f"v8_dot_exact_n2^{logn}", 2.125 * n, lambda: hip.check(lib.clv8_dot(q8.ptr, s3.ptr, q8b.ptr, s2.ptr, n, DOT_EXACT, out.ptr, None, None)), reps=2)
    q8c = hip.alloc(n)
    rec(f"v8_scale_and_add_n2^{logn}", 3.1875 * n, lambda: hip.check(lib.clv8_scale_and_add(q8.ptr, s3.ptr, q8b.ptr, s2.ptr, 0.5, n, q8c.ptr, s.ptr, None, None)))
    rec(f"v8_scale_and_add_stochastic_n2^{logn}", 3.1875 * n, lambda: hip.check(lib.clv8_scale_and_add(q8.ptr, s3.ptr, q8b.ptr, s2.ptr, 0.5, n, q8c.ptr, s.ptr, rng.ptr, None)))
    del q8c, q8b
    rec(f"v8_restore_n2^{logn}", 5.0625 * n, lambda: hip.check(lib.clv8_restore(q8.ptr, s3.ptr, n, x.ptr, None)))
    del x, q, s, q2, s2, q3, s3, q8

# ---- matrix ops: 32768 x 32768 (4 GiB fp32 source, 512 MiB quantized)
M = N = 32768
A = hip.alloc(4 * M * N)
hip.check(lib.clv_fill_random_ints_f32(A.ptr, M * N, 10, 6, 0, None))
qA, sA = hip.alloc(M * N // 2), hip.alloc((M // 64) * (N // 64) * 4)
qT, sT = hip.alloc(M * N // 2), hip.alloc((M // 64) * (N // 64) * 4)
rngm = hip.new_rng(3, 4)
rec("matrix_quantize_32768^2", 4.5625 * M * N, lambda: hip.check(lib.clm4_quantize(A.ptr, M, N, qA.ptr, sA.ptr, None, None)), reps=3)
rec("matrix_quantize_stochastic_32768^2", 4.5625 * M * N, lambda: hip.check(lib.clm4_quantize(A.ptr, M, N, qT.ptr, sT.ptr, rngm.ptr, None)), reps=3)
rec("transpose_32768^2", 2 * (M * N // 2 + 4 * (M // 64) * (N // 64)), lambda: hip.check(lib.clm4_transpose(qA.ptr, sA.ptr, M, N, qT.ptr, sT.ptr, None)), reps=3)
# shapes whose rows / cols are 128 * odd: edge tiles are masked on the same kernel (r6; the 64-thread kernel they used to fall to is gone)
for (Mr, Nr) in ((32640, 32640), (32768, 32640), (32640, 32768)):
    rec(f"transpose_{Mr}x{Nr}", 2 * (Mr * Nr // 2 + 4 * (Mr // 64) * (Nr // 64)),
        lambda Mr=Mr, Nr=Nr: hip.check(lib.clm4_transpose(qA.ptr, sA.ptr, Mr, Nr, qT.ptr, sT.ptr, None)), reps=3)
x, sx = hip.alloc(N // 2), hip.alloc(N // 16)
r, sr = hip.alloc(M // 2), hip.alloc(M // 16)
hip.check(lib.clv_fill_random_nibbles(x.ptr, x.nbytes, 9, 0, None))
hip.check(lib.clv_fill_random_scales(sx.ptr, sx.nbytes // 4, 10, 0, None))
mvb = M * N // 2 + 4 * (M // 64) * (N // 64) + (N // 2 + N // 16) + (M // 2 + M // 16)
rec("mvm_32768^2", mvb, lambda: hip.check(lib.clm4_mvm(qA.ptr, sA.ptr, M, N, x.ptr, sx.ptr, r.ptr, sr.ptr, None, None)))
rec("mvm_stochastic_32768^2", mvb, lambda: hip.check(lib.clm4_mvm(qA.ptr, sA.ptr, M, N, x.ptr, sx.ptr, r.ptr, sr.ptr, rngm.ptr, None)))
# ---- mixed precision: 4-bit matrix x 8-bit vector
x8, r8 = hip.alloc(N), hip.alloc(M)
hip.check(lib.clv_fill_random_nibbles(x8.ptr, x8.nbytes, 11, 0, None))          # any bytes; 0x80 never occurs (nibbles are in [-7,7])
mvb8 = M * N // 2 + 4 * (M // 64) * (N // 64) + (N + N // 16) + (M + M // 16)
rec("mvm_v8_32768^2", mvb8, lambda: hip.check(lib.clm4_mvm_v8(qA.ptr, sA.ptr, M, N, x8.ptr, sx.ptr, r8.ptr, sr.ptr, None, None)))
rec("mvm_v8_stochastic_32768^2", mvb8, lambda: hip.check(lib.clm4_mvm_v8(qA.ptr, sA.ptr, M, N, x8.ptr, sx.ptr, r8.ptr, sr.ptr, rngm.ptr, None)))
# ---- mixed precision: 4-bit matrix x fp32 vector (fp32 row dots out)
xf32, rf32 = hip.alloc(4 * N), hip.alloc(4 * M)
hip.check(lib.clv_fill_random_ints_f32(xf32.ptr, N, 10, 12, 0, None))
rec("mvm_f32_32768^2", M * N // 2 + 4 * (M // 64) * (N // 64) + 4 * N + 4 * M,
    lambda: hip.check(lib.clm4_mvm_f32(qA.ptr, sA.ptr, M, N, xf32.ptr, rf32.ptr, None)))
# ---- the headline shape, 65536 x 65536 (2 GiB of nibbles): 4-bit and mixed mvm side by side
del A, qT, sT
M2 = N2 = 65536
big, sbig = hip.alloc(M2 * N2 // 2), hip.alloc((M2 // 64) * (N2 // 64) * 4)
hip.check(lib.clv_fill_random_nibbles(big.ptr, big.nbytes, 21, 0, None))
hip.check(lib.clv_fill_random_scales(sbig.ptr, sbig.nbytes // 4, 22, 0, None))
xb4, xb8, sxb = hip.alloc(N2 // 2), hip.alloc(N2), hip.alloc(N2 // 16)
rb, srb = hip.alloc(M2), hip.alloc(M2 // 16)
hip.check(lib.clv_fill_random_nibbles(xb8.ptr, xb8.nbytes, 23, 0, None))
hip.check(lib.clv_fill_random_nibbles(xb4.ptr, xb4.nbytes, 24, 0, None))
hip.check(lib.clv_fill_random_scales(sxb.ptr, sxb.nbytes // 4, 25, 0, None))
base = M2 * N2 // 2 + 4 * (M2 // 64) * (N2 // 64)
rec("mvm_65536^2", base + (N2 // 2 + N2 // 16) + (M2 // 2 + M2 // 16),
    lambda: hip.check(lib.clm4_mvm(big.ptr, sbig.ptr, M2, N2, xb4.ptr, sxb.ptr, rb.ptr, srb.ptr, None, None)))
rec("mvm_v8_65536^2", base + (N2 + N2 // 16) + (M2 + M2 // 16),
    lambda: hip.check(lib.clm4_mvm_v8(big.ptr, sbig.ptr, M2, N2, xb8.ptr, sxb.ptr, rb.ptr, srb.ptr, None, None)))
# ---- CloverMatrix8: int8 values + one fp32 scale per 64x64 tile (1 + 4/4096 bytes per element)
del big, sbig, xb4, xb8, sxb, rb, srb, qA, sA
for n8 in (32768, 65536):
    vals, scs = n8 * n8, 4 * (n8 // 64) ** 2
    A8 = hip.alloc(4 * vals)
    hip.check(lib.clv_fill_random_ints_f32(A8.ptr, vals, 10, 31, 0, None))
    q8m, s8m, q8t, s8t = hip.alloc(vals), hip.alloc(scs), hip.alloc(vals), hip.alloc(scs)
    rng8 = hip.new_rng(5, 6)
    rec(f"m8_quantize_{n8}^2", 4 * vals + vals + scs, lambda: hip.check(lib.clm8_quantize(A8.ptr, n8, n8, q8m.ptr, s8m.ptr, None, None)), reps=3)
    rec(f"m8_quantize_stochastic_{n8}^2", 4 * vals + vals + scs,
        lambda: hip.check(lib.clm8_quantize(A8.ptr, n8, n8, q8t.ptr, s8t.ptr, rng8.ptr, None)), reps=3)
    del A8
    rec(f"m8_transpose_{n8}^2", 2 * (vals + scs), lambda: hip.check(lib.clm8_transpose(q8m.ptr, s8m.ptr, n8, n8, q8t.ptr, s8t.ptr, None)), reps=3)
    xv8, sxv8, rv8, srv8 = hip.alloc(n8), hip.alloc(n8 // 16), hip.alloc(n8), hip.alloc(n8 // 16)
    hip.check(lib.clv_fill_random_nibbles(xv8.ptr, n8, 41, 0, None))
    hip.check(lib.clv_fill_random_scales(sxv8.ptr, n8 // 64, 42, 0, None))
    mv8 = vals + scs + 2 * (n8 + n8 // 16)
    rec(f"m8_mvm_v8_{n8}^2", mv8, lambda: hip.check(lib.clm8_mvm(q8m.ptr, s8m.ptr, n8, n8, xv8.ptr, sxv8.ptr, rv8.ptr, srv8.ptr, None, None)))
    rec(f"m8_mvm_v8_stochastic_{n8}^2", mv8,
        lambda: hip.check(lib.clm8_mvm(q8m.ptr, s8m.ptr, n8, n8, xv8.ptr, sxv8.ptr, rv8.ptr, srv8.ptr, rng8.ptr, None)))
    # the same mvm with the scaleAndAdd behind it in its epilogue (clm8_mvm_scale_and_add): + u read and r written, one wave of work per row group
    uv8, suv8, r2v8, sr2v8 = hip.alloc(n8), hip.alloc(n8 // 16), hip.alloc(n8), hip.alloc(n8 // 16)
    hip.check(lib.clv_fill_random_nibbles(uv8.ptr, n8, 48, 0, None))
    hip.check(lib.clv_fill_random_scales(suv8.ptr, n8 // 64, 49, 0, None))
    rec(f"m8_mvm_scale_and_add_{n8}^2", mv8 + 2 * (n8 + n8 // 16),
        lambda: hip.check(lib.clm8_mvm_scale_and_add(q8m.ptr, s8m.ptr, n8, n8, xv8.ptr, sxv8.ptr, uv8.ptr, suv8.ptr, -1.0, rv8.ptr, srv8.ptr, r2v8.ptr,
                                                     sr2v8.ptr, None, None)))
    rec(f"m8_mvm_scale_and_add_stochastic_{n8}^2", mv8 + 2 * (n8 + n8 // 16),
        lambda: hip.check(lib.clm8_mvm_scale_and_add(q8m.ptr, s8m.ptr, n8, n8, xv8.ptr, sxv8.ptr, uv8.ptr, suv8.ptr, -1.0, rv8.ptr, srv8.ptr, r2v8.ptr,
                                                     sr2v8.ptr, rng8.ptr, None)))
    del uv8, suv8, r2v8, sr2v8
    xf, rf = hip.alloc(4 * n8), hip.alloc(4 * n8)
    hip.check(lib.clv_fill_random_ints_f32(xf.ptr, n8, 10, 43, 0, None))
    rec(f"m8_mvm_f32_{n8}^2", vals + scs + 8 * n8, lambda: hip.check(lib.clm8_mvm_f32(q8m.ptr, s8m.ptr, n8, n8, xf.ptr, rf.ptr, None)))
    del q8m, s8m, q8t, s8t, xv8, sxv8, rv8, srv8, xf, rf
# the published mvm size (doc/results/performance.txt, 8-bit column): 8192^2 = 64 MiB, cache-resident across calls
n8 = 8192
q8m, s8m = hip.alloc(n8 * n8), hip.alloc(4 * (n8 // 64) ** 2)
hip.check(lib.clv_fill_random_nibbles(q8m.ptr, n8 * n8, 44, 0, None))
hip.check(lib.clv_fill_random_scales(s8m.ptr, (n8 // 64) ** 2, 45, 0, None))
xv8, sxv8, rv8, srv8 = hip.alloc(n8), hip.alloc(n8 // 16), hip.alloc(n8), hip.alloc(n8 // 16)
hip.check(lib.clv_fill_random_nibbles(xv8.ptr, n8, 46, 0, None))
hip.check(lib.clv_fill_random_scales(sxv8.ptr, n8 // 64, 47, 0, None))
rec("m8_mvm_v8_8192^2", n8 * n8 + 4 * (n8 // 64) ** 2 + 2 * (n8 + n8 // 16),
    lambda: hip.check(lib.clm8_mvm(q8m.ptr, s8m.ptr, n8, n8, xv8.ptr, sxv8.ptr, rv8.ptr, srv8.ptr, None, None)))
del q8m, s8m, xv8, sxv8, rv8, srv8
# one iteration of Q_IHT<CloverMatrix8, CloverVector8> as CloverIHT.h's generic template issues it (Phi m x n with m = N/2, K = N/4):
# mvm, scaleAndAdd, mvm (PhiT), scaleAndAdd, threshold -- five launches; threshold in both tie rules (the headers' default is the reference's)
from clover_amd.lib_binding import THRESHOLD_FAST, THRESHOLD_REFERENCE  # noqa: E402
for N8 in (8192, 16384):
    m8r, n8c, K8 = N8 // 2, N8, N8 // 4
    P, sP, PT, sPT = hip.alloc(m8r * n8c), hip.alloc(4 * (m8r // 64) * (n8c // 64)), hip.alloc(m8r * n8c), hip.alloc(4 * (m8r // 64) * (n8c // 64))
    hip.check(lib.clv_fill_random_nibbles(P.ptr, m8r * n8c, 51, 0, None))
    hip.check(lib.clv_fill_random_scales(sP.ptr, (m8r // 64) * (n8c // 64), 52, 0, None))
    hip.check(lib.clm8_transpose(P.ptr, sP.ptr, m8r, n8c, PT.ptr, sPT.ptr, None))
    vx, svx, vt3, svt3 = hip.alloc(n8c), hip.alloc(n8c // 16), hip.alloc(n8c), hip.alloc(n8c // 16)
    vy, svy, vt1, svt1, vt2, svt2 = hip.alloc(m8r), hip.alloc(m8r // 16), hip.alloc(m8r), hip.alloc(m8r // 16), hip.alloc(m8r), hip.alloc(m8r // 16)
    hip.check(lib.clv_fill_random_nibbles(vx.ptr, n8c, 53, 0, None))
    hip.check(lib.clv_fill_random_scales(svx.ptr, n8c // 64, 54, 0, None))
    hip.check(lib.clv_fill_random_nibbles(vy.ptr, m8r, 55, 0, None))
    hip.check(lib.clv_fill_random_scales(svy.ptr, m8r // 64, 56, 0, None))

    def iht8_iteration(mode):
        hip.check(lib.clm8_mvm(P.ptr, sP.ptr, m8r, n8c, vx.ptr, svx.ptr, vt1.ptr, svt1.ptr, None, None))
        hip.check(lib.clv8_scale_and_add(vy.ptr, svy.ptr, vt1.ptr, svt1.ptr, -1.0, m8r, vt2.ptr, svt2.ptr, None, None))
        hip.check(lib.clm8_mvm(PT.ptr, sPT.ptr, n8c, m8r, vt2.ptr, svt2.ptr, vt3.ptr, svt3.ptr, None, None))
        hip.check(lib.clv8_scale_and_add(vx.ptr, svx.ptr, vt3.ptr, svt3.ptr, 0.5, n8c, vx.ptr, svx.ptr, None, None))
        hip.check(lib.clv8_threshold_mode(vx.ptr, svx.ptr, n8c, n8c, K8, mode, None, None))
    itb = 2 * (m8r * n8c + 4 * (m8r // 64) * (n8c // 64))
    rec(f"m8_q_iht_iteration_N{N8}", itb, lambda: iht8_iteration(THRESHOLD_REFERENCE), reps=5,
        extra={"note": "bytes = the two matrices only; threshold in the reference's tie rule (the headers' default)"})
    rec(f"m8_q_iht_iteration_fast_threshold_N{N8}", itb, lambda: iht8_iteration(THRESHOLD_FAST), reps=5,
        extra={"note": "bytes = the two matrices only; threshold with lowest-index ties (-DCLOVER_FAST)"})
    # the same loop as ONE call (clm8_iht): x.clear(), then per iteration two fused mvm + scaleAndAdd launches and the threshold -- three
    # launches instead of five (two for GD).  ms is per iteration: a call of LOOP_ITERS iterations, divided.  mu = 2^-24 keeps x finite over
    # the call on these random operands (the launch-by-launch rows above run on whatever their x has become; the kernels' time does not
    # depend on the data, the REFERENCE threshold's heap walk does)
    LOOP_ITERS = 10

    def iht8_loop(thr):
        hip.check(lib.clm8_iht(P.ptr, sP.ptr, PT.ptr, sPT.ptr, m8r, n8c, vx.ptr, svx.ptr, n8c, vy.ptr, svy.ptr, vt1.ptr, svt1.ptr, vt2.ptr, svt2.ptr,
                               vt3.ptr, svt3.ptr, LOOP_ITERS, K8, 2.0 ** -24, thr, None, None))
    for row, thr, note in ((f"m8_iht_loop_N{N8}", 1, "threshold with lowest-index ties (-DCLOVER_FAST)"),
                           (f"m8_iht_loop_reference_threshold_N{N8}", 2, "threshold in the reference's tie rule (the headers' default)"),
                           (f"m8_gd_loop_N{N8}", 0, "no threshold (Q_GD)")):
        if not selected(row):
            continue
        rec(row, itb * LOOP_ITERS, lambda thr=thr: iht8_loop(thr), reps=2,
            extra={"note": f"one clm8_iht call of {LOOP_ITERS} iterations, ms per iteration; bytes = the two matrices only; " + note})
        res[row]["ms"] = round(res[row]["ms"] / LOOP_ITERS, 5)
    del P, sP, PT, sPT, vx, svx, vt3, svt3, vy, svy, vt1, svt1, vt2, svt2
# ---- CloverVector16 / CloverMatrix16: raw binary16, 2 bytes per element, no scales
# the rows of the fused calls and the one-call loop (the second f16 block below); the first block is skipped when only those are asked for
# group sizes of the f16 batch rows: 2, 4 and 8 (every instantiation full); KB_F16_BATCH_GROUPS=3,5,6,7 times the partly filled ones
F16_GROUPS = tuple(int(g) for g in os.environ.get("KB_F16_BATCH_GROUPS", "2,4,8").split(","))
F16_BATCH_ROWS = tuple(f"f16_mvm_batch{g}_{nb}^2" for nb in (32768, 65536) for g in F16_GROUPS) + \
    tuple(f"f16_mvm_saa_batch{g}_8192x4096" for g in F16_GROUPS) + ("f16_iht_batch8_N8192",)
F16_FUSED_ROWS = ("f16_mvm_scale_and_add", "f16_threshold_fast_n8192", "f16_q_iht_iteration", "f16_iht_loop", "f16_gd_loop", "f16_mvm_batch",
                  "f16_mvm_saa_batch", "f16_iht_batch")
# ---- several CloverVector16 with one CloverMatrix16 (half16_batch.hip): every row pairs the batch call, on the batched kernel
# (CLV_MVM_BATCH=1), with the same vectors issued as single calls -- the rounds of the two ALTERNATED in one process, so that a drift of
# the clocks lands on both.  f16_mvm_batch{2,4,8}_{32768,65536}^2: the plain mvm (streaming); f16_mvm_saa_batch{2,4,8}_8192x4096: the fused
# x += mu Phi' t2 step of the IHT shape (cache-resident); f16_iht_batch8_N8192: clm_f16_iht_batch against 8 x clm_f16_iht, ms per iteration
# for 8 signals.  KB_ONLY=f16_mvm_batch,f16_mvm_saa_batch,f16_iht_batch selects them and the run ends after them.
def rec_pair_alternated(name, nbytes_single, g, single, batch, reps=10, per=1, rounds=5, held=None):
    """held: a second baseline (a batch call on a stored transpose), timed forced batched in every round beside the two sides"""
    if not selected(name):
        return

    def forced_batch(fn=batch):
        os.environ["CLV_MVM_BATCH"] = "1"
        try:
            return rounds_of(fn, reps=reps, rounds=1, warm=0)[0] / per
        finally:
            os.environ.pop("CLV_MVM_BATCH", None)
    os.environ.pop("CLV_MVM_BATCH", None)
    rounds_of(single, reps=1, rounds=1, warm=1)
    forced_batch()
    one, many, other = [], [], []
    if held:
        forced_batch(held)
    for _ in range(rounds):
        one.append(rounds_of(single, reps=reps, rounds=1, warm=0)[0] / per)
        many.append(forced_batch())
        if held:
            other.append(forced_batch(held))
    one, many = sorted(one), sorted(many)
    o, m, spread = one[len(one) // 2], many[len(many) // 2], one[-1] - one[0]
    res[name] = {"vectors": g, "batch_ms": round(m, 5), "single_calls_ms": round(o, 5), "single_calls_rounds_ms": [round(t, 5) for t in one],
                 "batch_rounds_ms": [round(t, 5) for t in many], "single_calls_spread_ms": round(spread, 5), "speedup": round(o / m, 3),
                 "batch_faster_by_more_than_the_spread": bool(o - m > spread),
                 "GB/s_per_vector_batch": round(g * nbytes_single / m / 1e6, 1), "GB/s_single_calls": round(g * nbytes_single / o / 1e6, 1)}
    if held:
        other = sorted(other)
        h = other[len(other) // 2]
        res[name].update({"held_transpose_batch_ms": round(h, 5), "held_transpose_batch_rounds_ms": [round(t, 5) for t in other],
                          "held_transpose_batch_spread_ms": round(other[-1] - other[0], 5), "batch_over_held_transpose_batch": round(m / h, 3)})


if any(selected(r) for r in F16_BATCH_ROWS):
    for nb in (32768, 65536):
        if not any(selected(f"f16_mvm_batch{g}_{nb}^2") for g in F16_GROUPS):
            continue
        hA = hip.alloc(2 * nb * nb)
        f16_fill(hA, nb * nb, 63)
        bx, br = [hip.alloc(2 * nb) for _ in range(8)], [hip.alloc(2 * nb) for _ in range(8)]
        for j, b in enumerate(bx):
            f16_fill(b, nb, 300 + j)
        for g in F16_GROUPS:
            def singles(g=g):
                for j in range(g):
                    hip.check(lib.clm_f16_mvm(hA.ptr, nb, nb, bx[j].ptr, br[j].ptr, None))
            rec_pair_alternated(f"f16_mvm_batch{g}_{nb}^2", 2 * nb * nb + 4 * nb, g, singles,
                                lambda g=g, a=(ptrs(bx[:g]), ptrs(br[:g])): hip.check(lib.clm_f16_mvm_batch(hA.ptr, nb, nb, g, a[0], a[1], None)),
                                reps=10 if nb == 32768 else 4)
        del hA, bx, br
    im, inn, ig, iters = 4096, 8192, 8, 10
    if any(selected(r) for r in F16_BATCH_ROWS[2 * len(F16_GROUPS):]):
        P, PT = hip.alloc(2 * im * inn), hip.alloc(2 * im * inn)
        f16_fill(P, im * inn, 68)
        hip.check(lib.clm_f16_transpose(P.ptr, im, inn, PT.ptr, None))
        V = {k: [hip.alloc(2 * ln) for _ in range(ig)] for k, ln in dict(y=im, x=inn, t1=im, t2=im, t3=inn, r=inn).items()}
        for k in ("y", "x", "t2"):
            for j, b in enumerate(V[k]):
                f16_fill(b, b.nbytes // 2, 500 + 10 * j + len(k))
        for sg in F16_GROUPS:
            def saa_singles(sg=sg):
                for j in range(sg):
                    hip.check(lib.clm_f16_mvm_scale_and_add(PT.ptr, inn, im, V["t2"][j].ptr, V["x"][j].ptr, 2.0 ** -24, V["t3"][j].ptr, V["r"][j].ptr, None))
            rec_pair_alternated(f"f16_mvm_saa_batch{sg}_8192x4096", 2 * im * inn + 2 * im + 6 * inn, sg, saa_singles,
                                lambda sg=sg, a=tuple(ptrs(V[k][:sg]) for k in ("t2", "x", "t3", "r")): hip.check(
                                    lib.clm_f16_mvm_scale_and_add_batch(PT.ptr, inn, im, sg, a[0], a[1], 2.0 ** -24, a[2], a[3], None)), reps=20)

        def iht_singles():
            for j in range(ig):
                hip.check(lib.clm_f16_iht(P.ptr, PT.ptr, im, inn, V["x"][j].ptr, inn, V["y"][j].ptr, V["t1"][j].ptr, V["t2"][j].ptr, V["t3"][j].ptr,
                                          iters, inn // 4, 2.0 ** -24, 1, None))
        A = {k: ptrs(v) for k, v in V.items()}
        rec_pair_alternated("f16_iht_batch8_N8192", 2 * 2 * im * inn, ig, iht_singles,
                            lambda: hip.check(lib.clm_f16_iht_batch(P.ptr, PT.ptr, im, inn, ig, A["x"], inn, A["y"], A["t1"], A["t2"], A["t3"], iters,
                                                                    inn // 4, 2.0 ** -24, 1, None)), reps=2, per=iters)
        if "f16_iht_batch8_N8192" in res:
            res["f16_iht_batch8_N8192"]["note"] = (f"ms per iteration for all 8 signals, calls of {iters} iterations, K = n / 4, FAST threshold; the single "
                                                   "calls are 8 x clm_f16_iht (three launches per iteration and signal)")
        del P, PT, V, A
    if ONLY and all(any(o in r for r in F16_BATCH_ROWS) for o in ONLY.split(",")):
        print(json.dumps(res, indent=1))
        sys.exit(0)


# ---- A' x[j] for several CloverVector16 straight from one CloverMatrix16 (half16_t_batch.hip): every row pairs the batch call, on the
# batched kernel (CLV_MVM_BATCH=1), with two baselines on the same vectors in the same process, rounds alternated: (a) the g single
# transposed calls and (b) the row-major batch call on a held transpose.  f16_mvm_transposed_batch{g}_{32768,65536}: the plain product
# (streaming); f16_mvm_transposed_saa_batch{g}_{8192x4096,65536^2}: the fused x += mu Phi' t2 step, on the IHT shape (Phi 4096 x 8192,
# cache-resident) and streaming; f16_iht_batch_one_matrix_N8192: clm_f16_iht_batch_one_matrix against 8 x clm_f16_iht_one_matrix and
# against clm_f16_iht_batch with a held transpose, ms per iteration for 8 signals.  g = 2, 4, 8, or KB_F16_BATCH_GROUPS.
# KB_ONLY=f16_mvm_transposed_batch,f16_mvm_transposed_saa_batch,f16_iht_batch_one_matrix selects them and the run ends after them.
F16TB_ROWS = tuple(f"f16_mvm_transposed_batch{g}_{nb}" for nb in (32768, 65536) for g in F16_GROUPS) + \
    tuple(f"f16_mvm_transposed_saa_batch{g}_{sz}" for sz in ("8192x4096", "65536^2") for g in F16_GROUPS) + ("f16_iht_batch_one_matrix_N8192",)
if any(selected(r) for r in F16TB_ROWS):
    for nb in (32768, 65536):
        plain = any(selected(f"f16_mvm_transposed_batch{g}_{nb}") for g in F16_GROUPS)
        fused = nb == 65536 and any(selected(f"f16_mvm_transposed_saa_batch{g}_65536^2") for g in F16_GROUPS)
        if not (plain or fused):
            continue
        hA, hAt = hip.alloc(2 * nb * nb), hip.alloc(2 * nb * nb)
        f16_fill(hA, nb * nb, 63)
        hip.check(lib.clm_f16_transpose(hA.ptr, nb, nb, hAt.ptr, None))
        bx, bu, bt, br = ([hip.alloc(2 * nb) for _ in range(8)] for _ in range(4))
        for j in range(8):
            f16_fill(bx[j], nb, 300 + j)
            f16_fill(bu[j], nb, 400 + j)
        for g in F16_GROUPS:
            a = tuple(ptrs(v[:g]) for v in (bx, bu, bt, br))

            def singles(g=g):
                for j in range(g):
                    hip.check(lib.clm_f16_mvm_transposed(hA.ptr, nb, nb, bx[j].ptr, br[j].ptr, None))
            if plain:
                rec_pair_alternated(f"f16_mvm_transposed_batch{g}_{nb}", 2 * nb * nb + 4 * nb, g, singles,
                                    lambda g=g, a=a: hip.check(lib.clm_f16_mvm_transposed_batch(hA.ptr, nb, nb, g, a[0], a[3], None)),
                                    reps=10 if nb == 32768 else 4,
                                    held=lambda g=g, a=a: hip.check(lib.clm_f16_mvm_batch(hAt.ptr, nb, nb, g, a[0], a[3], None)))

            def saa_singles(g=g):
                for j in range(g):
                    hip.check(lib.clm_f16_mvm_transposed_scale_and_add(hA.ptr, nb, nb, bx[j].ptr, bu[j].ptr, 2.0 ** -24, bt[j].ptr, br[j].ptr, None))
            if fused:
                rec_pair_alternated(f"f16_mvm_transposed_saa_batch{g}_65536^2", 2 * nb * nb + 8 * nb, g, saa_singles,
                                    lambda g=g, a=a: hip.check(lib.clm_f16_mvm_transposed_scale_and_add_batch(hA.ptr, nb, nb, g, a[0], a[1], 2.0 ** -24,
                                                                                                              a[2], a[3], None)), reps=4,
                                    held=lambda g=g, a=a: hip.check(lib.clm_f16_mvm_scale_and_add_batch(hAt.ptr, nb, nb, g, a[0], a[1], 2.0 ** -24,
                                                                                                        a[2], a[3], None)))
        del hA, hAt, bx, bu, bt, br
    im, inn, ig, iters = 4096, 8192, 8, 10
    if any(selected(r) for r in F16TB_ROWS if "8192" in r.split("_")[-1]):
        P, PT = hip.alloc(2 * im * inn), hip.alloc(2 * im * inn)
        f16_fill(P, im * inn, 68)
        hip.check(lib.clm_f16_transpose(P.ptr, im, inn, PT.ptr, None))
        V = {k: [hip.alloc(2 * ln) for _ in range(ig)] for k, ln in dict(y=im, x=inn, t1=im, t2=im, t3=inn, r=inn).items()}
        for k in ("y", "x", "t2"):
            for j, b in enumerate(V[k]):
                f16_fill(b, b.nbytes // 2, 500 + 10 * j + len(k))
        for sg in F16_GROUPS:
            a = tuple(ptrs(V[k][:sg]) for k in ("t2", "x", "t3", "r"))

            def step_singles(sg=sg):
                for j in range(sg):
                    hip.check(lib.clm_f16_mvm_transposed_scale_and_add(P.ptr, im, inn, V["t2"][j].ptr, V["x"][j].ptr, 2.0 ** -24, V["t3"][j].ptr,
                                                                       V["r"][j].ptr, None))
            rec_pair_alternated(f"f16_mvm_transposed_saa_batch{sg}_8192x4096", 2 * im * inn + 2 * im + 6 * inn, sg, step_singles,
                                lambda sg=sg, a=a: hip.check(lib.clm_f16_mvm_transposed_scale_and_add_batch(P.ptr, im, inn, sg, a[0], a[1], 2.0 ** -24,
                                                                                                            a[2], a[3], None)), reps=20,
                                held=lambda sg=sg, a=a: hip.check(lib.clm_f16_mvm_scale_and_add_batch(PT.ptr, inn, im, sg, a[0], a[1], 2.0 ** -24,
                                                                                                      a[2], a[3], None)))

        def iht1_singles():
            for j in range(ig):
                hip.check(lib.clm_f16_iht_one_matrix(P.ptr, im, inn, V["x"][j].ptr, inn, V["y"][j].ptr, V["t1"][j].ptr, V["t2"][j].ptr, V["t3"][j].ptr,
                                                     iters, inn // 4, 2.0 ** -24, 1, None))
        A = {k: ptrs(v) for k, v in V.items()}
        rec_pair_alternated("f16_iht_batch_one_matrix_N8192", 2 * 2 * im * inn, ig, iht1_singles,
                            lambda: hip.check(lib.clm_f16_iht_batch_one_matrix(P.ptr, im, inn, ig, A["x"], inn, A["y"], A["t1"], A["t2"], A["t3"], iters,
                                                                               inn // 4, 2.0 ** -24, 1, None)), reps=2, per=iters,
                            held=lambda: hip.check(lib.clm_f16_iht_batch(P.ptr, PT.ptr, im, inn, ig, A["x"], inn, A["y"], A["t1"], A["t2"], A["t3"], iters,
                                                                         inn // 4, 2.0 ** -24, 1, None)))
        if "f16_iht_batch_one_matrix_N8192" in res:
            res["f16_iht_batch_one_matrix_N8192"]["note"] = (f"ms per iteration for all 8 signals, calls of {iters} iterations, K = n / 4, FAST threshold; "
                                                             "the single calls are 8 x clm_f16_iht_one_matrix (three launches per iteration and signal); "
                                                             "held = clm_f16_iht_batch with a stored transpose")
        del P, PT, V, A
    if ONLY and all(any(o in r for r in F16TB_ROWS) for o in ONLY.split(",")):
        print(json.dumps(res, indent=1))
        sys.exit(0)


if not ONLY or any("f16" in o and not o.startswith(F16_FUSED_ROWS) for o in ONLY.split(",")):
    for logn in (24, 30):
        n = 1 << logn
        x = hip.alloc(4 * n)
        hip.check(lib.clv_fill_random_ints_f32(x.ptr, n, 10, 61, 0, None))
        hu, hv, hr, out = hip.alloc(2 * n), hip.alloc(2 * n), hip.alloc(2 * n), hip.alloc(8)
        f16_fill(hv, n, 62)
        rec(f"f16_quantize_n2^{logn}", 6 * n, lambda: hip.check(lib.clv_f16_quantize(x.ptr, n, hu.ptr, None)))
        rec(f"f16_scale_and_add_n2^{logn}", 6 * n, lambda: hip.check(lib.clv_f16_scale_and_add(hu.ptr, hv.ptr, 0.5, n, hr.ptr, None)))
        rec(f"f16_dot_fast_n2^{logn}", 4 * n, lambda: hip.check(lib.clv_f16_dot(hu.ptr, hv.ptr, n, DOT_FAST, out.ptr, None, None)))
        rec(f"f16_dot_exact_n2^{logn}", 4 * n, lambda: hip.check(lib.clv_f16_dot(hu.ptr, hv.ptr, n, DOT_EXACT, out.ptr, None, None)), reps=1,
            extra={"note": "32 sequential fma chains of n / 32 steps: latency-bound by definition"})
        rec(f"f16_threshold_fast_k25pct_n2^{logn}", 4 * n, lambda: hip.check(lib.clv_f16_threshold_mode(hr.ptr, n, n, n // 4, THRESHOLD_FAST, None, None)),
            reps=3, extra={"note": "the large-vector radix select (nine launches, four passes over the values); bytes = the values read and "
                                   "written once; thresholded in place, so calls after the first find the vector already thresholded"})
        rec(f"f16_restore_n2^{logn}", 6 * n, lambda: hip.check(lib.clv_f16_restore(hu.ptr, n, x.ptr, None)))
        del x, hu, hv, hr
    for nf in (8192, 32768, 65536):
        vals = nf * nf
        hA = hip.alloc(2 * vals)
        if nf == 65536:
            A32 = hip.alloc(4 * vals)
            hip.check(lib.clv_fill_random_ints_f32(A32.ptr, vals, 10, 63, 0, None))
            rec(f"f16_matrix_quantize_{nf}^2", 6 * vals, lambda: hip.check(lib.clm_f16_quantize(A32.ptr, nf, nf, hA.ptr, None)), reps=3)
            hip.check(lib.clm_f16_quantize(A32.ptr, nf, nf, hA.ptr, None))
            hip.sync()
            del A32
            hT = hip.alloc(2 * vals)
            rec(f"f16_transpose_{nf}^2", 4 * vals, lambda: hip.check(lib.clm_f16_transpose(hA.ptr, nf, nf, hT.ptr, None)), reps=3)
            del hT
        else:
            f16_fill(hA, vals, 63)
        hx, hr16, xf, rf = hip.alloc(2 * nf), hip.alloc(2 * nf), hip.alloc(4 * nf), hip.alloc(4 * nf)
        f16_fill(hx, nf, 64)
        hip.check(lib.clv_fill_random_ints_f32(xf.ptr, nf, 10, 65, 0, None))
        rec(f"f16_mvm_{nf}^2", 2 * vals + 4 * nf, lambda: hip.check(lib.clm_f16_mvm(hA.ptr, nf, nf, hx.ptr, hr16.ptr, None)))
        rec(f"f16_mvm_f32_{nf}^2", 2 * vals + 8 * nf, lambda: hip.check(lib.clm_f16_mvm_f32(hA.ptr, nf, nf, xf.ptr, rf.ptr, None)))
        del hA, hx, hr16, xf, rf
# ---- the half-precision IHT / GD loop: the fused mvm + scaleAndAdd, the one-workgroup threshold, the loop in one call
if not ONLY or "f16" in ONLY:
    def with_env(name, value, fn):
        """fn with the library switch `name` set (the library reads it per call)"""
        def run():
            os.environ[name] = value
            try:
                fn()
            finally:
                os.environ.pop(name, None)
        return run

    # the mvm of f16_mvm_{n}^2 with the scaleAndAdd behind it in its epilogue: + u read, t and r written
    for nf in (8192, 32768):
        if not selected(f"f16_mvm_scale_and_add_{nf}^2"):
            continue
        vals = nf * nf
        hA, hx, hu, ht, hr16 = hip.alloc(2 * vals), hip.alloc(2 * nf), hip.alloc(2 * nf), hip.alloc(2 * nf), hip.alloc(2 * nf)
        f16_fill(hA, vals, 63)
        f16_fill(hx, nf, 64)
        f16_fill(hu, nf, 66)
        rec(f"f16_mvm_scale_and_add_{nf}^2", 2 * vals + 8 * nf,
            lambda: hip.check(lib.clm_f16_mvm_scale_and_add(hA.ptr, nf, nf, hx.ptr, hu.ptr, -1.0, ht.ptr, hr16.ptr, None)))
        del hA, hx, hu, ht, hr16
    # FAST threshold at n = 8192: the one-workgroup kernel (one launch) and, with CLV_F16_THRESHOLD_SMALL=0, the large-vector radix select
    # (nine launches) that every n took before
    n16 = 8192
    hv = hip.alloc(2 * n16)
    f16_fill(hv, n16, 67)
    thr_note = "bytes = the values read and written once; thresholded in place, so calls after the first find the vector already thresholded"
    rec("f16_threshold_fast_n8192", 4 * n16, lambda: hip.check(lib.clv_f16_threshold_mode(hv.ptr, n16, n16, n16 // 4, THRESHOLD_FAST, None, None)),
        extra={"note": "k_f16_thresh_small, one launch; " + thr_note})
    rec("f16_threshold_fast_n8192_large_path",
        4 * n16, with_env("CLV_F16_THRESHOLD_SMALL", "0", lambda: hip.check(lib.clv_f16_threshold_mode(hv.ptr, n16, n16, n16 // 4, THRESHOLD_FAST, None, None))),
        extra={"note": "CLV_F16_THRESHOLD_SMALL=0: the large-vector radix select, nine launches; " + thr_note})
    del hv
    # one iteration of Q_IHT<CloverMatrix16, CloverVector16> at N = 8192 (Phi m x n with m = N/2, K = N/4, FAST threshold): the method calls
    # one by one with the large-vector threshold -- the 13 launches of the generic template before clm_f16_iht -- and the same loop as one
    # call (three launches per iteration, two for GD).  ms of the loop rows is per iteration: a call of LOOP_ITERS iterations, divided.
    # mu = 2^-24 as in the m8 rows; the kernels' time does not depend on the data
    N16 = 8192
    m16, c16, K16 = N16 // 2, N16, N16 // 4
    if any(selected(r) for r in (f"f16_q_iht_iteration_N{N16}", f"f16_iht_loop_N{N16}", f"f16_gd_loop_N{N16}")):
        P, PT = hip.alloc(2 * m16 * c16), hip.alloc(2 * m16 * c16)
        f16_fill(P, m16 * c16, 68)
        hip.check(lib.clm_f16_transpose(P.ptr, m16, c16, PT.ptr, None))
        vx, vt3, vy, vt1, vt2 = hip.alloc(2 * c16), hip.alloc(2 * c16), hip.alloc(2 * m16), hip.alloc(2 * m16), hip.alloc(2 * m16)
        hip.check(lib.clv_memset(vx.ptr, 0, 2 * c16, None))
        f16_fill(vy, m16, 69)
        MU16 = 2.0 ** -24
        LOOP_ITERS = 10

        def f16_iteration():
            hip.check(lib.clm_f16_mvm(P.ptr, m16, c16, vx.ptr, vt1.ptr, None))
            hip.check(lib.clv_f16_scale_and_add(vy.ptr, vt1.ptr, -1.0, m16, vt2.ptr, None))
            hip.check(lib.clm_f16_mvm(PT.ptr, c16, m16, vt2.ptr, vt3.ptr, None))
            hip.check(lib.clv_f16_scale_and_add(vx.ptr, vt3.ptr, MU16, c16, vx.ptr, None))
            hip.check(lib.clv_f16_threshold_mode(vx.ptr, c16, c16, K16, THRESHOLD_FAST, None, None))

        def f16_loop(thr):
            hip.check(lib.clm_f16_iht(P.ptr, PT.ptr, m16, c16, vx.ptr, c16, vy.ptr, vt1.ptr, vt2.ptr, vt3.ptr, LOOP_ITERS, K16, MU16, thr, None))
        itb16 = 2 * 2 * m16 * c16
        rec(f"f16_q_iht_iteration_N{N16}", itb16, with_env("CLV_F16_THRESHOLD_SMALL", "0", f16_iteration), reps=5,
            extra={"note": "the five method calls one by one, threshold on the large-vector path: 13 launches; bytes = the two matrices only"})
        for row, thr, note in ((f"f16_iht_loop_N{N16}", 1, "FAST threshold (k_f16_thresh_small): three launches per iteration"),
                               (f"f16_gd_loop_N{N16}", 0, "no threshold (Q_GD): two launches per iteration")):
            if not selected(row):
                continue
            rec(row, itb16 * LOOP_ITERS, lambda thr=thr: f16_loop(thr), reps=2,
                extra={"note": f"one clm_f16_iht call of {LOOP_ITERS} iterations, ms per iteration; bytes = the two matrices only; " + note})
            res[row]["ms"] = round(res[row]["ms"] / LOOP_ITERS, 5)
        del P, PT, vx, vt3, vy, vt1, vt2

# ---- CloverVector32 / CloverMatrix32 on the device (fp32.hip): the rows of the f16 blocks above at 4 bytes per element
if not ONLY or "f32" in ONLY:
    def f32_with_env(name, value, fn):
        """fn with the library switch `name` set (the library reads it per call)"""
        def run():
            os.environ[name] = value
            try:
                fn()
            finally:
                os.environ.pop(name, None)
        return run

    for logn in (24, 30):
        if not any(selected(f"f32_{r}_n2^{logn}") for r in ("scale_and_add", "dot_fast", "dot_exact", "threshold_fast_k25pct")):
            continue
        n = 1 << logn
        fu, fv, fr, out = hip.alloc(4 * n), hip.alloc(4 * n), hip.alloc(4 * n), hip.alloc(8)
        hip.check(lib.clv_fill_random_ints_f32(fu.ptr, n, 10, 81, 0, None))
        hip.check(lib.clv_fill_random_ints_f32(fv.ptr, n, 10, 82, 0, None))
        rec(f"f32_scale_and_add_n2^{logn}", 12 * n, lambda: hip.check(lib.clv_f32_scale_and_add(fu.ptr, fv.ptr, 0.5, n, fr.ptr, None)))
        rec(f"f32_dot_fast_n2^{logn}", 8 * n, lambda: hip.check(lib.clv_f32_dot(fu.ptr, fv.ptr, n, DOT_FAST, out.ptr, None, None)))
        rec(f"f32_dot_exact_n2^{logn}", 8 * n, lambda: hip.check(lib.clv_f32_dot(fu.ptr, fv.ptr, n, DOT_EXACT, out.ptr, None, None)), reps=1,
            extra={"note": "32 sequential fma chains of n / 32 steps: latency-bound by definition"})
        rec(f"f32_threshold_fast_k25pct_n2^{logn}", 8 * n, lambda: hip.check(lib.clv_f32_threshold_mode(fr.ptr, n, n, n // 4, THRESHOLD_FAST, None, None)),
            reps=3, extra={"note": "the large-vector radix select (nine launches, four passes over the values); bytes = the values read and "
                                   "written once; thresholded in place, so calls after the first find the vector already thresholded"})
        del fu, fv, fr
    for nf in (8192, 32768, 65536):
        if not any(selected(f"f32_{r}_{nf}^2") for r in ("transpose", "mvm", "mvm_scale_and_add")):
            continue
        vals = nf * nf
        fA = hip.alloc(4 * vals)
        hip.check(lib.clv_fill_random_ints_f32(fA.ptr, vals, 10, 83, 0, None))
        if selected(f"f32_transpose_{nf}^2"):
            fT = hip.alloc(4 * vals)
            rec(f"f32_transpose_{nf}^2", 8 * vals, lambda: hip.check(lib.clm_f32_transpose(fA.ptr, nf, nf, fT.ptr, None)), reps=3)
            del fT
        fx, fu, ft, fr = hip.alloc(4 * nf), hip.alloc(4 * nf), hip.alloc(4 * nf), hip.alloc(4 * nf)
        hip.check(lib.clv_fill_random_ints_f32(fx.ptr, nf, 10, 84, 0, None))
        hip.check(lib.clv_fill_random_ints_f32(fu.ptr, nf, 10, 85, 0, None))
        rec(f"f32_mvm_{nf}^2", 4 * vals + 8 * nf, lambda: hip.check(lib.clm_f32_mvm(fA.ptr, nf, nf, fx.ptr, fr.ptr, None)))
        rec(f"f32_mvm_scale_and_add_{nf}^2", 4 * vals + 16 * nf,
            lambda: hip.check(lib.clm_f32_mvm_scale_and_add(fA.ptr, nf, nf, fx.ptr, fu.ptr, -1.0, ft.ptr, fr.ptr, None)))
        del fA, fx, fu, ft, fr
    # FAST threshold at n = 8192: the one-workgroup kernel (one launch) and, with CLV_F32_THRESHOLD_SMALL=0, the large-vector radix select
    n32 = 8192
    fv = hip.alloc(4 * n32)
    hip.check(lib.clv_fill_random_ints_f32(fv.ptr, n32, 10, 86, 0, None))
    thr_note32 = "bytes = the values read and written once; thresholded in place, so calls after the first find the vector already thresholded"
    rec("f32_threshold_fast_n8192", 8 * n32, lambda: hip.check(lib.clv_f32_threshold_mode(fv.ptr, n32, n32, n32 // 4, THRESHOLD_FAST, None, None)),
        extra={"note": "k_f32_thresh_small, one launch; " + thr_note32})
    rec("f32_threshold_fast_n8192_large_path", 8 * n32,
        f32_with_env("CLV_F32_THRESHOLD_SMALL", "0", lambda: hip.check(lib.clv_f32_threshold_mode(fv.ptr, n32, n32, n32 // 4, THRESHOLD_FAST, None, None))),
        extra={"note": "CLV_F32_THRESHOLD_SMALL=0: the large-vector radix select, nine launches; " + thr_note32})
    del fv
    # one iteration of Q_IHT<CloverMatrix32, CloverVector32> at N = 8192 (Phi m x n with m = N/2, K = N/4, FAST threshold): the five method
    # calls one by one with the threshold on the large-vector path, and the same loop as one clm_f32_iht call (three launches per
    # iteration, two for GD).  ms of the loop rows is per iteration.  mu = 2^-24 as in the other widths' rows
    N32 = 8192
    m32, c32, K32 = N32 // 2, N32, N32 // 4
    if any(selected(r) for r in (f"f32_q_iht_iteration_N{N32}", f"f32_iht_loop_N{N32}", f"f32_gd_loop_N{N32}")):
        P, PT = hip.alloc(4 * m32 * c32), hip.alloc(4 * m32 * c32)
        hip.check(lib.clv_fill_random_ints_f32(P.ptr, m32 * c32, 10, 87, 0, None))
        hip.check(lib.clm_f32_transpose(P.ptr, m32, c32, PT.ptr, None))
        vx, vt3, vy, vt1, vt2 = hip.alloc(4 * c32), hip.alloc(4 * c32), hip.alloc(4 * m32), hip.alloc(4 * m32), hip.alloc(4 * m32)
        hip.check(lib.clv_memset(vx.ptr, 0, 4 * c32, None))
        hip.check(lib.clv_fill_random_ints_f32(vy.ptr, m32, 10, 88, 0, None))
        MU32 = 2.0 ** -24
        LOOP_ITERS32 = 10

        def f32_iteration():
            hip.check(lib.clm_f32_mvm(P.ptr, m32, c32, vx.ptr, vt1.ptr, None))
            hip.check(lib.clv_f32_scale_and_add(vy.ptr, vt1.ptr, -1.0, m32, vt2.ptr, None))
            hip.check(lib.clm_f32_mvm(PT.ptr, c32, m32, vt2.ptr, vt3.ptr, None))
            hip.check(lib.clv_f32_scale_and_add(vx.ptr, vt3.ptr, MU32, c32, vx.ptr, None))
            hip.check(lib.clv_f32_threshold_mode(vx.ptr, c32, c32, K32, THRESHOLD_FAST, None, None))

        def f32_loop(thr):
            hip.check(lib.clm_f32_iht(P.ptr, PT.ptr, m32, c32, vx.ptr, c32, vy.ptr, vt1.ptr, vt2.ptr, vt3.ptr, LOOP_ITERS32, K32, MU32, thr, None))
        itb32 = 2 * 4 * m32 * c32
        rec(f"f32_q_iht_iteration_N{N32}", itb32, f32_with_env("CLV_F32_THRESHOLD_SMALL", "0", f32_iteration), reps=5,
            extra={"note": "the five method calls one by one, threshold on the large-vector path: 13 launches; bytes = the two matrices only"})
        for row, thr, note in ((f"f32_iht_loop_N{N32}", 1, "FAST threshold (k_f32_thresh_small): three launches per iteration"),
                               (f"f32_gd_loop_N{N32}", 0, "no threshold (Q_GD): two launches per iteration")):
            if not selected(row):
                continue
            rec(row, itb32 * LOOP_ITERS32, lambda thr=thr: f32_loop(thr), reps=2,
                extra={"note": f"one clm_f32_iht call of {LOOP_ITERS32} iterations, ms per iteration; bytes = the two matrices only; " + note})
            res[row]["ms"] = round(res[row]["ms"] / LOOP_ITERS32, 5)
        del P, PT, vx, vt3, vy, vt1, vt2
print(json.dumps(res, indent=1))
