"""Variants of the batched fp32-vector kernel (clover_amd/csrc/mvm_f32_batch.hip) timed against the library's own build.

    python tools/mq_f32_batch_variants.py build      # compiles mvm_f32_batch.hip once per variant, links each with the product's objects
    python tools/mq_f32_batch_variants.py            # on the MI355X: one process, the rounds of all builds alternated, median of five

A variant overrides MVFB_R (rows per quad), MVFB_U (matrix loads requested ahead), MVFB_WAVES (waves per SIMD the register allocation
leaves room for) and MVFB_CHUNK (columns of x staged per pass) for EVERY instantiation on the compiler's command line; the libraries go to
tools/_build/mqf32b/.  `build` prints every variant's registers, LDS and whether an instantiation spills; a variant that spills is built
but not timed.  Every build's results are compared with the first build's bit for bit before anything is timed.  Rows: 8 vectors with the
4-bit matrix at 32768^2 and 65536^2 and with the 8-bit matrix at 65536^2, 4 vectors with the 4-bit matrix at 65536^2, the batch forced
(CLV_MVM_BATCH=1); "library 2 x 4" serves the 8 vectors as two calls of 4.  Prints one JSON object: {row: {variant: ms}}, plus per
variant the flags."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from clover_amd.build import EXTRA_FLAGS, HIP_FLAGS, HIP_SOURCES, _hipcc, build_hip_library, hip_library_path  # noqa: E402

OUT = ROOT / "tools" / "_build" / "mqf32b"
SOURCE = "mvm_f32_batch.hip"


def flags(r, u, waves=2, chunk=1024):
    return [f"-DMVFB_R={r}", f"-DMVFB_U={u}", f"-DMVFB_WAVES={waves}", f"-DMVFB_CHUNK={chunk}"]


VARIANTS = {
    "library": [],
    "R=1 U=4": flags(1, 4),
    "R=1 U=2": flags(1, 2),
    "R=2 U=2": flags(2, 2),                       # 4 bit, 8 vectors: spills under the two-wave bound
    "R=2 U=2 one wave": flags(2, 2, waves=1),     # up to 512 registers: one wave per SIMD
    "R=2 U=4 one wave": flags(2, 4, waves=1),
}


def lib_of(name):
    return OUT / ("libclover_hip_" + "".join(c if c.isalnum() else "_" for c in name) + ".so")


def build():
    build_hip_library()
    OUT.mkdir(parents=True, exist_ok=True)
    src_dir, obj_dir = ROOT / "clover_amd" / "csrc", hip_library_path().parent / "obj"
    others = [str(obj_dir / (Path(s).stem + ".o")) for s in HIP_SOURCES if s != SOURCE]
    listing = {}
    for name, fl in VARIANTS.items():
        obj = OUT / (lib_of(name).stem + ".o")
        cmd = [_hipcc(), *HIP_FLAGS, *EXTRA_FLAGS.get(SOURCE, []), *fl, f"-I{ROOT / 'include'}", f"-I{src_dir}", "-c", "-o", str(obj),
               str(src_dir / SOURCE), "-Rpass-analysis=kernel-resource-usage"]
        err = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
        rows, cur = {}, None
        for ln in err.splitlines():
            if "Function Name: _Z18k_mq_mvm_f32_batchILi" in ln:
                b, nv, r, u, nt, fu = (int(t) for t in re.findall(r"L[ib](\d+)E", ln.split("k_mq_mvm_f32_batchI")[1])[:6])
                cur = None if nt or fu else rows.setdefault(f"{b} bit NV={nv}", {})
            elif cur is not None and " VGPRs:" in ln:
                cur["VGPRs"] = int(ln.split("VGPRs:")[1].split()[0])
            elif cur is not None and "ScratchSize" in ln:
                cur["scratch"] = int(ln.split("]:")[1].split()[0])
            elif cur is not None and "Occupancy" in ln:
                cur["waves/SIMD"] = int(ln.split("]:")[1].split()[0])
            elif cur is not None and "LDS Size" in ln:
                cur["LDS"] = int(ln.split("]:")[1].split()[0])
        listing[name] = rows
        print(name, json.dumps(rows))
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(lib_of(name)), *others, str(obj), "-ldl"], check=True)
    (OUT / "listing.json").write_text(json.dumps(listing, indent=1))


def main():
    import numpy as np
    from clover_amd.lib_binding import CloverHip
    os.environ["CLV_MVM_BATCH"] = "1"
    listing = json.loads((OUT / "listing.json").read_text())
    hips = {name: CloverHip(lib_of(name)) for name in VARIANTS}
    base = hips["library"]
    vp = C.c_void_p

    def timed(fn, reps):
        a, b = vp(), vp()
        base.check(base.lib.clv_event_create(C.byref(a)))
        base.check(base.lib.clv_event_create(C.byref(b)))
        base.check(base.lib.clv_event_record(a, None))
        for _ in range(reps):
            fn()
        base.check(base.lib.clv_event_record(b, None))
        base.check(base.lib.clv_event_sync(b))
        ms = C.c_float()
        base.check(base.lib.clv_event_elapsed_ms(a, b, C.byref(ms)))
        base.lib.clv_event_destroy(a)
        base.lib.clv_event_destroy(b)
        return ms.value / reps

    res = {}
    rng = np.random.default_rng(5)
    for bits, nb, g in ((4, 32768, 8), (4, 65536, 8), (4, 65536, 4), (8, 65536, 8)):
        A, sA = base.alloc(nb * nb * bits // 8), base.to_device(rng.uniform(0.5, 2.0, size=(nb // 64) ** 2).astype(np.float32))
        base.check(base.lib.clv_fill_random_nibbles(A.ptr, A.nbytes, 7, 0, None))
        xs, rs = [base.to_device(rng.normal(size=nb).astype(np.float32)) for _ in range(g)], [base.alloc(4 * nb) for _ in range(g)]
        px, pr = base.ptr_array(xs), base.ptr_array(rs)
        fn = f"clm{bits}_mvm_f32_batch"
        key = f"{bits} bit NV={8 if g > 4 else 4}"
        calls = {v: (lambda h=h: h.check(getattr(h.lib, fn)(A.ptr, sA.ptr, nb, nb, g, px, pr, None))) for v, h in hips.items()
                 if not listing[v][key]["scratch"]}
        single = getattr(base.lib, f"clm{bits}_mvm_f32")
        calls[f"{g} single calls"] = lambda: [base.check(single(A.ptr, sA.ptr, nb, nb, xs[j].ptr, rs[j].ptr, None)) for j in range(g)]
        if g == 8:
            halves = [(base.ptr_array(xs[i:i + 4]), base.ptr_array(rs[i:i + 4])) for i in (0, 4)]
            calls["library 2 x 4"] = lambda: [base.check(getattr(base.lib, fn)(A.ptr, sA.ptr, nb, nb, 4, a, b, None)) for a, b in halves]
        want = None
        for vname, call in calls.items():          # the same bits from every build first (also the warm-up)
            for r in rs:
                base.check(base.lib.clv_memset(r.ptr, 0, r.nbytes, None))
            call()
            base.sync()
            got = np.concatenate([r.download(np.uint32, nb) for r in rs])
            want = got if want is None else want
            assert np.array_equal(got, want), (bits, nb, vname, "differs from the library's bits")
        times = {v: [] for v in calls}
        for _ in range(5):
            for vname, call in calls.items():
                times[vname].append(timed(call, 10 if nb <= 32768 else 4))
        name = f"m{bits}_mvm_f32_batch{g}_{nb}^2"
        res[name] = {v: round(sorted(ts)[2], 5) for v, ts in times.items()}
        res[name]["spread"] = {v: round(max(ts) - min(ts), 5) for v, ts in times.items()}
        res[name]["not timed (scratch)"] = [v for v in hips if v not in calls]
        del A, sA, xs, rs, calls
    res["variants"] = {k: " ".join(v) or "the library's constants" for k, v in VARIANTS.items()}
    res["resources (plain, not nontemporal)"] = listing
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    build() if sys.argv[1:] == ["build"] else main()
