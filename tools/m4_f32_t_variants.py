"""Lane maps of the transposed CloverMatrix4 x fp32-vector kernel (clover_amd/csrc/mvm_f32_t.hip) timed against the library's own build.

    python tools/m4_f32_t_variants.py build      # compiles mvm_f32_t.hip once per variant, links each with the product's objects
    python tools/m4_f32_t_variants.py            # on the MI355X: one process, the rounds of all builds alternated, median of five

A variant overrides M4FT_COLS (columns per workgroup), M4FT_WORDS (dwords per lane and row) and M4FT_U (32-row blocks of loads per
register set) on the compiler's command line; the libraries go to tools/_build/m4f32t/.  `build` prints every variant's registers, LDS
and whether an instantiation spills.  Every build's results are compared with the first build's bit for bit before anything is timed.
Rows: clm4_mvm_f32_transposed at 8192^2 (cache-resident), 32768^2 and 65536^2 (streaming), beside clm4_mvm_f32 on a held transpose in the
same rounds, and the fused step on Phi 4096 x 8192.  Prints one JSON object: {row: {variant: ms}}, plus per variant the flags."""
import ctypes as C
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from clover_amd.build import HIP_FLAGS, HIP_SOURCES, _hipcc, build_hip_library, hip_library_path  # noqa: E402

OUT = ROOT / "tools" / "_build" / "m4f32t"
SOURCE = "mvm_f32_t.hip"


def flags(cols, words, u):
    return [f"-DM4FT_COLS={cols}", f"-DM4FT_WORDS={words}", f"-DM4FT_U={u}"]


VARIANTS = {
    "library": [],
    "256x4 U=4": flags(256, 4, 4),        # a lane holds 32 columns: 16-byte loads, 256 threads
    "256x4 U=2": flags(256, 4, 2),
    "128x4 U=4": flags(128, 4, 4),        # 128 threads
    "256x2 U=4": flags(256, 2, 4),        # 16 columns per lane, 512 threads
    "128x2 U=8": flags(128, 2, 8),        # 256 threads
    "256x1 U=8": flags(256, 1, 8),        # 8 columns per lane, 1024 threads
    "128x1 U=8": flags(128, 1, 8),        # 512 threads
    "128x1 U=16": flags(128, 1, 16),
    "128x1 U=4": flags(128, 1, 4),
    "64x1 U=8": flags(64, 1, 8),          # 256 threads, 32 B of every row
}


def lib_of(name):
    return OUT / ("libclover_hip_" + "".join(c if c.isalnum() else "_" for c in name) + ".so")


def build():
    build_hip_library()
    OUT.mkdir(parents=True, exist_ok=True)
    src_dir, obj_dir = ROOT / "clover_amd" / "csrc", hip_library_path().parent / "obj"
    others = [str(obj_dir / (Path(s).stem + ".o")) for s in HIP_SOURCES if s != SOURCE]
    for name, fl in VARIANTS.items():
        obj = OUT / (lib_of(name).stem + ".o")
        cmd = [_hipcc(), *HIP_FLAGS, *fl, f"-I{ROOT / 'include'}", f"-I{src_dir}", "-c", "-o", str(obj), str(src_dir / SOURCE),
               "-Rpass-analysis=kernel-resource-usage"]
        err = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
        spill = [ln for ln in err.splitlines() if "ScratchSize" in ln and not ln.rstrip().endswith(": 0 [-Rpass-analysis=kernel-resource-usage]")]
        regs = sorted({int(ln.split("VGPRs:")[1].split()[0]) for ln in err.splitlines() if " VGPRs:" in ln})
        lds = sorted({int(ln.split("LDS Size [bytes/block]:")[1].split()[0]) for ln in err.splitlines() if "LDS Size" in ln})
        print(f"{name}: VGPRs {regs}, LDS {lds}, {'SCRATCH in ' + str(len(spill)) + ' instantiations' if spill else 'no scratch'}")
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(lib_of(name)), *others, str(obj), "-ldl"], check=True)


def main(sizes):
    import numpy as np
    from clover_amd.lib_binding import CloverHip
    hips = {name: CloverHip(lib_of(name)) for name in VARIANTS}
    base = hips["library"]
    vp = C.c_void_p

    def timed(h, fn, reps):
        a, b = vp(), vp()
        h.check(h.lib.clv_event_create(C.byref(a)))
        h.check(h.lib.clv_event_create(C.byref(b)))
        h.check(h.lib.clv_event_record(a, None))
        for _ in range(reps):
            fn()
        h.check(h.lib.clv_event_record(b, None))
        h.check(h.lib.clv_event_sync(b))
        ms = C.c_float()
        h.check(h.lib.clv_event_elapsed_ms(a, b, C.byref(ms)))
        h.lib.clv_event_destroy(a)
        h.lib.clv_event_destroy(b)
        return ms.value / reps

    res = {}
    rng = np.random.default_rng(5)

    def nibbles(nbytes):
        """device bytes whose nibbles lie in [-7, 7]: 32 MiB of them, copied until the matrix is full"""
        q = np.frombuffer(rng.bytes(min(nbytes, 1 << 25)), np.uint8).copy()
        q[(q >> 4) == 8] ^= 0x80
        q[(q & 0xF) == 8] ^= 0x08
        src, d = base.to_device(q), base.alloc(nbytes)
        for off in range(0, nbytes, src.nbytes):
            base.check(base.lib.clv_memcpy_d2d(d.ptr + off, src.ptr, min(src.nbytes, nbytes - off), None))
        base.sync()
        return d

    def fvec(n):
        return base.to_device(rng.normal(size=n).astype(np.float32))

    def row(name, calls, reps, out, n):
        """calls: variant -> enqueue; the same bits from every build first (also the warm-up), then five alternated rounds"""
        want = None
        for vname, call in calls.items():
            base.check(base.lib.clv_memset(out.ptr, 0, 4 * n, None))
            call()
            base.sync()
            got = out.download(np.uint32, n)
            want = got if want is None else want
            assert np.array_equal(got, want), (name, vname, "differs from the library's bits")
        times = {v: [] for v in calls}
        for _ in range(5):
            for vname, call in calls.items():
                times[vname].append(timed(base, call, reps))
        res[name] = {v: round(sorted(ts)[2], 5) for v, ts in times.items()}
        res[name]["spread"] = {v: round(max(ts) - min(ts), 5) for v, ts in times.items() if v in ("library", "held transpose")}

    for nb in sizes:
        A, sA = nibbles(nb * nb // 2), base.to_device(rng.uniform(0.5, 2.0, size=(nb // 64) ** 2).astype(np.float32))
        x, r = fvec(nb), base.alloc(4 * nb)
        calls = {v: (lambda h=h: h.check(h.lib.clm4_mvm_f32_transposed(A.ptr, sA.ptr, nb, nb, x.ptr, r.ptr, None))) for v, h in hips.items()}
        if nb <= 32768:                          # the held transpose: the same bits by contract, so it joins the comparison
            At, sAt = base.alloc(nb * nb // 2), base.alloc(4 * (nb // 64) ** 2)
            base.check(base.lib.clm4_transpose(A.ptr, sA.ptr, nb, nb, At.ptr, sAt.ptr, None))
            calls["held transpose"] = lambda: base.check(base.lib.clm4_mvm_f32(At.ptr, sAt.ptr, nb, nb, x.ptr, r.ptr, None))
        row(f"mvm_f32_transposed_{nb}^2", calls, 50 if nb <= 8192 else 10 if nb <= 32768 else 4, r, nb)
        del A, sA, x, r, calls
    m, n = 4096, 8192
    A, sA = nibbles(m * n // 2), base.to_device(rng.uniform(0.5, 2.0, size=(m // 64) * (n // 64)).astype(np.float32))
    x, u, t, r = fvec(m), fvec(n), base.alloc(4 * n), base.alloc(4 * n)
    row("mvm_f32_transposed_saa_8192x4096",
        {v: (lambda h=h: h.check(h.lib.clm4_mvm_f32_transposed_scale_and_add(A.ptr, sA.ptr, m, n, x.ptr, u.ptr, 0.37, t.ptr, r.ptr, None)))
         for v, h in hips.items()}, 50, r, n)
    res["variants"] = {k: " ".join(v) or "the library's constants" for k, v in VARIANTS.items()}
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    if sys.argv[1:] == ["build"]:
        build()
    else:
        main([int(a) for a in sys.argv[1:]] or [8192, 32768, 65536])
