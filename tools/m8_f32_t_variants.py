"""Variants of the transposed CloverMatrix8 x fp32-vector kernel (clover_amd/csrc/matrix8_f32_t.hip) timed against the library's own build.

    python tools/m8_f32_t_variants.py build      # compiles matrix8_f32_t.hip once per variant, links each with the product's objects
    python tools/m8_f32_t_variants.py            # on the MI355X: one process, the rounds of all builds alternated, median of five

A variant overrides M8FT_COLS (columns per workgroup), M8FT_U (32-row blocks of loads per register set) and M8FT_CVT (how a byte becomes a
float) on the compiler's command line; the libraries go to tools/_build/m8f32t/.  `build` prints every variant's registers, LDS and
whether an instantiation spills.  Every build's results are compared with the first build's bit for bit before anything is timed (the
bytes cover the whole range, -128 included).  Rows: clm8_mvm_f32_transposed at 8192^2 (cache-resident), 32768^2 and 65536^2 (streaming),
beside clm8_mvm_f32 on a held transpose in the same rounds (up to 32768^2), and the fused step on Phi 4096 x 8192.  Prints one JSON object:
{row: {variant: ms}}, plus per variant the flags."""
import ctypes as C
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from clover_amd.build import HIP_FLAGS, HIP_SOURCES, _hipcc, build_hip_library, hip_library_path  # noqa: E402

OUT = ROOT / "tools" / "_build" / "m8f32t"
SOURCE = "matrix8_f32_t.hip"


def flags(cols, u, cvt=0):
    return [f"-DM8FT_COLS={cols}", f"-DM8FT_U={u}", f"-DM8FT_CVT={cvt}"]


VARIANTS = {
    "library": [],
    "128 U=4": flags(128, 4),
    "128 U=16": flags(128, 16),
    "128 U=8 ubyte": flags(128, 8, 1),    # v_cvt_f32_ubyteN of q ^ 0x80, minus 128: two VALU per byte beside the fma
    "64 U=8": flags(64, 8),               # 128 threads, half a 128-byte line of every row per workgroup
    "64 U=16": flags(64, 16),
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

    def matrix_bytes(nbytes):
        """device bytes over the whole int8 range: 32 MiB of them, copied until the matrix is full"""
        src, d = base.to_device(np.frombuffer(rng.bytes(min(nbytes, 1 << 25)), np.uint8).copy()), base.alloc(nbytes)
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
        A, sA = matrix_bytes(nb * nb), base.to_device(rng.uniform(0.5, 2.0, size=(nb // 64) ** 2).astype(np.float32))
        x, r = fvec(nb), base.alloc(4 * nb)
        calls = {v: (lambda h=h: h.check(h.lib.clm8_mvm_f32_transposed(A.ptr, sA.ptr, nb, nb, x.ptr, r.ptr, None))) for v, h in hips.items()}
        if nb <= 32768:                          # the held transpose: the same bits by contract, so it joins the comparison
            At, sAt = base.alloc(nb * nb), base.alloc(4 * (nb // 64) ** 2)
            base.check(base.lib.clm8_transpose(A.ptr, sA.ptr, nb, nb, At.ptr, sAt.ptr, None))
            calls["held transpose"] = lambda: base.check(base.lib.clm8_mvm_f32(At.ptr, sAt.ptr, nb, nb, x.ptr, r.ptr, None))
        row(f"m8_mvm_f32_transposed_{nb}^2", calls, 50 if nb <= 8192 else 10 if nb <= 32768 else 4, r, nb)
        del A, sA, x, r, calls
    m, n = 4096, 8192
    A, sA = matrix_bytes(m * n), base.to_device(rng.uniform(0.5, 2.0, size=(m // 64) * (n // 64)).astype(np.float32))
    x, u, t, r = fvec(m), fvec(n), base.alloc(4 * n), base.alloc(4 * n)
    row("m8_mvm_f32_transposed_saa_8192x4096",
        {v: (lambda h=h: h.check(h.lib.clm8_mvm_f32_transposed_scale_and_add(A.ptr, sA.ptr, m, n, x.ptr, u.ptr, 0.37, t.ptr, r.ptr, None)))
         for v, h in hips.items()}, 50, r, n)
    res["variants"] = {k: " ".join(v) or "the library's constants" for k, v in VARIANTS.items()}
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    if sys.argv[1:] == ["build"]:
        build()
    else:
        main([int(a) for a in sys.argv[1:]] or [8192, 32768, 65536])
