"""Variants of the batched transposed half-precision kernel (clover_amd/csrc/half16_t_batch.hip) timed against the library's own build.

    python tools/f16_tb_variants.py build      # compiles half16_t_batch.hip once per variant, links each with the product's objects
    python tools/f16_tb_variants.py            # on the MI355X: one process, the rounds of all builds alternated, median of five

A variant overrides F16TB_COLS(NV) or F16TB_U(NV) on the compiler's command line; the libraries go to tools/_build/f16tb/.  `build` prints
every variant's registers and whether an instantiation spills: U = 8 beyond NV = 2, a chunk of 2048 rows and 256 columns with U = 4 did
(under the two waves per SIMD the kernel asks for) and are not in the list.
Every build's results are compared with the first build's bit for bit before anything is timed.  Rows: the plain product at 32768^2 and
65536^2 (streaming) and the fused step on Phi 4096 x 8192 (cache-resident), for 2, 4 and 8 vectors, CLV_MVM_BATCH=1.  Prints one JSON
object: {row: {variant: ms}}, plus per variant the flags."""
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from clover_amd.build import HIP_FLAGS, HIP_SOURCES, _hipcc, build_hip_library, hip_library_path  # noqa: E402

OUT = ROOT / "tools" / "_build" / "f16tb"
VARIANTS = {
    "library": [],
    "U=2": ["-DF16TB_U(NV)=2"],
    "U=8 at NV=2": ["-DF16TB_U(NV)=((NV) == 2 ? 8 : 4)"],
    "64 columns for every NV": ["-DF16TB_COLS(NV)=64"],
    "256 columns at NV=2, U=2": ["-DF16TB_COLS(NV)=((NV) == 2 ? 256 : (NV) == 8 ? 64 : 128)", "-DF16TB_U(NV)=((NV) == 2 ? 2 : 4)"],
}


def lib_of(name):
    return OUT / ("libclover_hip_" + "".join(c if c.isalnum() else "_" for c in name) + ".so")


def build():
    build_hip_library()
    OUT.mkdir(parents=True, exist_ok=True)
    src_dir, obj_dir = ROOT / "clover_amd" / "csrc", hip_library_path().parent / "obj"
    others = [str(obj_dir / (Path(s).stem + ".o")) for s in HIP_SOURCES if s != "half16_t_batch.hip"]
    for name, flags in VARIANTS.items():
        obj = OUT / (lib_of(name).stem + ".o")
        cmd = [_hipcc(), *HIP_FLAGS, *flags, f"-I{ROOT / 'include'}", f"-I{src_dir}", "-c", "-o", str(obj), str(src_dir / "half16_t_batch.hip"),
               "-Rpass-analysis=kernel-resource-usage"]
        err = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
        spill = [ln for ln in err.splitlines() if "ScratchSize" in ln and not ln.rstrip().endswith(": 0 [-Rpass-analysis=kernel-resource-usage]")]
        regs = sorted({int(ln.split("VGPRs:")[1].split()[0]) for ln in err.splitlines() if " VGPRs:" in ln})
        print(f"{name}: VGPRs {regs}, {'SCRATCH in ' + str(len(spill)) + ' instantiations' if spill else 'no scratch'}")
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(lib_of(name)), *others, str(obj), "-ldl"], check=True)


def main():
    import numpy as np
    from clover_amd.lib_binding import CloverHip
    os.environ["CLV_MVM_BATCH"] = "1"
    hips = {name: CloverHip(lib_of(name)) for name in VARIANTS}
    base = hips["library"]
    vp = C.c_void_p

    def ptrs(bufs):
        return (vp * len(bufs))(*[b.ptr for b in bufs])

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

    def row(name, rows, cols, g, fused, reps, A, x, u, t, r):
        def call(h):
            if fused:
                h.check(h.lib.clm_f16_mvm_transposed_scale_and_add_batch(A.ptr, rows, cols, g, ptrs(x[:g]), ptrs(u[:g]), 2.0 ** -24, ptrs(t[:g]),
                                                                         ptrs(r[:g]), None))
            else:
                h.check(h.lib.clm_f16_mvm_transposed_batch(A.ptr, rows, cols, g, ptrs(x[:g]), ptrs(r[:g]), None))
        want = None
        for vname, h in hips.items():            # the same bits from every build, and a warm-up
            call(h)
            h.sync()
            got = np.concatenate([b.download(np.uint16, cols) for b in r[:g]])
            want = got if want is None else want
            assert np.array_equal(got, want), (name, vname, "differs from the library's bits")
        times = {v: [] for v in hips}
        for _ in range(5):
            for vname, h in hips.items():
                times[vname].append(timed(h, lambda h=h: call(h), reps))
        res[name] = {v: round(sorted(ts)[2], 5) for v, ts in times.items()}
        res[name]["spread of the library's rounds"] = round(max(times["library"]) - min(times["library"]), 5)

    rng = np.random.default_rng(5)

    def vec(n):
        return base.to_device(rng.integers(0x2C00, 0x3C00, size=n, dtype=np.uint16) | (rng.integers(0, 2, size=n, dtype=np.uint16) << 15))
    for nb in (32768, 65536):
        A = base.alloc(2 * nb * nb)
        src = vec(1 << 24)                       # 32 MiB of finite patterns, copied until the matrix is full
        for off in range(0, 2 * nb * nb, src.nbytes):
            base.check(base.lib.clv_memcpy_d2d(A.ptr + off, src.ptr, min(src.nbytes, 2 * nb * nb - off), None))
        x, r = [vec(nb) for _ in range(8)], [base.alloc(2 * nb) for _ in range(8)]
        for g in (2, 4, 8):
            row(f"f16_mvm_transposed_batch{g}_{nb}", nb, nb, g, False, 10 if nb == 32768 else 4, A, x, None, None, r)
        del A, x, r
    m, n = 4096, 8192
    A = vec(m * n)
    x, u, t, r = [vec(m) for _ in range(8)], [vec(n) for _ in range(8)], [base.alloc(2 * n) for _ in range(8)], [base.alloc(2 * n) for _ in range(8)]
    for g in (2, 4, 8):
        row(f"f16_mvm_transposed_saa_batch{g}_8192x4096", m, n, g, True, 20, A, x, u, t, r)
    res["variants"] = {k: " ".join(v) or "the library's constants" for k, v in VARIANTS.items()}
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    build() if sys.argv[1:] == ["build"] else main()
