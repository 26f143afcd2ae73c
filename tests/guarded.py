"""An arena with guard bands: what a call may write is what its contract names, byte for byte.

Every buffer of the other tests is its own allocation, whose granularity swallows an overrun, and every workspace is the library's own
grow-only scratch.  Here ONE clv_malloc holds all operands of a call.  The host keeps an image of it, filled with random bytes (a constant
or strided pattern would let a stray store of the same value go unseen); regions are carved at 256-byte boundaries, at least GUARD bytes
apart, with END_GUARD bytes at either end of the arena.  A region's declared range is the exact byte count of the contract -- for clm4_mvm
with rows = 64, r is 32 bytes and sr is 4 -- and the bytes up to the next boundary belong to the guard.

    kind      what check() requires
    input     back unchanged
    output    prefilled with the random bytes; the whole declared range equals the reference (so every byte was written)
    inout     holds data before the call (a threshold's vector); the reference carries whatever must stay
    scratch   a caller workspace (optionally prefilled with one byte value); content after the call is free
    state     the 256-byte rng buffer: seeded with clv_rng_seed after the upload, compared through clv_rng_get; raw bytes are free

Sequence: add regions, upload(), the ABI call on arena.ptr(name) pointers, clv_stream_sync, check(expected).  check() downloads the whole
arena: everything outside the output / inout / scratch / state ranges must equal the image, and a failure names the nearest region, the
offset relative to its start and the number of changed bytes.  Out-of-bounds READS cannot be seen this way."""
import ctypes as C

import numpy as np

ALIGN = 256
GUARD = 4096
END_GUARD = 64 << 10
MAX_ARENA = 64 << 20
KINDS = ("input", "output", "inout", "scratch", "state")
RNG_STATE_BYTES = 256


class GuardError(AssertionError):
    pass


class Region:
    def __init__(self, name, kind, nbytes, data, fill, shift):
        self.name, self.kind, self.nbytes, self.data, self.fill, self.shift = name, kind, int(nbytes), data, fill, int(shift)
        self.offset = None

    @property
    def end(self):
        return self.offset + self.nbytes


def _bytes_of(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


class Arena:
    def __init__(self, hip, seed=0):
        self.hip, self.L = hip, hip.lib
        self.seed = seed
        self.regions = {}
        self.base = 0
        self.image = None
        self.size = 0

    # ---- carving
    def add(self, name, kind, data=None, nbytes=None, fill=None, shift=0):
        """data: the region's content (input, inout) -- its byte count is the declared range; nbytes: the declared range of an output or
        a scratch region (0 is allowed: a pointer with nothing behind it but guard); fill: a byte value for a scratch region; shift: the
        region starts that many bytes behind a 256-byte boundary (a shard of a larger result)."""
        assert kind in KINDS and name not in self.regions and self.image is None
        if kind == "state":
            nbytes = RNG_STATE_BYTES
        if data is not None:
            assert kind in ("input", "inout")
            data = _bytes_of(data).copy()
            nbytes = data.size
        assert nbytes is not None and (data is not None or kind in ("output", "scratch", "state"))
        self.regions[name] = Region(name, kind, nbytes, data, fill, shift)
        return self

    def upload(self):
        off = END_GUARD
        for r in self.regions.values():
            r.offset = off + r.shift
            off = (r.end + GUARD + ALIGN - 1) // ALIGN * ALIGN
        self.size = off - GUARD + END_GUARD if self.regions else 2 * END_GUARD
        self.size = (self.size + ALIGN - 1) // ALIGN * ALIGN
        assert self.size <= MAX_ARENA, f"arena of {self.size} bytes: keep a case under 64 MiB"
        self.image = np.frombuffer(np.random.default_rng(self.seed).bytes(self.size), np.uint8).copy()
        for r in self.regions.values():
            if r.data is not None:
                self.image[r.offset:r.end] = r.data
            elif r.fill is not None:
                self.image[r.offset:r.end] = r.fill
        p = C.c_void_p()
        self.hip.check(self.L.clv_malloc(C.byref(p), self.size))
        self.base = p.value
        assert self.base % ALIGN == 0
        self.hip.check(self.L.clv_memcpy_h2d(self.base, self.image.ctypes.data, self.size, None))
        self.hip.check(self.L.clv_stream_sync(None))
        return self

    def seed_state(self, name, key1, key2):
        assert self.regions[name].kind == "state"
        self.hip.check(self.L.clv_rng_seed(self.ptr(name), key1, key2, None))
        self.hip.check(self.L.clv_stream_sync(None))

    def ptr(self, name):
        return self.base + self.regions[name].offset

    def close(self):
        if self.base:
            self.hip.check(self.L.clv_free(self.base))
            self.base = 0

    def __del__(self):
        if self.base:                                  # not closed by its user: free it, and let a failing free be reported
            self.close()

    # ---- checking
    def download(self):
        got = np.empty(self.size, np.uint8)
        self.hip.check(self.L.clv_memcpy_d2h(got.ctypes.data, self.base, self.size, None))
        self.hip.check(self.L.clv_stream_sync(None))
        return got

    def _nearest(self, offsets):
        """index of the nearest region (distance to its declared range) per arena offset"""
        regs = list(self.regions.values())
        dist = np.stack([np.maximum(np.maximum(r.offset - offsets, offsets - (r.end - 1)), 0) for r in regs])
        return regs, np.argmin(dist, axis=0)

    def check(self, expected=None, states=None, got=None):
        """expected: name -> array for every output and inout region; states: name -> (key1[4], key2[4]) for every state region.
        Returns name -> the bytes found in the output, inout and scratch regions."""
        expected, states = dict(expected or {}), dict(states or {})
        got = self.download() if got is None else got
        free = np.zeros(self.size, bool)
        for r in self.regions.values():
            if r.kind != "input":
                free[r.offset:r.end] = True
        changed = np.flatnonzero((got != self.image) & ~free)
        if changed.size:
            regs, near = self._nearest(changed)
            lines = []
            for i in np.unique(near):
                offs = changed[near == i]
                r = regs[i]
                where = "inside" if r.offset <= offs[0] < r.end else ("before" if offs[0] < r.offset else "behind")
                lines.append(f"{offs.size} byte(s) changed near `{r.name}` ({r.kind}, {r.nbytes} bytes): first at offset {int(offs[0]) - r.offset:+d} "
                             f"from its start ({where} its declared range), last at {int(offs[-1]) - r.offset:+d}")
            raise GuardError("the call wrote outside what its contract names:\n  " + "\n  ".join(lines))
        out = {}
        for r in self.regions.values():
            if r.kind in ("output", "inout"):
                assert r.name in expected, f"no reference given for `{r.name}`"
                want = _bytes_of(expected.pop(r.name))
                assert want.size == r.nbytes, f"`{r.name}`: the reference has {want.size} bytes, the declared range {r.nbytes}"
                have = got[r.offset:r.end]
                bad = np.flatnonzero(have != want)
                if bad.size:
                    unwritten = int((have[bad] == self.image[r.offset:r.end][bad]).sum()) if r.kind == "output" else 0
                    raise GuardError(f"`{r.name}` ({r.kind}, {r.nbytes} bytes): {bad.size} byte(s) differ from the reference, first at offset "
                                     f"{int(bad[0])} ({unwritten} of them still hold the prefill)")
            if r.kind == "state":
                assert r.name in states, f"no reference keys given for `{r.name}`"
                k1, k2 = (C.c_uint64 * 4)(), (C.c_uint64 * 4)()
                self.hip.check(self.L.clv_rng_get(self.ptr(r.name), k1, k2, None))
                w1, w2 = states.pop(r.name)
                if list(k1) != [int(v) for v in w1] or list(k2) != [int(v) for v in w2]:
                    raise GuardError(f"`{r.name}`: the rng state the call left differs from the reference's keys")
            if r.kind != "input":
                out[r.name] = got[r.offset:r.end].copy()
        assert not expected and not states, f"references for unknown regions: {list(expected) + list(states)}"
        return out
