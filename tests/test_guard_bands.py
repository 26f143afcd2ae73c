"""Every entry point of the C ABI that writes device memory, called on the raw pointers of a guarded arena (tests/guarded.py): the outputs
equal the references the suite already trusts bit for bit over their WHOLE declared range, the inputs come back unchanged, and not one
byte outside the ranges the contract names is touched -- at the ragged edges of the contracts (64-row shards, results at a shard's
offset, n < n_pad, the 256-byte rng state, t == NULL) and once per kernel form the host-side dispatchers can choose, at the smallest size
that selects it.  Every call here passes workspace = NULL; tests/test_caller_workspace.py is the same harness with caller workspaces.

A case is name -> builder(refs) -> Case(regions, call, expect): the regions of the arena, the ABI call on their pointers, the reference
bytes of every output.  The references are computed on the CPU (the oracle, matrix8_restate.c, half16_restate.c, the lowest-index rule of
test_threshold_large3.py) with three exceptions named where they occur: the FAST dots (their summation order is the library's own:
the same call into plain buffers), the clv_fill_random_* generators (no restatement exists) and the heap array of the 4- and 8-bit heap
forms (the restated walk of half16_restate.c on an order-preserving relabelling of the magnitudes)."""
import os

import numpy as np
import pytest

from clover_amd.lib_binding import DOT_EXACT, DOT_FAST, SIGNATURES, THRESHOLD_FAST, THRESHOLD_REFERENCE
from conftest import random_packed
from guarded import Arena, GuardError
from half16_helpers import random_f16_bits, rh  # noqa: F401
from matrix8_helpers import full_range_bytes, m8  # noqa: F401
from test_threshold_large3 import lowest_index_rule
from test_threshold_large3 import make as make_v4

HEAP = 2                    # the third threshold form of the tables below: the heap entry points (REFERENCE order + heap_dev)
KEYS = (20240, 7)           # clv_rng_seed keys of the stochastic cases


class Refs:
    def __init__(self, oracle, m8, rh):
        self.oracle, self.m8, self.rh = oracle, m8, rh


@pytest.fixture(scope="module")
def refs(oracle, m8, rh):  # noqa: F811
    return Refs(oracle, m8, rh)


class Case:
    """regions: (name, kind, payload[, shift]) -- payload is the content of an input / inout region, the byte count of an output /
    scratch region, None for a state; call(L, p): the ABI call(s) on the pointers p[name], returning the status; expect: name -> reference
    array, or a function of hip that returns it (references that need the device); orng: the oracle's generator the reference consumed,
    whose keys the state region must hold afterwards; env: environment switches during the call; segments: clv_rng_set_segments;
    untouched: scratch regions the call must leave as they were.  The byte count of a scratch region may be a function of the library
    (a *_workspace_bytes query: some of them ask the device)."""

    def __init__(self, regions, call, expect, orng=None, env=None, segments=0, untouched=()):
        self.regions, self.call, self.expect, self.orng, self.env, self.segments = regions, call, expect, orng, env or {}, segments
        self.untouched = untouched


def run_case(hip, case, seed=1, scratch_fill=None):
    """the case on a fresh arena; scratch_fill: the byte value every scratch region holds before the call (None: the random bytes)"""
    from oracle.binding import Oracle
    A = Arena(hip, seed=seed)
    for name, kind, payload, *shift in case.regions:
        if kind in ("input", "inout"):
            A.add(name, kind, data=payload, shift=shift[0] if shift else 0)
        elif kind == "state":
            A.add(name, kind)
        else:
            nbytes = payload(hip.lib) if callable(payload) else payload
            A.add(name, kind, nbytes=nbytes, fill=scratch_fill if kind == "scratch" else None, shift=shift[0] if shift else 0)
    A.upload()
    try:
        states = {}
        for name, r in A.regions.items():
            if r.kind == "state":
                A.seed_state(name, *KEYS)
                states[name] = Oracle.rng_keys(case.orng)
        saved = {k: os.environ.get(k) for k in case.env}
        os.environ.update(case.env)
        try:
            if case.segments:
                hip.check(hip.lib.clv_rng_set_segments(case.segments))
            hip.check(case.call(hip.lib, {n: A.ptr(n) for n in A.regions}))
            hip.check(hip.lib.clv_stream_sync(None))
        finally:
            hip.lib.clv_rng_set_segments(0)
            for k, v in saved.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        out = A.check(case.expect(hip) if callable(case.expect) else case.expect, states)
        for name in case.untouched:
            r = A.regions[name]
            assert np.array_equal(out[name], A.image[r.offset:r.end]), f"`{name}` was written by a call that has no use for it"
    finally:
        A.close()                                                           # a failing clv_free (after a device fault) is an error of its own
    return out


def first_error(*rcs):
    return next((rc for rc in rcs if rc), 0)


# ---------------------------------------------------------------- data
def f32vec(seed, n):
    return (np.random.default_rng(seed).normal(size=n) * 3).astype(np.float32)


def v4(seed, n):
    return random_packed(np.random.default_rng(seed), n)


def v8(seed, n):
    rng = np.random.default_rng(seed)
    return full_range_bytes(rng, n), rng.uniform(0.5, 2.0, size=n // 64).astype(np.float32)


def v16(seed, n):
    return random_f16_bits(np.random.default_rng(seed), n, -4, 4, 0.05)


def m4(seed, rows, cols):
    rng = np.random.default_rng(seed)
    return random_packed(rng, rows * cols)[0], rng.uniform(0.5, 2.0, size=(rows // 64) * (cols // 64)).astype(np.float32)


def m8data(seed, rows, cols):
    rng = np.random.default_rng(seed)
    return full_range_bytes(rng, rows * cols), rng.uniform(0.5, 2.0, size=(rows // 64) * (cols // 64)).astype(np.float32)


def keep_lowest_index(mags, k):
    """FAST's rule on n magnitudes: everything above the k-th largest, then the ties of lowest index (lowest_index_rule of
    test_threshold_large3.py, for the widths it is not written for)"""
    if k == 0:
        return np.zeros(mags.size, bool)
    tau = np.sort(mags)[::-1][k - 1]
    keep = mags > tau
    keep[np.flatnonzero(mags == tau)[: max(k - int(keep.sum()), 0)]] = True
    return keep


def heap_entries(R, mags, n, k):
    """heap_dev after the reference's walk over n magnitudes: k entries {fp32 |value|, uint32 index}.  The walk compares magnitudes and
    nothing else, so it is the walk of half16_restate.c (pinned against std::make_heap in test_half16_cpu.py) over f16 bit patterns with
    the same order and the same ties: the rank of every magnitude among the distinct ones, which as a positive f16 pattern is monotonic."""
    ranks = np.unique(mags[:n], return_inverse=True)[1]
    assert ranks.max() < 0x7C00, "too many distinct magnitudes for a relabelling in f16"
    _, _, idx = R.rh.threshold_heap(ranks.astype(np.uint16), n, k)
    out = np.empty((k, 2), np.uint32)
    out[:, 0] = mags[idx].astype(np.float32).view(np.uint32)
    out[:, 1] = idx
    return out


CASES = {}


def case(name):
    def reg(build):
        assert name not in CASES, name
        CASES[name] = build
        return build
    return reg


# ---------------------------------------------------------------- vectors of the three widths
# n_pad: one block pair, three, and (1 << 18) -+ 128: clv4_scale_and_add changes kernels at 4096 blocks (test_next_rows.py brackets it
# there too).  The other thresholds of the vector calls lie where operands leave the 256 MiB Infinity Cache: beyond a 64 MiB arena.
V_SIZES = [128, 384, (1 << 18) - 128, 1 << 18, (1 << 18) + 128]
# stochastic vector kernels: the shape (segments per wave) is chosen by size -- 1 up to 8192 blocks (n_pad = 1 << 19, the last size of
# that shape, and the first of the next), 4 up to 2^18 blocks (64 MiB of fp32 input: beyond an arena) -- or forced
ST_SHAPES = [(128, 0), (384, 0), ((1 << 18) + 128, 0), (1 << 19, 0), ((1 << 19) + 128, 0), (384, 4), (384, 16), (384, 64), (8192 + 128, 4), (8192 + 128, 16),
             (8192 + 128, 64)]


def _quantize(fn, n, qbytes, st, seg, quant):
    def build(R):
        x = f32vec(n, n)
        o = R.oracle.rng(*KEYS) if st else None
        q, s = quant(R)(x, o)
        regs = [("x", "input", x), ("q", "output", qbytes), ("s", "output", n // 16)] + ([("rng", "state", None)] if st else [])
        return Case(regs, lambda L, p: getattr(L, fn)(p["x"], n, p["q"], p["s"], p.get("rng"), None), {"q": q, "s": s}, orng=o, segments=seg)
    return build


def _scale_and_add(fn, n, data, st, seg, in_place, saa):
    def build(R):
        (qu, su), (qv, sv) = data(n + 1, n), data(n + 2, n)
        o = R.oracle.rng(*KEYS) if st else None
        r, sr = saa(R)(qu, su, qv, sv, 0.37, o)
        regs = [("qv", "input", qv), ("sv", "input", sv)] + ([("rng", "state", None)] if st else [])
        if in_place:
            regs += [("qu", "inout", qu), ("su", "inout", su)]
            return Case(regs, lambda L, p: getattr(L, fn)(p["qu"], p["su"], p["qv"], p["sv"], 0.37, n, p["qu"], p["su"], p.get("rng"), None),
                        {"qu": r, "su": sr}, orng=o, segments=seg)
        regs += [("qu", "input", qu), ("su", "input", su), ("r", "output", r.nbytes), ("sr", "output", sr.nbytes)]
        return Case(regs, lambda L, p: getattr(L, fn)(p["qu"], p["su"], p["qv"], p["sv"], 0.37, n, p["r"], p["sr"], p.get("rng"), None),
                    {"r": r, "sr": sr}, orng=o, segments=seg)
    return build


def _dot(fn, n, data, mode, exact, fast, ws=None):
    """ws: None (workspace = NULL), or the byte count of a caller workspace as a function of the library (tests/test_caller_workspace.py)"""
    def build(R):
        (qu, su), (qv, sv) = data(n + 3, n), data(n + 4, n)
        # FAST: exact block integers in the library's own fp32 tree, deterministic -- the same call on plain buffers is the reference
        want = (lambda hip: {"out": np.array([fast(hip)(qu, su, qv, sv, DOT_FAST)], np.float32)}) if mode == DOT_FAST else \
            {"out": np.array([exact(R)(qu, su, qv, sv)], np.float32)}
        regs = [("qu", "input", qu), ("su", "input", su), ("qv", "input", qv), ("sv", "input", sv), ("out", "output", 4)]
        regs += [("ws", "scratch", ws)] if ws else []
        return Case(regs, lambda L, p: getattr(L, fn)(p["qu"], p["su"], p["qv"], p["sv"], n, mode, p["out"], p.get("ws"), None), want)
    return build


for _n in V_SIZES:
    case(f"clv4_quantize n_pad={_n}")(_quantize("clv4_quantize", _n, _n // 2, False, 0, lambda R: R.oracle.v4_quantize))
    case(f"clv8_quantize n_pad={_n}")(_quantize("clv8_quantize", _n, _n, False, 0, lambda R: R.oracle.v8_quantize))
    for _ip in (False, True):
        case(f"clv4_scale_and_add n_pad={_n} in_place={_ip}")(_scale_and_add("clv4_scale_and_add", _n, v4, False, 0, _ip, lambda R: R.oracle.v4_scale_and_add))
        case(f"clv8_scale_and_add n_pad={_n} in_place={_ip}")(_scale_and_add("clv8_scale_and_add", _n, v8, False, 0, _ip, lambda R: R.oracle.v8_scale_and_add))
    for _m in (DOT_EXACT, DOT_FAST):
        case(f"clv4_dot n_pad={_n} mode={_m}")(_dot("clv4_dot", _n, v4, _m, lambda R: R.oracle.v4_dot, lambda hip: hip.v4_dot))
        case(f"clv8_dot n_pad={_n} mode={_m}")(_dot("clv8_dot", _n, v8, _m, lambda R: R.oracle.v8_dot, lambda hip: hip.v8_dot))
for _n, _seg in ST_SHAPES:
    case(f"clv4_quantize stochastic n_pad={_n} segments={_seg}")(_quantize("clv4_quantize", _n, _n // 2, True, _seg, lambda R: R.oracle.v4_quantize))
    case(f"clv8_quantize stochastic n_pad={_n} segments={_seg}")(_quantize("clv8_quantize", _n, _n, True, _seg, lambda R: R.oracle.v8_quantize))
    for _ip in (False, True):
        case(f"clv4_scale_and_add stochastic n_pad={_n} segments={_seg} in_place={_ip}")(
            _scale_and_add("clv4_scale_and_add", _n, v4, True, _seg, _ip, lambda R: R.oracle.v4_scale_and_add))
        case(f"clv8_scale_and_add stochastic n_pad={_n} segments={_seg} in_place={_ip}")(
            _scale_and_add("clv8_scale_and_add", _n, v8, True, _seg, _ip, lambda R: R.oracle.v8_scale_and_add))
# the single-launch FAST dots keep two loads in flight per thread up to two steps per thread, one beyond: 2 x 1024 x 256 lanes of 32 nibbles
# / 16 bytes on a part with 256 CUs
for _n in (1 << 24, (1 << 24) + 128):
    case(f"clv4_dot n_pad={_n} mode={DOT_FAST}")(_dot("clv4_dot", _n, v4, DOT_FAST, None, lambda hip: hip.v4_dot))
for _n in (1 << 23, (1 << 23) + 128):
    case(f"clv8_dot n_pad={_n} mode={DOT_FAST}")(_dot("clv8_dot", _n, v8, DOT_FAST, None, lambda hip: hip.v8_dot))


def _restore(fn, n, data, restore):
    def build(R):
        q, s = data(n + 5, n)
        return Case([("q", "input", q), ("s", "input", s), ("x", "output", 4 * n)],
                    lambda L, p: getattr(L, fn)(p["q"], p["s"], n, p["x"], None), {"x": restore(R)(q, s)})
    return build


def _word_isums(n):
    def build(R):
        (qu, _), (qv, _) = v4(n + 6, n), v4(n + 7, n)
        return Case([("qu", "input", qu), ("qv", "input", qv), ("isums", "output", n // 2)],
                    lambda L, p: L.clv4_word_isums(p["qu"], p["qv"], n, p["isums"], None), {"isums": R.oracle.v4_word_isums(qu, qv)})
    return build


def _f16_vec(kind, n, in_place=False, mode=DOT_EXACT, ws=None):
    def build(R):
        u, v = v16(n + 8, n), v16(n + 9, n)
        if kind == "quantize":
            x = f32vec(n + 10, n)
            return Case([("x", "input", x), ("h", "output", 2 * n)], lambda L, p: L.clv_f16_quantize(p["x"], n, p["h"], None), {"h": R.rh.quantize(x)})
        if kind == "restore":
            return Case([("h", "input", u), ("x", "output", 4 * n)], lambda L, p: L.clv_f16_restore(p["h"], n, p["x"], None), {"x": R.rh.restore(u)})
        if kind == "scale_and_add":
            want = R.rh.scale_and_add(u, v, 0.37)
            if in_place:
                return Case([("u", "inout", u), ("v", "input", v)], lambda L, p: L.clv_f16_scale_and_add(p["u"], p["v"], 0.37, n, p["u"], None), {"u": want})
            return Case([("u", "input", u), ("v", "input", v), ("r", "output", 2 * n)],
                        lambda L, p: L.clv_f16_scale_and_add(p["u"], p["v"], 0.37, n, p["r"], None), {"r": want})
        want = (lambda hip: {"out": np.array([hip.f16_dot(u, v, DOT_FAST)], np.float32)}) if mode == DOT_FAST else {"out": np.array([R.rh.dot(u, v)], np.float32)}
        return Case([("u", "input", u), ("v", "input", v), ("out", "output", 4)] + ([("ws", "scratch", ws)] if ws else []),
                    lambda L, p: L.clv_f16_dot(p["u"], p["v"], n, mode, p["out"], p.get("ws"), None), want)
    return build


for _n in V_SIZES:
    case(f"clv4_restore n_pad={_n}")(_restore("clv4_restore", _n, v4, lambda R: R.oracle.v4_restore))
    case(f"clv8_restore n_pad={_n}")(_restore("clv8_restore", _n, v8, lambda R: R.oracle.v8_restore))
    case(f"clv4_word_isums n_pad={_n}")(_word_isums(_n))
    case(f"clv_f16_quantize n_pad={_n}")(_f16_vec("quantize", _n))
    case(f"clv_f16_restore n_pad={_n}")(_f16_vec("restore", _n))
    for _ip in (False, True):
        case(f"clv_f16_scale_and_add n_pad={_n} in_place={_ip}")(_f16_vec("scale_and_add", _n, in_place=_ip))
    for _m in (DOT_EXACT, DOT_FAST):
        case(f"clv_f16_dot n_pad={_n} mode={_m}")(_f16_vec("dot", _n, mode=_m))


# ---------------------------------------------------------------- the mvm family
# rows 64 (one shard: 32 result bytes and one scale in the 4-bit form), 192, 128 x 3; cols 128 and 640 (one chunk of x and a ragged second)
MVM_SHAPES = [(r, c) for r in (64, 192, 384) for c in (128, 640)]


def _mvm4(fn, rows, cols, st=False, shard=False, with_t=True, in_place=False):
    """fn: clm4_mvm | clm4_rowdots | clm4_mvm_scale_and_add | clm4_mvm_f32 and their _v8 forms.  shard: r / sr lie where row block 1 of a
    larger result would have them, 32 (64 for 8-bit results) and 4 bytes behind a 256-byte boundary."""
    eight = "_v8" in fn
    rb = rows if eight else rows // 2                                       # result bytes

    def build(R):
        orc = R.oracle
        qA, sA = m4(rows * cols + 1, rows, cols)
        o = orc.rng(*KEYS) if st else None
        regs = [("A", "input", qA), ("sA", "input", sA)] + ([("rng", "state", None)] if st else [])
        if fn == "clm4_mvm_f32":
            x = f32vec(cols, cols)
            return Case(regs + [("x", "input", x), ("r", "output", 4 * rows)],
                        lambda L, p: L.clm4_mvm_f32(p["A"], p["sA"], rows, cols, p["x"], p["r"], None), {"r": orc.m4_mvm_f32(qA, sA, rows, cols, x)})
        qx, sx = (v8 if eight else v4)(cols + 2, cols)
        regs += [("x", "input", qx), ("sx", "input", sx)]
        mvm = orc.m4_mvm_v8 if eight else orc.m4_mvm
        if "rowdots" in fn:
            d = (orc.m4_rowdots_v8 if eight else orc.m4_rowdots)(qA, sA, rows, cols, qx, sx)
            return Case(regs + [("d", "output", 4 * rows)], lambda L, p: getattr(L, fn)(p["A"], p["sA"], rows, cols, p["x"], p["sx"], p["d"], None), {"d": d})
        if "scale_and_add" not in fn:
            r, sr = mvm(qA, sA, rows, cols, qx, sx, o)
            regs += [("r", "output", rb, (64 if eight else 32) if shard else 0), ("sr", "output", rows // 16, 4 if shard else 0)]
            return Case(regs, lambda L, p: getattr(L, fn)(p["A"], p["sA"], rows, cols, p["x"], p["sx"], p["r"], p["sr"], p.get("rng"), None),
                        {"r": r, "sr": sr}, orng=o)
        qu, su = (v8 if eight else v4)(rows + 3, rows)
        t, st_ = mvm(qA, sA, rows, cols, qx, sx, o)
        r, sr = (orc.v8_scale_and_add if eight else orc.v4_scale_and_add)(qu, su, t, st_, -0.5, o)
        want = {}
        if with_t:
            regs += [("t", "output", rb), ("st", "output", rows // 16)]
            want.update(t=t, st=st_)
        if in_place:
            regs += [("u", "inout", qu), ("su", "inout", su)]
            want.update(u=r, su=sr)
        else:
            regs += [("u", "input", qu), ("su", "input", su), ("r", "output", rb), ("sr", "output", rows // 16)]
            want.update(r=r, sr=sr)
        return Case(regs, lambda L, p: getattr(L, fn)(p["A"], p["sA"], rows, cols, p["x"], p["sx"], p["u"], p["su"], -0.5, p.get("t"), p.get("st"),
                                                      p["u" if in_place else "r"], p["su" if in_place else "sr"], p.get("rng"), None), want, orng=o)
    return build


for _r, _c in MVM_SHAPES:
    for _fn in ("clm4_mvm", "clm4_mvm_v8"):
        for _st in (False, True):
            case(f"{_fn} {_r}x{_c} stochastic={_st}")(_mvm4(_fn, _r, _c, st=_st))
    for _fn in ("clm4_rowdots", "clm4_rowdots_v8", "clm4_mvm_f32"):
        case(f"{_fn} {_r}x{_c}")(_mvm4(_fn, _r, _c))
    for _fn in ("clm4_mvm_scale_and_add", "clm4_mvm_v8_scale_and_add"):
        for _st in (False, True):
            for _t in (True, False):
                case(f"{_fn} {_r}x{_c} stochastic={_st} t={_t}")(_mvm4(_fn, _r, _c, st=_st, with_t=_t))
for _fn in ("clm4_mvm", "clm4_mvm_v8"):
    for _st in (False, True):
        case(f"{_fn} 64x640 stochastic={_st} at a shard's offset")(_mvm4(_fn, 64, 640, st=_st, shard=True))
for _fn in ("clm4_mvm_scale_and_add", "clm4_mvm_v8_scale_and_add"):
    case(f"{_fn} 192x640 in place")(_mvm4(_fn, 192, 640, in_place=True))
    case(f"{_fn} 64x128 in place t=False")(_mvm4(_fn, 64, 128, with_t=False, in_place=True))


def _mvm8(fn, rows, cols, st=False, shard=False):
    def build(R):
        qA, sA = m8data(rows * cols + 5, rows, cols)
        regs = [("A", "input", qA), ("sA", "input", sA)]
        if fn == "clm8_mvm_f32":
            x = f32vec(cols + 1, cols)
            return Case(regs + [("x", "input", x), ("r", "output", 4 * rows)],
                        lambda L, p: L.clm8_mvm_f32(p["A"], p["sA"], rows, cols, p["x"], p["r"], None), {"r": R.m8.mvm_f32(qA, sA, rows, cols, x)})
        qx, sx = v8(cols + 2, cols)
        o = R.oracle.rng(*KEYS) if st else None
        r, sr = R.m8.mvm(qA, sA, rows, cols, qx, sx, o)
        regs += [("x", "input", qx), ("sx", "input", sx), ("r", "output", rows, 64 if shard else 0), ("sr", "output", rows // 16, 4 if shard else 0)]
        regs += [("rng", "state", None)] if st else []
        return Case(regs, lambda L, p: L.clm8_mvm(p["A"], p["sA"], rows, cols, p["x"], p["sx"], p["r"], p["sr"], p.get("rng"), None), {"r": r, "sr": sr}, orng=o)
    return build


for _r, _c in MVM_SHAPES:
    for _st in (False, True):
        case(f"clm8_mvm {_r}x{_c} stochastic={_st}")(_mvm8("clm8_mvm", _r, _c, st=_st))
    case(f"clm8_mvm_f32 {_r}x{_c}")(_mvm8("clm8_mvm_f32", _r, _c))
case("clm8_mvm 64x640 at a shard's offset")(_mvm8("clm8_mvm", 64, 640, shard=True))


def _mvm16(fn, rows, cols):
    def build(R):
        A = v16(rows * cols + 1, rows * cols)
        if fn == "clm_f16_mvm":
            x = v16(cols + 2, cols)
            return Case([("A", "input", A), ("x", "input", x), ("r", "output", 2 * rows)],
                        lambda L, p: L.clm_f16_mvm(p["A"], rows, cols, p["x"], p["r"], None), {"r": R.rh.mvm(A, rows, cols, x)})
        x = f32vec(cols + 3, cols)
        return Case([("A", "input", A), ("x", "input", x), ("r", "output", 4 * rows)],
                    lambda L, p: L.clm_f16_mvm_f32(p["A"], rows, cols, p["x"], p["r"], None), {"r": R.rh.mvm_f32(A, rows, cols, x)})
    return build


# any row count: 1, 17 (one wave and a ragged second), 200; 32768 + 17 rows: four waves per workgroup (from two workgroups per CU on)
for _fn in ("clm_f16_mvm", "clm_f16_mvm_f32"):
    for _r, _c in [(1, 128), (17, 640), (200, 128), (200, 640), (32768 + 17, 128)]:
        case(f"{_fn} {_r}x{_c}")(_mvm16(_fn, _r, _c))


# ---------------------------------------------------------------- matrix quantize, restore, transpose
M_SHAPES = [(128, 128), (128, 384), (384, 128)]


def _mquant(fn, rows, cols, st=False):
    def build(R):
        A = f32vec(rows * cols + 7, rows * cols).reshape(rows, cols)
        ng = (rows // 64) * (cols // 64)
        if fn == "clm_f16_quantize":
            return Case([("A", "input", A), ("h", "output", 2 * rows * cols)], lambda L, p: L.clm_f16_quantize(p["A"], rows, cols, p["h"], None),
                        {"h": R.rh.quantize(A.reshape(-1))})
        o = R.oracle.rng(*KEYS) if st else None
        q, s = (R.oracle.m4_quantize if fn == "clm4_quantize" else R.m8.quantize)(A, o)
        regs = [("A", "input", A), ("q", "output", q.nbytes), ("s", "output", 4 * ng)] + ([("rng", "state", None)] if st else [])
        return Case(regs, lambda L, p: getattr(L, fn)(p["A"], rows, cols, p["q"], p["s"], p.get("rng"), None), {"q": q, "s": s}, orng=o)
    return build


def _mrestore(fn, rows, cols):
    def build(R):
        q, s = (m4 if fn == "clm4_restore" else m8data)(rows * cols + 8, rows, cols)
        want = (R.oracle.m4_restore if fn == "clm4_restore" else R.m8.restore)(q, s, rows, cols)
        return Case([("q", "input", q), ("s", "input", s), ("A", "output", 4 * rows * cols)],
                    lambda L, p: getattr(L, fn)(p["q"], p["s"], rows, cols, p["A"], None), {"A": want})
    return build


def _mtranspose(fn, rows, cols):
    def build(R):
        if fn == "clm_f16_transpose":
            h = v16(rows * cols + 9, rows * cols)
            return Case([("h", "input", h), ("ht", "output", 2 * rows * cols)], lambda L, p: L.clm_f16_transpose(p["h"], rows, cols, p["ht"], None),
                        {"ht": R.rh.transpose(h, rows, cols)})
        q, s = (m4 if fn == "clm4_transpose" else m8data)(rows * cols + 10, rows, cols)
        qt, st_ = (R.oracle.m4_transpose if fn == "clm4_transpose" else R.m8.transpose)(q, s, rows, cols)
        return Case([("q", "input", q), ("s", "input", s), ("qt", "output", qt.nbytes), ("st", "output", st_.nbytes)],
                    lambda L, p: getattr(L, fn)(p["q"], p["s"], rows, cols, p["qt"], p["st"], None), {"qt": qt, "st": st_})
    return build


for _r, _c in M_SHAPES:
    for _fn in ("clm4_quantize", "clm8_quantize"):
        for _st in (False, True):
            case(f"{_fn} {_r}x{_c} stochastic={_st}")(_mquant(_fn, _r, _c, st=_st))
    case(f"clm_f16_quantize {_r}x{_c}")(_mquant("clm_f16_quantize", _r, _c))
    for _fn in ("clm4_restore", "clm8_restore"):
        case(f"{_fn} {_r}x{_c}")(_mrestore(_fn, _r, _c))
    for _fn in ("clm4_transpose", "clm8_transpose", "clm_f16_transpose"):
        case(f"{_fn} {_r}x{_c}")(_mtranspose(_fn, _r, _c))
for _r, _c in [(8, 8), (72, 200), (8, 1000)]:                              # multiples of 8 that are no multiple of the tile
    case(f"clm_f16_transpose {_r}x{_c}")(_mtranspose("clm_f16_transpose", _r, _c))


# ---------------------------------------------------------------- thresholds
SCALE_POOL = np.array([0.5, 0.625, 0.75, 1.0, 1.25, 1.5, 1.75, 1.9375], np.float32)      # few distinct magnitudes: ties, and heap_entries' relabelling


def threshold_data(bits, n_pad, seed):
    rng = np.random.default_rng(seed)
    if bits == 16:
        h = random_f16_bits(rng, n_pad, -3, 3)
        h[rng.integers(0, n_pad, size=n_pad // 2)] = np.float16(1.5).view(np.uint16)
        return h, None
    s = SCALE_POOL[rng.integers(0, SCALE_POOL.size, size=n_pad // 64)]
    if bits == 4:
        return make_v4(rng, n_pad, "uniform")[0], s                          # raw nibbles, -8 included
    return full_range_bytes(rng, n_pad), s


def threshold_reference(R, bits, q, s, n, k, mode):
    """(vector after the call, heap entries or None)"""
    orc = R.oracle
    # |CloverVector8::get| is f32(q * s) / 127 (the oracle's v8_abs, the expression of test_mixed8.py), not restore's q * f32(s / 127)
    mags = np.abs(orc.v4_restore(q, s) if bits == 4 else (q.astype(np.float32) * np.repeat(s, 64)) / np.float32(127.0) if bits == 8 else
                  R.rh.restore(q))[:n]
    if mode == THRESHOLD_FAST:
        if bits == 4:
            return (lowest_index_rule(orc, q, s, n, k) if k else orc.v4_threshold(q, s, n, 0)), None
        out = q.copy()
        out[:n][~keep_lowest_index(mags, k)] = 0
        return out, None
    out = orc.v4_threshold(q, s, n, k) if bits == 4 else orc.v8_threshold(q, s, n, k) if bits == 8 else R.rh.threshold(q, n, k)
    return out, (heap_entries(R, mags, n, k) if mode == HEAP else None)


def threshold_call(bits, mode, n, n_pad, k, ws="ws"):
    """the ABI call of the (width, form) on p["q"], p["s"], p["heap"] and p[ws] (absent: NULL)"""
    if bits == 16:
        if mode == HEAP:
            return lambda L, p: L.clv_f16_threshold_heap(p["q"], n, n_pad, k, p["heap"], p.get(ws), None)
        return lambda L, p: L.clv_f16_threshold_mode(p["q"], n, n_pad, k, mode, p.get(ws), None)
    pre = "clv4" if bits == 4 else "clv8"
    if mode == HEAP:
        return lambda L, p: getattr(L, pre + "_threshold_heap")(p["q"], p["s"], n, n_pad, k, p["heap"], p.get(ws), None)
    return lambda L, p: getattr(L, pre + "_threshold_mode")(p["q"], p["s"], n, n_pad, k, mode, p.get(ws), None)


def threshold_name(bits, mode):
    pre = {4: "clv4", 8: "clv8", 16: "clv_f16"}[bits]
    return f"{pre}_threshold_heap" if mode == HEAP else f"{pre}_threshold_mode {'FAST' if mode == THRESHOLD_FAST else 'REFERENCE'}"


def _threshold(bits, mode, n_pad, k_of, env=None, plain=False, n=None, ws=None, untouched=False):
    """n: n_pad - 37 unless given; ws: None (workspace = NULL), or the byte count of a caller workspace as a function of (library, n_pad,
    k); untouched: the call must leave that workspace as it was"""
    def build(R, n=n):
        n = n_pad - 37 if n is None else n
        k = k_of(n)
        q, s = threshold_data(bits, n_pad, n_pad + bits)
        out, heap = threshold_reference(R, bits, q, s, n, k, mode)
        regs, want = [("q", "inout", q)], {"q": out}
        if s is not None:
            regs.append(("s", "input", s))
        if mode == HEAP:
            regs.append(("heap", "output", 8 * k))
            want["heap"] = heap
        if ws:
            regs.append(("ws", "scratch", lambda L: ws(L, n_pad, k)))
        call = threshold_call(bits, mode, n, n_pad, k)
        if plain:                                                           # clv4_threshold / clv8_threshold: FAST without the mode argument
            call = (lambda L, p: getattr(L, f"clv{bits}_threshold")(p["q"], p["s"], n, n_pad, k, p.get("ws"), None))
        return Case(regs, call, want, env=env, untouched=("ws",) if untouched else ())
    return build


# both sides of the one-workgroup limits of the FAST kernels (4-bit: 131072, 8-bit: 32768; f16 has the large form only)
TH_PADS = {4: [128, 131072, 131072 + 128], 8: [128, 32768, 32768 + 128], 16: [128, 8192 + 128]}
KS = {"0": lambda n: 0, "1": lambda n: 1, "n/4": lambda n: n // 4, "n-1": lambda n: n - 1}
SIX = {"CLV_THRESHOLD_THREE_LAUNCH": "0"}
CAND = {"CLV_THRESHOLD_FORCE_CAND": "1"}
for _bits, _pads in TH_PADS.items():
    for _pad in _pads:
        for _mode in (THRESHOLD_FAST, THRESHOLD_REFERENCE, HEAP):
            for _kn, _kf in KS.items():
                if not (_mode == HEAP and _kn == "0"):                      # the heap forms take 1 <= k <= n
                    case(f"{threshold_name(_bits, _mode)} n_pad={_pad} k={_kn}")(_threshold(_bits, _mode, _pad, _kf))
for _kn, _kf in KS.items():
    case(f"clv4_threshold_mode FAST n_pad={131072 + 128} k={_kn} six launches")(_threshold(4, THRESHOLD_FAST, 131072 + 128, _kf, env=SIX))
    case(f"clv4_threshold_mode FAST n_pad={131072 + 128} k={_kn} candidate words through memory")(_threshold(4, THRESHOLD_FAST, 131072 + 128, _kf, env=CAND))
for _bits, _pad in ((4, 128), (4, 131072 + 128), (8, 128), (8, 32768 + 128)):
    case(f"clv{_bits}_threshold n_pad={_pad} k=n/4")(_threshold(_bits, THRESHOLD_FAST, _pad, KS["n/4"], plain=True))


# ---------------------------------------------------------------- GEMM
def _gemm(fn, M, K, N, kb=None):
    def build(R):
        (qA, sA), (qB, sB) = m4(M * K + 11, M, K), m4(N * K + 12, N, K)
        regs = [("A", "input", qA), ("sA", "input", sA), ("B", "input", qB), ("sB", "input", sB), ("C", "output", 4 * M * N)]
        if fn == "clm4_gemm":
            return Case(regs, lambda L, p: L.clm4_gemm(p["A"], p["sA"], M, K, p["B"], p["sB"], N, p["C"], None), {"C": R.oracle.m4_gemm(qA, sA, M, K, qB, sB, N)})
        import ctypes as C

        def prepared(L, p, enqueue):
            """B prepared once (clm4_gemm_prepare allocates its own image), A raw"""
            op = C.c_void_p()
            rc = L.clm4_gemm_prepare(p["B"], N, K, C.byref(op), None)
            rc = rc or enqueue(op)
            rc = rc or L.clv_stream_sync(None)
            return first_error(rc, L.clm4_gemm_release(op))
        if fn == "clm4_gemm_prepared":
            return Case(regs, lambda L, p: prepared(L, p, lambda op: L.clm4_gemm_prepared(None, p["A"], p["sA"], M, K, op, p["B"], p["sB"], N, p["C"], None)),
                        {"C": R.oracle.m4_gemm(qA, sA, M, K, qB, sB, N)})
        b, c = kb
        S = R.oracle.m4_gemm_isums(qA, M, K, qB, N)[:, :, b:b + c].sum(axis=2, dtype=np.int32)
        regs = [r for r in regs if r[0] not in ("sA", "sB")]
        if fn == "clm4_gemm_i32":
            return Case(regs, lambda L, p: L.clm4_gemm_i32(p["A"], M, K, p["B"], N, b, c, p["C"], None), {"C": S})
        return Case(regs, lambda L, p: prepared(L, p, lambda op: L.clm4_gemm_i32_prepared(None, p["A"], M, K, op, p["B"], N, b, c, p["C"], None)), {"C": S})
    return build


for _M, _K, _N in [(128, 128, 128), (128, 256, 384)]:
    case(f"clm4_gemm {_M}x{_K}x{_N}")(_gemm("clm4_gemm", _M, _K, _N))
    case(f"clm4_gemm_prepared {_M}x{_K}x{_N}")(_gemm("clm4_gemm_prepared", _M, _K, _N))
    for _fn in ("clm4_gemm_i32", "clm4_gemm_i32_prepared"):
        case(f"{_fn} {_M}x{_K}x{_N} all K-blocks (even: the matrix kernel)")(_gemm(_fn, _M, _K, _N, kb=(0, _K // 64)))
        case(f"{_fn} {_M}x{_K}x{_N} K-blocks from 1 (odd: the VALU kernel)")(_gemm(_fn, _M, _K, _N, kb=(1, _K // 64 - 1)))


# ---------------------------------------------------------------- Q_IHT / Q_GD
def _iht(fn, thr, persistent, m=128, n=256, iters=3):
    eight = fn == "clm4_iht_v8"

    def build(R):
        orc = R.oracle
        x_len, K, mu = n - 5, n // 4, np.float32(0.002)
        qP, sP = m4(m * n + 13, m, n)
        qT, sT = orc.m4_transpose(qP, sP, m, n)
        y = (v8 if eight else v4)(m + 14, m)
        mvm, saa = (orc.m4_mvm_v8, orc.v8_scale_and_add) if eight else (orc.m4_mvm, orc.v4_scale_and_add)
        x = (np.zeros(n if eight else n // 2, np.int8 if eight else np.uint8), np.ones(n // 64, np.float32))      # x.clear()
        t1 = t2 = t3 = None
        for _ in range(iters):
            t1 = mvm(qP, sP, m, n, *x)
            t2 = saa(*y, *t1, -1.0)
            t3 = mvm(qT, sT, n, m, *t2)
            x = saa(*x, *t3, float(mu))
            if thr:
                x = (threshold_reference(R, 8 if eight else 4, x[0], x[1], x_len, K, THRESHOLD_FAST)[0], x[1])
        want = dict(x=x[0], sx=x[1], t1=t1[0], st1=t1[1], t2=t2[0], st2=t2[1], t3=t3[0], st3=t3[1])
        regs = [("Phi", "input", qP), ("sPhi", "input", sP), ("PhiT", "input", qT), ("sPhiT", "input", sT), ("y", "input", y[0]), ("sy", "input", y[1])]
        regs += [(k, "output", v.nbytes) for k, v in want.items()]

        def call(L, p):
            before = L.clv_iht_persistent_launches()
            rc = getattr(L, fn)(p["Phi"], p["sPhi"], p["PhiT"], p["sPhiT"], m, n, p["x"], p["sx"], x_len, p["y"], p["sy"], p["t1"], p["st1"], p["t2"],
                                p["st2"], p["t3"], p["st3"], iters, K, float(mu), thr, None, None)
            assert L.clv_iht_persistent_launches() - before == (1 if persistent else 0), "the call did not take the form this case is about"
            return rc
        return Case(regs, call, want, env={"CLV_IHT_PERSISTENT": "1" if persistent else "0"})
    return build


for _fn in ("clm4_iht", "clm4_iht_v8"):
    for _thr in (0, 1):
        for _pers in (True, False):
            case(f"{_fn} 128x256 threshold={_thr} {'persistent' if _pers else 'launch per step'}")(_iht(_fn, _thr, _pers))


# ---------------------------------------------------------------- synthetic data and the rng state
def _fill(fn, count):
    """No restatement of these generators exists here: the guards are checked, and that the output equals the same call into a plain buffer."""
    def build(R):
        nbytes = count if fn == "clv_fill_random_nibbles" else 4 * count

        def args(ptr):
            return (ptr, count, 3, 77, 8, None) if fn == "clv_fill_random_ints_f32" else (ptr, count, 77, 8, None)      # offset 8 into the stream

        def plain(hip):
            buf = hip.alloc(nbytes)
            hip.check(getattr(hip.lib, fn)(*args(buf.ptr)))
            hip.check(hip.lib.clv_stream_sync(None))
            return {"out": buf.download(np.uint8, nbytes)}
        return Case([("out", "output", nbytes)], lambda L, p: getattr(L, fn)(*args(p["out"])), plain)
    return build


case("clv_fill_random_nibbles 4100 bytes")(_fill("clv_fill_random_nibbles", 4100))
case("clv_fill_random_scales 1025 elements")(_fill("clv_fill_random_scales", 1025))
case("clv_fill_random_ints_f32 1025 elements")(_fill("clv_fill_random_ints_f32", 1025))


@case("clv_rng_seed")
def _rng_seed(R):
    return Case([("rng", "state", None)], lambda L, p: L.clv_rng_seed(p["rng"], 99, 100, None), {}, orng=R.oracle.rng(99, 100))


@case("clv_rng_set")
def _rng_set(R):
    import ctypes as C
    o = R.oracle.rng(5, 6)
    k1, k2 = (C.c_uint64 * 4)(*o.s0), (C.c_uint64 * 4)(*o.s1)
    return Case([("rng", "state", None)], lambda L, p: L.clv_rng_set(p["rng"], k1, k2, None), {}, orng=o)


@case("clv_rng_graph_mode")
def _rng_graph_mode(R):
    """the launch stamps move into the state buffer, a tick kernel runs in front of the stochastic kernel: same bits, same keys, 256 bytes"""
    n = 384
    x = f32vec(n, n)
    o = R.oracle.rng(*KEYS)
    q, s = R.oracle.v4_quantize(x, o)
    return Case([("x", "input", x), ("q", "output", n // 2), ("s", "output", n // 16), ("rng", "state", None)],
                lambda L, p: first_error(L.clv_rng_graph_mode(p["rng"], 1, None), L.clv4_quantize(p["x"], n, p["q"], p["s"], p["rng"], None),
                                         L.clv_rng_graph_mode(p["rng"], 0, None)), {"q": q, "s": s}, orng=o)


# ================================================================ the tests
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_call_writes_its_outputs_and_nothing_else(hip, refs, name):
    run_case(hip, CASES[name](refs))


# clv8_scale_and_add takes its once-per-block kernel from 2^21 blocks on (384 MiB of operands: beyond an arena); CLV_SAA8_BLK_MIN_BLOCKS moves
# the threshold and is read once per process, so these sizes run in a child process (as in test_mixed8.py): one block pair, three, and a
# ragged last chunk of a second workgroup (a wave owns 64 blocks, a workgroup 256)
SAA8_BLK_SIZES = [128, 384, 64 * 256 + 128 * 3]


def saa8_blk_child():
    from clover_amd.lib_binding import CloverHip
    from oracle.binding import Oracle
    hip, R = CloverHip(), Refs(Oracle(), None, None)
    for n in SAA8_BLK_SIZES:
        for in_place in (False, True):
            run_case(hip, _scale_and_add("clv8_scale_and_add", n, v8, False, 0, in_place, lambda R: R.oracle.v8_scale_and_add)(R))
    print("guarded", 2 * len(SAA8_BLK_SIZES))


@pytest.mark.gpu
def test_block_kernel_of_the_8_bit_scale_and_add_writes_its_outputs_and_nothing_else():
    import subprocess
    import sys
    from pathlib import Path
    here = Path(__file__).resolve().parent
    code = f"import sys; sys.path[:0] = [{str(here)!r}, {str(here.parent)!r}]; import test_guard_bands as G; G.saa8_blk_child()"
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CLV_SAA8_BLK_MIN_BLOCKS="1"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and f"guarded {2 * len(SAA8_BLK_SIZES)}" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])


def _one_output(hip):
    A = Arena(hip, seed=3).add("a", "input", data=np.arange(100, dtype=np.uint8)).add("out", "output", nbytes=36).add("b", "input", data=np.zeros(7, np.uint8))
    return A.upload()


@pytest.mark.gpu
@pytest.mark.parametrize("where,offset", [("behind", 36), ("before", -1)])
def test_the_checker_reports_one_byte_outside_a_declared_range(hip, where, offset):
    """one byte just past / just before an output's declared range (inside the allocation: nothing faults) is reported with the region's
    name and the offset; the same arena untouched, and written inside the range only, passes"""
    want = np.arange(36, dtype=np.uint8)
    A = _one_output(hip)
    hip.check(hip.lib.clv_memcpy_h2d(A.ptr("out"), want.ctypes.data, 36, None))
    A.check({"out": want})
    at = A.regions["out"].offset + offset
    hip.check(hip.lib.clv_memset(A.base + at, int(A.image[at]) ^ 0xFF, 1, None))
    hip.check(hip.lib.clv_stream_sync(None))
    with pytest.raises(GuardError) as e:
        A.check({"out": want})
    msg = str(e.value)
    assert "1 byte(s) changed near `out`" in msg and f"first at offset {offset:+d} from its start ({where} its declared range)" in msg, msg
    A.close()


@pytest.mark.gpu
def test_the_checker_reports_an_unwritten_output_and_a_changed_input(hip):
    want = np.arange(36, dtype=np.uint8)
    A = _one_output(hip)
    hip.check(hip.lib.clv_memcpy_h2d(A.ptr("out"), want.ctypes.data, 35, None))           # the last byte keeps its prefill
    if A.image[A.regions["out"].end - 1] == 35:
        want[35] = 36
    with pytest.raises(GuardError, match=r"`out` \(output, 36 bytes\): 1 byte\(s\) differ from the reference, first at offset 35 \(1 of them still hold the prefill\)"):
        A.check({"out": want})
    hip.check(hip.lib.clv_memset(A.ptr("b") + 6, 1, 1, None))
    with pytest.raises(GuardError, match=r"1 byte\(s\) changed near `b` \(input, 7 bytes\): first at offset \+6 from its start \(inside"):
        A.check({"out": want})
    A.close()


# ---------------------------------------------------------------- coverage (no GPU)
# Entry points that no case of this file calls, each with its reason.  Everything else include/clover_hip.h declares has a case.
EXCLUDED = {
    **{n: "runtime: device, memory, stream and event management; no kernel of the library writes through them" for n in (
        "clv_version", "clv_last_error", "clv_device_count", "clv_set_device", "clv_get_device", "clv_device_info", "clv_malloc", "clv_free", "clv_memset",
        "clv_memcpy_h2d", "clv_memcpy_d2h", "clv_memcpy_d2d", "clv_host_alloc", "clv_host_free", "clv_stream_create", "clv_stream_destroy",
        "clv_stream_sync", "clv_device_sync", "clv_event_create", "clv_event_destroy", "clv_event_record", "clv_event_sync", "clv_event_elapsed_ms")},
    "clv_rng_get": "reads the state into host arrays (every stochastic case compares the state through it)",
    "clv_rng_set_segments": "a process-wide tuning knob, no device pointer (the stochastic cases set it)",
    "clv_iht_persistent_launches": "a host counter (the clm4_iht cases read it)",
    **{n: "a size query, no device pointer (tests/test_caller_workspace.py allocates exactly what they return)" for n in (
        "clv4_dot_workspace_bytes", "clv8_dot_workspace_bytes", "clv4_threshold_workspace_bytes", "clv8_threshold_workspace_bytes",
        "clv_threshold_reference_workspace_bytes", "clv_threshold_reference_workspace_bytes_k", "clv_f16_dot_workspace_bytes",
        "clv_f16_threshold_workspace_bytes")},
    "clm4_gemm_prepare": "allocates the memory it writes (the clm4_gemm_prepared cases call it)",
    "clm4_gemm_release": "frees what clm4_gemm_prepare allocated",
    "clm4_shard_partition": "host arithmetic, no device pointer",
    **{n: "the clm4_sharded_* family allocates its own device memory" for n in SIGNATURES if n.startswith("clm4_sharded_")},
}


def test_the_case_list_covers_every_entry_point_that_writes_device_memory():
    covered = {c.split()[0] for c in CASES}
    assert covered.isdisjoint(EXCLUDED), covered & set(EXCLUDED)
    assert covered | set(EXCLUDED) == set(SIGNATURES), (set(SIGNATURES) - covered - set(EXCLUDED), (covered | set(EXCLUDED)) - set(SIGNATURES))
    # the plain FAST entry points are called as themselves, not only through the _mode forms
    assert {"clv4_threshold", "clv8_threshold"} <= covered
