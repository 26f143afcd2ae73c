"""The fp32-vector calls of CloverMatrix4 (include/clover_hip_m4_f32.h) and CloverMatrix8 (include/clover_hip_m8_f32.h) are one host
driver (clover_amd/csrc/mvm_f32_host.h) behind two sets of names, without a GPU:

- every bad-argument case of the table below -- built from the cases tests/test_m4_f32_cpu.py and tests/test_m8_f32_cpu.py exercise one
  width at a time -- goes to the 4-bit and to the 8-bit entry point of the call; both answer CLV_ERR_INVALID and the two messages are the
  same text once clm4_ / clm8_ is taken out;
- what the widths do NOT share is the bound behind "matrix too large": rows * cols <= 2^48 - 1 for the 4-bit calls, <= 2^48 for the 8-bit
  ones.  Each answers as before on either side of its own bound; 2^24 x 2^24 is the one shape that tells them apart;
- the valid empty calls return CLV_OK for both.

The addresses are never dereferenced: every call either fails validation or has rows == 0 or cols == 0, so nothing runs.  A shape at a
"too large" bound that passes the bound is still refused, by the overlap check behind it: every address of the table lies inside a matrix
of 2^47 bytes or more."""
import pytest

from clover_amd.lib_binding import load_library
from test_mvm_batch_cpu import addr, failed

FUSED, MVT, FUSED_T, IHT, IHT1 = "mvm_f32_scale_and_add", "mvm_f32_transposed", "mvm_f32_transposed_scale_and_add", "iht_f32", "iht_f32_one_matrix"
CALLS = (FUSED, MVT, FUSED_T, IHT, IHT1)
WIDTHS = ("clm4_", "clm8_")

# 128 x 256: at most 32768 bytes of matrix, the grid 2 x 4 scales.  Row-major: x 1024 bytes, u / t / r2 512; transposed: x 512, the others 1024
A_, S_, X_, R_, U_, T_ = addr(0), addr(2), addr(4), addr(6), addr(8), addr(10)
LOOP_PTRS = ("Phi", "sPhi", "PhiT", "sPhiT", "x", "y", "t1", "t2", "t3")
LOOP = {k: addr(20 + 2 * i) for i, k in enumerate(LOOP_PTRS)}


@pytest.fixture(scope="module")
def lib():
    return load_library()


def call(lib, width, fn, **kw):
    """the entry point `fn` of one width on 128 x 256 and the addresses above, with `kw` replacing arguments"""
    f = getattr(lib, width + fn)
    if fn in (IHT, IHT1):
        p = dict(LOOP, m=128, n=256, x_len=256, thr=1)
        p.update(kw)
        mats = (p["Phi"], p["sPhi"]) + ((p["PhiT"], p["sPhiT"]) if fn == IHT else ())
        return f(*mats, p["m"], p["n"], p["x"], p["x_len"], p["y"], p["t1"], p["t2"], p["t3"], 3, 8, 0.5, p["thr"], None)
    p = dict(rows=128, cols=256, A=A_, sA=S_, x=X_, r=R_, u=U_, t=T_, r2=R_)
    p.update(kw)
    if fn == MVT:
        return f(p["A"], p["sA"], p["rows"], p["cols"], p["x"], p["r"], None)
    return f(p["A"], p["sA"], p["rows"], p["cols"], p["x"], p["u"], 0.5, p["t"], p["r2"], None)


def loop_ptrs(fn):
    return [k for k in LOOP_PTRS if fn == IHT or "PhiT" not in k]


def cases():
    """(call, replaced arguments, words the message holds) -- the words from the single-width tests, which pin the text"""
    out = []
    # each NULL
    out += [(MVT, {k: None}, (f"{k} is NULL",)) for k in ("A", "sA", "x", "r")]
    out += [(MVT, {k: None, "rows": 0}, (f"{k} is NULL",)) for k in ("A", "sA", "x", "r")]          # checked even where nothing would run
    for fn in (FUSED, FUSED_T):
        out += [(fn, {k: None}, (f"{k} is NULL",)) for k in ("A", "sA", "x", "u", "r2")]
    for fn in (IHT, IHT1):
        out += [(fn, {k: None}, (f"{k} is NULL",)) for k in loop_ptrs(fn)]
    # each misalignment
    out += [(MVT, {"A": A_ + 8}, ("A must be 16-byte aligned",)), (MVT, {"x": X_ + 4}, ("x must be 16-byte aligned",)),
            (MVT, {"r": R_ + 2}, ("r must be 4-byte aligned",)), (MVT, {"sA": S_ + 1}, ("sA", "4-byte aligned"))]
    for fn in (FUSED, FUSED_T):
        out += [(fn, {"A": A_ + 4}, ("A must be 16-byte aligned",)), (fn, {"x": X_ + 8}, ("x must be 16-byte aligned",))]
        out += [(fn, {k: addr(12) + 2}, ("u, t and r2 must be 4-byte aligned",)) for k in ("u", "t", "r2")]
        out += [(fn, {"sA": S_ + 2}, ("sA, u, t and r2 must be 4-byte aligned",))]
    for fn in (IHT, IHT1):
        out += [(fn, {"Phi": LOOP["Phi"] + 8}, ("matrices must be 16-byte aligned",)), (fn, {"x": LOOP["x"] + 4}, ("x must be 16-byte aligned",)),
                (fn, {"t2": LOOP["t2"] + 8}, ("t2 must be 16-byte aligned",))]
        out += [(fn, {k: LOOP[k] + 2}, ("the scales, y, t1 and t3 must be 4-byte aligned",)) for k in ("sPhi", "y", "t1", "t3")]
    out += [(IHT, {"PhiT": LOOP["PhiT"] + 8}, ("matrices must be 16-byte aligned",)), (IHT, {"sPhiT": LOOP["sPhiT"] + 1}, ("4-byte aligned",))]
    # a shape that is not a multiple of 128 (row-major: rows of 64)
    out += [(MVT, {"cols": 100}, ("cols=100", "multiples of 128")), (MVT, {"rows": 64}, ("rows=64", "multiples of 128")),
            (MVT, {"rows": 200, "cols": 0}, ("rows=200",)), (FUSED_T, {"rows": 192}, ("rows=192", "multiples of 128")),
            (FUSED_T, {"cols": 64}, ("cols=64", "multiples of 128")), (FUSED, {"rows": 96}, ("rows=96", "multiple of 64")),
            (FUSED, {"cols": 192}, ("cols=192", "of 128"))]
    for fn in (IHT, IHT1):
        out += [(fn, {"m": 64}, ("m=64", "multiples of 128")), (fn, {"n": 192}, ("n=192", "multiples of 128")),
                (fn, {"x_len": 257}, ("x_len=257", "n=256")),                                  # x_len > n
                (fn, {"thr": 3}, ("threshold 3",)), (fn, {"thr": -1}, ("threshold -1",))]          # an unknown threshold
    # an overlap of the result with x; t overlapping A
    out += [(MVT, {"r": X_}, ("overlaps", "`r`", "`x`")), (MVT, {"r": A_}, ("overlaps", "`A`"))]
    for fn in (FUSED, FUSED_T):
        out += [(fn, {"r2": X_}, ("overlaps", "`r2`", "`x`")), (fn, {"t": A_ + 4096}, ("overlaps", "`t`", "`A`")),
                (fn, {"t": R_}, ("overlaps", "`t`", "`r2`")), (fn, {"u": U_, "r2": U_, "t": X_}, ("overlaps", "`t`"))]
    for fn in (IHT, IHT1):
        out += [(fn, {"t3": LOOP["x"]}, ("overlaps", "`t3`", "`x`")), (fn, {"t2": LOOP["Phi"]}, ("overlaps", "`t2`", "`Phi`"))]
    return out


CASES = cases()


def test_the_table_reaches_every_call_and_every_kind_of_rule():
    assert {c[0] for c in CASES} == set(CALLS)
    for word in ("is NULL", "aligned", "multiples of 128", "x_len=", "threshold", "`x`", "`A`"):
        assert any(any(word in w for w in c[2]) for c in CASES), word


@pytest.mark.parametrize("fn,kw,words", CASES, ids=[f"{c[0]}-{'-'.join(c[1])}-{i}" for i, c in enumerate(CASES)])
def test_both_widths_refuse_with_the_same_words(lib, fn, kw, words):
    texts = []
    for width in WIDTHS:
        failed(lib, call(lib, width, fn, **kw), width + fn, *words)
        texts.append(lib.clv_last_error().decode().replace(width, "clmN_"))
    assert texts[0] == texts[1]


# rows * cols = 2^48 - 2^31 (4-bit: the largest product of this column count below its bound), 2^48 (the 8-bit bound itself, the 4-bit
# bound plus one) and 2^48 + 2^31 (one step of 128 rows beyond).  rows / 32 and cols / 64 stay below 2^31, so the second rule is silent
BOUND_COLS = 1 << 24
BOUND_ROWS = {"clm4_": ((1 << 24) - 128, 1 << 24), "clm8_": (1 << 24, (1 << 24) + 128)}      # (the last shape accepted, the first refused)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("fn", CALLS)
def test_each_width_keeps_its_own_bound(lib, width, fn):
    shape = (lambda rows: dict(m=rows, n=BOUND_COLS)) if fn in (IHT, IHT1) else (lambda rows: dict(rows=rows, cols=BOUND_COLS))
    inside, beyond = BOUND_ROWS[width]
    failed(lib, call(lib, width, fn, **shape(inside)), width + fn, "overlaps")           # past the bound; the overlap check refuses it
    assert b"too large" not in lib.clv_last_error()
    failed(lib, call(lib, width, fn, **shape(beyond)), width + fn, "matrix too large")
    failed(lib, call(lib, width, fn, **shape(beyond + 128)), width + fn, "matrix too large")


def test_the_two_bounds_differ_by_one(lib):
    for fn in CALLS:
        shape = dict(m=1 << 24, n=BOUND_COLS) if fn in (IHT, IHT1) else dict(rows=1 << 24, cols=BOUND_COLS)
        failed(lib, call(lib, "clm4_", fn, **shape), "clm4_" + fn, "matrix too large")
        failed(lib, call(lib, "clm8_", fn, **shape), "clm8_" + fn, "overlaps")


def test_the_valid_empty_calls_return_ok_for_both(lib):
    for width in WIDTHS:
        for kw in (dict(rows=0), dict(cols=0), dict(rows=0, cols=0)):
            assert call(lib, width, MVT, **kw) == 0, (width, kw)
            for fn in (FUSED, FUSED_T):
                assert call(lib, width, fn, **kw) == 0 and call(lib, width, fn, t=None, **kw) == 0, (width, fn, kw)
                assert call(lib, width, fn, u=U_, r2=U_, **kw) == 0, (width, fn, kw)                 # the in-place form
        assert call(lib, width, MVT, rows=0, r=X_) == 0                                              # no rows: x is empty
        assert call(lib, width, FUSED, rows=64, cols=0) == 0                                         # row-major: rows of 64
