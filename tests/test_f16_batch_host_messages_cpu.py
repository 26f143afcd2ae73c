"""The return code and the exact clv_last_error text of the batched half-precision entry points, call by call, against a recording
(tests/golden/f16_batch_host_messages.json): the two row-major products (clm_f16_mvm_batch, clm_f16_mvm_scale_and_add_batch), the two
transposed ones, the two loops (clm_f16_iht_batch, clm_f16_iht_batch_one_matrix) and clv_f16_threshold_batch, which has a host side of its
own and is here as a control.  The six share one host driver (clover_amd/csrc/half16_batch_host.h); the recording was made at commit
2a63ec0, when each family still had a driver of its own, so that the order of the checks -- which message wins when a call is wrong in two
ways --, "matrices" against "matrix" and the (x of vector N) suffixes stay what they were.

Every call either fails validation or is empty: the addresses are never dereferenced and nothing touches a device.  A call that returns
CLV_OK must leave the last message alone.

    python tests/test_f16_batch_host_messages_cpu.py --record      # writes the fixture from the library as built"""
import json
import sys
from pathlib import Path

import pytest

sys.path[:0] = [str(Path(__file__).resolve().parent), str(Path(__file__).resolve().parent.parent)]      # for --record
from clover_amd.lib_binding import load_library  # noqa: E402
from test_mvm_batch_cpu import addr, arr  # noqa: E402

GOLDEN = Path(__file__).resolve().parent / "golden" / "f16_batch_host_messages.json"
MVM, FUSED, IHT = "clm_f16_mvm_batch", "clm_f16_mvm_scale_and_add_batch", "clm_f16_iht_batch"
MVM_T, FUSED_T, IHT_1 = "clm_f16_mvm_transposed_batch", "clm_f16_mvm_transposed_scale_and_add_batch", "clm_f16_iht_batch_one_matrix"
THRESH = "clv_f16_threshold_batch"
PRODUCTS, PLAIN, FUSEDS, LOOPS = (MVM, FUSED, MVM_T, FUSED_T), (MVM, MVM_T), (FUSED, FUSED_T), (IHT, IHT_1)
# 128 x 256: the matrix has 65536 bytes; row-major x has 512 bytes and r / u / t 256, transposed the other way round.  addr(i) are 1 MiB apart
A_ = addr(0)
VECTORS = dict(x=(2, 3), r=(6, 7), u=(10, 11), t=(14, 15))
SIGNALS = dict(x=(20, 21), y=(22, 23), t1=(24, 25), t2=(26, 27), t3=(28, 29))


def array(v):
    return None if v is None else arr(*v)


def call(lib, fn, **kw):
    f = getattr(lib, fn)
    if fn == THRESH:
        p = dict(h=(addr(2), addr(3)), nvec=2, n=200, n_pad=256, k=8, mode=0)
        p.update(kw)
        return f(array(p["h"]), p["nvec"], p["n"], p["n_pad"], p["k"], p["mode"], None)
    if fn in LOOPS:
        p = dict(m=128, n=256, nvec=2, x_len=256, thr=1, Phi=A_, PhiT=addr(1), **{k: (addr(a), addr(b)) for k, (a, b) in SIGNALS.items()})
        p.update(kw)
        mats = (p["Phi"], p["PhiT"]) if fn == IHT else (p["Phi"],)
        return f(*mats, p["m"], p["n"], p["nvec"], array(p["x"]), p["x_len"], array(p["y"]), array(p["t1"]), array(p["t2"]), array(p["t3"]), 3, 8,
                 0.5, p["thr"], None)
    p = dict(rows=128, cols=256, nvec=2, A=A_, **{k: (addr(a), addr(b)) for k, (a, b) in VECTORS.items()})
    p.update(kw)
    if fn in FUSEDS:
        return f(p["A"], p["rows"], p["cols"], p["nvec"], array(p["x"]), array(p["u"]), 0.5, array(p["t"]), array(p["r"]), None)
    return f(p["A"], p["rows"], p["cols"], p["nvec"], array(p["x"]), array(p["r"]), None)


def table():
    """label -> (entry point, arguments that differ from a valid call of two vectors on a 128 x 256 matrix)"""
    T = {}

    def add(label, fn, **kw):
        key = f"{fn}: {label}"
        assert key not in T, key
        T[key] = (fn, kw)
    x0, x1, r0, r1, u0, u1, t0, t1 = (addr(i) for i in (2, 3, 6, 7, 10, 11, 14, 15))
    for fn in PRODUCTS:
        tr = fn in (MVM_T, FUSED_T)
        xb, rb = (256, 512) if tr else (512, 256)            # bytes of x and of r / u / t
        # ---- one thing wrong: what the two existing CPU tests ask, for both families
        add("A NULL", fn, A=None)
        add("x array NULL", fn, x=None)
        add("r array NULL", fn, r=None)
        add("x[0] NULL", fn, x=(None, x1))
        add("r[1] NULL", fn, r=(r0, None))
        add("r[1] NULL, rows 0", fn, rows=0, r=(r0, None))
        add("cols 100", fn, cols=100)
        if tr:                                               # valid and not empty for the row-major pair: they would run
            add("rows 64", fn, rows=64)
            add("rows 192", fn, rows=192)
            add("rows 200, cols 0", fn, rows=200, cols=0)
        add("A + 8", fn, A=A_ + 8)
        add("A + 2", fn, A=A_ + 2)
        add("x[1] + 2", fn, x=(x0, x1 + 2))
        add("x[0] + 8", fn, x=(x0 + 8, x1))
        add("r[1] + 1", fn, r=(r0, r1 + 1))
        add("r[0] + 1", fn, r=(r0 + 1, r1))
        add("2^40 x 2^40, nvec 0", fn, rows=1 << 40, cols=1 << 40, nvec=0, x=None, r=None)
        add("2^37 x 128, nvec 0", fn, rows=1 << 37, cols=128, nvec=0, x=None, r=None)
        add("128 x 2^38, nvec 0", fn, rows=128, cols=1 << 38, nvec=0, x=None, r=None)
        add("r[1] == x[1]", fn, r=(r0, x1))
        add("r[0] == x[1]", fn, r=(x1, r1))
        add("r[0] ends inside x[1]", fn, r=(x1 - rb + 2, r1))
        add("r[0] begins inside x[1]", fn, r=(x1 + xb - 2, r1))
        add("r[0] == r[1]", fn, r=(r0, r0))
        add("r[1] begins inside r[0]", fn, r=(r0, r0 + rb - 2))
        add("r[1] == A", fn, r=(r0, A_))
        add("r[1] on the last element of A", fn, r=(r0, A_ + 2 * 128 * 256 - 2))
        # ---- wrong in two ways: the order of the checks
        add("A + 8 and cols 100", fn, A=A_ + 8, cols=100)
        add("A + 8 and rows 64", fn, A=A_ + 8, rows=64)
        add("A NULL and cols 100", fn, A=None, cols=100)
        add("x array NULL and cols 100", fn, x=None, cols=100)
        add("x array NULL and rows 64", fn, x=None, rows=64)
        add("r array NULL and A + 8", fn, r=None, A=A_ + 8)
        add("x array NULL and 2^40 x 2^40", fn, x=None, rows=1 << 40, cols=1 << 40)
        add("x[1] + 2 and r[0] == x[0]", fn, x=(x0, x1 + 2), r=(x0, r1))
        add("x[1] + 2 and r[0] + 1", fn, x=(x0, x1 + 2), r=(r0 + 1, r1))
        add("x[1] NULL and x[0] + 2", fn, x=(x0 + 2, None))
        add("r[0] == x[0] and r[1] inside A", fn, r=(x0, A_ + 4096))
        add("r[0] inside A and r[1] == r[0]", fn, r=(A_ + 4096, A_ + 4096))
        # ---- empty calls
        add("nvec 0", fn, nvec=0, x=None, r=None, u=None, t=None)
        add("rows 0", fn, rows=0)
        add("rows 0 and cols 0", fn, rows=0, cols=0)
        add("rows 0, nvec 1", fn, rows=0, nvec=1)
        add("rows 0, r with element alignment only", fn, rows=0, r=(r0 + 2, r1 + 6))
        add("rows 0, r[0] behind x[1]", fn, rows=0, r=(x1 + xb, r1))
        add("rows 0, r[0] in front of x[1]", fn, rows=0, r=(x1 - rb, r1))
        add("rows 0, x twice", fn, rows=0, x=(x0, x0))
        if tr:                                               # a matrix without columns is empty for the transposed pair alone
            add("cols 0", fn, cols=0)
            add("cols 0, nvec 1", fn, cols=0, nvec=1)
            add("cols 0, r[0] behind x[1]", fn, cols=0, r=(x1 + xb, r1))
            add("cols 0, x twice", fn, cols=0, x=(x0, x0))
        # ---- the range check
        add("r[0] inside A", fn, r=(A_ + 4096, r1))
    for fn in FUSEDS:
        tr = fn == FUSED_T
        rb = 512 if tr else 256
        add("u array NULL", fn, u=None)
        add("u[1] NULL", fn, u=(u0, None))
        add("t[0] NULL", fn, t=(None, t1))
        add("u[1] + 3", fn, u=(u0, u1 + 3))
        add("t[1] + 1", fn, t=(t0, t1 + 1))
        add("t[1] == x[1]", fn, t=(t0, x1))
        add("t[1] == r[1]", fn, t=(t0, r1))
        add("t[0] == u[0]", fn, t=(u0, t1))
        add("r[1] == u[0]", fn, r=(r0, u0))
        add("r[1] begins inside u[0]", fn, r=(r0, u0 + rb - 2))
        add("t[1] == r[0]", fn, t=(t0, r0))
        add("t[0] == t[1]", fn, t=(t0, t0))
        add("t[1] == x[0]", fn, t=(t0, x0))
        add("t[0] inside A", fn, t=(A_ + 4096, t1))
        add("in place, u[1] == r[0]", fn, r=(u0, r1), u=(u0, u0))
        add("u array NULL and cols 100", fn, u=None, cols=100)
        add("t[0] NULL and t[1] + 1", fn, t=(None, t1 + 1))
        add("t[1] == r[1] and x[0] + 8", fn, t=(t0, r1), x=(x0 + 8, x1))
        add("t[0] == u[0] and t[1] == x[1]", fn, t=(u0, x1))
        add("t[1] ends on the first element of x[0]", fn, t=(t0, x0 - rb + 2))
        add("t[1] ends in front of x[0], rows 0", fn, rows=0, t=(t0, x0 - rb))
        add("rows 0, t NULL", fn, rows=0, t=None)
        add("rows 0, u twice", fn, rows=0, u=(u0, u0))
        add("rows 0, in place", fn, rows=0, r=(u0, u1))
        add("rows 0, in place, t NULL", fn, rows=0, r=(u0, u1), t=None)
        if tr:
            add("cols 0, t NULL", fn, cols=0, t=None)
            add("cols 0, u twice", fn, cols=0, u=(u0, u0))
            add("cols 0, in place", fn, cols=0, r=(u0, u1))
    sx0, sx1, sy0, sy1, s10, s11, s20, s21, s30, s31 = (addr(i) for i in range(20, 30))
    for fn in LOOPS:
        add("Phi NULL", fn, Phi=None)
        for k in SIGNALS:
            add(f"{k} array NULL", fn, **{k: None})
        add("y[1] NULL", fn, y=(sy0, None))
        add("t3[0] NULL", fn, t3=(None, s31))
        add("m 64", fn, m=64)
        add("n 192", fn, n=192)
        add("x_len 257", fn, x_len=257)
        add("threshold 3", fn, thr=3)
        add("threshold -1", fn, thr=-1)
        add("Phi + 8", fn, Phi=A_ + 8)
        add("x[1] + 2", fn, x=(sx0, sx1 + 2))
        add("t2[0] + 8", fn, t2=(s20 + 8, s21))
        add("t1[1] + 1", fn, t1=(s10, s11 + 1))
        add("y[0] + 1", fn, y=(sy0 + 1, sy1))
        add("2^40 x 2^40, nvec 0", fn, m=1 << 40, n=1 << 40, x_len=0, nvec=0)
        add("2^36 x 128, nvec 0", fn, m=1 << 36, n=128, x_len=0, nvec=0)
        add("t3[1] == x[0]", fn, t3=(s30, sx0))
        add("t1[1] == y[0]", fn, t1=(s10, sy0))
        add("x[0] == x[1]", fn, x=(sx0, sx0))
        add("t2[1] inside t1[0]", fn, t2=(s20, s10 + 128))
        add("t2[1] == Phi", fn, t2=(s20, A_))
        add("x[1] inside Phi", fn, x=(sx0, A_ + 4096))
        add("Phi + 8 and threshold 3", fn, Phi=A_ + 8, thr=3)
        add("x_len 257 and Phi NULL", fn, x_len=257, Phi=None)
        add("x_len 257 and threshold 3", fn, x_len=257, thr=3)
        add("Phi + 8 and 2^40 x 2^40", fn, Phi=A_ + 8, m=1 << 40, n=1 << 40)
        add("x array NULL and Phi + 8", fn, x=None, Phi=A_ + 8)
        add("y[1] NULL and x[0] + 2", fn, y=(sy0, None), x=(sx0 + 2, sx1))
        add("x[1] + 2 and y[0] + 1", fn, x=(sx0, sx1 + 2), y=(sy0 + 1, sy1))
        add("t1[1] + 1 and t3[1] == x[0]", fn, t1=(s10, s11 + 1), t3=(s30, sx0))
        add("nvec 0", fn, nvec=0, x=None, y=None, t1=None, t2=None, t3=None)
        add("nvec 0, threshold 0", fn, nvec=0, thr=0)
    add("PhiT NULL", IHT, PhiT=None)
    add("PhiT + 8", IHT, PhiT=addr(1) + 8)
    add("PhiT + 8 and threshold 3", IHT, PhiT=addr(1) + 8, thr=3)
    add("x_len 257 and PhiT NULL", IHT, x_len=257, PhiT=None)
    add("t2[1] inside PhiT", IHT, t2=(addr(26), addr(1) + 4096))
    # ---- the control: a host side this change does not touch
    add("nvec 0", THRESH, h=None, nvec=0, n=100, n_pad=128, k=4)
    add("h NULL", THRESH, h=None)
    add("h[1] NULL", THRESH, h=(addr(2), None))
    add("mode 7", THRESH, mode=7)
    add("n_pad 200", THRESH, n_pad=200)
    add("n 257", THRESH, n=257)
    add("h[0] == h[1]", THRESH, h=(addr(2), addr(2)))
    add("h[1] begins inside h[0]", THRESH, h=(addr(2), addr(2) + 510))
    return T


TABLE = table()


def outcome(lib, fn, kw):
    """the return code and the message the call left; None where it left the message alone"""
    before = lib.clv_last_error()
    rc = call(lib, fn, **kw)
    after = lib.clv_last_error()
    if rc == 0:
        assert after == before, ("a call that returns CLV_OK set a message", after)
        return {"rc": 0, "error": None}
    return {"rc": rc, "error": after.decode()}


@pytest.fixture(scope="module")
def lib():
    return load_library()


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


def test_the_recording_covers_the_table_and_nothing_else(golden):
    assert sorted(golden["calls"]) == sorted(TABLE)
    fails = [k for k, v in golden["calls"].items() if v["rc"] != 0]
    assert len(fails) >= 250 and len(TABLE) - len(fails) >= 50
    for k, v in golden["calls"].items():
        assert (v["rc"] == 0) == (v["error"] is None), k
        assert v["rc"] in (0, -1), k                         # CLV_ERR_INVALID: every refusal here is an argument check
        assert v["error"] is None or v["error"].startswith(k.split(":")[0] + ": "), k


def test_every_call_returns_the_recorded_code_and_leaves_the_recorded_message(lib, golden):
    launches = lib.clv_mvm_batch_launches()
    wrong = {k: (got, golden["calls"][k]) for k, (fn, kw) in TABLE.items() if (got := outcome(lib, fn, kw)) != golden["calls"][k]}
    assert not wrong, wrong
    assert lib.clv_mvm_batch_launches() == launches


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    import subprocess
    root = Path(__file__).resolve().parent.parent
    head = subprocess.run(["git", "-C", str(root), "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    L = load_library()
    calls = {k: outcome(L, fn, kw) for k, (fn, kw) in TABLE.items()}
    assert all(v["rc"] in (0, -1) for v in calls.values()), "a call of the table passed validation and was not empty"
    GOLDEN.write_text(json.dumps({"recorded_at_commit": head, "calls": calls}, indent=1) + "\n")
    print(f"{len(TABLE)} calls recorded at {head}")
