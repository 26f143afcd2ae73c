"""The argument checks, early returns and workspace sizes of the threshold entries of all four element widths, as one table, without a GPU.
Every row is a call that never reaches a launch: a rejected argument (CLV_ERR_INVALID and the complete clv_last_error() text, under the
name it is reported with), or a call with nothing to do (CLV_OK).  Rows that break two adjacent checks at once pin the order in which the
checks fire.  The pointers are small integers that are never dereferenced; the pointer arrays of the batch calls are HOST arrays.  Texts and
byte counts were recorded from the library as it was before the host side of threshold4.hip became one driver; the table passes on both."""
import pytest

from clover_amd.lib_binding import load_library
from test_mvm_batch_cpu import addr, arr

Q, S, HEAP, WS, Q2, S2 = (addr(i) for i in range(2, 8))          # 16-byte aligned, 1 MiB apart
T32 = 1 << 32
FAST, REFERENCE = 0, 1

# entry -> its parameters in call order with the defaults of a row: n = 100 of n_pad = 128 elements, k = 10 (a call that passed every check
# would launch, so every row below is rejected or has nothing to do)
SINGLE = dict(n=100, n_pad=128, k=10, ws=None, stream=None)
ENTRIES = {
    "clv4_threshold": dict(q=Q, s=S, **SINGLE),
    "clv8_threshold": dict(q=Q, s=S, **SINGLE),
    "clv4_threshold_mode": dict(q=Q, s=S, n=100, n_pad=128, k=10, mode=REFERENCE, ws=None, stream=None),
    "clv8_threshold_mode": dict(q=Q, s=S, n=100, n_pad=128, k=10, mode=REFERENCE, ws=None, stream=None),
    "clv4_threshold_heap": dict(q=Q, s=S, n=100, n_pad=128, k=10, heap=HEAP, ws=None, stream=None),
    "clv8_threshold_heap": dict(q=Q, s=S, n=100, n_pad=128, k=10, heap=HEAP, ws=None, stream=None),
    "clv4_threshold_batch": dict(q=(Q, Q2), s=(S, S2), nvec=2, n=100, n_pad=128, k=10, mode=FAST, stream=None),
    "clv8_threshold_batch": dict(q=(Q, Q2), s=(S, S2), nvec=2, n=100, n_pad=128, k=10, mode=FAST, stream=None),
    "clv_f16_threshold_mode": dict(q=Q, n=100, n_pad=128, k=10, mode=FAST, ws=None, stream=None),
    "clv_f16_threshold_heap": dict(q=Q, n=100, n_pad=128, k=10, heap=HEAP, ws=None, stream=None),
    "clv_f32_threshold_mode": dict(q=Q, n=100, n_pad=128, k=10, mode=FAST, ws=None, stream=None),
}

BAD_PAD = dict(n=100, n_pad=192)                       # n_pad % 128 != 0
TOO_LONG = dict(n=200, n_pad=128)                      # n > n_pad
HUGE = dict(n=T32, n_pad=T32)                          # n == 2^32
HUGE_AND_LONG = dict(n=2 * T32, n_pad=T32)             # both size rules: the n / n_pad text comes first
BAD_WS = dict(ws=WS + 8)
SIZES = "n=%d n_pad=%d"
NO_2_32 = "vectors of 2^32 or more elements are not supported"
WS_TEXT = "workspace must be 16-byte aligned"


def single_rows(entry, name, null_args, mode=None):
    """the rows every single-vector entry shares; `name`: what its errors are reported under; `mode`: the mode the rows run in"""
    m = {} if mode is None else dict(mode=mode)
    rows = [(entry, dict(m, **{a: None}), -1, f"{name}: null pointer") for a in null_args]
    rows += [
        (entry, dict(m, **BAD_PAD), -1, f"{name}: " + SIZES % (100, 192)),
        (entry, dict(m, **TOO_LONG), -1, f"{name}: " + SIZES % (200, 128)),
        (entry, dict(m, **HUGE), -1, f"{name}: {NO_2_32}"),
        (entry, dict(m, **BAD_WS), -1, f"{name}: {WS_TEXT}"),
        # two adjacent checks at once: the earlier one answers
        (entry, dict(m, **TOO_LONG, **{null_args[0]: None}), -1, f"{name}: null pointer"),
        (entry, dict(m, **HUGE_AND_LONG), -1, f"{name}: " + SIZES % (2 * T32, T32)),
    ]
    return rows


def plain_rows(entry):
    return single_rows(entry, entry, ("q", "s")) + [
        (entry, dict(**HUGE, **BAD_WS), -1, f"{entry}: {NO_2_32}"),
        (entry, dict(**TOO_LONG, **BAD_WS), -1, f"{entry}: " + SIZES % (200, 128)),
        (entry, dict(k=100), 0, None),                 # k >= n: everything survives
        (entry, dict(k=500), 0, None),
        (entry, dict(n=0, k=0), 0, None),
    ]


def mode48_rows(entry):
    """clv4/8_threshold_mode: FAST is the plain call before any check of this entry, errors under the plain name included"""
    plain = entry[:-len("_mode")]
    return single_rows(entry, plain, ("q", "s"), FAST) + single_rows(entry, entry, ("q", "s"), REFERENCE) + [
        (entry, dict(mode=7), -1, f"{entry}: unknown mode 7"),
        (entry, dict(mode=-1, q=None), -1, f"{entry}: unknown mode -1"),           # the mode before the pointers
        (entry, dict(mode=REFERENCE, **HUGE, **BAD_WS), -1, f"{entry}: {NO_2_32}"),
        (entry, dict(mode=FAST, **HUGE, **BAD_WS), -1, f"{plain}: {NO_2_32}"),
        (entry, dict(mode=REFERENCE, k=100), 0, None),                              # the early return comes before the mode is dispatched
        (entry, dict(mode=FAST, k=100), 0, None),
        (entry, dict(mode=REFERENCE, n=0, k=0), 0, None),
        (entry, dict(mode=FAST, n=0, k=0), 0, None),
    ]


def mode_rows(entry, aligned_x):
    """clv_f16 / clv_f32_threshold_mode: the mode first, then the pointer, (alignment of x,) sizes, workspace"""
    rows = single_rows(entry, entry, ("q",), FAST) + single_rows(entry, entry, ("q",), REFERENCE) + [
        (entry, dict(mode=5), -1, f"{entry}: unknown mode 5"),
        (entry, dict(mode=5, q=None), -1, f"{entry}: unknown mode 5"),
        (entry, dict(**HUGE, **BAD_WS), -1, f"{entry}: {NO_2_32}"),
        (entry, dict(mode=FAST, k=100), 0, None),
        (entry, dict(mode=REFERENCE, k=100), 0, None),                              # the early return comes before the mode is dispatched
        (entry, dict(mode=FAST, n=0, k=0), 0, None),
        (entry, dict(mode=REFERENCE, n=0, k=0), 0, None),
    ]
    if aligned_x:
        rows += [
            (entry, dict(q=Q + 4), -1, f"{entry}: x must be 16-byte aligned"),
            (entry, dict(q=Q + 8, mode=REFERENCE), -1, f"{entry}: x must be 16-byte aligned"),
            (entry, dict(q=Q + 4, **TOO_LONG), -1, f"{entry}: x must be 16-byte aligned"),      # alignment before the sizes
            (entry, dict(q=Q + 4, mode=5), -1, f"{entry}: unknown mode 5"),
        ]
    else:
        rows += [(entry, dict(q=Q + 2, k=100), 0, None)]                                        # no alignment rule of its own
    return rows


def heap_rows(entry, null_args):
    """1 <= k <= n, checked before the workspace; k == n is a real call, so no row here passes"""
    return single_rows(entry, entry, null_args) + [
        (entry, dict(k=0), -1, f"{entry}: k=0 must lie in 1 .. n=100"),
        (entry, dict(k=101), -1, f"{entry}: k=101 must lie in 1 .. n=100"),
        (entry, dict(k=0, **HUGE), -1, f"{entry}: {NO_2_32}"),
        (entry, dict(k=0, **BAD_WS), -1, f"{entry}: k=0 must lie in 1 .. n=100"),
        (entry, dict(n=0, k=0), -1, f"{entry}: k=0 must lie in 1 .. n=0"),
    ]


def batch_rows(entry, q_bytes):
    """mode, sizes, nvec == 0, the arrays, each element, the overlap check, k >= n; q_bytes: a vector's q at n_pad = 128"""
    return [
        (entry, dict(mode=7), -1, f"{entry}: unknown mode 7"),
        (entry, BAD_PAD, -1, f"{entry}: " + SIZES % (100, 192)),
        (entry, TOO_LONG, -1, f"{entry}: " + SIZES % (200, 128)),
        (entry, HUGE, -1, f"{entry}: {NO_2_32}"),
        (entry, dict(q=None), -1, f"{entry}: null pointer array"),
        (entry, dict(s=None), -1, f"{entry}: null pointer array"),
        (entry, dict(q=(Q, None)), -1, f"{entry}: null pointer in vector 1"),
        (entry, dict(s=(None, S2)), -1, f"{entry}: null pointer in vector 0"),
        (entry, dict(q=(Q, Q + q_bytes - 1)), -1, f"{entry}: output `q` of vector 1 overlaps output `q` of vector 0"),
        (entry, dict(s=(S, Q + 4)), -1, f"{entry}: input `s` of vector 1 overlaps output `q` of vector 0"),
        (entry, dict(q=(Q, S + 4)), -1, f"{entry}: output `q` of vector 1 overlaps input `s` of vector 0"),      # s is n_pad / 64 floats
        # two adjacent checks at once
        (entry, dict(mode=7, **TOO_LONG), -1, f"{entry}: unknown mode 7"),
        (entry, HUGE_AND_LONG, -1, f"{entry}: " + SIZES % (2 * T32, T32)),
        (entry, dict(nvec=0, q=None, s=None, **TOO_LONG), -1, f"{entry}: " + SIZES % (200, 128)),
        (entry, dict(nvec=0, q=None, s=None, mode=7), -1, f"{entry}: unknown mode 7"),
        (entry, dict(q=None, **HUGE), -1, f"{entry}: {NO_2_32}"),
        (entry, dict(q=None, s=(None, S2)), -1, f"{entry}: null pointer array"),
        (entry, dict(q=(Q, Q + q_bytes - 1), s=(None, S2)), -1, f"{entry}: null pointer in vector 0"),
        (entry, dict(q=(Q, Q + q_bytes - 1), k=100), -1, f"{entry}: output `q` of vector 1 overlaps output `q` of vector 0"),
        # nothing to do
        (entry, dict(nvec=0, q=None, s=None), 0, None),
        (entry, dict(nvec=0, q=None, s=None, mode=REFERENCE), 0, None),
        (entry, dict(k=100), 0, None),
        (entry, dict(k=100, mode=REFERENCE), 0, None),
        (entry, dict(n=0, k=0), 0, None),
        (entry, dict(k=100, q=(Q, Q + q_bytes)), 0, None),                          # back to back
        (entry, dict(k=100, s=(S, S)), 0, None),                                    # inputs may repeat
        (entry, dict(k=100, nvec=1, q=(Q,), s=(S,)), 0, None),
    ]


CALLS = (plain_rows("clv4_threshold") + plain_rows("clv8_threshold") + mode48_rows("clv4_threshold_mode") + mode48_rows("clv8_threshold_mode")
         + heap_rows("clv4_threshold_heap", ("q", "s", "heap")) + heap_rows("clv8_threshold_heap", ("q", "s", "heap"))
         + batch_rows("clv4_threshold_batch", 64) + batch_rows("clv8_threshold_batch", 128)
         + [("clv4_threshold_batch", dict(k=100, q=(Q, Q + 127)), 0, None),        # a CloverVector4 of 128 elements is 64 bytes, not 128
            ("clv8_threshold_batch", dict(q=(Q, Q + 64)), -1, "clv8_threshold_batch: output `q` of vector 1 overlaps output `q` of vector 0")]
         + mode_rows("clv_f16_threshold_mode", False) + heap_rows("clv_f16_threshold_heap", ("q", "heap"))
         + mode_rows("clv_f32_threshold_mode", True))

N_PADS = (128, 32768, 131072 + 128, 1 << 20, 1 << 28)
WORKSPACE_BYTES = {
    "clv4_threshold_workspace_bytes": (51992, 58112, 76568, 248832, 50449152),
    "clv8_threshold_workspace_bytes": (16900, 16912, 16964, 17408, 147968),
    "clv_f16_threshold_workspace_bytes": (16900, 16928, 17028, 17920, 279040),
    "clv_f32_threshold_workspace_bytes": (16900, 16960, 17156, 18944, 541184),
    "clv_threshold_reference_workspace_bytes": (1280, 397832, 1591560, 12714504, 3254780424),
}
# clv_threshold_reference_workspace_bytes_k at k = 1, 20000 (the largest heap that lives in LDS whole), 20001 and n_pad
REFERENCE_BYTES_K = {
    128: (1280, 1280, 1280, 1280),
    32768: (135680, 135680, 295696, 397832),
    131072 + 128: (541952, 541952, 701968, 1591560),
    1 << 20: (4325888, 4325888, 4485904, 12714504),
    1 << 28: (1107296768, 1107296768, 1107456784, 3254780424),
}


@pytest.fixture(scope="module")
def lib():
    return load_library()


def call(lib, entry, changes):
    args = dict(ENTRIES[entry], **changes)
    assert set(changes) <= set(ENTRIES[entry]), (entry, changes)
    return getattr(lib, entry)(*[arr(*v) if isinstance(v, tuple) else v for v in args.values()])


def test_the_table_covers_the_eleven_entries():
    assert {row[0] for row in CALLS} == set(ENTRIES) and len(ENTRIES) == 11
    for entry in ENTRIES:
        assert any(row[0] == entry and row[2] == -1 for row in CALLS)


def test_every_row_answers_as_recorded(lib):
    wrong = []
    for entry, changes, rc, text in CALLS:
        got = call(lib, entry, changes)
        msg = lib.clv_last_error().decode()
        if got != rc or (text is not None and msg != text):
            wrong.append((entry, changes, (got, msg), (rc, text)))
    assert not wrong, wrong


def test_a_call_with_nothing_to_do_leaves_the_last_error_alone(lib):
    assert call(lib, "clv4_threshold", dict(q=None)) == -1
    before = lib.clv_last_error()
    for entry, changes, rc, _ in CALLS:
        if rc == 0:
            assert call(lib, entry, changes) == 0 and lib.clv_last_error() == before, (entry, changes)


def test_workspace_sizes_are_what_they_were(lib):
    for name, want in WORKSPACE_BYTES.items():
        assert tuple(getattr(lib, name)(n_pad) for n_pad in N_PADS) == want, name
    for n_pad, want in REFERENCE_BYTES_K.items():
        got = tuple(lib.clv_threshold_reference_workspace_bytes_k(n_pad, k) for k in (1, 20000, 20001, n_pad))
        assert got == want, n_pad
        assert lib.clv_threshold_reference_workspace_bytes_k(n_pad, 2 * n_pad) == want[3]      # k counts up to n_pad
        assert lib.clv_threshold_reference_workspace_bytes(n_pad) == want[3]
