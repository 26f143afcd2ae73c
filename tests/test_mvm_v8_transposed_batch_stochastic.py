"""The batched transposed mixed calls (CloverMatrix4 x CloverVector8) WITH a generator on the GPU: k_m4_mvm8_t_batch<., ., ., ., ST = true>
(clover_amd/csrc/mvm_t8_batch.hip) reads the matrix once for a group of vectors and places every vector's draws where the sequence of
single calls has them.

The reference side is never the new kernel.  It is (a) the CPU oracle run in stream order with ONE OrcRng on the stored transpose --
oracle.m4_mvm_v8(At, ..., rng), then oracle.v8_scale_and_add(..., rng) per vector -- with Oracle.rng_keys for the state, and (b) the single
device calls clm4_mvm_v8_transposed / clm4_mvm_v8_transposed_scale_and_add on one device state.  For clm4_mvm_v8_transposed_batch_at the generator
is moved to a vector's window on the test side (test_mvm_batch_stochastic.moved) and loaded into a device state with clv_rng_set.

Shapes (mvm_v8_transposed_batch_data.py; G = cols / 64 output blocks): the small ones plus the chunk shapes (C - 128, C, C + 128, 2 C + 128 rows and the
odd three-workgroup one: the re-staging barriers beside the generator starts and raw draws in LDS).  nvec: 2; 3 and 5 (masked slots);
8; 9 and 17 (the state is handed from launch to launch; forced, the remainder of one runs on the batched kernel too)."""
import numpy as np
import pytest

from mvm_v8_transposed_batch_data import A_FUSED, C_, CHUNKY, FIRST4, KEYS, NVMAX, SMALL, dev, eq
from oracle.binding import Oracle
from test_m8_mvm_batch import get8, pairs8
from test_mvm_v8_transposed_batch import fused_batch, mvm_batch
from test_mvm_batch import batch_kernel, pa
from test_mvm_batch_stochastic import keys_equal, moved, orng_at, set_state

pytestmark = pytest.mark.gpu

SHAPES = SMALL + CHUNKY
NVECS = (2, 3, 5, 8, 9, 17)
AT_SHAPES = FIRST4[:3] + [SMALL[-1], (C_ + 128, 128)]


class Stochastic:
    """per shape, once: the CPU sequence and the single device calls for NVMAX vectors from KEYS, plain and fused, with the state after
    every vector"""

    def __init__(self, hip, oracle, rows, cols):
        L = hip.lib
        S = self.S = dev(hip, oracle, rows, cols)
        D = S.D
        self.fresh = Oracle.rng_keys(oracle.rng(*KEYS))
        o = oracle.rng(*KEYS)
        self.o_mvm, self.o_mvm_keys = [], []
        for x in D.x:
            self.o_mvm.append(oracle.m4_mvm_v8(*D.At, cols, rows, *x, o))
            self.o_mvm_keys.append(Oracle.rng_keys(o))
        o = oracle.rng(*KEYS)
        self.o_t, self.o_r, self.o_fused_keys = [], [], []
        for x, u in zip(D.x, D.u):
            t = oracle.m4_mvm_v8(*D.At, cols, rows, *x, o)
            self.o_t.append(t)
            self.o_r.append(oracle.v8_scale_and_add(*u, *t, A_FUSED, o))
            self.o_fused_keys.append(Oracle.rng_keys(o))
        st, out = hip.new_rng(*KEYS), pairs8(hip, NVMAX, cols)
        self.d_mvm_keys = []
        for (dq, ds), (r, sr) in zip(S.dx, out):
            hip.check(L.clm4_mvm_v8_transposed(S.dA.ptr, S.dsA.ptr, rows, cols, dq.ptr, ds.ptr, r.ptr, sr.ptr, st.ptr, None))
            self.d_mvm_keys.append(hip.rng_get(st))
        self.d_mvm = [get8(p, cols) for p in out]
        st, t, r = hip.new_rng(*KEYS), pairs8(hip, NVMAX, cols), pairs8(hip, NVMAX, cols)
        self.d_fused_keys = []
        for j in range(NVMAX):
            hip.check(L.clm4_mvm_v8_transposed_scale_and_add(S.dA.ptr, S.dsA.ptr, rows, cols, S.dx[j][0].ptr, S.dx[j][1].ptr, S.du[j][0].ptr,
                                                          S.du[j][1].ptr, A_FUSED, t[j][0].ptr, t[j][1].ptr, r[j][0].ptr, r[j][1].ptr, st.ptr, None))
            self.d_fused_keys.append(hip.rng_get(st))
        self.d_t, self.d_r = [get8(p, cols) for p in t], [get8(p, cols) for p in r]
        assert not eq(self.o_mvm[0], D.t(0)), "the noise changed nothing: the comparison shows less than it should"


_st = {}


def stochastic(hip, oracle, rows, cols):
    if (rows, cols) not in _st:
        _st[(rows, cols)] = Stochastic(hip, oracle, rows, cols)
    return _st[(rows, cols)]


CONTIG = [(r, c, nv, "1") for r, c in SHAPES for nv in NVECS] + [(r, c, nv, None) for r, c in FIRST4[:2] for nv in NVECS]


# ---------------------------------------------------------------- contiguous windows
@pytest.mark.parametrize("rows,cols,nvec,force", CONTIG)
def test_the_stochastic_batch_equals_the_cpu_sequence_and_the_single_calls(hip, oracle, rows, cols, nvec, force):
    T = stochastic(hip, oracle, rows, cols)
    st = hip.new_rng(*KEYS)
    before = hip.lib.clv_mvm_batch_launches()
    with batch_kernel(force):
        got = mvm_batch(hip, T.S, nvec, rng=st)
    if force:
        assert hip.lib.clv_mvm_batch_launches() - before == (nvec + 7) // 8, "forced, a remainder of one runs batched too"
    for j in range(nvec):
        assert eq(T.d_mvm[j], T.o_mvm[j]), f"clm4_mvm_v8_transposed itself differs from the CPU sequence, vector {j}"
        assert eq(got[j], T.o_mvm[j]), f"vector {j} differs from the CPU sequence"
        assert eq(got[j], T.d_mvm[j]), f"vector {j} differs from the single calls"
    keys = hip.rng_get(st)
    assert keys_equal(keys, T.o_mvm_keys[nvec - 1]), "the state left behind differs from the oracle generator's"
    assert keys_equal(keys, T.d_mvm_keys[nvec - 1]), "the state left behind differs from the single calls'"
    assert not keys_equal(keys, T.fresh)


@pytest.mark.parametrize("rows,cols,nvec,force", CONTIG)
def test_the_stochastic_fused_batch_equals_the_cpu_sequence_and_the_single_calls(hip, oracle, rows, cols, nvec, force):
    """t stored, t not stored, in place: r is the same in all three"""
    T = stochastic(hip, oracle, rows, cols)
    D = T.S.D
    for with_t, in_place in ((True, False), (False, False), (True, True)):
        st = hip.new_rng(*KEYS)
        with batch_kernel(force):
            r, t, u = fused_batch(hip, T.S, nvec, A_FUSED, with_t, in_place, rng=st)
        what = f"t={with_t} in_place={in_place}"
        for j in range(nvec):
            assert eq(r[j], T.o_r[j]), f"{what}: r of vector {j} against the CPU sequence"
            assert eq(r[j], T.d_r[j]), f"{what}: r of vector {j} against the single calls"
            if with_t:
                assert eq(t[j], T.o_t[j]) and eq(t[j], T.d_t[j]), f"{what}: t of vector {j}"
            if not in_place:
                assert eq(u[j], D.u[j]), f"{what}: u of vector {j} was written"
        keys = hip.rng_get(st)
        assert keys_equal(keys, T.o_fused_keys[nvec - 1]) and keys_equal(keys, T.d_fused_keys[nvec - 1]), f"{what}: the state left behind"


def test_the_stochastic_batch_equals_the_held_batch_on_the_stored_transpose(hip, oracle):
    """clm4_mvm_v8_batch on clm4_transpose(A) with the same keys: the same bytes, the same state, across a group boundary"""
    rows, cols, nvec = 384, 640, 9
    T = stochastic(hip, oracle, rows, cols)
    S = T.S
    st, held = hip.new_rng(*KEYS), pairs8(hip, nvec, cols)
    with batch_kernel("1"):
        hip.check(hip.lib.clm4_mvm_v8_batch(S.dAt[0].ptr, S.dAt[1].ptr, cols, rows, nvec, *S.xs(nvec), pa([o[0] for o in held]),
                                         pa([o[1] for o in held]), st.ptr, None))
    hip.sync()
    for j in range(nvec):
        assert eq(get8(held[j], cols), T.d_mvm[j]), j
    assert keys_equal(hip.rng_get(st), T.d_mvm_keys[nvec - 1])


# ---------------------------------------------------------------- clm4_mvm_v8_transposed_batch_at
def at_call(hip, T, nvec, st, base, stride, commit):
    S = T.S
    D = S.D
    out = pairs8(hip, nvec, D.cols)
    rc = hip.lib.clm4_mvm_v8_transposed_batch_at(S.dA.ptr, S.dsA.ptr, D.rows, D.cols, nvec, *S.xs(nvec), pa([o[0] for o in out]),
                                              pa([o[1] for o in out]), st.ptr if st else None, base, stride, commit, None)
    return rc, out


@pytest.mark.parametrize("rows,cols", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("nvec", NVECS)
def test_batch_at_with_the_windows_of_the_contiguous_call_is_the_contiguous_call(hip, oracle, rows, cols, nvec):
    T = stochastic(hip, oracle, rows, cols)
    G = cols // 64
    st = hip.new_rng(*KEYS)
    with batch_kernel("1"):
        rc, out = at_call(hip, T, nvec, st, 0, 2 * G, nvec * 2 * G)
    hip.check(rc)
    hip.sync()
    for j in range(nvec):
        assert eq(get8(out[j], cols), T.o_mvm[j]) and eq(get8(out[j], cols), T.d_mvm[j]), j
    assert keys_equal(hip.rng_get(st), T.o_mvm_keys[nvec - 1])


def windows(G):
    """(base, stride, commit): every vector on the same draws and the state untouched; odd positions, overlapping windows and a commit
    unrelated to them; windows away from where single calls would draw with the state left untouched; bases that need the table rounds of
    the jump-ahead beyond 8 and beyond 16 bits, up to bit 54"""
    return [(0, 0, 0), (7, 3, 5), (7, 2 * G + 3, 0), ((1 << 33) + 12345, 2 * G, (1 << 20) + 1), (1 << 54, 1, (1 << 54) + 3)]


@pytest.mark.parametrize("rows,cols,force", [(r, c, "1") for r, c in AT_SHAPES] + [(r, c, None) for r, c in AT_SHAPES[:2]] + [(256, 128, "0")])
@pytest.mark.parametrize("nvec", [1, 3, 9])
def test_batch_at_places_every_window_where_it_is_told(hip, oracle, rows, cols, nvec, force):
    """vector j against the CPU and against clm4_mvm_v8_transposed, each on a generator moved to base + j * stride on the test side; the
    state afterwards is the initial one moved by commit (untouched for commit 0).  nvec = 1 with a non-zero base is among them, nvec = 9
    crosses a group.  CLV_MVM_BATCH=0 changes nothing: the positioned call always runs the batched kernel."""
    T = stochastic(hip, oracle, rows, cols)
    S, L = T.S, hip.lib
    D = S.D
    for base, stride, commit in windows(cols // 64):
        st = hip.new_rng(*KEYS)
        before = L.clv_mvm_batch_launches()
        with batch_kernel(force):
            rc, out = at_call(hip, T, nvec, st, base, stride, commit)
        hip.check(rc)
        hip.sync()
        assert L.clv_mvm_batch_launches() - before == (nvec + 7) // 8, "the positioned call did not run the batched kernel"
        what = f"(base, stride, commit) = ({base}, {stride}, {commit})"
        assert keys_equal(hip.rng_get(st), moved(oracle, T.fresh, commit)), f"{what}: the state left behind"
        one, single = hip.new_rng(*KEYS), pairs8(hip, 1, cols)[0]
        for j in range(nvec):
            at = moved(oracle, T.fresh, base + j * stride)
            want = oracle.m4_mvm_v8(*D.At, cols, rows, *D.x[j], orng_at(at))
            set_state(hip, one, at)
            hip.check(L.clm4_mvm_v8_transposed(S.dA.ptr, S.dsA.ptr, rows, cols, S.dx[j][0].ptr, S.dx[j][1].ptr, single[0].ptr, single[1].ptr, one.ptr,
                                            None))
            hip.sync()
            got = get8(out[j], cols)
            assert eq(got, want), f"{what}: vector {j} against the CPU at its window"
            assert eq(got, get8(single, cols)), f"{what}: vector {j} against clm4_mvm_v8_transposed at its window"
            if (base, stride) == (0, 0):
                assert eq(got, T.o_mvm[0]) or j, "stride 0: vector 0 is the first single call from the fresh state"


def test_batch_at_without_a_generator_is_the_deterministic_call_and_a_position_beyond_the_tables_is_refused(hip, oracle):
    rows, cols, nvec = 256, 128, 5
    T = stochastic(hip, oracle, rows, cols)
    with batch_kernel("1"):
        rc, out = at_call(hip, T, nvec, None, 1 << 60, 1 << 60, 1 << 60)      # ignored without an rng
    hip.check(rc)
    hip.sync()
    for j in range(nvec):
        assert eq(get8(out[j], cols), T.S.single[j]), j
    st = hip.new_rng(*KEYS)
    before = hip.lib.clv_mvm_batch_launches()
    for base, stride, commit in (((1 << 55) - 3, 0, 0), (0, 1 << 53, 0), (0, 6, 1 << 55), ((1 << 64) - 1, (1 << 64) - 1, 0)):
        rc, out = at_call(hip, T, nvec, st, base, stride, commit)
        assert rc == -1 and b"clm4_mvm_v8_transposed_batch_at" in hip.lib.clv_last_error() and b"2^55" in hip.lib.clv_last_error(), (base, stride, commit)
        hip.sync()
        assert all(np.all(get8(o, cols)[0] == 0x5A) for o in out), "a refused call wrote a result"
    assert hip.lib.clv_mvm_batch_launches() == before, "a refused call launched"
    assert keys_equal(hip.rng_get(st), T.fresh)
