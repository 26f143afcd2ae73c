"""clv_f16_threshold_batch (include/clover_hip_batch_f16.h) on the GPU: CloverVector16::threshold(k) on several vectors, FAST up to one
workgroup's 32768 elements in one launch per 64 vectors.  Each vector equals clv_f16_threshold_mode on it, bit for bit, in both modes; the
padding behind n stays as it was.  The reference side is the single call that existed before (and, at the small sizes, the lowest-index
rule stated in Python and the restatement's heap walk)."""
import ctypes as C
import os

import numpy as np
import pytest

from clover_amd.lib_binding import THRESHOLD_FAST, THRESHOLD_REFERENCE
from f16_batch_helpers import THRESH_KINDS, _threshold_vector
from half16_helpers import pad128, rh  # noqa: F401
from test_half16 import lowest_index_threshold

# every W of the one-workgroup kernel, odd n, n < n_pad; the last n_pad is beyond one workgroup: forwarded to the single calls
THRESH_N = [1, 127, 128, 129, 2048, 8191, 8192, 32767, 32768, 32896 - 37]
NVECS = [1, 2, 64, 65]                       # one vector (the single call), one group, a full group, a group and a remainder
C_VP = C.c_void_p


def _ks(kind, mode, n):
    """FAST: 0, 1, n / 4 and n - 1 on the random vectors, n / 4 on the others.  REFERENCE is the heap walk of the single call, vector after
    vector, whose time grows with k: one k of at most 64 (the walk of 65 vectors of 32768 elements stays within a second)"""
    if mode == THRESHOLD_REFERENCE:
        return [min(n // 4, 64)]
    return sorted({0, 1, n // 4, n - 1}) if kind == "random" else [n // 4]


def _vectors(kind, n, n_pad, count):
    """`count` vectors of the kind that differ from one another: rotations of the kind's vector within its first n elements"""
    h = _threshold_vector(kind, n, n_pad)
    out = []
    for j in range(count):
        v = h.copy()
        v[:n] = np.roll(h[:n], 3 * j)
        out.append(v)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", THRESH_N)
def test_gpu_threshold_batch_equals_the_single_call_per_vector(hip, rh, n):  # noqa: F811
    n_pad = pad128(n)
    L = hip.lib
    for kind in THRESH_KINDS:
        hs = _vectors(kind, n, n_pad, max(NVECS))
        bufs = [hip.to_device(h) for h in hs]
        for mode in (THRESHOLD_FAST, THRESHOLD_REFERENCE):
            for k in _ks(kind, mode, n):
                # the single call on every vector, once per (kind, mode, k)
                want = []
                for b, h in zip(bufs, hs):
                    b.upload(h)
                    hip.check(L.clv_f16_threshold_mode(b.ptr, n, n_pad, k, mode, None, None))
                    want.append(b.download(np.uint16, n_pad))
                if n <= 8192:
                    cpu = lowest_index_threshold(hs[0], n, k) if mode == THRESHOLD_FAST else rh.threshold(hs[0], n, k)
                    assert np.array_equal(want[0], cpu), (kind, mode, k)
                for nvec in NVECS:
                    for b, h in zip(bufs[:nvec], hs):
                        b.upload(h)
                    hip.check(L.clv_f16_threshold_batch((C_VP * nvec)(*[b.ptr for b in bufs[:nvec]]), nvec, n, n_pad, k, mode, None))
                    for j in range(nvec):
                        got = bufs[j].download(np.uint16, n_pad)
                        assert np.array_equal(got, want[j]), (kind, mode, k, nvec, j, np.flatnonzero(got != want[j])[:8])
                        assert np.array_equal(got[n:], hs[j][n:]), "the padding was touched"


@pytest.mark.gpu
def test_gpu_threshold_batch_follows_the_single_calls_switch_and_the_binding(hip):
    """CLV_F16_THRESHOLD_SMALL=0 keeps the single calls on the large-vector path: the batch forwards to them and gives the same bits;
    CloverHip.f16_threshold_batch takes lists"""
    n, n_pad = 1000, 1024
    hs = _vectors("ties", n, n_pad, 5)
    want = [lowest_index_threshold(h, n, n // 4) for h in hs]
    got = hip.f16_threshold_batch(hs, n, n // 4)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    os.environ["CLV_F16_THRESHOLD_SMALL"] = "0"
    try:
        got = hip.f16_threshold_batch(hs, n, n // 4)
    finally:
        os.environ.pop("CLV_F16_THRESHOLD_SMALL", None)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
