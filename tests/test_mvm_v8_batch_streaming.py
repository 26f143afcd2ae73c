"""The nontemporal (NT = true) instantiations of k_m4_mvm8_batch (clover_amd/csrc/mvm_batch8.hip), each launched once and compared, whole
result, with the scalar oracle (oracle.m4_mvm_v8 / oracle.v8_scale_and_add run in stream order on one generator) -- not with a device
kernel.  launch_mvm8_batch picks them by the rule of launch_mvm8: rows cols / 2 > T = 256 MiB; every case asserts that predicate on its
shape, so a shape that stops selecting the streaming form fails instead of passing on the cached kernel.

- k_m4_mvm8_batch<2, U, true, false, false>, <4, ...>, <8, ...>: test_m4_mvm_v8_batch_streaming[plain-deterministic-g] g = 2, 3, 8
- k_m4_mvm8_batch<NV, U, true, true, false>: test_m4_mvm_v8_batch_streaming[fused-deterministic-g]
- k_m4_mvm8_batch<NV, U, true, false, true>: test_m4_mvm_v8_batch_streaming[plain-generator-g]
- k_m4_mvm8_batch<NV, U, true, true, true>: test_m4_mvm_v8_batch_streaming[fused-generator-g]

The matrix is the 192 x 2 796 288 one of test_streaming_instantiations.py (3 row groups, rows no multiple of 128, 268 443 648 bytes, 682
full LDS chunks of MVMB8_CHUNK columns and a ragged one), filled on the device and downloaded once."""
import numpy as np
import pytest

from matrix8_helpers import binade_scales, full_range_bytes
from test_mvm_batch import batch_kernel, pa
from test_mvm_v8_batch import CHUNK, eq, get8, pairs8
from test_streaming_instantiations import A_FUSED, COLS, KEYS, NVEC, ROWS, T, keys_equal

pytestmark = pytest.mark.gpu


class Shared:
    def __init__(self, hip):
        L = hip.lib
        self.dA, self.dsA = hip.alloc(ROWS * COLS // 2), hip.alloc((ROWS // 64) * (COLS // 64) * 4)
        hip.check(L.clv_fill_random_nibbles(self.dA.ptr, self.dA.nbytes, 0x57, 0, None))
        hip.check(L.clv_fill_random_scales(self.dsA.ptr, self.dsA.nbytes // 4, 0x58, 0, None))
        self.qA, self.sA = self.dA.download(np.uint8), self.dsA.download(np.float32)
        rng = np.random.default_rng(COLS + 8)
        self.x = [(full_range_bytes(rng, COLS), binade_scales(rng, COLS // 64, -4, 4)) for _ in range(NVEC)]
        self.u = [(full_range_bytes(rng, ROWS), binade_scales(rng, ROWS // 64, -4, 4)) for _ in range(NVEC)]
        self.x[0][0][[5, COLS - 1]] = [-128, 127]
        self.dx = [(hip.to_device(q), hip.to_device(s)) for q, s in self.x]
        self.du = [(hip.to_device(q), hip.to_device(s)) for q, s in self.u]
        self._seq = {}

    def sequence(self, oracle, fused, generator):
        """the oracle's results for the NVEC vectors in stream order on ONE generator (what the batch call and the sequence of single
        calls both give), as [(t, r or None, keys after the vector or None)]; computed once"""
        key = (fused, generator)
        if key not in self._seq:
            o = oracle.rng(*KEYS) if generator else None
            ts = [v[0] for v in self._seq[(False, False)]] if not generator and (False, False) in self._seq else None
            out = []
            for j in range(NVEC):
                t = ts[j] if ts else oracle.m4_mvm_v8(self.qA, self.sA, ROWS, COLS, *self.x[j], o)
                r = oracle.v8_scale_and_add(*self.u[j], *t, A_FUSED, o) if fused else None
                out.append((t, r, oracle.rng_keys(o) if generator else None))
            self._seq[key] = out
        return self._seq[key]


@pytest.fixture(scope="module")
def shared(hip):
    assert ROWS * (COLS // 2) > T and ROWS % 128 == 64 and COLS % CHUNK != 0
    s = Shared(hip)
    yield s
    del s


@pytest.mark.parametrize("g", [2, 3, 8])
@pytest.mark.parametrize("generator", [False, True], ids=["deterministic", "generator"])
@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
def test_m4_mvm_v8_batch_streaming(hip, oracle, shared, fused, generator, g):
    """groups of 2, 3 and 8 vectors run as NV = 2, 4 and 8 (CLV_MVM_BATCH=1: the batched kernel whatever the measured rule says); every
    vector against the oracle's sequence, and the state left behind"""
    assert ROWS * (COLS // 2) > T
    L = hip.lib
    want = shared.sequence(oracle, fused, generator)
    st = hip.new_rng(*KEYS) if generator else None
    x, sx = pa([d[0] for d in shared.dx[:g]]), pa([d[1] for d in shared.dx[:g]])
    t = pairs8(hip, g, ROWS)
    launches = L.clv_mvm_batch_launches()
    with batch_kernel("1"):
        if fused:
            r = pairs8(hip, g, ROWS)
            hip.check(L.clm4_mvm_v8_scale_and_add_batch(shared.dA.ptr, shared.dsA.ptr, ROWS, COLS, g, x, sx, pa([d[0] for d in shared.du[:g]]),
                                                        pa([d[1] for d in shared.du[:g]]), A_FUSED, pa([d[0] for d in t]), pa([d[1] for d in t]),
                                                        pa([d[0] for d in r]), pa([d[1] for d in r]), st.ptr if st else None, None))
        else:
            hip.check(L.clm4_mvm_v8_batch(shared.dA.ptr, shared.dsA.ptr, ROWS, COLS, g, x, sx, pa([d[0] for d in t]), pa([d[1] for d in t]),
                                          st.ptr if st else None, None))
    hip.sync()
    assert L.clv_mvm_batch_launches() - launches == 1
    for j in range(g):
        assert eq(get8(t[j], ROWS), want[j][0]), f"A x of vector {j}"
        if fused:
            assert eq(get8(r[j], ROWS), want[j][1]), f"r of vector {j}"
            assert eq(get8(shared.du[j], ROWS), shared.u[j]), f"u of vector {j} was written"
    assert np.any(want[0][0][0]) and not eq(want[0][0], want[1][0])
    if generator:
        assert keys_equal(hip, st, want[g - 1][2])
