"""The nontemporal (NT = true) instantiations of k_m8_mvm_batch (clover_amd/csrc/matrix8_batch.hip), each launched once and compared, whole
result, with the OpenMP build of the CPU restatement (m8p.mvm, then oracle.v8_scale_and_add, in stream order on one generator) -- not with
a device kernel.  launch_m8_batch picks them by the rule of clm8_mvm: rows cols > T = 256 MiB; every case asserts that predicate on its
shape, so a shape that stops selecting the streaming form fails instead of passing on the cached kernel.

- k_m8_mvm_batch<2, U, true, false, false>, <8, ...>: test_m8_mvm_batch_streaming[plain-deterministic-g] g = 2, 8
- k_m8_mvm_batch<NV, U, true, true, false>: test_m8_mvm_batch_streaming[fused-deterministic-g]
- k_m8_mvm_batch<NV, U, true, false, true>: test_m8_mvm_batch_streaming[plain-generator-g]
- k_m8_mvm_batch<NV, U, true, true, true>: test_m8_mvm_batch_streaming[fused-generator-g]

The matrix is 128 x (2^21 + 128): 268 451 840 bytes, just above the rule, two row groups, 512 full LDS chunks of M8B_CHUNK columns and a
ragged one of two blocks.  It is made and uploaded once."""
import numpy as np
import pytest

from matrix8_helpers import binade_scales, full_range_bytes, m8p  # noqa: F401
from test_m8_mvm_batch import CHUNK, eq, get8, pairs8
from test_mvm_batch import batch_kernel, pa
from test_streaming_instantiations import A_FUSED, KEYS, T, keys_equal

pytestmark = pytest.mark.gpu
ROWS, COLS, NVEC = 128, (1 << 21) + 128, 8


class Shared:
    def __init__(self, hip):
        rng = np.random.default_rng(COLS + 88)
        self.qA, self.sA = full_range_bytes(rng, ROWS * COLS), binade_scales(rng, (ROWS // 64) * (COLS // 64), -4, 4)
        self.qA[[7, ROWS * COLS - 1]] = [127, -127]
        self.dA, self.dsA = hip.to_device(self.qA), hip.to_device(self.sA)
        self.x = [(full_range_bytes(rng, COLS), binade_scales(rng, COLS // 64, -4, 4)) for _ in range(NVEC)]
        self.u = [(full_range_bytes(rng, ROWS), binade_scales(rng, ROWS // 64, -4, 4)) for _ in range(NVEC)]
        self.x[0][0][[5, COLS - 1]] = [-127, 127]
        self.dx = [(hip.to_device(q), hip.to_device(s)) for q, s in self.x]
        self.du = [(hip.to_device(q), hip.to_device(s)) for q, s in self.u]
        self._seq = {}

    def sequence(self, cpu, oracle, fused, generator):
        """the CPU results for the NVEC vectors in stream order on ONE generator (what the batch call and the sequence of single calls
        both give), as [(t, r or None, keys after the vector or None)]; computed once"""
        key = (fused, generator)
        if key not in self._seq:
            o = oracle.rng(*KEYS) if generator else None
            ts = [v[0] for v in self._seq[(not fused, False)]] if not generator and (not fused, False) in self._seq else None
            out = []
            for j in range(NVEC):
                t = ts[j] if ts else cpu.mvm(self.qA, self.sA, ROWS, COLS, *self.x[j], o)
                r = oracle.v8_scale_and_add(*self.u[j], *t, A_FUSED, o) if fused else None
                out.append((t, r, oracle.rng_keys(o) if generator else None))
            self._seq[key] = out
        return self._seq[key]


@pytest.fixture(scope="module")
def shared(hip):
    assert ROWS * COLS > T and COLS % CHUNK != 0
    s = Shared(hip)
    yield s
    del s


@pytest.mark.parametrize("g", [2, 8])
@pytest.mark.parametrize("generator", [False, True], ids=["deterministic", "generator"])
@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
def test_m8_mvm_batch_streaming(hip, oracle, m8p, shared, fused, generator, g):  # noqa: F811
    """groups of 2 and 8 vectors run as NV = 2 and 8 (CLV_MVM_BATCH=1: the batched kernel whatever the measured rule says); every vector
    against the CPU sequence, and the state left behind"""
    assert ROWS * COLS > T, "the launcher's predicate: this shape must select the nontemporal kernel"
    assert ROWS * COLS == 268451840
    L = hip.lib
    want = shared.sequence(m8p, oracle, fused, generator)
    st = hip.new_rng(*KEYS) if generator else None
    x, sx = pa([d[0] for d in shared.dx[:g]]), pa([d[1] for d in shared.dx[:g]])
    t = pairs8(hip, g, ROWS)
    launches = L.clv_mvm_batch_launches()
    with batch_kernel("1"):
        if fused:
            r = pairs8(hip, g, ROWS)
            hip.check(L.clm8_mvm_scale_and_add_batch(shared.dA.ptr, shared.dsA.ptr, ROWS, COLS, g, x, sx, pa([d[0] for d in shared.du[:g]]),
                                                     pa([d[1] for d in shared.du[:g]]), A_FUSED, pa([d[0] for d in t]), pa([d[1] for d in t]),
                                                     pa([d[0] for d in r]), pa([d[1] for d in r]), st.ptr if st else None, None))
        else:
            hip.check(L.clm8_mvm_batch(shared.dA.ptr, shared.dsA.ptr, ROWS, COLS, g, x, sx, pa([d[0] for d in t]), pa([d[1] for d in t]),
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
