"""The forms of test_edge_bands_mvm.py once each WITH a generator, on the band grid of edge_band_data.py: the single fused call, the
batched mvm, the fused batch, the transposed call and its two batched forms, for the three operand pairs.

4-bit and mixed: against the oracle called with the same XORShift keys in the order of the single calls (per vector: the mvm's draws, then
the scaleAndAdd's), and the state left behind.  All three pairs: against the single calls on the device in order, state included.  Band T
is what matters here: the reference's k = inf makes every element 0 WHATEVER the noise, and k within 8 x of FLT_MAX (band E) times a
value plus noise must not leave the int32 range on the device where it does not in the reference."""
import numpy as np
import pytest

import edge_band_data as D
from edge_band_gpu import KEYS, NVECS_RNG, cases, devs, eq, fresh, groups, m8, oracle_state, read, ref, state  # noqa: F401  (cases, devs, m8, ref: fixtures)

pytestmark = pytest.mark.gpu

CASES = [(pair, out, in_) for pair in D.PAIRS for out, in_ in D.shapes_of(pair)]
A = 0.37
NVEC = max(NVECS_RNG)                              # the single calls run once, on all of them


def t_bands_are_zero(S, t):
    el = D.elements(D.VECTOR_BITS[S.c.pair], t[0]).reshape(-1, 64)
    rows = [i for i in range(S.out // 64) if D.BANDS[i % 8] == "T"]
    return rows and all(not el[i].any() and 0 < t[1][i] < D.FLT_MIN * 32 and t[1][i] != 1.0 for i in rows)


@pytest.mark.parametrize("transposed", [False, True], ids=["held", "transposed"])
@pytest.mark.parametrize("pair,out,in_", CASES)
def test_with_a_generator_every_form_draws_as_the_single_calls_do(hip, devs, ref, oracle, pair, out, in_, transposed):  # noqa: F811
    S = devs(pair, out, in_)
    c = S.c
    with_oracle = pair != "m8"
    unused = state(hip, hip.new_rng(*KEYS))

    # the sequence of single calls on one state: mvm per vector; then mvm + scale_and_add per vector; the state behind every vector
    st = hip.new_rng(*KEYS)
    outs = fresh(hip, S.abi, NVEC, out)
    mvm1_states = []
    for j in range(NVEC):
        S.call_mvm(transposed, S.x[j], outs[j], st)
        mvm1_states.append(state(hip, st))
    mvm1, mvm1_state = [read(S.abi, o, out) for o in outs], mvm1_states[-1]
    st = hip.new_rng(*KEYS)
    two, two_states = [], []
    for j in range(NVEC):
        two.append(S.two_calls(transposed, j, A, st))
        two_states.append(state(hip, st))
    two_state = two_states[-1]
    assert t_bands_are_zero(S, mvm1[0]), "band T with noise: every element 0, the subnormal maximum as the scale"
    assert not np.array_equal(mvm1_state, unused) and not eq(mvm1[0], c.t(0)), "the generator was not used"

    if with_oracle:
        o = oracle.rng(*KEYS)
        want = [ref.mvm(pair, c.B, out, in_, c.x[j], o) for j in range(NVEC)]
        for j in range(NVEC):
            assert eq(mvm1[j], want[j]), f"the single mvm with a generator, vector {j}, against the oracle"
        assert np.array_equal(mvm1_state, oracle_state(oracle, o))
        o = oracle.rng(*KEYS)
        for j in range(NVEC):
            wt = ref.mvm(pair, c.B, out, in_, c.x[j], o)
            wr = ref.scale_and_add(pair, c.u[j], wt, A, o)
            assert eq(two[j][1], wt) and eq(two[j][0], wr), f"mvm + scale_and_add with a generator, vector {j}, against the oracle"
        assert np.array_equal(two_state, oracle_state(oracle, o))

    # the single fused call, vector by vector on one state
    st = hip.new_rng(*KEYS)
    for j in range(NVEC):
        r, t, _ = S.fused(transposed, j, A, rng=st)
        assert eq(r, two[j][0]) and eq(t, two[j][1]), f"the single fused call, vector {j}"
    assert np.array_equal(state(hip, st), two_state), "the single fused calls: the state left behind"

    for nvec in NVECS_RNG:
        # the batched mvm
        st = hip.new_rng(*KEYS)
        got, launches = S.batch(transposed, nvec, rng=st)
        assert launches == groups(nvec, stochastic=True), f"nvec={nvec}: forced, with a generator every group runs batched, one vector too"
        for j in range(nvec):
            assert eq(got[j], mvm1[j]), f"the batched mvm of {nvec}, vector {j}"
        assert np.array_equal(state(hip, st), mvm1_states[nvec - 1]), f"the batched mvm of {nvec}: the state left behind"

        # the fused batch
        st = hip.new_rng(*KEYS)
        r, t, _, launches = S.fused_batch(transposed, nvec, A, rng=st)
        assert launches == groups(nvec, stochastic=True)
        for j in range(nvec):
            assert eq(r[j], two[j][0]) and eq(t[j], two[j][1]), f"the fused batch of {nvec}, vector {j}"
        assert np.array_equal(state(hip, st), two_states[nvec - 1]), f"the fused batch of {nvec}: the state left behind"
