"""Pins the oracle, the restatements and the HIP kernels on the REFERENCE's own container code.

tests/golden/ref_*.json are written by oracle/_ref/clover_ref_gen: the reference's include/Clover*.h compiled as they lie behind
oracle/ref_containers.cpp (declarations of Intel IPP / MKL from oracle/ref_shim/, no stand-in takes part in a value; recipe: `make -C oracle
ref-fixtures`).  tests/ref_fixture_cases.py holds the case list and the input formula.  A case's record is the SHA-256 of all its outputs
and, for stochastic rounding, of the generator lanes afterwards (a dot's four bytes are kept whole); a fixture file holds one SHA-256 per
group of cases -- one operation at one shape with one kind of rounding, over the data kinds -- plus one over the input bytes the generator
received and one over the quantised operands it derived from them with the reference's deterministic quantize.  A digest cannot say where
two results differ, so on a mismatch the test runs a second engine (the live reference build or the oracle) on the group and names the
case, the output and the first differing byte, and which of reference, oracle and HIP disagree.

CPU: every case through the restatement the GPU tests of that family use (oracle, fast_oracle where it has the call, tests/*_restate.c):
every output byte, scale bit and generator lane identical; where oracle/_ref/libclover_ref*.so is present the live reference build must
reproduce the fixtures too.  GPU: the same cases through the C ABI, compared with the fixture directly.

Not pinned, because the reference's method ends in an Intel call: every transpose, CloverMatrix32::mvm.  Not a
case: threshold(0), which the reference cannot run (it reads a heap it never allocated).  The loop calls clm4_iht / clm4_iht_v8 / clm8_iht
draw from ONE generator, the reference's loop from four (each mvm from its matrix, each scaleAndAdd from its vector), so the stochastic loop
fixtures are checked on the CPU only, where the oracle's steps are composed with four generators.  The FAST threshold, and with it the
persistent loop kernels, equal the reference only where the kept set is unique: they are compared on the (data, k) for which that holds,
among them the k of THRESHOLD_K_TIE_FREE and LOOP_K_TIE_FREE, which exist for that."""
import functools
import json
from pathlib import Path

import numpy as np
import pytest

import ref_fixture_cases as rc
from clover_amd.lib_binding import DOT_EXACT, DOT_FAST, THRESHOLD_FAST, THRESHOLD_REFERENCE
from fp32_helpers import fast_dot_bound, rf  # noqa: F401
from half16_helpers import rh  # noqa: F401
from matrix8_helpers import m8  # noqa: F401

ROOT = Path(__file__).resolve().parent.parent
MAX_REPORTED = 6


# ---------------------------------------------------------------------------------------------------------------- shared data
@functools.lru_cache(maxsize=None)
def _input(key):
    a = rc.make_input(json.loads(key))
    a.setflags(write=False)              # computed once, shared by every test, never changed
    return a


def inputs_of(c):
    return [_input(json.dumps(spec, sort_keys=True)) for spec in c["inputs"]]


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def bits_of(family):
    return {"v4": 4, "v8": 8, "v16": 16, "v32": 32, "m4": 4, "m8": 8, "m16": 16}[family]


def names(bits, vec):
    """blob names of a vector / matrix tuple: (q, s), (h,) or (x,)"""
    return dict(zip(("q", "s") if bits in (4, 8) else ("h",) if bits == 16 else ("x",), vec))


def zero_vec(bits, n):
    """what clear() leaves: zero values, scales of 1"""
    if bits == 4:
        return np.zeros(n // 2, np.uint8), np.ones(n // 64, np.float32)
    if bits == 8:
        return np.zeros(n, np.int8), np.ones(n // 64, np.float32)
    return (np.zeros(n, np.uint16),)


# ---------------------------------------------------------------------------------------------------------------- the three engines
class OracleEngine:
    """the restatements: oracle (4-bit, CloverVector8, mixed), tests/matrix8_restate.c, half16_restate.c, fp32_restate.cpp"""
    name = "oracle"

    def __init__(self, oracle, m8, rh, rf):
        self.o, self.m8, self.rh, self.rf = oracle, m8, rh, rf

    def rng(self, k1, k2):
        return self.o.rng(k1, k2)

    def state(self, r):
        return np.concatenate(self.o.rng_keys(r))

    def vq(self, bits, x, rng=None):
        return self.o.v4_quantize(x, rng) if bits == 4 else self.o.v8_quantize(x, rng) if bits == 8 else (self.rh.quantize(x),)

    def vrestore(self, bits, v):
        return self.o.v4_restore(*v) if bits == 4 else self.o.v8_restore(*v) if bits == 8 else self.rh.restore(*v)

    def vdot(self, bits, u, v):
        if bits == 4:
            return self.o.v4_dot(*u, *v)
        if bits == 8:
            return self.o.v8_dot(*u, *v)
        return self.rh.dot(*u, *v) if bits == 16 else self.rf.dot(*u, *v)

    def vsaa(self, bits, u, v, a, rng=None, in_place=False):
        if bits == 4:
            return self.o.v4_scale_and_add(*u, *v, a, rng)
        if bits == 8:
            return self.o.v8_scale_and_add(*u, *v, a, rng)
        return (self.rh.scale_and_add(*u, *v, a),) if bits == 16 else (self.rf.scale_and_add(*u, *v, a),)

    def vthr(self, bits, v, n, k):
        if bits == 4:
            return self.o.v4_threshold(*v, n, k)
        if bits == 8:
            return self.o.v8_threshold(*v, n, k)
        return self.rh.threshold(*v, n, k) if bits == 16 else self.rf.threshold(*v, n, k)

    def mq(self, bits, A, rng=None):
        return self.o.m4_quantize(A, rng) if bits == 4 else self.m8.quantize(A, rng) if bits == 8 else (self.rh.quantize(A).reshape(-1),)

    def mrestore(self, m, rows, cols):
        return self.m8.restore(*m, rows, cols)

    def mvm(self, mbits, xbits, m, rows, cols, x, rng=None):
        if xbits == 32:
            f = {4: self.o.m4_mvm_f32, 8: self.m8.mvm_f32, 16: self.rh.mvm_f32}[mbits]
            return (f(*m, rows, cols, *x),)
        if mbits == 16:
            return (self.rh.mvm(*m, rows, cols, *x),)
        f = self.m8.mvm if mbits == 8 else self.o.m4_mvm if xbits == 4 else self.o.m4_mvm_v8
        return f(*m, rows, cols, *x, rng)


class HipEngine:
    """the C ABI of include/clover_hip.h and clover_hip_fp32.h on the device; thresholds in REFERENCE mode, dots in EXACT mode"""
    name = "HIP"

    def __init__(self, hip):
        self.h = hip

    def rng(self, k1, k2):
        return self.h.new_rng(k1, k2)

    def state(self, r):
        return np.concatenate(self.h.rng_get(r))

    def vq(self, bits, x, rng=None):
        return self.h.v4_quantize(x, rng) if bits == 4 else self.h.v8_quantize(x, rng) if bits == 8 else (self.h.f16_quantize(x),)

    def vrestore(self, bits, v):
        return self.h.v4_restore(*v) if bits == 4 else self.h.v8_restore(*v) if bits == 8 else self.h.f16_restore(*v)

    def vdot(self, bits, u, v, mode=DOT_EXACT):
        if bits == 4:
            return self.h.v4_dot(*u, *v, mode)
        if bits == 8:
            return self.h.v8_dot(*u, *v, mode)
        return self.h.f16_dot(*u, *v, mode) if bits == 16 else self.h.f32_dot(*u, *v, mode)

    def vsaa(self, bits, u, v, a, rng=None, in_place=False):
        if bits == 4:
            return self.h.v4_scale_and_add(*u, *v, a, rng, in_place)
        if bits == 8:
            return self.h.v8_scale_and_add(*u, *v, a, rng, in_place)
        return (self.h.f16_scale_and_add(*u, *v, a, in_place),) if bits == 16 else (self.h.f32_scale_and_add(*u, *v, a, in_place=in_place),)

    def vthr(self, bits, v, n, k, mode=THRESHOLD_REFERENCE):
        if bits == 4:
            return self.h.v4_threshold(*v, n, k, mode)
        if bits == 8:
            return self.h.v8_threshold(*v, n, k, mode)
        return self.h.f16_threshold(*v, n, k, mode) if bits == 16 else self.h.f32_threshold(*v, n, k, mode)

    def mq(self, bits, A, rng=None):
        return self.h.m4_quantize(A, rng) if bits == 4 else self.h.m8_quantize(A, rng) if bits == 8 else (self.h.mf16_quantize(A),)

    def mrestore(self, m, rows, cols):
        return self.h.m8_restore(*m, rows, cols)

    def mvm(self, mbits, xbits, m, rows, cols, x, rng=None):
        if xbits == 32:
            f = {4: self.h.m4_mvm_f32, 8: self.h.m8_mvm_f32, 16: self.h.mf16_mvm_f32}[mbits]
            return (f(*m, rows, cols, *x),)
        if mbits == 16:
            return (self.h.mf16_mvm(*m, rows, cols, *x),)
        f = self.h.m8_mvm if mbits == 8 else self.h.m4_mvm if xbits == 4 else self.h.m4_mvm_v8
        return f(*m, rows, cols, *x, rng)


class RefEngine:
    """the live reference build (oracle/_ref): the regeneration check"""
    name = "live reference"

    def __init__(self):
        from oracle.binding import RefContainers, RefXorshift
        self.det, self.sto, self.xs = RefContainers(False), RefContainers(True), RefXorshift()

    def rng(self, k1, k2):
        return np.concatenate(self.xs.init(k1, k2))

    def state(self, r):
        return r

    def _lib(self, rng):
        return self.det if rng is None else self.sto

    @staticmethod
    def _vec(bits, n):
        if bits in (4, 8):
            return np.zeros(n // 2 if bits == 4 else n, np.int8), np.zeros(n // 64, np.float32)
        return (np.zeros(n, np.uint16 if bits == 16 else np.float32),)

    def vq(self, bits, x, rng=None):
        out = self._vec(bits, x.size)
        self._lib(rng).call(f"v{bits}_quantize", np.ascontiguousarray(x), x.size, *out, *(() if bits == 16 else (rng,)))
        return out

    def vrestore(self, bits, v):
        n = v[0].size * (2 if bits == 4 else 1)
        x = np.zeros(n, np.float32)
        self.det.call(f"v{bits}_restore", *v, n, x)
        return x

    def vdot(self, bits, u, v):
        n = u[0].size * (2 if bits == 4 else 1)
        return np.float32(self.det.call(f"v{bits}_dot", *u, *v, n))

    def vsaa(self, bits, u, v, a, rng=None, in_place=False):
        n = u[0].size * (2 if bits == 4 else 1)
        out = self._vec(bits, n)
        self._lib(rng).call(f"v{bits}_scale_and_add", *u, *v, float(a), n, *out, *((rng,) if bits in (4, 8) else ()), int(in_place))
        return out

    def vthr(self, bits, v, n, k):
        out = np.array(v[0], copy=True)
        assert self.det.call(f"v{bits}_threshold", out, *v[1:], n, k) == 0
        return out

    def mq(self, bits, A, rng=None):
        rows, cols = A.shape
        if bits == 16:
            out = (np.zeros(rows * cols, np.uint16),)
            self.det.call("m16_quantize", np.ascontiguousarray(A), rows, cols, *out)
            return out
        out = np.zeros(rows * cols // (2 if bits == 4 else 1), np.int8), np.zeros((rows // 64) * (cols // 64), np.float32)
        self._lib(rng).call(f"m{bits}_quantize", np.ascontiguousarray(A), rows, cols, *out, rng)
        return out

    def mrestore(self, m, rows, cols):
        A = np.zeros(rows * cols, np.float32)
        self.det.call("m8_restore", *m, rows, cols, A)
        return A

    def mvm(self, mbits, xbits, m, rows, cols, x, rng=None):
        if xbits == 32:
            r = np.zeros(rows, np.float32)
            self.det.call(f"m{mbits}_mvm_f32", *m, rows, cols, *x, r)
            return (r,)
        out = self._vec(xbits, rows)
        if mbits == 16:
            self.det.call("m16_mvm", *m, rows, cols, *x, *out)
        else:
            self._lib(rng).call("m4_mvm_v8" if (mbits, xbits) == (4, 8) else f"m{mbits}_mvm", *m, rows, cols, *x, *out, rng)
        return out


# ---------------------------------------------------------------------------------------------------------------- one case through an engine
def loop_bits(pair):
    return {"m4v4": (4, 4), "m4v8": (4, 8), "m8v8": (8, 8), "m16v16": (16, 16)}[pair]


def run_loop(E, c, Phi, PhiT, y, rngs, on_threshold=None):
    """the five steps from the engine's single operations, in the reference's order; rngs: generators of Phi, PhiT, x, y (or None);
    on_threshold(x before, values after) sees every threshold step"""
    mb, vb = loop_bits(c["op"])
    m, n, K, mu = c["rows"], c["cols"], c["k"], np.float32(c["a"])
    g = rngs or (None, None, None, None)
    x = zero_vec(vb, n)
    trace = []
    for _ in range(c["iterations"]):
        t1 = E.mvm(mb, vb, Phi, m, n, x, g[0])
        t2 = E.vsaa(vb, y, t1, -1.0, g[3])
        t3 = E.mvm(mb, vb, PhiT, n, m, t2, g[1])
        x = E.vsaa(vb, x, t3, float(mu), g[2], in_place=True)
        if K:
            kept = E.vthr(vb, x, n, K)
            if on_threshold:
                on_threshold(x, kept)
            x = (kept,) + tuple(x[1:])
        trace.append((x, t1, t2, t3))
    return trace


def trace_blobs(vb, trace):
    if vb == 16:
        return {"trace.h": np.concatenate([raw(v[0]) for it in trace for v in it])}
    return {"trace.q": np.concatenate([raw(v[0]) for it in trace for v in it]), "trace.s": np.concatenate([raw(v[1]) for it in trace for v in it])}


def run_case(E, c):
    """(operands under the fixture's names, outputs in the fixture's order, generator lanes afterwards or None) of a case"""
    fam, op = c["family"], c["op"]
    ins = inputs_of(c)
    keys = c["keys"]
    rng = E.rng(*keys) if keys else None
    operands, out = {}, {}

    def operand(index, kind, bits, vec):
        operands[f"{kind}{bits}:{rc.input_name(c['inputs'][index])}"] = np.concatenate([raw(a) for a in vec])      # values, then scales
        return vec

    if fam == "loop":
        mb, vb = loop_bits(op)
        Phi, PhiT, y = operand(0, "m", mb, E.mq(mb, ins[0])), operand(1, "m", mb, E.mq(mb, ins[1])), operand(2, "v", vb, E.vq(vb, ins[2]))
        rngs = [E.rng(keys[0] + g, keys[1] + g) for g in range(4)] if keys else None
        out = trace_blobs(vb, run_loop(E, c, Phi, PhiT, y, rngs))
        return operands, out, np.concatenate([E.state(r) for r in rngs]) if keys else None
    bits = bits_of(fam)
    if fam[0] == "v":
        n = c["n"]
        if op == "quantize":
            out = names(bits, E.vq(bits, ins[0], rng))
        else:
            u = operand(0, "v", bits, E.vq(bits, ins[0])) if bits != 32 else (ins[0],)
            if op == "restore":
                out = {"x": E.vrestore(bits, u)}
            elif op == "threshold":
                out = {("q" if bits in (4, 8) else "h" if bits == 16 else "x"): E.vthr(bits, u, n, c["k"])}
            else:
                v = operand(1, "v", bits, E.vq(bits, ins[1])) if bits != 32 else (ins[1],)
                out = {"dot": np.float32(E.vdot(bits, u, v))} if op == "dot" else names(bits, E.vsaa(bits, u, v, c["a"], rng, bool(c["in_place"])))
    else:
        rows, cols = c["rows"], c["cols"]
        if op == "quantize":
            out = names(bits, E.mq(bits, ins[0], rng))
        else:
            m = operand(0, "m", bits, E.mq(bits, ins[0]))
            if op == "restore":
                out = {"A": E.mrestore(m, rows, cols)}
            elif op == "mvm_f32":
                out = {"r": E.mvm(bits, 32, m, rows, cols, (ins[1],))[0]}
            else:
                xb = 8 if op == "mvm_v8" else bits
                x = operand(1, "v", xb, E.vq(xb, ins[1]))
                out = names(xb, E.mvm(bits, xb, m, rows, cols, x, rng))
    return operands, out, E.state(rng) if rng is not None else None


def first_difference(a, b):
    a, b = raw(a), raw(b)
    if a.size != b.size:
        return f"sizes {a.size} and {b.size}"
    d = np.flatnonzero(a != b)
    return "equal" if d.size == 0 else f"first differing byte {int(d[0])} ({d.size} of {a.size} differ)"


def record_of(c, out, state):
    return rc.record(list(out.values()) + ([state.astype("<u8")] if c["keys"] else []))


def groups_of(cases):
    groups = {}
    for c in cases:
        groups.setdefault(rc.group_of(c), []).append(c)
    return groups


def differences(E, c, mine, against):
    """where engine E's run of case c departs from engine `against`'s, output by output"""
    theirs = run_case(against, c)
    parts = [f"{k}: {first_difference(a, theirs[i][k])}" for i in (0, 1) for k, a in mine[i].items()]
    if c["keys"]:
        parts.append(f"generator lanes: {first_difference(mine[2], theirs[2])}")
    return f"{c['id']}: {E.name} against {against.name}: " + "; ".join(parts)


def run_file(E, file, against=None, only=None):
    """Every case of a fixture file through engine E: the digest of each group of cases, of all inputs and of all quantised operands must be
    the fixture's.  The fixture holds digests, so on a difference `against` -- another engine -- is run on the group's cases to name the case
    and the first differing byte, and to say whether that engine agrees with the reference.  only: a predicate that selects whole groups."""
    fx = rc.load_cached(file)
    cases = rc.cases_of(file)
    names = sorted({rc.input_name(spec) for c in cases for spec in c["inputs"]})
    by_name = {rc.input_name(spec): spec for c in cases for spec in c["inputs"]}
    got = rc.digest_over(rc.sha256(np.ascontiguousarray(_input(json.dumps(by_name[n], sort_keys=True)), dtype="<f4")) for n in names)
    assert got == fx["inputs_sha256"], f"{file}: INPUTS differ from what the generator received: the input formula drifted, nothing was compared"
    bad, operands = [], {}
    for group, members in groups_of(cases).items():
        picked = [c for c in members if only is None or only(c)]
        if not picked:
            continue
        assert len(picked) == len(members), group
        runs = [run_case(E, c) for c in members]
        for ops, _, _ in runs:
            operands.update({k: rc.sha256(a) for k, a in ops.items()})
        mine = rc.digest_over(record_of(c, out, state) for c, (_, out, state) in zip(members, runs))
        if mine == fx["groups"][group]:
            continue
        msg = f"{group}: {E.name} differs from the reference in at least one of {[c['id'] for c in members]}"
        if against is not None:
            theirs = rc.digest_over(record_of(c, *run_case(against, c)[1:]) for c in members)
            msg += f"; reference and {against.name} {'agree' if theirs == fx['groups'][group] else 'DISAGREE'}; " + " | ".join(
                differences(E, c, r, against) for c, r in zip(members, runs) if record_of(c, *r[1:]) != record_of(c, *run_case(against, c)[1:]))
        bad.append(msg)
    if only is None:
        assert set(fx["groups"]) == set(groups_of(cases))
        if rc.digest_over(operands[k] for k in sorted(operands)) != fx["operands_sha256"]:
            bad.append(f"{file}: {E.name}'s deterministic quantize of some input differs from the reference's (operand digest)"
                       + ("" if against is None else ": " + str([k for k, v in operands.items() if v != _operands_of(against, file)[k]])))
    assert not bad, f"{len(bad)} differences in {file}:\n" + "\n".join(bad[:MAX_REPORTED])


@functools.lru_cache(maxsize=None)
def _operands_of(E, file):
    return {k: rc.sha256(a) for c in rc.cases_of(file) for k, a in run_case(E, c)[0].items()}


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_fixture_files_hold_exactly_the_case_list():
    for file in rc.FILES:
        fx, cases = rc.load_cached(file), rc.cases_of(file)
        assert list(fx["groups"]) == list(groups_of(cases)), file
        assert "-ffp-contract=off" in fx["flags"] and fx["pinned"] == rc.PINNED and fx["unpinned"] == rc.UNPINNED and fx["whole_max"] == rc.WHOLE_MAX
        assert set(fx["values"]) == {c["id"] for c in cases if c["op"] == "dot"}, file
        assert (rc.GOLDEN / file).stat().st_size < 32 * 1024, file


def test_pinned_and_unpinned_lists_match_the_design_document():
    """DESIGN.md section 4 carries one table row per class between the two markers: | class | pinned operations | unpinned operations |.
    It must say what the fixtures say, so the list of what is left out cannot grow silently."""
    text = (ROOT / "DESIGN.md").read_text()
    block = text[text.index("<!-- reference-pins:begin -->"):text.index("<!-- reference-pins:end -->")]
    rows = [[cell.strip() for cell in line.strip().strip("|").split("|")] for line in block.splitlines() if line.startswith("| `")]
    pinned = {r[0].strip("`"): [v.strip().strip("`") for v in r[1].split(";")] for r in rows if r[1] != "-"}
    unpinned = {r[0].strip("`"): [v.strip().strip("`") for v in r[2].split(";")] for r in rows if r[2] != "-"}
    assert pinned == rc.PINNED
    assert unpinned == rc.UNPINNED


@pytest.fixture(scope="module")
def restated(oracle, m8, rh, rf):
    return OracleEngine(oracle, m8, rh, rf)


@pytest.mark.parametrize("file", rc.FILES)
def test_restatements_equal_reference_fixture(restated, file):
    """a difference is located against the live reference build where oracle/_ref holds it (the fixtures hold digests)"""
    from oracle.binding import RefContainers, RefXorshift
    run_file(restated, file, against=RefEngine() if RefContainers.available() and RefXorshift.available() else None)


def test_fast_oracle_equals_reference_fixture(fast_oracle, restated):
    """the AVX2 restatement has three of the calls: quantize and dot of CloverVector4, the 4-bit mvm, rounding disabled"""
    class Fast(OracleEngine):
        name = "fast_oracle"

        def vq(self, bits, x, rng=None):
            return fast_oracle.v4_quantize(x) if bits == 4 and rng is None else super().vq(bits, x, rng)

        def vdot(self, bits, u, v):
            return fast_oracle.v4_dot(*u, *v) if bits == 4 else super().vdot(bits, u, v)

        def mvm(self, mbits, xbits, m, rows, cols, x, rng=None):
            return fast_oracle.m4_mvm(*m, rows, cols, *x) if (mbits, xbits, rng) == (4, 4, None) else super().mvm(mbits, xbits, m, rows, cols, x, rng)

    E = Fast(restated.o, restated.m8, restated.rh, restated.rf)
    det = lambda c: c["keys"] is None  # noqa: E731
    run_file(E, "ref_v4.json", against=restated, only=lambda c: c["op"] in ("quantize", "dot") and det(c))
    run_file(E, "ref_m4.json", against=restated, only=lambda c: c["op"] == "mvm" and det(c))


@pytest.mark.parametrize("file", rc.FILES)
def test_live_reference_build_reproduces_fixture_when_present(file):
    """the regeneration check (as in test_xorshift_ref.py): where oracle/_ref holds the reference build, it gives the committed bytes"""
    from oracle.binding import RefContainers, RefXorshift
    if not (RefContainers.available() and RefXorshift.available()):
        return
    run_file(RefEngine(), file)


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def device(hip):
    return HipEngine(hip)


@pytest.mark.gpu
@pytest.mark.parametrize("file", [f for f in rc.FILES if f != "ref_loops.json"])
def test_gpu_equals_reference_fixture(device, restated, file):
    """quantize / restore / dot EXACT / scaleAndAdd / threshold REFERENCE / the mvm forms, both roundings, against the fixture directly; the
    oracle only serves to say where a difference lies"""
    run_file(device, file, against=restated)


def kept_set_is_unique(bits, u, thr, n):
    """FAST keeps the K largest magnitudes with lowest-index ties, the reference whatever its heap walk leaves: the two must agree only
    where no dropped element is as large as a kept one.  Magnitudes as CloverVector*::getAbs computes them, |q| * (scale / 7 or 127)."""
    if bits == 4:
        b = raw(u[0])
        q = np.stack([(b.view(np.int8) >> 4), ((b << 4).view(np.int8) >> 4)], 1).reshape(-1)
        t = raw(thr)
        kq = np.stack([(t.view(np.int8) >> 4), ((t << 4).view(np.int8) >> 4)], 1).reshape(-1)
        mag = np.abs(q.astype(np.float32)) * np.repeat(u[1] / np.float32(7.0), 64)
    elif bits == 8:
        q, kq = u[0].view(np.int8), np.asarray(thr).view(np.int8)
        mag = np.abs(q.astype(np.float32)) * np.repeat(u[1] / np.float32(127.0), 64)
    else:
        q = u[0].view(np.float16).astype(np.float32) if bits == 16 else u[0]
        kq = np.asarray(thr).view(np.float16).astype(np.float32) if bits == 16 else np.asarray(thr)
        mag = np.abs(q)
    mag, kept = mag[:n], (kq[:n] != 0)
    dropped = mag[~kept & (mag > 0)]
    return kept.sum() == 0 or dropped.size == 0 or mag[kept].min() > dropped.max()


@pytest.mark.gpu
@pytest.mark.parametrize("file", ["ref_v4.json", "ref_v8.json", "ref_v16.json", "ref_v32.json"])
def test_gpu_threshold_fast_equals_reference_where_the_kept_set_is_unique(device, restated, file):
    """group by group: the oracle's survivors are the reference's (the group's digest is the fixture's), and where no dropped element is as
    large as a kept one FAST leaves those same bytes"""
    groups = rc.load_cached(file)["groups"]
    selections = 0                          # compared cases with 1 < k < n - 1: k = 1, n - 1 and n hardly select
    for group, members in groups_of([c for c in rc.cases_of(file) if c["op"] == "threshold"]).items():
        bits = bits_of(members[0]["family"])
        us = [restated.vq(bits, inputs_of(c)[0]) if bits != 32 else (inputs_of(c)[0],) for c in members]
        wants = [restated.vthr(bits, u, c["n"], c["k"]) for c, u in zip(members, us)]
        assert rc.digest_over(rc.record([w]) for w in wants) == groups[group], group
        for c, u, want in zip(members, us, wants):
            unique = kept_set_is_unique(bits, u, want, c["n"])
            if bits in (4, 8) and c["inputs"][0]["kind"] == "normal" and c["k"] == rc.THRESHOLD_K_TIE_FREE[c["n"]]:
                assert unique, c["id"]                  # the case that exists for this comparison must qualify for it
            if not unique:
                continue
            got = device.vthr(bits, u, c["n"], c["k"], THRESHOLD_FAST)
            assert np.array_equal(raw(got), raw(want)), f"{c['id']}: FAST against the reference's survivors: {first_difference(got, want)}"
            selections += 1 < c["k"] < c["n"] - 1
    assert selections >= len(rc.LENGTHS), selections                          # at least the tie-free k of every length


@pytest.mark.gpu
@pytest.mark.parametrize("file", ["ref_v4.json", "ref_v8.json", "ref_v16.json", "ref_v32.json"])
def test_gpu_dot_fast_within_the_fast_bound_of_the_reference_value(hip, device, restated, file):
    """|fast - reference's value| <= B, B the bound the existing FAST-dot tests hold |fast - float64 value| to: 2e-6 sum|terms| + 1e-6 (4- and
    8-bit: test_gpu_parity.py, test_mixed8.py), 2e-6 sum|terms| (half: test_half16.py), fp32_helpers.fast_dot_bound (fp32).  The reference's
    value is in the fixture."""
    recs = rc.load_cached(file)["values"]
    cus = hip.device_info()["compute_units"]
    for c in rc.cases_of(file):
        if c["op"] != "dot":
            continue
        bits, n = bits_of(c["family"]), c["n"]
        x, y = inputs_of(c)
        u, v = ((x,), (y,)) if bits == 32 else (restated.vq(bits, x), restated.vq(bits, y))
        r = float(np.frombuffer(bytes.fromhex(recs[c["id"]]), "<f4")[0])
        if bits in (4, 8):
            exact = restated.o.v4_dot_f64(*u, *v) if bits == 4 else restated.o.v8_dot_f64(*u, *v)
            fu, fv = restated.vrestore(bits, u).astype(np.float64), restated.vrestore(bits, v).astype(np.float64)
            if bits == 4:             # test_gpu_parity.py: |block integer| * su * sv / 49 per block
                terms = float(np.sum(np.abs((np.rint(fu * 7 / np.repeat(u[1], 64).astype(np.float64)) * np.rint(fv * 7 / np.repeat(v[1], 64).astype(np.float64)))
                                            .reshape(-1, 64).sum(1)) * u[1].astype(np.float64) * v[1].astype(np.float64) / 49.0))
            else:                     # test_mixed8.py: sum |q q'| s s' / 127^2
                terms = float(np.abs(np.repeat(u[1] * v[1], 64).astype(np.float64) * u[0].astype(np.float64) * v[0].astype(np.float64)).sum() / (127.0 * 127.0))
            bound = 2e-6 * terms + 1e-6
        elif bits == 16:
            e, a = restated.rh.mvm64(u[0], 1, n, v[0])
            exact, bound = float(e[0]), 2e-6 * float(a[0])
        else:
            exact, absum = restated.rf.dot64(x, y)
            bound = fast_dot_bound(absum, n, cus)
        fast = float(device.vdot(bits, u, v, DOT_FAST))
        print(f"{c['id']}: |fast - reference| = {abs(fast - r):.3e}, bound {bound:.3e} (|reference - float64| = {abs(r - exact):.3e})")
        assert abs(fast - r) <= bound, c["id"]


def _batch_groups(file, op):
    """per shape: the three deterministic cases that share the `normal` matrix (vectors normal, ints, edges)"""
    groups = {}
    for c in rc.cases_of(file):
        if c["op"] == op and c["keys"] is None and c["inputs"][0]["kind"] == "normal":
            groups.setdefault((c["rows"], c["cols"]), []).append(c)
    assert all(len(g) == 3 for g in groups.values())
    return groups


@pytest.mark.gpu
@pytest.mark.parametrize("file,op,xbits", [("ref_m4.json", "mvm", 4), ("ref_m4.json", "mvm_v8", 8), ("ref_m8.json", "mvm", 8)])
def test_gpu_batched_mvm_of_three_fixture_vectors(hip, device, file, op, xbits):
    """clm4_mvm_batch / clm4_mvm_v8_batch / clm8_mvm_batch with a group of 3: their contract is "the single calls in order", so each vector's
    result is the fixture's of the single mvm.  The fixture's digest covers the five deterministic cases of a shape; the three that share
    the `normal` matrix come from the batched call, the other two from single calls."""
    fx = rc.load_cached(file)
    mbits = 8 if "m8" in file else 4
    for group, members in groups_of([c for c in rc.cases_of(file) if c["op"] == op and c["keys"] is None]).items():
        rows, cols = members[0]["rows"], members[0]["cols"]
        batch = [c for c in members if c["inputs"][0]["kind"] == "normal"]
        assert len(batch) == 3 and len(members) == 5, group
        A = device.mq(mbits, inputs_of(batch[0])[0])
        xs = [device.vq(xbits, inputs_of(c)[1]) for c in batch]
        if (mbits, xbits) == (4, 4):
            got = hip.m4_mvm_batch(*A, rows, cols, xs)
        else:
            dA = [hip.to_device(a) for a in A]
            dx = [(hip.to_device(q), hip.to_device(s)) for q, s in xs]
            dr = [(hip.alloc(rows), hip.alloc(max(rows // 16, 4))) for _ in xs]
            pa = hip.ptr_array
            fn = hip.lib.clm4_mvm_v8_batch if mbits == 4 else hip.lib.clm8_mvm_batch
            hip.check(fn(dA[0].ptr, dA[1].ptr, rows, cols, len(xs), pa([d[0] for d in dx]), pa([d[1] for d in dx]), pa([d[0] for d in dr]),
                         pa([d[1] for d in dr]), None, None))
            got = [(r.download(np.int8, rows), sr.download(np.float32, rows // 64)) for r, sr in dr]
        single = {c["id"]: list(run_case(device, c)[1].values()) for c in members}
        recs = [rc.record(got[batch.index(c)] if c in batch else single[c["id"]]) for c in members]
        if rc.digest_over(recs) != fx["groups"][group]:
            raise AssertionError(f"{group} with the `normal` matrix's three vectors in one batch differs from the reference; batch against single calls: "
                                 + "; ".join(f"{c['id']}: q {first_difference(g[0], single[c['id']][0])}, s {first_difference(g[1], single[c['id']][1])}"
                                             for c, g in zip(batch, got)))


def _hip_loop(hip, pair, Phi, PhiT, m, n, y, iterations, K, mu, thr):
    """x, t1, t2, t3 after `iterations` of the one-call loop; thr: 0 none (GD), 1 FAST, 2 REFERENCE"""
    mu = float(mu)
    if pair == "m16v16":
        v = hip.mf16_iht(Phi[0], PhiT[0], m, n, y[0], iterations, K, mu, thr)
        return [(v[k],) for k in ("x", "t1", "t2", "t3")]
    if pair == "m8v8":
        v = hip.m8_iht(*Phi, *PhiT, m, n, *y, iterations, K, mu, thr)
        return [v[k] for k in ("x", "t1", "t2", "t3")]
    four = pair == "m4v4"
    b = [hip.to_device(a) for a in (*Phi, *PhiT, *y)]
    lens = {"x": n, "t1": m, "t2": m, "t3": n}
    v = {k: (hip.alloc(ln // 2 if four else ln), hip.alloc(ln // 16)) for k, ln in lens.items()}
    for q, s in v.values():
        hip.check(hip.lib.clv_memset(q.ptr, 0x5A, q.nbytes, None))
        hip.check(hip.lib.clv_memset(s.ptr, 0x5A, s.nbytes, None))
    fn = hip.lib.clm4_iht if four else hip.lib.clm4_iht_v8
    hip.check(fn(b[0].ptr, b[1].ptr, b[2].ptr, b[3].ptr, m, n, v["x"][0].ptr, v["x"][1].ptr, n, b[4].ptr, b[5].ptr, v["t1"][0].ptr, v["t1"][1].ptr,
                 v["t2"][0].ptr, v["t2"][1].ptr, v["t3"][0].ptr, v["t3"][1].ptr, iterations, K, float(mu), thr, None, None))
    hip.check(hip.lib.clv_device_sync())
    return [(v[k][0].download(np.uint8, ln // 2 if four else ln), v[k][1].download(np.float32, ln // 64)) for k, ln in lens.items()]


def _loop_is_tie_free(restated, c):
    """does every threshold step of the case keep a unique set (the oracle's walk; its trace is the reference's: the CPU test)"""
    mb, vb = loop_bits(c["op"])
    ins = inputs_of(c)
    unique = []
    run_loop(restated, c, restated.mq(mb, ins[0]), restated.mq(mb, ins[1]), restated.vq(vb, ins[2]), None,
             on_threshold=lambda x, kept: unique.append(kept_set_is_unique(vb, x, kept, c["cols"])))
    return all(unique)


@pytest.mark.gpu
@pytest.mark.parametrize("pair,persistent", [("m4v4", "1"), ("m4v4", "0"), ("m4v8", "1"), ("m4v8", "0"), ("m8v8", None), ("m16v16", None)])
def test_gpu_loop_calls_equal_reference_loop(hip, device, restated, pair, persistent, monkeypatch):
    """The one-call loops, rounding disabled: the call with 1, 2 and 3 iterations gives the reference's x, t1, t2, t3 after that iteration --
    the three calls together are the fixture's whole trace.

    clm4_iht and clm4_iht_v8 run as ONE persistent launch only with the FAST threshold or none (iht_persist.hip), and FAST agrees with the
    reference only where no threshold step meets a tie at its boundary.  So each IHT case runs in FAST mode where the oracle's walk says
    every step is tie-free (the K of LOOP_K_TIE_FREE is, by construction) and in REFERENCE mode otherwise; GD has no threshold.  With
    CLV_IHT_PERSISTENT=1 (read per call, set the way test_iht_persistent.py sets it) clv_iht_persistent_launches() must show that the
    FAST and GD calls DID run the persistent kernel and the REFERENCE calls did not; with 0 that none did: the launch-per-step loop, in
    the same modes.  clm8_iht and clm_f16_iht have no persistent form and do not read the variable: REFERENCE mode, one run."""
    if persistent is not None:
        monkeypatch.setenv("CLV_IHT_PERSISTENT", persistent)
    fx = rc.load_cached("ref_loops.json")
    launches = hip.lib.clv_iht_persistent_launches
    persistent_iht = 0
    for group, members in groups_of([c for c in rc.cases_of("ref_loops.json") if c["keys"] is None and c["op"] == pair]).items():
        got, want, modes = [], [], []
        for c in members:                     # the two IHT loops and the GD loop of the pair at one size
            mb, vb = loop_bits(pair)
            ins = inputs_of(c)
            Phi, PhiT, y = device.mq(mb, ins[0]), device.mq(mb, ins[1]), device.vq(vb, ins[2])
            thr = 0 if not c["k"] else 1 if persistent is not None and _loop_is_tie_free(restated, c) else 2
            if persistent is not None and c["k"] == rc.LOOP_K_TIE_FREE[(c["rows"], c["cols"])]:
                assert thr == 1, c["id"]                # the case that exists for the persistent kernel must qualify for it
            before = int(launches())
            trace = [_hip_loop(hip, pair, Phi, PhiT, c["rows"], c["cols"], y, it + 1, c["k"], np.float32(c["a"]), thr) for it in range(c["iterations"])]
            ran = int(launches()) - before
            assert ran == (c["iterations"] if persistent == "1" and thr != 2 else 0), (c["id"], thr, ran)
            persistent_iht += thr == 1 and ran > 0
            got.append(trace_blobs(vb, trace))
            modes.append(thr)
        if rc.digest_over(rc.record(g.values()) for g in got) == fx["groups"][group]:
            continue
        for c in members:
            mb, vb = loop_bits(pair)
            ins = inputs_of(c)
            want.append(trace_blobs(vb, run_loop(restated, c, restated.mq(mb, ins[0]), restated.mq(mb, ins[1]), restated.vq(vb, ins[2]), None)))
        agree = rc.digest_over(rc.record(w.values()) for w in want) == fx["groups"][group]
        raise AssertionError(f"{group} (CLV_IHT_PERSISTENT={persistent}, threshold modes {modes}): reference and oracle {'agree' if agree else 'DISAGREE'}; "
                             "HIP against the oracle: " + "; ".join(f"{c['id']} {k}: {first_difference(g[k], w[k])}" for c, g, w in zip(members, got, want) for k in g))
    assert persistent_iht >= (len(rc.LOOP_SIZES) if persistent == "1" else 0)          # the persistent IHT kernel was compared at every size
