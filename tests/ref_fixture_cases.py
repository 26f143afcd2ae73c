"""The case list and the input data of the reference fixtures (tests/golden/ref_*.json), in one place.

The fixtures are written by oracle/_ref/clover_ref_gen -- the reference's own container code behind oracle/ref_containers.cpp -- from the
manifest and the input bytes this module lays down (`python tests/ref_fixture_cases.py <directory>`, run by `make -C oracle ref-fixtures`).
The tests (tests/test_reference_fixtures.py) rebuild the same inputs from the same formula and compare their SHA-256 with the one the
generator recorded for the bytes it received, so a drift of this formula reads "input differs", not "kernel wrong".

Inputs depend on no library's random generator: element i of stream `seed` is a splitmix64 hash of (seed, i) in uint64 arithmetic, mapped to
the data kind with exact float operations only (no libm call):
  normal      sum of four 16-bit fields, centred: a bell-shaped multiple of 2^-13 in (-8, 8)
  ints        integers in [-10, 10]: many equal magnitudes, many rounding ties after scaling
  edges:BIG   built 64-block by 64-block, block b of type EDGE_ORDER[b mod 7] (the tie blocks first, so that the shortest vector has them):
                0 all zero                         1 maximum is denormal (multiples of 2^-149, either sign)
                2 only +-m (nibbles +-7, bytes +-127)   3 zeros of both signs and +-1
                4 small integers and one +-BIG     5 4-bit rounding ties: x 7 / max = k + 0.5 exactly (max = 7 * 2^e, x = (k + 0.5) 2^e)
                6 8-bit rounding ties: x 127 / max = k + 0.5 exactly (max = 127 * 2^e)
              BIG is 3e38 where one operand is quantised or restored; smaller where two operands meet, because the reference has no contract
              for the Inf and NaN that 3e38 * 3e38 produces.
Matrices use the same kinds tile by tile (64 x 64 tile t of type EDGE_ORDER[t mod 7], each of its rows one block of that type)."""
import functools
import hashlib
import json
import struct
import sys
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
LENGTHS = (128, 256, 384, 1024, 8320, 65664)
SHAPES = tuple((128 * i, 128 * j) for i in (1, 2, 3) for j in (1, 2, 3, 4)) + ((128, 16512),)   # 16512: one block past mvm_f32's 16384 chunk
KEYS = ((12345, 67890), (445560390295639063, 2935984234003016713))       # the two pairs of tests/golden/xorshift_ref.json
LOOP_SIZES = ((128, 256), (256, 384))                                     # (m, N)
LOOP_ITERATIONS = 3
# a second K per size at which, with these inputs, no iteration's threshold meets equal magnitudes at its boundary, for the 4-bit and for the
# 8-bit vectors (found by a search with the oracle; tests/test_reference_fixtures.py re-checks it).  There the lowest-index tie rule of the
# FAST threshold and the reference's heap walk must keep the same elements, which is what lets the persistent loop kernels -- FAST or no
# threshold only -- be compared with the reference.  n / 8 meets ties for CloverVector4 at both sizes.
# the same for the single threshold: no quantised data is free of equal magnitudes (a 4-bit block has seven), so "tie-free" is a property
# of (data, k).  Per length the k nearest n / 4 at which the `normal` vector, quantised to 4 and to 8 bits, has its k-th magnitude strictly
# above its (k + 1)-th: FAST and the reference must then keep the same elements, on a real selection.
THRESHOLD_K_TIE_FREE = {128: 39, 256: 58, 384: 95, 1024: 254, 8320: 2075, 65664: 16408}
LOOP_K_TIE_FREE = {(128, 256): 13, (256, 384): 31}
EDGE_ORDER = (5, 6, 2, 4, 1, 3, 0)
FILES = ("ref_v4.json", "ref_v8.json", "ref_v16.json", "ref_v32.json", "ref_m4.json", "ref_m8.json", "ref_m16.json", "ref_loops.json")
WHOLE_MAX = 16            # a record of at most this many bytes (a dot's float) is stored in hex, everything else as its SHA-256

# what the fixtures pin and what they cannot (the Intel-backed methods); DESIGN.md section 4 carries the same two lists
PINNED = {
    "CloverVector4": ["quantize", "restore", "dot", "scaleAndAdd", "threshold"],
    "CloverVector8": ["quantize", "restore", "dot", "scaleAndAdd", "threshold"],
    "CloverVector16": ["quantize", "restore", "dot", "scaleAndAdd", "threshold"],
    "CloverVector32": ["dot", "scaleAndAdd", "threshold"],
    "CloverMatrix4": ["quantize", "mvm(CloverVector4)", "mvm(CloverVector8)", "mvm(CloverVector32)"],
    "CloverMatrix8": ["quantize", "get (every element: restore)", "mvm(CloverVector8)", "mvm(CloverVector32)"],
    "CloverMatrix16": ["quantize", "mvm(CloverVector16)", "mvm(CloverVector32)"],
    "loops": ["IHT", "GD"],
}
UNPINNED = {
    "CloverMatrix4": ["transpose"],
    "CloverMatrix8": ["transpose"],
    "CloverMatrix16": ["transpose"],
    "CloverMatrix32": ["mvm", "transpose"],
    "threshold": ["k = 0"],
}


# ---------------------------------------------------------------------------------------------------------------- the formula
def _mix(z):
    """splitmix64's output function on a uint64 array"""
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def hashes(seed, count, offset=0):
    """count uint64 hashes of stream `seed`, elements offset, offset + 1, ..."""
    with np.errstate(over="ignore"):
        base = _mix(np.array([seed], dtype=np.uint64))[0]
        return _mix(base + np.arange(offset, offset + count, dtype=np.uint64) * np.uint64(0xD1342543DE82EF95))


def _normal(h):
    f = [((h >> np.uint64(16 * j)) & np.uint64(0xFFFF)).astype(np.int64) for j in range(4)]
    return ((f[0] + f[1] + f[2] + f[3] - 2 * 65535).astype(np.float64) / 8192.0).astype(np.float32)


def _ints(h):
    return ((h % np.uint64(21)).astype(np.int64) - 10).astype(np.float32)


def _sign(h, bit):
    return (1 - 2 * ((h >> np.uint64(bit)) & np.uint64(1)).astype(np.int64)).astype(np.float32)


def edge_block(kind, h, big):
    """one 64-block of type `kind` from its 64 hashes"""
    e = np.float32(2.0) ** np.float32(int(h[0] >> np.uint64(40)) % 5 - 2)
    if kind == 0:
        return np.zeros(64, np.float32)
    if kind == 1:
        bits = ((h >> np.uint64(8)) % np.uint64(24)).astype(np.uint32) | (((h >> np.uint64(3)) & np.uint64(1)).astype(np.uint32) << np.uint32(31))
        return bits.view(np.float32)
    if kind == 2:
        return _sign(h, 5) * np.float32(2.5) * e
    if kind == 3:
        v = np.array([0.0, -0.0, 1.0, -1.0], np.float32)
        return v[(h >> np.uint64(9)).astype(np.int64) % 4]
    if kind == 4:
        x = _ints(h >> np.uint64(7))
        x[int(h[1] >> np.uint64(20)) % 64] = np.float32(big) * _sign(h[2:3], 11)[0]
        return x
    steps = 7 if kind == 5 else 127
    k = ((h >> np.uint64(12)) % np.uint64(2 * steps)).astype(np.int64) - steps       # k in [-steps, steps - 1]
    x = (k.astype(np.float32) + np.float32(0.5)) * e
    x[int(h[1] >> np.uint64(20)) % 64] = np.float32(steps) * e                       # the block's maximum
    return x


def vector(kind, n, seed):
    h = hashes(seed, n)
    if kind == "normal":
        return _normal(h)
    if kind == "ints":
        return _ints(h)
    big = float(kind.split(":")[1])
    return np.concatenate([edge_block(EDGE_ORDER[b % 7], h[64 * b:64 * b + 64], big) for b in range(n // 64)])


def matrix(kind, rows, cols, seed):
    if not kind.startswith("edges"):
        return vector(kind, rows * cols, seed).reshape(rows, cols)
    big = float(kind.split(":")[1])
    h = hashes(seed, rows * cols).reshape(rows, cols)
    A = np.empty((rows, cols), np.float32)
    for bi in range(rows // 64):
        for bj in range(cols // 64):
            t = EDGE_ORDER[(bi * (cols // 64) + bj) % 7]
            for r in range(64 * bi, 64 * bi + 64):
                A[r, 64 * bj:64 * bj + 64] = edge_block(t, h[r, 64 * bj:64 * bj + 64], big)
    return A


def make_input(spec):
    """the float32 array of an input description {"kind", "shape", "seed", "transposed"?}"""
    shape = spec["shape"]
    if len(shape) == 1:
        return vector(spec["kind"], shape[0], spec["seed"])
    if spec.get("transposed"):
        return np.ascontiguousarray(matrix(spec["kind"], shape[1], shape[0], spec["seed"]).T)
    return matrix(spec["kind"], shape[0], shape[1], spec["seed"])


# ---------------------------------------------------------------------------------------------------------------- the cases
def _roundings(stochastic_op):
    return [None] + list(KEYS) if stochastic_op else [None]


def _edges(family, two_operands):
    if family in ("v16", "m16"):
        return "edges:8" if two_operands else "edges:60000"
    if family == "v32":
        return "edges:1e15" if two_operands else "edges:3e38"
    return "edges:1e15" if two_operands else "edges:3e38"


def _vec_cases(family):
    stochastic = family in ("v4", "v8")
    out = []
    for li, n in enumerate(LENGTHS):
        for ki, base in enumerate(("normal", "ints", "edges")):
            one = _edges(family, False) if base == "edges" else base
            two = _edges(family, True) if base == "edges" else base
            u1 = {"kind": one, "shape": [n], "seed": 100 + ki}
            u2 = {"kind": two, "shape": [n], "seed": 100 + ki}
            v2 = {"kind": two, "shape": [n], "seed": 200 + ki}
            if family != "v32":
                for keys in _roundings(stochastic):
                    out.append({"family": family, "op": "quantize", "n": n, "keys": keys, "inputs": [u1]})
                out.append({"family": family, "op": "restore", "n": n, "keys": None, "inputs": [u1]})
            out.append({"family": family, "op": "dot", "n": n, "keys": None, "inputs": [u2, v2]})
            a = (-1.0, 0.37, 2.5)[(li + ki) % 3]
            for in_place in (0, 1):
                for keys in _roundings(stochastic):
                    out.append({"family": family, "op": "scale_and_add", "n": n, "a": a, "in_place": in_place, "keys": keys, "inputs": [u2, v2]})
            if base != "edges":          # once on data with few equal magnitudes, once on `ints`, which has many; k = 0: see UNPINNED
                for k in (1, n // 4, n - 1, n) + ((THRESHOLD_K_TIE_FREE[n],) if base == "normal" else ()):
                    out.append({"family": family, "op": "threshold", "n": n, "k": k, "keys": None, "inputs": [u1]})
    return out


def _mat_cases(family):
    stochastic = family in ("m4", "m8")
    out = []
    for rows, cols in SHAPES:
        for ki, base in enumerate(("normal", "ints", "edges")):
            one = _edges(family, False) if base == "edges" else base
            two = _edges(family, True) if base == "edges" else base
            A1 = {"kind": one, "shape": [rows, cols], "seed": 300 + ki}
            A2 = {"kind": two, "shape": [rows, cols], "seed": 300 + ki}
            x2 = {"kind": two, "shape": [cols], "seed": 400 + ki}
            for keys in _roundings(stochastic):
                out.append({"family": family, "op": "quantize", "rows": rows, "cols": cols, "keys": keys, "inputs": [A1]})
            if family == "m8":
                out.append({"family": family, "op": "restore", "rows": rows, "cols": cols, "keys": None, "inputs": [A1]})
            for op in (("mvm", "mvm_v8") if family == "m4" else ("mvm",)):
                for keys in _roundings(stochastic):
                    out.append({"family": family, "op": op, "rows": rows, "cols": cols, "keys": keys, "inputs": [A2, x2]})
            out.append({"family": family, "op": "mvm_f32", "rows": rows, "cols": cols, "keys": None, "inputs": [A2, x2]})
        if stochastic:                # one matrix with the three vectors: what the batched mvm forms are compared with, vector by vector
            A = {"kind": "normal", "shape": [rows, cols], "seed": 300}
            for ki, base in ((1, "ints"), (2, _edges(family, True))):
                for op in (("mvm", "mvm_v8") if family == "m4" else ("mvm",)):
                    out.append({"family": family, "op": op, "rows": rows, "cols": cols, "keys": None,
                                "inputs": [A, {"kind": base, "shape": [cols], "seed": 400 + ki}]})
    return out


def _loop_cases():
    out = []
    for pair in ("m4v4", "m4v8", "m8v8", "m16v16"):
        for m, n in LOOP_SIZES:
            Phi = {"kind": "normal", "shape": [m, n], "seed": 500}
            PhiT = {"kind": "normal", "shape": [n, m], "seed": 500, "transposed": 1}
            y = {"kind": "normal", "shape": [m], "seed": 501}
            for K in (n // 8, LOOP_K_TIE_FREE[(m, n)], 0):         # K = 0: the GD loop (no threshold step)
                for keys in _roundings(pair != "m16v16"):
                    out.append({"family": "loop", "op": pair, "rows": m, "cols": n, "k": K, "a": 2.0 ** -8, "iterations": LOOP_ITERATIONS,
                                "keys": keys, "inputs": [Phi, PhiT, y]})
    return out


def cases_of(file):
    fam = file[len("ref_"):-len(".json")]
    cs = _loop_cases() if fam == "loops" else _vec_cases(fam) if fam[0] == "v" else _mat_cases(fam)
    for c in cs:
        c["id"] = case_id(c)
    assert len({c["id"] for c in cs}) == len(cs)
    return cs


def case_id(c):
    parts = [c["family"], c["op"], "x".join(str(d) for d in c["inputs"][0]["shape"]), c["inputs"][0]["kind"].split(":")[0]]
    if len(c["inputs"]) == 2 and c["inputs"][1]["kind"].split(":")[0] != parts[-1]:
        parts.append("by-" + c["inputs"][1]["kind"].split(":")[0])
    if "k" in c:
        parts.append(f"k{c['k']}")
    if c.get("in_place"):
        parts.append("inplace")
    parts.append("det" if c["keys"] is None else f"keys{KEYS.index(tuple(c['keys']))}")
    return "-".join(parts)


def group_of(c):
    """the cases whose records share one digest in the fixture: one operation at one shape with one kind of rounding"""
    return "-".join([c["family"], c["op"], "x".join(str(d) for d in c["inputs"][0]["shape"]), "det" if c["keys"] is None else "stochastic"])


def digest_over(records) -> str:
    """the digest of a sequence of records or digests, as the generator forms it"""
    return hashlib.sha256("".join(records).encode()).hexdigest()


def input_name(spec):
    """what the fixtures call an input: kind/shape/seed, /T for the transposed matrix"""
    return f"{spec['kind']}/{'x'.join(str(d) for d in spec['shape'])}/{spec['seed']}" + ("/T" if spec.get("transposed") else "")


# ---------------------------------------------------------------------------------------------------------------- the manifest
def write_manifest(directory: Path) -> None:
    directory.mkdir(parents=True, exist_ok=True)
    written = {}
    lines = []
    for file in FILES:
        lines.append(f"file {file}")
        head = json.dumps({"pinned": PINNED, "unpinned": UNPINNED}, sort_keys=True)
        lines.append("header " + head[1:-1])
        for c in cases_of(file):
            names = []
            for spec in c["inputs"]:
                key = input_name(spec)
                if key not in written:
                    written[key] = f"in{len(written):04d}.bin"
                    (directory / written[key]).write_bytes(np.ascontiguousarray(make_input(spec), dtype="<f4").tobytes())
                    lines.append(f"input {written[key]} {key}")
                names.append(written[key])
            keys = c["keys"] or (0, 0)
            abits = struct.unpack("<I", struct.pack("<f", c.get("a", 0.0)))[0]
            lines.append(" ".join(str(v) for v in ("case", c["family"], c["op"], int(c["keys"] is not None), c.get("n", 0), c.get("rows", 0),
                                                   c.get("cols", 0), c.get("k", 0), f"{abits:x}", keys[0], keys[1], c.get("in_place", 0),
                                                   c.get("iterations", 0), len(names), *names, "|", group_of(c), json.dumps(c["id"]))))
    (directory / "manifest.txt").write_text("\n".join(lines) + "\n")


# ---------------------------------------------------------------------------------------------------------------- reading a fixture
@functools.lru_cache(maxsize=None)
def load_cached(file):
    return json.loads((GOLDEN / file).read_text())


def sha256(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def record(parts) -> str:
    """a case's record as the generator writes it: the outputs in order (values before scales), then the generator lanes afterwards if the
    rounding is stochastic -- in hex if that is at most WHOLE_MAX bytes, else its SHA-256"""
    b = b"".join(np.ascontiguousarray(p).tobytes() for p in parts)
    return b.hex() if len(b) <= WHOLE_MAX else hashlib.sha256(b).hexdigest()


if __name__ == "__main__":
    write_manifest(Path(sys.argv[1]))
