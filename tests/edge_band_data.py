"""Edge-valued operands for every mvm form: raw quantised data (nibbles or int8 bytes, plus scales) laid out so that each 64-element OUTPUT
block of an mvm falls into a chosen category of the re-quantising epilogue.  Written once; the CPU test (test_edge_band_data_cpu.py)
asserts the categories on the reference alone, the GPU tests (test_edge_bands_*.py) compare every form with the reference on this data.

The matrix B is in PRODUCT orientation, out x in: the held-matrix families get B, the transposed families its transpose (Ref.transpose).

x: 64-block b is of kind X_KINDS[(b + rot) % 6]
    ord    scale in [0.5, 2)                 zero   all zero, scale 1.0            small  scale x 2^-20
    big    scale x 2^20                      sub    scale 1e-40 (subnormal)        ord    again

B: one 64-row band per output block, every tile of a tile row of the band's kind BANDS[i % 8]; "facing" = the kind of x's block (rot = 0)
that the tile's columns multiply
    N    tile scales 2^e [1, 2), e uniform in [-20, 20]                          -> an ordinary block over tiles spread by > 2^40 (the first and last tile are pinned 2^-20 and 1.25 2^20)
    Z    zero tiles, scale 1.0                                                   -> dots exactly 0: elements 0, scale 1.0 (fix_zero_max)
    Zx   non-zero only where it faces x's zero blocks                            -> a non-zero matrix, dots exactly 0: scale 1.0
    T    subnormal tile scales T_BASE (1 .. 7); zero where it faces `big`        -> non-zero subnormal dots, maximum < STEPS / FLT_MAX:
                                                                                    k = STEPS / max = inf, every element 0, scale = that
                                                                                    subnormal maximum (not 1.0)
    H    tile scales 1e28 [0.5, 2)                                               -> finite, block scale > 1e30
    E    tile scales E_BASE [0.5, 2) / sqrt(facing ord blocks / 2), zero where   -> maximum in [STEPS / FLT_MAX, E_HI): k finite and
         it faces small / big / sub; the band's seed is SEARCHED (E_SEEDS)          within 8 x of FLT_MAX, non-zero elements
    M    tile scales alternate 1e-30 / 1e20; rows 0 .. 31 of the 1e20 tiles zero -> 32 rows about 2^160 below the other 32 of one block:
                                                                                    element 0 beside non-zero elements
    N2   as N, other draws                                                       -> ordinary
STEPS = 7 for a 4-bit result (the 4-bit pair), 127 for an int8 result (the mixed and the 8-bit pair); T_BASE and E_BASE depend on the pair
because the block factor does ((s / 7) (sx / 7), (s / 7) (sx / 127), (s / 127) (sx / 127)).

No operand is infinite or NaN and the reference produces none: a band of 3e38 scales gives 0 * inf = NaN against x's zero block, which is
outside the reference's contract and stays out.

u (the fused operand, out elements): block b of kind U_KINDS[b % 16]: ord, zero, big (scale 1e30 [0.5, 2)), sub (scale 1e-40).  A Z band
under a `sub` block of u gives a fused block whose maximum makes k = inf; an H band under a `big` block one of scale > 1e30.

int8 vectors carry the image of the int8 split in every non-zero block (127, -127, 120, 119, -120, -121, 112, 0: x >= 120 carries)."""
import numpy as np

PAIRS = ("v4", "mixed", "m8")                      # CloverMatrix4 x CloverVector4, CloverMatrix4 x CloverVector8, CloverMatrix8 x CloverVector8
MATRIX_BITS = {"v4": 4, "mixed": 4, "m8": 8}
VECTOR_BITS = {"v4": 4, "mixed": 8, "m8": 8}
STEPS = {4: 7, 8: 127}
X_KINDS = ("ord", "zero", "small", "big", "sub", "ord")
BANDS = ("N", "Z", "Zx", "T", "H", "E", "M", "N2")
U_KINDS = ("ord", "sub", "zero", "sub", "big", "ord", "ord", "ord", "zero", "ord", "sub", "zero", "ord", "sub", "big", "ord")
A_VALUES = (-1.0, 0.37, 2.5)
SHAPES = ((512, 384), (1024, 768))                 # eight bands, six x kinds, three 128-column steps; everything twice, in % 512 != 0
CHUNK_SHAPE = (512, 4224)                          # the mixed and 8-bit batched / transposed kernels stage 4096 elements of x: re-staged once
LOOP_SHAPES = ((256, 512), (384, 640))
NVEC_MAX = 9
FLT_MAX = np.float32(3.4028234663852886e38)
FLT_MIN = np.float32(1.1754943508222875e-38)
T_BASE = {"v4": 2.0 ** -140, "mixed": 2.0 ** -134, "m8": 2.0 ** -134}
E_BASE = {"v4": 1.8e-39, "mixed": 5e-38, "m8": 6e-38}
CARRY = np.array([127, -127, 120, 119, -120, -121, 112, 0], np.int8)
# the seed of every E band, found by find_e_seed (the first of 0, 1, ... at which the reference's block maximum is in range):
# (pair, out, in, band row) -> seed.  test_edge_band_data_cpu.py repeats the search and compares.
E_SEEDS = {
    ("v4", 512, 384, 5): 0, ("v4", 1024, 768, 5): 0, ("v4", 1024, 768, 13): 0,
    ("mixed", 512, 384, 5): 0, ("mixed", 1024, 768, 5): 0, ("mixed", 1024, 768, 13): 0, ("mixed", 512, 4224, 5): 0,
    ("m8", 512, 384, 5): 0, ("m8", 1024, 768, 5): 0, ("m8", 1024, 768, 13): 0, ("m8", 512, 4224, 5): 0,
}


def shapes_of(pair):
    return SHAPES + ((CHUNK_SHAPE,) if pair != "v4" else ())


def e_range(pair):
    """[lo, hi) of an E block's maximum: k = STEPS / max finite and within 8 x of FLT_MAX (the 4-bit pair: below 2^-123)"""
    steps = np.float32(STEPS[VECTOR_BITS[pair]])
    return float(steps / FLT_MAX), 2.0 ** -123 if pair == "v4" else float(np.float32(8) * steps / FLT_MAX)


# ---------------------------------------------------------------- raw operands
def pack4(q):
    """int8 values in [-7, 7] -> bytes, the even element in the high nibble"""
    q = q.astype(np.uint8)
    return (((q[..., 0::2] & 0xF) << 4) | (q[..., 1::2] & 0xF)).astype(np.uint8)


def unpack4(b):
    hi = (b.astype(np.int8) >> 4).astype(np.int8)
    lo = ((b << 4).astype(np.int8) >> 4).astype(np.int8)
    return np.stack([hi, lo], -1).reshape(*b.shape[:-1], -1)


def elements(bits, q):
    """the signed integers of a raw vector or matrix, whatever its width"""
    return unpack4(q) if bits == 4 else q.view(np.int8)


def _values(rng, bits, shape):
    s = STEPS[bits]
    return rng.integers(-s, s + 1, size=shape).astype(np.int8)


def _ord(rng, n=None):
    return rng.uniform(0.5, 2.0, size=n).astype(np.float32)


def vector(bits, n, kinds, seed):
    """a raw vector of n elements whose block b is of kind kinds[b]: (bytes, scales)"""
    rng = np.random.default_rng([seed, n, bits])
    q = _values(rng, bits, n).reshape(-1, 64)
    if bits == 8:
        q[:, :8] = CARRY
    s = _ord(rng, n // 64)
    for b, kind in enumerate(kinds):
        if kind == "zero":
            q[b], s[b] = 0, 1.0
        elif kind == "small":
            s[b] *= np.float32(2.0 ** -20)
        elif kind == "big":
            s[b] *= np.float32(2.0 ** 20)
        elif kind == "sub":
            s[b] = np.float32(1e-40)
        elif kind == "huge":
            s[b] *= np.float32(1e30)
    q = q.reshape(-1)
    return (pack4(q) if bits == 4 else q), s


def x_vector(pair, n, rot=0, seed=1):
    return vector(VECTOR_BITS[pair], n, [X_KINDS[(b + rot) % 6] for b in range(n // 64)], seed + 16 * rot)


def zero_vector(pair, n):
    return vector(VECTOR_BITS[pair], n, ["zero"] * (n // 64), 0)


def u_vector(pair, n, seed=7):
    kinds = [{"big": "huge"}.get(U_KINDS[b % 16], U_KINDS[b % 16]) for b in range(n // 64)]
    return vector(VECTOR_BITS[pair], n, kinds, 1000 + seed)


def band(pair, kind, i, in_, seed, scale=1.0, t_clear=True):
    """the 64 rows of band row i: int8 values (64, in) and tile scales (in / 64).  `scale` multiplies the scales of H and the large
    scale of M (the loops need them smaller); t_clear=False leaves T's tiles facing `big` non-zero (the loops' x has no such blocks)"""
    bits = MATRIX_BITS[pair]
    rng = np.random.default_rng([seed, i, in_, bits])
    nb = in_ // 64
    facing = [X_KINDS[j % 6] for j in range(nb)]
    q = _values(rng, bits, (64, in_))
    q[q == 0] = 1                                                            # a zero element only where the band says so
    s = _ord(rng, nb)
    e = rng.integers(-20, 21, size=nb)
    k = rng.integers(1, 8, size=nb)

    def clear(j):
        q[:, 64 * j:64 * j + 64] = 0
    if kind in ("N", "N2"):
        s = (np.float32(2.0) ** e.astype(np.float32)) * (np.float32(1.0) + (s - np.float32(0.5)) / np.float32(1.5))
        s[0], s[nb - 1] = np.float32(2.0 ** -20), np.float32(2.0 ** 20) * np.float32(1.25)      # the spread, whatever the draw
    elif kind == "Z":
        q[:], s[:] = 0, 1.0
    elif kind == "Zx":
        for j in range(nb):
            if facing[j] != "zero":
                clear(j)
    elif kind == "T":
        s = (np.float64(T_BASE[pair]) * k).astype(np.float32)
        for j in range(nb):
            if facing[j] == "big" and t_clear:
                clear(j)
    elif kind == "H":
        s = (s.astype(np.float64) * 1e28 * scale).astype(np.float32)
    elif kind == "E":
        n_ord = sum(f == "ord" for f in facing)
        s = (s.astype(np.float64) * E_BASE[pair] / np.sqrt(n_ord / 2.0)).astype(np.float32)
        for j in range(nb):
            if facing[j] in ("small", "big", "sub"):
                clear(j)
    elif kind == "M":
        for j in range(nb):
            s[j] = np.float32(1e-30) if j % 2 == 0 else np.float32(1e20 * scale)
            if j % 2:
                q[:32, 64 * j:64 * j + 64] = 0
    else:
        raise ValueError(kind)
    return q, s.astype(np.float32)


def matrix(pair, out, in_, kinds=None, seed=3, scale=1.0, e_seeds=None, t_clear=True, columns=None):
    """B, out x in: (bytes, tile scales row-major).  kinds: the band kind per 64 rows (default BANDS cycled); e_seeds: band row -> seed of
    an E band (default E_SEEDS); columns: tile column -> "zero" (every tile of it zero, scale 1.0) or one scale for all its tiles"""
    kinds = kinds or [BANDS[i % 8] for i in range(out // 64)]
    q = np.empty((out, in_), np.int8)
    s = np.empty((out // 64, in_ // 64), np.float32)
    for i, kind in enumerate(kinds):
        sd = seed
        if kind == "E":
            sd = e_seeds[i] if e_seeds is not None else E_SEEDS[(pair, out, in_, i)]
        q[64 * i:64 * i + 64], s[i] = band(pair, kind, i, in_, sd, scale, t_clear)
    for j, what in (columns or {}).items():
        if isinstance(what, str):
            q[:, 64 * j:64 * j + 64], s[:, j] = 0, 1.0
        else:
            s[:, j] = np.float32(what)
    q = pack4(q) if MATRIX_BITS[pair] == 4 else q
    return np.ascontiguousarray(q).reshape(-1), s.reshape(-1)


# ---------------------------------------------------------------- the reference: the pinned single operations, composed
class Ref:
    """oracle = oracle.binding.Oracle, m8 = matrix8_helpers.Restate (the restatement behind the m8 fixture)"""

    def __init__(self, oracle, m8):
        self.oracle, self.m8 = oracle, m8

    def mvm(self, pair, B, out, in_, x, rng=None):
        if pair == "v4":
            return self.oracle.m4_mvm(*B, out, in_, *x, rng)
        if pair == "mixed":
            return self.oracle.m4_mvm_v8(*B, out, in_, *x, rng)
        return self.m8.mvm(*B, out, in_, *x, rng)

    def rowdots(self, pair, B, out, in_, x):
        if pair == "v4":
            return self.oracle.m4_rowdots(*B, out, in_, *x)
        if pair == "mixed":
            return self.oracle.m4_rowdots_v8(*B, out, in_, *x)
        return self.m8.rowdots(*B, out, in_, *x)

    def scale_and_add(self, pair, u, v, a, rng=None):
        return (self.oracle.v4_scale_and_add if pair == "v4" else self.oracle.v8_scale_and_add)(*u, *v, float(a), rng)

    def transpose(self, pair, B, rows, cols):
        return (self.m8.transpose if pair == "m8" else self.oracle.m4_transpose)(*B, rows, cols)

    def restore(self, pair, v):
        return (self.oracle.v4_restore if pair == "v4" else self.oracle.v8_restore)(*v)


def find_e_seed(ref, pair, out, in_, i, x, limit=400):
    """the first seed at which the reference's maximum of band row i against x is inside e_range(pair)"""
    lo, hi = e_range(pair)
    for seed in range(limit):
        q, s = band(pair, "E", i, in_, seed)
        q = pack4(q) if MATRIX_BITS[pair] == 4 else q
        d = ref.rowdots(pair, (np.ascontiguousarray(q).reshape(-1), s), 64, in_, x)
        if lo <= float(np.abs(d).max()) < hi:
            return seed
    raise LookupError((pair, out, in_, i))


class Case:
    """one pair at one shape, host side: B, its transpose, NVEC_MAX vectors x (x, a zero vector, x again -- the same object --, then x
    with its block kinds rotated by 1, 2, ...) and u, and the reference's t = B x and r = u + a t per vector (computed on first use)"""

    def __init__(self, ref, pair, out, in_):
        self.ref, self.pair, self.out, self.in_ = ref, pair, out, in_
        self.B = matrix(pair, out, in_)
        self.Bt = ref.transpose(pair, self.B, out, in_)
        x = x_vector(pair, in_)
        self.x = [x, zero_vector(pair, in_), x] + [x_vector(pair, in_, rot) for rot in range(1, NVEC_MAX - 2)]
        self.u = [u_vector(pair, out, seed=j) for j in range(NVEC_MAX)]
        self._t, self._r = {}, {}

    def t(self, j):
        if j not in self._t:
            self._t[j] = self._t[0] if j == 2 and 0 in self._t else self.ref.mvm(self.pair, self.B, self.out, self.in_, self.x[j])
        return self._t[j]

    def r(self, j, a):
        if (j, a) not in self._r:
            self._r[(j, a)] = self.ref.scale_and_add(self.pair, self.u[j], self.t(j), a)
        return self._r[(j, a)]


# ---------------------------------------------------------------- the IHT / GD loops
LOOP_BANDS = {256: ("N", "T", "Z", "M"), 384: ("N", "Z", "Zx", "T", "H", "E")}
LOOP_SCALE = 1e-22                                 # H tiles about 1e6, M's large tiles 1e-2: the loop squares the matrix every iteration
LOOP_Y_SCALE = 2.0 ** -12                          # y small enough that t1's T block is of category T once x is no longer zero
LOOP_ITERATIONS, LOOP_MU = 3, 2.0 ** -8


# Tile columns of Phi that decide what the threshold sees in x after the first iteration (x = mu Phi' y there, t1 being zero): two
# zero columns leave two blocks of x exactly zero in every iteration; the scales of the other two are computed from the reference's
# own t3 for y[0] so that one block of x has a subnormal scale below STEPS / FLT_MAX (k = inf: elements 0) and one has the smallest
# scale with a finite k, whose small elements are non-zero subnormal magnitudes
LOOP_ZERO_COLUMNS, LOOP_T_COLUMN, LOOP_S_COLUMN = (1, 4), 2, 3
LOOP_X_SCALE = {4: {LOOP_T_COLUMN: 1e-39, LOOP_S_COLUMN: 4e-38}, 8: {LOOP_T_COLUMN: 5e-39, LOOP_S_COLUMN: 7e-37}}


def loop_problem(ref, pair, m, n):
    """Phi (m x n, LOOP_BANDS with the columns above), its transpose, and NVEC_MAX measurements y (ordinary blocks times LOOP_Y_SCALE;
    y[1] has a zero block)"""
    ys = []
    for j in range(NVEC_MAX):
        q, s = vector(VECTOR_BITS[pair], m, ["zero" if (j == 1 and b == 1) else "ord" for b in range(m // 64)], 2000 + j)
        ys.append((q, np.where(s == 1.0, s, s * np.float32(LOOP_Y_SCALE)).astype(np.float32)))          # the zero block keeps scale 1.0
    columns = {j: "zero" for j in LOOP_ZERO_COLUMNS}
    columns.update({LOOP_T_COLUMN: 1.0, LOOP_S_COLUMN: 1.0})

    def build():
        Phi = matrix(pair, m, n, kinds=LOOP_BANDS[m], seed=11, scale=LOOP_SCALE, e_seeds={i: 0 for i in range(m // 64)}, t_clear=False,
                     columns=columns)
        return Phi, ref.transpose(pair, Phi, m, n)
    Phi, PhiT = build()
    st3 = loop_reference(ref, pair, Phi, PhiT, ys[0], m, n, 0, 0, iterations=1)[0]["t3"][1]          # t3 = Phi' y with unit columns
    for j, target in LOOP_X_SCALE[VECTOR_BITS[pair]].items():
        columns[j] = target / (float(st3[j]) * LOOP_MU)
    Phi, PhiT = build()
    return Phi, PhiT, ys


def magnitudes(ref, pair, v, n):
    """as the vector classes define them: |restore| for CloverVector4, |q s / 127| for CloverVector8"""
    if VECTOR_BITS[pair] == 4:
        return np.abs(ref.oracle.v4_restore(*v))[:n]
    q = elements(8, v[0]).astype(np.float32)
    return np.abs((q * np.repeat(v[1], 64)) / np.float32(127.0))[:n]


def threshold_stats(ref, pair, v, n, k):
    """what a threshold to the k largest of v meets: tau (the k-th magnitude), the elements equal to it, the non-zero magnitudes"""
    mags = magnitudes(ref, pair, v, n)
    tau = np.sort(mags)[::-1][k - 1]
    return float(tau), int((mags == tau).sum()), int((mags != 0).sum())


def lowest_index_threshold(ref, pair, v, n, k):
    """FAST mode's tie rule on the CPU: everything above the K-th magnitude, then the first ties by index"""
    bits = VECTOR_BITS[pair]
    q = elements(bits, v[0]).astype(np.int8)
    mags = magnitudes(ref, pair, v, n)
    out = q.copy()
    if k < n:
        tau = np.sort(mags)[::-1][k - 1] if k > 0 else np.inf
        keep = mags > tau
        ties = np.flatnonzero(mags == tau)[: max(k - int(keep.sum()), 0)]
        keep[ties] = True
        out[:n] = out[:n] * keep
    return (pack4(out) if bits == 4 else out), v[1]


def loop_reference(ref, pair, Phi, PhiT, y, m, n, K, thr, iterations=LOOP_ITERATIONS, mu=LOOP_MU, x_len=None):
    """the composition of the pinned single operations (test_iht_persistent.py's) -> the final x, t1, t2, t3 and every iteration's
    (there also `pre`, x before the threshold)"""
    x = zero_vector(pair, n)
    steps = []
    for _ in range(iterations):
        t1 = ref.mvm(pair, Phi, m, n, x)
        t2 = ref.scale_and_add(pair, y, t1, -1.0)
        t3 = ref.mvm(pair, PhiT, n, m, t2)
        x = pre = ref.scale_and_add(pair, x, t3, float(mu))
        if thr:
            x = lowest_index_threshold(ref, pair, x, n if x_len is None else x_len, K)
        steps.append(dict(x=x, t1=t1, t2=t2, t3=t3, pre=pre))
    return steps[-1], steps


def block_categories(bits, v):
    """per block of a vector: "Z" (elements 0, scale 1.0), "T" (elements 0, scale below STEPS / FLT_MAX and not 1.0: k = inf) or "" """
    el = elements(bits, v[0]).reshape(-1, 64)
    steps = np.float32(STEPS[bits])
    out = []
    for b in range(el.shape[0]):
        zero = not el[b].any()
        with np.errstate(over="ignore"):
            kinf = np.isinf(steps / v[1][b])
        out.append("Z" if zero and v[1][b] == 1.0 else "T" if zero and kinf and v[1][b] > 0 else "")
    return out
