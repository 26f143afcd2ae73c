"""Shared pieces of tests/test_gemm8_cpu.py and tests/test_gemm8.py (clm8_gemm, clm8_gemm_i32, clm4_gemm_m8).

- Restate: tests/gemm8_restate.c, the plain-C restatement of the three definitions, built as cc -O2 -ffp-contract=off -fno-fast-math, once
  plain (`rg`) and once with -mfma -fopenmp on at most 16 threads (`rgp`); test_gemm8_cpu.py checks that the two builds agree bit for bit.
- inputs: bytes over the whole range (-128 and the nibble -8 included), scales spread over the binades 2^-40 .. 2^40, different in every
  tile and every K-block, and a `tiny` kind whose 4-bit operand has scales near 2^-120.
- exact64 / bound: the float64 evaluation (same fp32-rounded c_b, promoted, order-free sum) and the derived bound against it.
- reference(): every restatement result is computed once per process and handed out read-only."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

RESTATE = Path(__file__).parent / "gemm8_restate.c"
U = 2.0 ** -24              # fp32 unit roundoff
R127 = np.float32(1.0) / np.float32(127.0)
R7 = np.float32(1.0) / np.float32(7.0)

_i8 = C.POINTER(C.c_int8)
_u8 = C.POINTER(C.c_uint8)
_i32 = C.POINTER(C.c_int32)
_fp = C.POINTER(C.c_float)
_u64 = C.c_uint64


def _p(a, t):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(t)


class Restate:
    def __init__(self, so: Path):
        self.L = C.CDLL(str(so))
        for name in ("rg8_gemm", "rg8_gemm_i32", "rg8_gemm_m8", "rg8_gemm_m8_i32", "rg8_fold_step"):
            getattr(self.L, name).restype = None

    def gemm(self, qA, sA, M, K, qB, sB, N):
        c = np.zeros((M, N), np.float32)
        self.L.rg8_gemm(_p(qA, _i8), _p(sA, _fp), _u64(M), _u64(K), _p(qB, _i8), _p(sB, _fp), _u64(N), _p(c, _fp))
        return c

    def gemm_i32(self, qA, M, K, qB, N, kb_begin, kb_count):
        s = np.zeros((M, N), np.int32)
        self.L.rg8_gemm_i32(_p(qA, _i8), _u64(M), _u64(K), _p(qB, _i8), _u64(N), _u64(kb_begin), _u64(kb_count), _p(s, _i32))
        return s

    def gemm_m8(self, qA4, sA, M, K, qB, sB, N):
        c = np.zeros((M, N), np.float32)
        self.L.rg8_gemm_m8(_p(qA4, _u8), _p(sA, _fp), _u64(M), _u64(K), _p(qB, _i8), _p(sB, _fp), _u64(N), _p(c, _fp))
        return c

    def gemm_m8_i32(self, qA4, M, K, qB, N, kb_begin, kb_count):
        s = np.zeros((M, N), np.int32)
        self.L.rg8_gemm_m8_i32(_p(qA4, _u8), _u64(M), _u64(K), _p(qB, _i8), _u64(N), _u64(kb_begin), _u64(kb_count), _p(s, _i32))
        return s

    def fold_step(self, Sb, sA, sB, M, N, K, b, c):
        """c = fmaf(c_b, (float)Sb, c) in place, the 8 x 8 factor"""
        self.L.rg8_fold_step(_p(Sb, _i32), _p(sA, _fp), _p(sB, _fp), _u64(M), _u64(N), _u64(K), _u64(b), _p(c, _fp))


@functools.lru_cache(maxsize=None)
def _build(out: Path, flags: tuple) -> Path:
    subprocess.run(["cc", "-O2", "-ffp-contract=off", "-fno-fast-math", *flags, "-fPIC", "-shared", "-o", str(out), str(RESTATE), "-lm"], check=True)
    return out


def build_restate(base: Path, parallel: bool) -> Restate:
    return Restate(_build(base / ("librg8_omp.so" if parallel else "librg8.so"), ("-mfma", "-fopenmp") if parallel else ()))


@pytest.fixture(scope="session")
def rg(tmp_path_factory):
    return build_restate(tmp_path_factory.getbasetemp(), parallel=False)


@pytest.fixture(scope="session")
def rgp(tmp_path_factory):
    return build_restate(tmp_path_factory.getbasetemp(), parallel=True)


# ---------------------------------------------------------------- inputs
def bytes8(rng, rows, K):
    """rows x K int8 over the whole range; -128 (which no quantiser writes, and the definition covers) is planted in every row"""
    q = rng.integers(-128, 128, size=(rows, K), dtype=np.int16).astype(np.int8)
    q[np.arange(rows), rng.integers(0, K, size=rows)] = -128
    return np.ascontiguousarray(q.reshape(-1))


def nibbles4(rng, rows, K):
    """rows x K / 2 packed bytes, every byte pattern: both nibbles run over -8 .. 7"""
    b = rng.integers(0, 256, size=(rows, K // 2), dtype=np.uint16).astype(np.uint8)
    b[np.arange(rows), rng.integers(0, K // 2, size=rows)] = 0x88            # -8 beside -8
    return np.ascontiguousarray(b.reshape(-1))


def unpack_nibbles(b, rows, K):
    """the int8 values of a packed image (element 2p in the high nibble of byte p), by a route of its own: numpy shifts"""
    b = b.reshape(rows, K // 2)
    hi = (b.view(np.int8) >> 4).astype(np.int8)                                 # arithmetic shift: the sign comes along
    lo = ((b << 4).astype(np.uint8).view(np.int8) >> 4).astype(np.int8)
    out = np.empty((rows, K), np.int8)
    out[:, 0::2], out[:, 1::2] = hi, lo
    return out


def scales(rng, rows, K, lo=-40, hi=40):
    """(rows / 64) x (K / 64) positive fp32 scales 2^U(lo, hi): all different, all binades of the range"""
    return np.exp2(rng.uniform(lo, hi, size=(rows // 64) * (K // 64))).astype(np.float32)


KINDS = ("wide", "tiny")


@functools.lru_cache(maxsize=None)
def operands(M, N, K, kind="wide"):
    """(qA8, sA, qA4, sA4, qB8, sB): an 8-bit and a 4-bit A, an 8-bit B.  tiny: A's scales lie near 2^-120 and B's within 2^-8 .. 2^8, so
    every c_b of the mixed form is far below the smallest factor whose sixteenth is exact"""
    rng = np.random.default_rng(M * 1_000_003 + N * 1009 + K + (7 if kind == "tiny" else 0))
    qA8, qA4, qB8 = bytes8(rng, M, K), nibbles4(rng, M, K), bytes8(rng, N, K)
    if kind == "tiny":
        sA, sA4, sB = scales(rng, M, K, -122, -118), scales(rng, M, K, -122, -118), scales(rng, N, K, -8, 8)
    else:
        sA, sA4, sB = scales(rng, M, K), scales(rng, M, K), scales(rng, N, K)
    out = (qA8, sA, qA4, sA4, qB8, sB)
    for a in out:
        a.setflags(write=False)
    return out


def factors(sA, sB, M, N, K, mixed):
    """c_b as the definition rounds it, fp32 [M/64, N/64, K/64]: numpy float32 products are single IEEE operations"""
    nb = K // 64
    fa = (sA.reshape(M // 64, nb) * (R7 if mixed else R127)).astype(np.float32)
    fb = (sB.reshape(N // 64, nb) * R127).astype(np.float32)
    return (fa[:, None, :] * fb[None, :, :]).astype(np.float32)


def sixteenth_is_exact(c):
    """the kernel's test for folding the 2^-4 of the nibble image into c_b (gemm8.hip)"""
    return (np.abs(c) >= np.float32(2.0 ** -100)) | (c == 0)


def block_sums(a, b, M, N, K):
    """int64 [M, N, K/64] of the int8 matrices a (M x K) and b (N x K)"""
    nb = K // 64
    return np.einsum("ibk,jbk->ijb", a.reshape(M, nb, 64).astype(np.int64), b.reshape(N, nb, 64).astype(np.int64))


def exact64(S, c, M, N, K):
    """(value, sum of magnitudes) in float64 from block sums S [M, N, nb] and factors c [M/64, N/64, nb]"""
    terms = S.astype(np.float64) * np.repeat(np.repeat(c.astype(np.float64), 64, axis=0), 64, axis=1)
    return terms.sum(axis=2), np.abs(terms).sum(axis=2)


def bound(absum, K):
    """|C - exact| <= (nb + 4) 2^-24 sum_b |c_b S_b|: c_b and (float)S_b enter exactly, every fma of the chain rounds once (relative error
    <= u), so the standard bound of a recursive sum of nb terms is gamma_nb = nb u / (1 - nb u) times the sum of the magnitudes; the 4
    covers the second-order part for every nb < 2^20.  Derived, not measured."""
    return (K // 64 + 4) * U * absum


# ---------------------------------------------------------------- references, once per process
_REFS = {}


def reference(R, call, M, N, K, kind="wide", kb=None):
    """call: "gemm" | "gemm_m8" | "i32" (kb = (begin, count)); read-only arrays"""
    key = (call, M, N, K, kind, kb)
    if key not in _REFS:
        qA8, sA, qA4, sA4, qB8, sB = operands(M, N, K, kind)
        if call == "gemm":
            r = R.gemm(qA8, sA, M, K, qB8, sB, N)
        elif call == "gemm_m8":
            r = R.gemm_m8(qA4, sA4, M, K, qB8, sB, N)
        else:
            r = R.gemm_i32(qA8, M, K, qB8, N, *kb)
        r.setflags(write=False)
        _REFS[key] = r
    return _REFS[key]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
