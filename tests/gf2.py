"""The step of the XORShift128+ generator as a 64 x 64 matrix over GF(2), written independently of the library (clover_amd/csrc/rng_device.h
states the same facts): a draw never reads part1, so each of the four generator lanes is one 64-bit word a with  n = T(a), out = n + a,
a <- n.  After e >= 1 draws a lane holds part2 = T^e(a), part1 = T^(e - 1)(a).  T^e by square and multiply; a matrix is its 64 columns
(column i = the image of bit i) as Python integers."""
import numpy as np

MASK = (1 << 64) - 1


def step(a):
    t = (a ^ (a << 23)) & MASK
    return (t ^ a ^ (t >> 18) ^ (a >> 5)) & MASK


def apply(M, v):
    r, i = 0, 0
    while v:
        if v & 1:
            r ^= M[i]
        v >>= 1
        i += 1
    return r


def matmul(M, N):
    return [apply(M, c) for c in N]


T = [step(1 << i) for i in range(64)]
IDENTITY = [1 << i for i in range(64)]


def power(e):
    R, B = IDENTITY, T
    while e:
        if e & 1:
            R = matmul(B, R)
        B = matmul(B, B)
        e >>= 1
    return R


def advance_keys(keys, e):
    """(part1[4], part2[4]) as clv_rng_get returns them, `e` draws further on"""
    if e == 0:
        return np.array(keys[0], np.uint64), np.array(keys[1], np.uint64)
    M = power(e - 1)
    p1 = [apply(M, int(a)) for a in keys[1]]
    return np.array(p1, np.uint64), np.array([step(a) for a in p1], np.uint64)
