"""An independent reference of the chain's own random numbers (hmcmt_chain_seed, hmcmt_rng_*, include/hmcmt.h): Philox4x32-10 in
Python integers, the uniforms as exact fractions of 2^53, and the Box-Muller step in numpy's longdouble from those exact uniforms.  It
uses nothing of the library's -- neither its item functions nor its Python side -- and is written from the header's description and
the generator's paper (Salmon, Moraes, Dror, Shaw: Parallel random numbers: as easy as 1, 2, 3, SC'11)."""
import numpy as np

LD = np.longdouble
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
C0_SCALARS = 0xFFFFFFFF
ZCLIP = 2.5
TWO_PI = LD(8) * np.arctan(LD(1))                 # 2 pi to the longdouble's own precision

# Random123's known answers for philox4x32_10 (its kat_vectors): (counter, key, output)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]

# |z - z_ref| of one normal, absolute.  r = sqrt(-2 ln u) <= sqrt(2 * 53 ln 2) = 8.57 since u >= 2^-53.  The fp64 product 2 pi u2
# (with the fp64 2 pi) misses the angle by up to 2 pi 2^-53 + 2.5e-16 = 9.5e-16, which cos passes on at most unchanged: 8.57 * 9.5e-16
# = 8.1e-15.  log, the product by -2, sqrt, cos and the last product add a few ulp of a result of at most 8.57 (ulp(8.57) = 1.8e-15)
# or of a factor of at most 1 (1.1e-16 * 8.57): about 6e-15 together.  Sum 1.4e-14; the tolerance is three times that.
NORMAL_TOL = 4e-14


def philox4x32(c, k, rounds=10):
    c, k = [int(x) for x in c], [int(x) for x in k]
    for _ in range(rounds):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> 32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return tuple(c)


def block(seed, stream, t, c0):
    """the four words of the block (c0, stream, t) under the key seed"""
    return philox4x32((c0, stream, t & MASK, t >> 32), (seed & MASK, seed >> 32))


def u52_k(hi, lo):
    """the 52-bit integer k of U = (2 k + 1) / 2^53"""
    return ((hi >> 6) << 26) | (lo >> 6)


def u52(hi, lo):
    """U as a Python float: 2 k + 1 < 2^53, so the value is exact"""
    return float(2 * u52_k(hi, lo) + 1) * 2.0 ** -53


def normal_of_block(x):
    """the longdouble normal of the block's four words"""
    u1, u2 = LD(u52(x[0], x[1])), LD(u52(x[2], x[3]))
    return np.sqrt(LD(-2) * np.log(u1)) * np.cos(TWO_PI * u2)


def normals(seed, stream, t, n, a0=0):
    """the unclipped normals of the cells a0 .. a0 + n - 1 in draw t, longdouble"""
    return np.array([normal_of_block(block(seed, stream, t, a0 + i)) for i in range(n)], dtype=LD)


def clipped(z):
    return np.clip(z, LD(-ZCLIP), LD(ZCLIP))


def scalars(seed, stream, t, Lmin, Lmax):
    """(L, u) of draw t"""
    x = block(seed, stream, t, C0_SCALARS)
    return Lmin + ((x[2] * (Lmax - Lmin + 1)) >> 32), u52(x[0], x[1])
