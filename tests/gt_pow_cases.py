"""Inputs shared by the tests of the Gt power over a four-way Frobenius split (bn254/gtpow4.h): tests/test_gt_pow_split4.py on the CPU and
tests/test_gpu_gt_pow_rows.py on the device.  Scalars are raw 256-bit words: the routine accepts any of them."""
import functools
import random

from oracle import bn254 as bn

LAMBDA = bn.P % bn.R          # the power Frobenius is on Gt
RND = random.Random(0x67747034)

SPECIAL_SCALARS = [0, 1, 2, bn.R - 1, bn.R, bn.R + 1, (1 << 256) - 1, LAMBDA, LAMBDA - 1, LAMBDA + 1, pow(LAMBDA, 2, bn.R), pow(LAMBDA, 3, bn.R),
                   1 << 64, (1 << 65) - 1]
RANDOM_SCALARS = [RND.randrange(1 << 256) if i % 4 == 0 else RND.randrange(bn.R) for i in range(32)]
SCALARS = SPECIAL_SCALARS + RANDOM_SCALARS


def le(x):
    return int(x).to_bytes(32, "little")


@functools.lru_cache(maxsize=None)
def bases():
    """1, e(g1, g2) and three other pairing outputs (one from its own Miller loop, two as powers of e(g1, g2) = pairings of multiples)"""
    e = bn.pairing(bn.G1_GEN, bn.G2_GEN)
    other = bn.pairing(bn.g1_mul(bn.G1_GEN, RND.randrange(1, bn.R)), bn.g2_mul(bn.G2_GEN, RND.randrange(1, bn.R)))
    return [bn.GT_ONE, e, other, bn.gt_pow(e, RND.randrange(1, bn.R)), bn.gt_pow(e, RND.randrange(1, bn.R))]


def expected(a, k, invert, mul):
    """the oracle's (mul *) a^(+-k)"""
    p = bn.gt_pow(a, (-k if invert else k) % bn.R)
    return bn.gt_to_le(bn.gt_mul(mul, p) if mul is not None else p)
