"""TEST INFRASTRUCTURE: scalars that aim at the window walks of rabe_amd/csrc/bn254/table_walk.h -- the constructions
tests/test_gpu_g1_walk_forms.py makes for the signed 20-bit walk, for any window width.  All below r."""
import random

from oracle import bn254 as bn

R = bn.R


def common():
    return [0, 1, 2, R - 1, R - 2, 1 << 253, ((1 << 254) - 1) % R]


def windows(w):
    return (254 + w - 1) // w


def edge(w):
    """every digit at half; every digit at half + 1 (a signed walk's carry runs through all windows); one non-zero window at each
    position (the last of them: only the top window); the low 1 .. 3 windows zero"""
    rnd = random.Random("walk edges %d" % w)
    half, n = 1 << (w - 1), windows(w)
    out = [sum(half << (w * i) for i in range(n - 1)), sum((half + 1) << (w * i) for i in range(n - 1))]
    for pos in range(n):
        lim = (1 << w) if pos < n - 1 else (R >> (w * pos)) + 1          # the top window of a scalar below r
        out.append(rnd.randrange(1, lim) << (w * pos))
    for j in (1, 2, 3):
        k = rnd.randrange(1 << 250, R)
        out.append((k >> (w * j)) << (w * j))
    assert all(0 < k < R for k in out)
    return out


def dense(w):
    """more of the same at every position: the digits 1, half, half + 1 and 2^w - 1 alone, and the largest top window"""
    half, n = 1 << (w - 1), windows(w)
    out = [d << (w * pos) for pos in range(n - 1) for d in (1, half, half + 1, (1 << w) - 1)]
    out += [1 << (w * (n - 1)), (R >> (w * (n - 1))) << (w * (n - 1))]
    assert all(0 < k < R for k in out)
    return out
