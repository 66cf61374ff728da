"""The four-way split of a G2 scalar (bn254/gls4.h) through rabe_fr_split4, against Python integers -- no GPU.

k = k0 + k1 L + k2 L^2 + k3 L^3 (mod r) with L = p mod r, the eigenvalue of the twist endomorphism psi on G2.  Whatever the rounding, the
relation must hold exactly; the SIZE of the sub-scalars is what the kernel's chain length (RB_GLS4_BITS, constants.h) assumes.  That bound
is derived here from the generated basis, not read off the routine's outputs: with exact nearest-integer rounding |k_i| is at most half the
absolute column sum of the basis (Babai's round-off); the routine rounds c_j = floor((k g_j + 2^255) / 2^256) with a truncated multiplier
g_j = floor(2^256 |A_j| / D), which is off by less than k / 2^256 < 1/4 (k < r < 2^254) on top of the 1/2 -- 3/4 of the column sum in all."""
import ctypes
import os
import random
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 4965661367192848881
P = 36 * U**4 + 36 * U**3 + 24 * U**2 + 6 * U + 1
R = 36 * U**4 + 36 * U**3 + 18 * U**2 + 6 * U + 1
LAM = P % R


def _constants():
    return open(os.path.join(ROOT, "rabe_amd", "csrc", "bn254", "constants.h")).read()


def _macro_ints(name, words):
    """the integers of a (nested) brace list of 32-bit little-endian limbs, `words` limbs each"""
    line = re.search(r"^#define %s (.*)$" % name, _constants(), flags=re.M).group(1).split("//")[0]
    limbs = [int(x, 16) for x in re.findall(r"0x([0-9a-f]{8})u", line)]
    assert len(limbs) % words == 0
    return [sum(l << (32 * i) for i, l in enumerate(limbs[j:j + words])) for j in range(0, len(limbs), words)]


def _lib():
    from rabe_amd.hostlib import _lib as load
    return load()


def split4(lib, k):
    mag = (ctypes.c_uint8 * 64)()
    neg = (ctypes.c_uint8 * 4)()
    assert lib.rabe_fr_split4((k % (1 << 256)).to_bytes(32, "little"), mag, neg) == 0
    out = []
    for i in range(4):
        m = int.from_bytes(bytes(mag[16 * i:16 * i + 16]), "little")
        assert neg[i] in (0, 1)
        out.append(-m if neg[i] else m)
    return out


def _basis_and_bound():
    """the basis back out of RB_GLS4_N (N[j][i] = -sign(A_j) B[j][i] mod 2^128) and the bound its column sums give"""
    n = _macro_ints("RB_GLS4_N", 4)
    assert len(n) == 16
    rows = [[(v - (1 << 128) if v >> 127 else v) for v in n[4 * j:4 * j + 4]] for j in range(4)]
    for row in rows:          # every row (up to the folded sign) lies in the lattice sum b_i L^i = 0 mod r
        assert sum(b * LAM**i for i, b in enumerate(row)) % R == 0
    col = [sum(abs(rows[j][i]) for j in range(4)) for i in range(4)]
    return rows, max((3 * c + 3) // 4 for c in col)          # ceil(3/4 column sum)


EDGE = [0, 1, 2, 3, R - 1, R - 2, (R - 1) // 2, LAM, LAM + 1, LAM - 1, LAM * LAM % R, LAM**3 % R, R - LAM]


def test_lambda_constant():
    assert _macro_ints("RB_GLS4_LAMBDA", 8) == [LAM]
    assert (LAM**4 - LAM**2 + 1) % R == 0          # psi satisfies the 12th cyclotomic polynomial on G2


def test_split_relation_and_bound():
    lib = _lib()
    _, bound = _basis_and_bound()
    bits = int(re.search(r"^#define RB_GLS4_BITS (\d+)", _constants(), flags=re.M).group(1))
    print("bound bits", bound.bit_length(), "RB_GLS4_BITS", bits)
    assert bits >= bound.bit_length()
    assert (bits + 32) // 32 <= 3          # NAF digits up to bit `bits` fit the three mask words per sub-scalar
    rng = random.Random(20261016)
    ks = EDGE + [1 << j for j in range(254)] + [rng.randrange(R) for _ in range(10000)]
    worst = 0
    for k in ks:
        s = split4(lib, k)
        assert sum(x * LAM**i for i, x in enumerate(s)) % R == k % R, hex(k)
        worst = max(worst, max(abs(x) for x in s))
        assert max(abs(x) for x in s) <= bound, hex(k)
    print("largest |k_i| seen: %d bits" % worst.bit_length())
    assert worst < 1 << bits


def test_split_reduces_any_256_bit_word():
    """like the engine's scalar loads, the split brings a word >= r below r first: multiples of r split as 0"""
    lib = _lib()
    for k in (R, 2 * R, 5 * R, (1 << 256) - 1, R + 7):
        s = split4(lib, k)
        assert sum(x * LAM**i for i, x in enumerate(s)) % R == k % R
    assert split4(lib, R) == [0, 0, 0, 0] and split4(lib, 5 * R) == [0, 0, 0, 0]


def test_small_scalars_stay_whole():
    lib = _lib()
    for k in (1, 2, 3, 1000, U):
        assert split4(lib, k) == [k, 0, 0, 0]


def test_constants_are_what_the_generator_emits():
    """no hand-typed constants: the RB_GLS4_* lines of constants.h are those tools/gen_constants.py writes now"""
    src = open(os.path.join(ROOT, "tools", "gen_constants.py")).read()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "tools"))
        os.makedirs(os.path.join(tmp, "rabe_amd", "csrc", "bn254"))
        open(os.path.join(tmp, "tools", "gen_constants.py"), "w").write(src)
        subprocess.run([sys.executable, os.path.join(tmp, "tools", "gen_constants.py")], check=True, capture_output=True, timeout=600)
        fresh = open(os.path.join(tmp, "rabe_amd", "csrc", "bn254", "constants.h")).read()
    pick = lambda text: [l for l in text.splitlines() if "RB_GLS4_" in l]
    assert pick(fresh) and pick(fresh) == pick(_constants())
