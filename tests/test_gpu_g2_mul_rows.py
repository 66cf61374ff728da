"""rhip_g2_mul_rows (variable-base G2 over rows that share a scalar; four-way split over the twist endomorphism, bn254/gls4.h) against the
CPU oracle (exact integers) and byte for byte against Engine.g2_mul (the binary chain)."""
import random

import pytest

from oracle import bn254 as bn
from rabe_amd import Engine

pytestmark = pytest.mark.gpu
R, P = bn.R, bn.P
LAM = P % R
EDGE = [0, 1, 2, 3, R - 1, R - 2, (R - 1) // 2, LAM, LAM + 1, LAM - 1, LAM * LAM % R, LAM**3 % R, R - LAM]
INF = bytes(128)


def le(k):
    return (k % (1 << 256)).to_bytes(32, "little")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def test_edge_scalars_on_generator_member_and_infinity(eng):
    """accumulator equal / opposite to an addend (k = 1, 2, L +- 1, ...), k = 0, multiples of r and other words >= r, infinity in"""
    a = 0x1234567890abcdef1234567890abcdef1234567890abcdef % R
    member = bn.g2_mul(bn.G2_GEN, a)
    scalars = EDGE + [R, 2 * R, 5 * R, R + 1, (1 << 256) - 1]
    points = [bn.g2_to_le(bn.G2_GEN), bn.g2_to_le(member), INF]
    # one item per scalar, its rows = the three points
    rows = [p for _ in scalars for p in points]
    off = [3 * i for i in range(len(scalars) + 1)]
    got = eng.g2_mul_rows(rows, off, [le(k) for k in scalars])
    ref = eng.g2_mul(rows, [le(k) for k in scalars for _ in points])
    assert got == ref
    for i, k in enumerate(scalars):
        assert got[3 * i] == bn.g2_to_le(bn.g2_mul(bn.G2_GEN, k % R) if k % R else None), hex(k)
        assert got[3 * i + 1] == bn.g2_to_le(bn.g2_mul(bn.G2_GEN, a * k % R) if k % R else None), hex(k)
        assert got[3 * i + 2] == INF


def test_powers_of_two(eng):
    g = bn.g2_to_le(bn.G2_GEN)
    ks = [le(1 << j) for j in range(254)]
    got = eng.g2_mul_rows([g] * 254, list(range(255)), ks)
    assert got == eng.g2_mul([g] * 254, ks)
    acc = bn.G2_GEN
    for j in range(254):
        assert got[j] == bn.g2_to_le(acc), j
        acc = bn.g2_add(acc, acc)


def test_random_rows_ragged_items(eng):
    """>= 2 000 rows in items of 1 .. 130 rows (and a few empty items): waves holding one item, several items and item boundaries"""
    rnd = random.Random(20261016)
    sizes = []
    while sum(sizes) < 2100:
        sizes.append(rnd.choice([1, 1, 2, 3, 5, 17, 63, 64, 65, 100, 128, 129, 130, 0, rnd.randrange(1, 131)]))
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    n_rows = off[-1]
    a = [rnd.randrange(1, R) for _ in range(n_rows)]
    for t in rnd.sample(range(n_rows), 9):
        a[t] = 0                                             # infinity among the rows
    g = bn.g2_to_le(bn.G2_GEN)
    pts = eng.g2_mul([g] * n_rows, [le(x) for x in a])       # members: a_t * G (the binary chain, pinned against the oracle elsewhere)
    ks = [rnd.randrange(R) for _ in sizes]
    got = eng.g2_mul_rows(pts, off, [le(k) for k in ks])
    row_k = [ks[i] for i, s in enumerate(sizes) for _ in range(s)]
    assert got == eng.g2_mul(pts, [le(k) for k in row_k])
    for t in range(n_rows):
        e = a[t] * row_k[t] % R
        assert got[t] == bn.g2_to_le(bn.g2_mul(bn.G2_GEN, e) if e else None), t


def test_argument_checks(eng):
    g = bn.g2_to_le(bn.G2_GEN)
    with pytest.raises(ValueError):
        eng.g2_mul_rows([g, g], [0, 1], [le(1)])
    with pytest.raises(ValueError):
        eng.g2_mul_rows([g, g], [0, 2, 1, 2], [le(1)] * 3)
    assert eng.g2_mul_rows([], [0], []) == []
