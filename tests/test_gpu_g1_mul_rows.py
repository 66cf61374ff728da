"""rhip_g1_mul_rows (variable-base G1 over rows that share a scalar; one GLV decomposition and one set of NAF masks per scalar, one joint
chain per row, one inversion per block) against the CPU oracle (exact integers) and byte for byte against Engine.g1_mul."""
import random

import pytest

from oracle import bn254 as bn
from rabe_amd import Engine

pytestmark = pytest.mark.gpu
R, P = bn.R, bn.P
LAM = 0xb3c4d79d41a917585bfc41088d8daaa78b17ea66b99c90dd          # bn254/constants.h: RB_GLV_LAMBDA, phi(P) = LAM * P
assert (LAM * LAM + LAM + 1) % R == 0
# accumulator equal / opposite to an addend, halves of either sign, a zero half
EDGE = [0, 1, 2, 3, R - 1, R - 2, (R - 1) // 2, LAM, LAM + 1, LAM - 1, LAM + 2, 2 * LAM, 2 * LAM + 1, 2 * LAM - 1, LAM * LAM % R, R - LAM, R - LAM - 1,
        R - LAM + 1, 3 * LAM % R, (1 << 128) - 1, 1 << 129, (1 << 253) + 1]
INF = bytes(64)


def le(k):
    return (k % (1 << 256)).to_bytes(32, "little")


def want(a, k):
    """k * (a * G) as wire bytes"""
    e = a * k % R
    return bn.g1_to_le(bn.g1_mul(bn.G1_GEN, e) if e else None)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def test_edge_scalars_on_generator_random_point_and_infinity(eng):
    """k = 0, 1, 2, r - 1, lambda, lambda +- 1, ..., multiples of r and other words >= r; infinity in"""
    a = 0x1234567890abcdef1234567890abcdef1234567890abcdef % R
    scalars = EDGE + [R, 2 * R, 5 * R, R + 1, R + LAM, (1 << 256) - 1]
    points = [bn.g1_to_le(bn.G1_GEN), bn.g1_to_le(bn.g1_mul(bn.G1_GEN, a)), INF]
    rows = [p for _ in scalars for p in points]
    off = [3 * i for i in range(len(scalars) + 1)]
    got = eng.g1_mul_rows(rows, off, [le(k) for k in scalars])
    assert got == eng.g1_mul(rows, [le(k) for k in scalars for _ in points])
    for i, k in enumerate(scalars):
        assert got[3 * i] == want(1, k), hex(k)
        assert got[3 * i + 1] == want(a, k), hex(k)
        assert got[3 * i + 2] == INF


def test_powers_of_two(eng):
    g = bn.g1_to_le(bn.G1_GEN)
    ks = [le(1 << j) for j in range(254)]
    got = eng.g1_mul_rows([g] * 254, list(range(255)), ks)
    assert got == eng.g1_mul([g] * 254, ks)
    acc = bn.G1_GEN
    for j in range(254):
        assert got[j] == bn.g1_to_le(acc), j
        acc = bn.g1_add(acc, acc)


def test_random_rows_ragged_items(eng):
    """>= 2 000 rows (eight blocks and a tail) in items of 0 .. 300 rows: waves holding one item, several items and item boundaries"""
    rnd = random.Random(20261017)
    sizes = []
    while sum(sizes) < 2100:
        sizes.append(rnd.choice([1, 1, 2, 3, 5, 17, 63, 64, 65, 100, 128, 129, 255, 256, 257, 300, 0, 0, rnd.randrange(1, 131)]))
    sizes += [0, 7]                                          # an empty item next to the end
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    n_rows = off[-1]
    assert n_rows % 256 != 0
    a = [rnd.randrange(1, R) for _ in range(n_rows)]
    for t in rnd.sample(range(n_rows), 9):
        a[t] = 0                                             # infinity among the rows
    g = bn.g1_to_le(bn.G1_GEN)
    pts = eng.g1_mul([g] * n_rows, [le(x) for x in a])       # random points a_t * G
    ks = [rnd.randrange(R) for _ in sizes]
    got = eng.g1_mul_rows(pts, off, [le(k) for k in ks])
    row_k = [ks[i] for i, s in enumerate(sizes) for _ in range(s)]
    assert got == eng.g1_mul(pts, [le(k) for k in row_k])
    for t in range(n_rows):
        assert pts[t] == want(a[t], 1)
        assert got[t] == want(a[t], row_k[t]), t


def test_one_scalar_many_rows(eng):
    """the shape of an authority's call: one scalar against a few hundred users' points"""
    rnd = random.Random(5)
    n = 700
    a = [rnd.randrange(1, R) for _ in range(n)]
    g = bn.g1_to_le(bn.G1_GEN)
    pts = eng.g1_mul([g] * n, [le(x) for x in a])
    k = rnd.randrange(R)
    got = eng.g1_mul_rows(pts, [0, n], [le(k)])
    for t in range(n):
        assert got[t] == want(a[t], k), t


def test_argument_checks(eng):
    g = bn.g1_to_le(bn.G1_GEN)
    with pytest.raises(ValueError):
        eng.g1_mul_rows([g, g], [0, 1], [le(1)])
    with pytest.raises(ValueError):
        eng.g1_mul_rows([g, g], [0, 2, 1, 2], [le(1)] * 3)
    assert eng.g1_mul_rows([], [0], []) == []
