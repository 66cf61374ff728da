"""GPU: the G2 and Gt fixed-base table entry points on the edge scalars of the window walks (rabe_amd/csrc/bn254/table_walk.h), byte for
byte against oracle.bn254.  rhip_g2_table_mul on the 8-bit and on the 16-bit table (128-thread blocks with a shared inversion: 1, 127,
128, 129 and 257 rows); rhip_gt_table_pow on the 8-bit table (64-thread blocks: 1, 63, 64 and 65 rows) -- that entry point reads the
8-bit table whether or not the handle has 16-bit windows, so it is called before and after add_w16 and has to give the same bytes.

The scalars are tests/walk_scalars.py's edge list for 8-bit and 16-bit windows (0, 1, 2, r - 1, r - 2, 2^253, 2^254 - 1 mod r; every
digit at half and at half + 1, one non-zero window at each position, low windows zero, only the top window: 65 in all), padded with
seeded random scalars.  Every
row count takes the head of one list, so each expected value is computed once per module: as a sum of oracle-made 8-bit window
entries in G2, by the oracle's power in Gt."""
import random

import pytest

from oracle import bn254 as bn
from tests import walk_scalars as ws

pytestmark = pytest.mark.gpu
R = bn.R
G2_ROWS = (1, 127, 128, 129, 257)
GT_ROWS = (1, 63, 64, 65)


def word(k):
    return int(k).to_bytes(32, "little")


EDGE = ws.common() + ws.edge(8) + ws.edge(16)          # 7 + 37 + 21: the 65 rows of the largest Gt call hold them all


def pick(n, seed):
    """the edge scalars, then seeded random ones up to n"""
    rnd = random.Random(seed)
    return EDGE + [rnd.randrange(R) for _ in range(n - len(EDGE))]


@pytest.fixture(scope="module")
def eng():
    from rabe_amd import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def g2_case():
    base = bn.g2_mul(bn.G2_GEN, 0x5EED2)
    rows, b = [], base
    for _ in range(32):                                          # (d 2^(8 i)) * base, d = 1 .. 255, by the oracle's own addition
        row, acc = [None], None
        for _d in range(255):
            acc = bn.g2_add(acc, b)
            row.append(acc)
        rows.append(row)
        b = bn.g2_add(row[-1], b)
    ks = pick(max(G2_ROWS), "g2 edges")
    want = []
    for k in ks:
        acc, x = None, k
        for row in rows:
            if x & 255:
                acc = bn.g2_add(acc, row[x & 255])
            x >>= 8
        want.append(bn.g2_to_le(acc))
    assert want[0] == bytes(128) and want[1] == bn.g2_to_le(base) and want[3] == bn.g2_to_le(bn.g2_neg(base))
    return base, ks, want


@pytest.fixture(scope="module")
def gt_case():
    base = bn.gt_pow(bn.pairing(bn.G1_GEN, bn.G2_GEN), 0x5EED7)
    ks = pick(max(GT_ROWS), "gt edges")
    want = [bn.gt_to_le(bn.gt_pow(base, k)) for k in ks]
    assert want[0] == bn.gt_to_le(bn.FP12_ONE) and want[1] == bn.gt_to_le(base) and want[3] == bn.gt_to_le(bn.gt_inv(base))
    return base, ks, want


def differing(got, want):
    return [t for t in range(max(len(got), len(want))) if t >= len(got) or t >= len(want) or got[t] != want[t]]


def test_g2_table_mul_on_8_bit_and_16_bit_windows(eng, g2_case):
    base, ks, want = g2_case
    tab = eng.g2_table(bn.g2_to_le(base))
    try:
        for n in G2_ROWS:
            assert differing(tab.mul([word(k) for k in ks[:n]]), want[:n]) == [], "8-bit windows, %d rows" % n
        tab.add_w16()
        for n in G2_ROWS:
            assert differing(tab.mul([word(k) for k in ks[:n]]), want[:n]) == [], "16-bit windows, %d rows" % n
    finally:
        tab.destroy()


def test_gt_table_pow_on_8_bit_windows(eng, gt_case):
    base, ks, want = gt_case
    tab = eng.gt_table(bn.gt_to_le(base))
    try:
        for n in GT_ROWS:
            assert differing(tab.mul([word(k) for k in ks[:n]]), want[:n]) == [], "%d rows" % n
        tab.add_w16()
        assert differing(tab.mul([word(k) for k in ks]), want) == [], "with 16-bit windows on the handle"
    finally:
        tab.destroy()
