"""rhip_gt_multiexp_rows (Gt multi-exponentiation per item over width-4 signed windows, bn254/gtmexp4.h) byte for byte against rhip_gt_pow ->
rhip_gt_inv -> rhip_gt_product -> rhip_gt_mul on the same inputs, in all four (mul, invert) modes, and against the CPU oracle for a handful of
items."""
import ctypes
import random

import pytest

from oracle import bn254 as bn
from rabe_amd import Engine
from tests import gt_pow_cases as gc

pytestmark = pytest.mark.gpu
ONE = bn.gt_to_le(bn.GT_ONE)
MODES = [(False, False), (False, True), (True, False), (True, True)]          # (mul given, invert)
EXTRA_SCALARS = [0, 1, bn.R - 1, bn.R, (1 << 256) - 1, 7, 8, 9]


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def pool(eng):
    """400 members of Gt: the oracle's five bases, then powers of e(g1, g2) made on the device by the window routine"""
    rnd = random.Random(0x6d726f77)
    base = [bn.gt_to_le(a) for a in gc.bases()]
    more = eng.gt_pow([base[1]] * 395, [gc.le(rnd.randrange(1, bn.R)) for _ in range(395)])
    return base + more


class Case:
    """one set of rows; the powers a[t]^k[t] and their inverses are computed once and shared by the four modes and every chunking"""

    def __init__(self, eng, rows, scalars, off, mul):
        self.rows, self.ks, self.off, self.mul = rows, [gc.le(k) for k in scalars], off, mul
        self.scalars = scalars
        self.n = len(off) - 1
        pw = eng.gt_pow(rows, self.ks)
        self.prod = {False: self._product(eng, pw), True: self._product(eng, eng.gt_inv(pw))}
        self.with_mul = {inv: eng.gt_mul(mul, p) for inv, p in self.prod.items()}

    def _product(self, eng, elems):
        d_off, d_a, out = eng.upload_u32(self.off), eng.upload(b"".join(elems)), eng.alloc(self.n * 384)
        eng._check(eng.lib.rhip_gt_product(eng.ctx, ctypes.c_size_t(self.n), d_off.ptr, d_a.ptr, out.ptr))
        raw = eng.download(out, self.n * 384)
        return [raw[384 * i:384 * i + 384] for i in range(self.n)]

    def want(self, with_mul, invert):
        return self.with_mul[invert] if with_mul else self.prod[invert]

    def got(self, eng, with_mul, invert, chunk_terms=0):
        return eng.gt_multiexp_rows(self.rows, self.off, self.ks, mul=self.mul if with_mul else None, invert=invert, chunk_terms=chunk_terms)


@pytest.fixture(scope="module")
def one_row_each(eng, pool):
    """70 items of one row -- a wave and a tail, every lane with its own digits: the 46 scalars of the CPU test, the special words and 16 more
    random ones; the base 1 and the oracle's bases sit under the first twenty"""
    rnd = random.Random(70)
    scalars = gc.SCALARS + EXTRA_SCALARS + [rnd.randrange(bn.R) for _ in range(16)]
    assert len(scalars) == 70
    rows = [pool[i % 5] if i < 20 else pool[i] for i in range(70)]
    return Case(eng, rows, scalars, list(range(71)), [pool[399 - i] for i in range(70)])


@pytest.fixture(scope="module")
def one_item_of_130(eng, pool):
    rnd = random.Random(130)
    scalars = [rnd.randrange(1 << 256) if i % 9 == 0 else rnd.randrange(bn.R) for i in range(130)]
    return Case(eng, pool[5:135], scalars, [0, 130], [pool[200]])


RAGGED = [0, 0, 1, 9, 2, 0, 3, 4, 0, 0, 5, 6, 7, 8, 9, 1, 2, 3, 0, 4] + [(3 * i + 1) % 10 for i in range(48)] + [9, 0]


@pytest.fixture(scope="module")
def ragged(eng, pool):
    """70 items of 0 to 9 rows; items without rows at the front, in the middle and at the end"""
    assert len(RAGGED) == 70 and RAGGED[0] == RAGGED[1] == RAGGED[5] == RAGGED[8] == RAGGED[9] == RAGGED[-1] == 0 and max(RAGGED) == 9
    off = [0]
    for c in RAGGED:
        off.append(off[-1] + c)
    assert off[-1] <= 395
    rnd = random.Random(0x726167)
    scalars = [rnd.randrange(bn.R) for _ in range(off[-1])]
    return Case(eng, pool[5:5 + off[-1]], scalars, off, [pool[399 - i] for i in range(70)])


@pytest.mark.parametrize("with_mul,invert", MODES)
def test_70_items_of_one_row(eng, one_row_each, with_mul, invert):
    c = one_row_each
    got = c.got(eng, with_mul, invert)
    assert got == c.want(with_mul, invert)
    for i in (1, 3, 6, 7, 12, 46, 47, 48, 50, 51, 53):          # 1, r - 1, 2^256 - 1, lambda, 2^64;  0, 1, r - 1, 2^256 - 1, 7, 9
        mul = bn.gt_from_le(c.mul[i]) if with_mul else None
        assert got[i] == gc.expected(bn.gt_from_le(c.rows[i]), c.scalars[i], invert, mul), hex(c.scalars[i])
    assert len(set(got)) > 35          # real results, not a wall of ones


@pytest.mark.parametrize("with_mul,invert", MODES)
def test_one_item_of_130_rows_under_every_chunking(eng, one_item_of_130, with_mul, invert):
    c = one_item_of_130
    want = c.want(with_mul, invert)
    assert want != [ONE]
    for chunk in (0, 1, 2, 3, 7, 130):
        assert c.got(eng, with_mul, invert, chunk) == want, chunk


@pytest.mark.parametrize("with_mul,invert", MODES)
def test_ragged_items_with_two_rows_per_lane(eng, ragged, with_mul, invert):
    c = ragged
    got = c.got(eng, with_mul, invert, 2)
    assert got == c.want(with_mul, invert)
    for i, cnt in enumerate(RAGGED):
        if cnt == 0:
            assert got[i] == (c.mul[i] if with_mul else ONE)
    # an item of three rows against the oracle
    i = RAGGED.index(3)
    acc = bn.gt_from_le(c.mul[i]) if with_mul else bn.GT_ONE
    for t in range(c.off[i], c.off[i + 1]):
        acc = bn.gt_mul(acc, bn.gt_pow(bn.gt_from_le(c.rows[t]), (-c.scalars[t] if invert else c.scalars[t]) % bn.R))
    assert got[i] == bn.gt_to_le(acc)


@pytest.mark.parametrize("with_mul,invert", MODES)
def test_scalars_zero_throughout_give_mul(eng, ragged, with_mul, invert):
    c = ragged
    zeros = [gc.le(0 if t % 2 else bn.R) for t in range(len(c.rows))]          # 0 and r: both are the exponent 0
    got = eng.gt_multiexp_rows(c.rows, c.off, zeros, mul=c.mul if with_mul else None, invert=invert, chunk_terms=2)
    assert got == (c.mul if with_mul else [ONE] * 70)


def test_no_items_and_items_without_any_row(eng, pool):
    assert eng.gt_multiexp_rows([], [0], []) == []
    assert eng.gt_multiexp_rows([], [0, 0, 0], [], invert=True) == [ONE, ONE]
    assert eng.gt_multiexp_rows([], [0, 0, 0], [], mul=pool[7:9]) == pool[7:9]


def test_bad_flags_and_offsets_are_refused(eng, pool):
    d, k, out = eng.upload(b"".join(pool[:2])), eng.upload(gc.le(3) + gc.le(5)), eng.alloc(2 * 384)

    def call(off, n_rows, flags):
        d_off = eng.upload_u32(off)
        return eng.lib.rhip_gt_multiexp_rows(eng.ctx, ctypes.c_size_t(n_rows), d_off.ptr, d.ptr, k.ptr, ctypes.c_size_t(len(off) - 1), None,
                                             ctypes.c_uint32(flags), ctypes.c_uint32(0), out.ptr)
    assert call([0, 1, 2], 2, 0) == 0
    assert call([0, 1, 2], 2, 2) != 0          # an unknown flag
    assert call([0, 2, 1], 2, 0) != 0          # decreasing offsets
    assert call([1, 1, 2], 2, 0) != 0          # not from 0
    assert call([0, 1, 3], 2, 0) != 0          # past the rows
