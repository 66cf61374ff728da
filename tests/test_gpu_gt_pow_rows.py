"""rhip_gt_pow_rows (Gt powers over rows that share an exponent; four-way split over the Frobenius map, bn254/gtpow4.h) byte for byte
against rhip_gt_pow + rhip_gt_inv / rhip_gt_mul on the same inputs, and against the CPU oracle for a handful of rows."""
import random

import pytest

from oracle import bn254 as bn
from rabe_amd import Engine
from tests import gt_pow_cases as gc

pytestmark = pytest.mark.gpu
ONE = bn.gt_to_le(bn.GT_ONE)
MODES = [(False, False), (False, True), (True, False), (True, True)]          # (mul given, invert)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def pool(eng):
    """140 members of Gt: the oracle's five bases, then powers of e(g1, g2) made on the device by the window routine"""
    rnd = random.Random(0x726f7773)
    base = [bn.gt_to_le(a) for a in gc.bases()]
    more = eng.gt_pow([base[1]] * 135, [gc.le(rnd.randrange(1, bn.R)) for _ in range(135)])
    return base + more


def reference(eng, rows, scalars_per_row, mul, invert):
    p = eng.gt_pow(rows, scalars_per_row)
    if invert:
        p = eng.gt_inv(p)
    return eng.gt_mul(mul, p) if mul is not None else p


def per_row(off, scalars):
    return [scalars[i] for i in range(len(scalars)) for _ in range(off[i + 1] - off[i])]


@pytest.mark.parametrize("with_mul,invert", MODES)
def test_one_item_of_130_rows(eng, pool, with_mul, invert):
    """two waves and a two-row tail under one scalar: a random one, the all-ones word, and 0 (an accumulator that never starts)"""
    rows = pool[:130]
    mul = pool[10:140] if with_mul else None
    for k in (gc.RANDOM_SCALARS[1], (1 << 256) - 1, 0):
        got = eng.gt_pow_rows(rows, [0, 130], [gc.le(k)], mul=mul, invert=invert)
        assert got == reference(eng, rows, [gc.le(k)] * 130, mul, invert), hex(k)
        if k == 0:
            assert got == (mul if with_mul else [ONE] * 130)
    assert len(set(got)) > 1 or not with_mul


@pytest.mark.parametrize("with_mul,invert", MODES)
def test_70_items_of_one_row_cover_every_scalar(eng, pool, with_mul, invert):
    """one wave and a tail in which every lane has its own digits: the 46 scalars of the CPU test and 24 more random ones; the base 1 and
    the oracle's bases sit under the special scalars"""
    rnd = random.Random(70)
    scalars = gc.SCALARS + [rnd.randrange(bn.R) for _ in range(24)]
    assert len(scalars) == 70
    rows = [pool[i % 5] if i < 20 else pool[i] for i in range(70)]
    mul = [pool[139 - i] for i in range(70)] if with_mul else None
    ks = [gc.le(k) for k in scalars]
    got = eng.gt_pow_rows(rows, list(range(71)), ks, mul=mul, invert=invert)
    assert got == reference(eng, rows, ks, mul, invert)
    bases = gc.bases()
    for i in (1, 3, 6, 7, 8, 12, 13):          # 1, r - 1, 2^256 - 1, lambda, lambda - 1, 2^64, 2^65 - 1 on oracle bases
        want = gc.expected(bases[i % 5], scalars[i], invert, bn.gt_from_le(mul[i]) if with_mul else None)
        assert got[i] == want, hex(scalars[i])


@pytest.mark.parametrize("with_mul,invert", MODES)
def test_items_without_rows_at_the_front_in_the_middle_and_at_the_end(eng, pool, with_mul, invert):
    off = [0, 0, 3, 3, 3, 5, 70, 70]
    scalars = [gc.SCALARS[i] for i in (15, 7, 16, 17, 9, 18, 19)]
    rows = pool[5:75]
    mul = pool[60:130] if with_mul else None
    ks = [gc.le(k) for k in scalars]
    got = eng.gt_pow_rows(rows, off, ks, mul=mul, invert=invert)
    assert got == reference(eng, rows, per_row(off, ks), mul, invert)


def test_no_rows(eng):
    assert eng.gt_pow_rows([], [0], []) == []
    assert eng.gt_pow_rows([], [0, 0, 0], [gc.le(5), gc.le(7)], invert=True) == []


def test_unknown_flag_is_refused(eng, pool):
    import ctypes
    d = eng.upload(pool[0])
    k = eng.upload(gc.le(3))
    off = eng.upload_u32([0, 1])
    out = eng.alloc(384)
    rc = eng.lib.rhip_gt_pow_rows(eng.ctx, ctypes.c_size_t(1), off.ptr, d.ptr, ctypes.c_size_t(1), k.ptr, None, ctypes.c_uint32(2), out.ptr)
    assert rc != 0
