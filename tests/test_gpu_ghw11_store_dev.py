"""The range operations on a prepared-lines handle, driven directly (include/rabe_hip.h: rhip_g2_lines_reserve, _prepare_range, _scrub_range,
_range_is_zero): a handle of 12 blocks that holds three keys of 1, 3 and 2 attributes at blocks 0, 3 and 8.  The yardstick is
rhip_g2_lines_prepare over the concatenated elements: rhip_ghw11_transform_batch_keyed must return the same bits from either handle.  The
queue has six items, two per key, whose selections name every attribute of their key; the G1 arrays are the synthetic pools of
tests/decrypt_launch_cases.py.  The shapes are the smallest at which the addressing can go wrong: a range that starts at a non-zero block, a
range between two live ones, the handle's last block, a hole that is reused, a point at infinity inside a range."""
import ctypes

import pytest

from oracle import bn254 as bn
from rabe_amd import engine as E
from tests import decrypt_launch_cases as cases

pytestmark = pytest.mark.gpu
GT = cases.GT
ATTRS = (1, 3, 2)                      # keys A, B, C
BASES = (0, 3, 8)                      # their k_z in the handle
CAPACITY = 12
ITEM_KEY = (0, 1, 2, 2, 1, 0)
ITEM_M = (1, 3, 2, 1, 2, 1)            # selection entries of the item: attributes 0 .. m - 1 of its key
RHIP_ERR_ARG = -3
INF = bytes(128)                       # the point at infinity of G2 in the engine's byte form


class Dev:
    pass


@pytest.fixture(scope="module")
def dev():
    d = Dev()
    d.eng = eng = E.Engine(0)
    d.w = w = cases.World(eng)
    d.keys = [w.g2_list(2 + ATTRS[0], 1), w.g2_list(2 + ATTRS[1], 4), w.g2_list(2 + ATTRS[2], 9)]
    d.other = w.g2_list(4, 6)          # key D: 2 attributes, for B's hole
    n = len(ITEM_KEY)
    off = cases.offsets([m + 2 for m in ITEM_M])
    start = cases.offsets(ITEM_M)
    n_sel = start[-1]
    tk_attr = [e for m in ITEM_M for e in range(m)]
    d.args = (n, max(ITEM_M) + 2, off[-1], n_sel, w.u32(off), w.u32(start[:-1]), w.u32([e % cases.ROWS for e in range(n_sel)]), w.u32(tk_attr),
              eng.upload(b"".join(int(cases.COEFFS[e % len(cases.COEFFS)]).to_bytes(32, "little") for e in range(n_sel))),
              w.g1(n, 3), w.g1(cases.ROWS * n, 5), w.g1(cases.ROWS * n, 10), w.u32(cases.offsets([cases.ROWS] * n)))
    d.whole = E.G2Lines(eng, CAPACITY, eng.upload(b"".join(b"".join(k) for k in d.keys)))          # the yardstick's handle
    d.ref = run(d, d.whole)
    assert len({d.ref[i] for i in range(n)}) == n
    yield d
    d.whole.destroy()
    eng.close()


def run(d, lines, bases=None):
    """the six items' outputs from `lines`, item i under the key whose k_z is block bases[i]"""
    n = len(ITEM_KEY)
    d_out = d.eng.upload(bytes(n * GT))
    E.ghw11_transform_keyed_dev(d.eng, *d.args, d.w.u32(bases or [BASES[u] for u in ITEM_KEY]), None, lines, d_out)
    got = d.eng.download(d_out, n * GT)
    return [got[GT * i:GT * (i + 1)] for i in range(n)]


def put(d, lines, first, points):
    lines.prepare_range(first, len(points), d.eng.upload(b"".join(points)))


def filled(d, order=(0, 1, 2)):
    h = E.G2Lines.reserve(d.eng, CAPACITY)
    for u in order:
        put(d, h, BASES[u], d.keys[u])
    return h


def test_ranges_equal_one_preparation_in_any_order(dev):
    h = E.G2Lines.reserve(dev.eng, CAPACITY)
    assert h.nbytes() == dev.whole.nbytes()          # the reserved size is that of a preparation over as many points
    assert h.range_is_zero(0, CAPACITY)
    put(dev, h, BASES[1], dev.keys[1])               # a range that starts at a non-zero block, between two empty ones
    assert not h.range_is_zero(BASES[1], 5) and h.range_is_zero(0, 3) and h.range_is_zero(8, 4) and not h.range_is_zero(0, CAPACITY)
    for first in range(BASES[1], BASES[1] + 5):
        assert not h.range_is_zero(first, 1), first
    put(dev, h, BASES[0], dev.keys[0])
    put(dev, h, BASES[2], dev.keys[2])
    assert run(dev, h) == dev.ref
    h.destroy()
    h = filled(dev, (2, 0, 1))
    assert run(dev, h) == dev.ref
    h.destroy()


def test_scrub_empties_its_range_only_and_the_hole_is_reused(dev):
    h = filled(dev)
    h.scrub_range(BASES[1], 5)
    assert h.range_is_zero(BASES[1], 5)
    assert not h.range_is_zero(0, 3) and not h.range_is_zero(2, 1) and not h.range_is_zero(8, 1) and not h.range_is_zero(8, 4)
    got = run(dev, h)
    for i, u in enumerate(ITEM_KEY):
        if u != 1:
            assert got[i] == dev.ref[i], i
        else:
            assert got[i] == bn.gt_to_le(bn.GT_ONE), i          # every pair on an empty block contributes 1
    # another key into the same blocks: what it is on a fresh handle, nothing left over from B
    put(dev, h, BASES[1], dev.other)
    assert h.range_is_zero(BASES[1] + 4, 1) and not h.range_is_zero(BASES[1], 4)
    fresh = E.G2Lines(dev.eng, 4, dev.eng.upload(b"".join(dev.other)))
    # items 2 and 3 carry selections of 2 and 1 entries: served under D from either handle
    bases = [BASES[u] for u in ITEM_KEY]
    in_hole = list(bases)
    in_hole[2] = in_hole[3] = BASES[1]
    alone = [0, 0, 0, 0, 0, 0]
    got, want = run(dev, h, in_hole), run(dev, fresh, alone)
    assert got[2] == want[2] and got[3] == want[3] and got[2] != dev.ref[2]
    assert got[0] == dev.ref[0] and got[5] == dev.ref[5]
    fresh.destroy()
    h.destroy()


def test_a_handle_from_prepare_takes_the_range_calls(dev):
    lines = E.G2Lines(dev.eng, CAPACITY, dev.eng.upload(b"".join(b"".join(k) for k in dev.keys)))
    assert not lines.range_is_zero(0, CAPACITY)
    lines.scrub_range(BASES[2], 4)
    assert lines.range_is_zero(BASES[2], 4) and not lines.range_is_zero(BASES[1], 5)
    put(dev, lines, BASES[2], dev.keys[2])
    assert run(dev, lines) == dev.ref
    lines.destroy()


def test_bounds_and_empty_ranges(dev):
    eng, sz = dev.eng, ctypes.c_size_t
    h = filled(dev)
    dq = eng.upload(b"".join(dev.other))
    zero = ctypes.c_int32(7)
    for first, n in ((9, 4), (12, 1), (13, 0), (0, 13), (1, 2 ** 64 - 1)):
        assert eng.lib.rhip_g2_lines_prepare_range(eng.ctx, h.h, sz(first), sz(n), dq.ptr) == RHIP_ERR_ARG, (first, n)
        assert eng.lib.rhip_g2_lines_scrub_range(eng.ctx, h.h, sz(first), sz(n)) == RHIP_ERR_ARG, (first, n)
        assert eng.lib.rhip_g2_lines_range_is_zero(eng.ctx, h.h, sz(first), sz(n), ctypes.byref(zero)) == RHIP_ERR_ARG and zero.value == 7, (first, n)
    with pytest.raises(E.EngineError):
        h.prepare_range(9, 4, dq)
    for first in (0, 5, 12):          # n = 0: nothing is done, wherever inside the handle
        h.prepare_range(first, 0, None)
        h.scrub_range(first, 0)
        assert h.range_is_zero(first, 0)
    assert run(dev, h) == dev.ref          # nothing was touched by any of it
    h.destroy()


def test_the_last_block_and_points_at_infinity(dev):
    eng = dev.eng
    # one point in the very last block; the blocks in front of it stay empty.  The yardstick: a preparation over eleven points at
    # infinity and that point.  An item whose key starts at block 9 reads blocks 9, 10 (empty: 1) and 11 (attribute 0).
    point = dev.keys[1][2]
    h = E.G2Lines.reserve(eng, CAPACITY)
    put(dev, h, CAPACITY - 1, [point])
    assert h.range_is_zero(0, CAPACITY - 1) and not h.range_is_zero(CAPACITY - 1, 1)
    whole = E.G2Lines(eng, CAPACITY, eng.upload(INF * (CAPACITY - 1) + point))
    bases = [CAPACITY - 3] * len(ITEM_KEY)
    got, want = run(dev, h, bases), run(dev, whole, bases)
    assert got == want and got[0] != bn.gt_to_le(bn.GT_ONE)
    whole.destroy()
    h.destroy()
    # a point at infinity inside a range (B's l_z): flagged as rhip_g2_lines_prepare flags it, its pair contributes 1 as on a fresh handle
    dented = [list(k) for k in dev.keys]
    dented[1][1] = INF
    whole = E.G2Lines(eng, CAPACITY, eng.upload(b"".join(b"".join(k) for k in dented)))
    h = filled(dev)                       # B's range holds the full key first: the block of the point at infinity must not keep its lines
    put(dev, h, BASES[1], dented[1])
    assert h.range_is_zero(BASES[1] + 1, 1) and not h.range_is_zero(BASES[1], 1) and not h.range_is_zero(BASES[1] + 2, 1)
    got, want = run(dev, h), run(dev, whole)
    assert got == want
    assert got[1] != dev.ref[1] and got[0] == dev.ref[0]
    whole.destroy()
    h.destroy()
