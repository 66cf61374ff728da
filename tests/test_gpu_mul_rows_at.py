"""rhip_g1_mul_rows_at / rhip_g2_mul_rows_at (out[row_dst[t]] = k[item of t] * p[row_src[t]]) driven directly: edge scalars, the row lists
request_sk_packed builds, arbitrary indices, untouched slots and the shadow lanes of a tail, byte for byte against the CPU oracle (exact
integers), against the forms without an index (the G2 kernel repeats that body) and against Engine.g1_mul / g2_mul.

The points of a case are P_j = m_j * (a0 * G) with small known m_j, so k * P_j = m_j * ((a0 * k mod r) * G): the oracle multiplies G once per
scalar (~150 times per group over the whole file, by its own additions over a table of G) and adds from there."""
import ctypes
import random

import pytest

from oracle import bn254 as bn
from rabe_amd import Engine, EngineError
from tests import test_gpu_g1_mul_rows as g1rows
from tests import test_gpu_g2_mul_rows as g2rows

pytestmark = pytest.mark.gpu
R = bn.R
RHIP_ERR_ARG = -3
FILL = 0xA5


class Group:
    def __init__(self, name, gen, add, mul, to_le, elem, block, edge):
        self.name, self.gen, self.add, self.mul, self.to_le, self.elem, self.block, self.edge = name, gen, add, mul, to_le, elem, block, edge
        self.inf, self.fill = bytes(elem), bytes([FILL]) * elem
        self.cache, self.table = {}, None

    def times_gen(self, e):
        """e * G by the oracle's additions over a table of d * 16^w * G (a sixth of the time of its binary chain, checked against it once)"""
        if self.table is None:
            self.table, base = [], self.gen
            for _ in range(64):
                row = [None]
                for _ in range(15):
                    row.append(self.add(row[-1], base))
                self.table.append(row)
                base = self.add(row[15], base)
            assert self.times_gen(R - A0) == self.mul(self.gen, R - A0)
        acc = None
        for w in range(64):
            acc = self.add(acc, self.table[w][(e >> 4 * w) & 15])
        return acc

    def multiple(self, e, m):
        """m * (e * G) as wire bytes: one multiplication per e, additions from there"""
        if not m or not e % R:
            return self.inf
        if e % R not in self.cache:
            self.cache[e % R] = (self.times_gen(e % R), [])
        base, wire = self.cache[e % R]
        acc = wire[-1][0] if wire else None
        while len(wire) < m:
            acc = self.add(acc, base)
            wire.append((acc, self.to_le(acc)))
        return wire[m - 1][1]

    def mul_rows(self, eng):
        return getattr(eng, self.name + "_mul_rows")

    def mul_rows_at(self, eng):
        return getattr(eng, self.name + "_mul_rows_at")

    def mul_each(self, eng):
        return getattr(eng, self.name + "_mul")


GROUPS = {"g1": Group("g1", bn.G1_GEN, bn.g1_add, bn.g1_mul, bn.g1_to_le, 64, 256, g1rows.EDGE),
          "g2": Group("g2", bn.G2_GEN, bn.g2_add, bn.g2_mul, bn.g2_to_le, 128, 128, g2rows.EDGE)}
A0 = 0x1234567890abcdef1234567890abcdef1234567890abcdef % R


class Points:
    """P_j = mult[j] * (a0 * G); mult[j] = 0 is infinity"""

    def __init__(self, grp, a0, mult):
        self.grp, self.a0, self.mult = grp, a0, list(mult)
        self.wire = [grp.multiple(a0, m) for m in self.mult]

    def times(self, j, k):
        return self.grp.multiple(self.a0 * k % R, self.mult[j])


def le(k):
    return (k % (1 << 256)).to_bytes(32, "little")


def offsets(sizes):
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    return off


def owners(off):
    return [i for i in range(len(off) - 1) for _ in range(off[i + 1] - off[i])]


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(params=["g1", "g2"])
def grp(request):
    return GROUPS[request.param]


def check_rows(grp, got, pts, row_src, off, ks, row_dst, untouched=()):
    """every slot of `got`: the product of the row that names it, or the fill"""
    row_of = {d: t for t, d in enumerate(row_dst)}
    assert len(row_of) == len(row_dst)
    item = owners(off)
    for d, bytes_d in enumerate(got):
        if d in row_of:
            t = row_of[d]
            assert bytes_d == pts.times(row_src[t], ks[item[t]]), (grp.name, "slot", d, "row", t)
        else:
            assert bytes_d == grp.fill, (grp.name, "slot", d, "was written")
    assert set(untouched) == set(range(len(got))) - set(row_of)


def test_identity_indices_give_the_bytes_of_the_form_without_an_index(eng, grp):
    """edge scalars and words >= r on {G, a * G, infinity}, row_src = row_dst = range(n_rows): the same bytes as g*_mul_rows, whose tests pin
    them against the oracle -- the G2 kernel is a repeated copy of that one's body"""
    scalars = grp.edge + [R, 2 * R, 5 * R, R + 1, (1 << 256) - 1]
    points = [grp.to_le(grp.gen), grp.multiple(A0, 1), grp.inf]
    rows = [p for _ in scalars for p in points]
    off = [3 * i for i in range(len(scalars) + 1)]
    ks = [le(k) for k in scalars]
    ident = list(range(len(rows)))
    got = grp.mul_rows_at(eng)(rows, ident, off, ks, ident)
    assert got == grp.mul_rows(eng)(rows, off, ks)
    for i, k in enumerate(scalars):
        assert got[3 * i + 1] == grp.multiple(A0 * k % R, 1), hex(k)
        assert got[3 * i + 2] == grp.inf
    # the three points stored once, every row reading its own through the index
    assert grp.mul_rows_at(eng)(points, [t % 3 for t in ident], off, ks, ident) == got


def caller_rows(sets, item_set):
    """scal_row, row_src, row_dst, item_row the way request_sk_packed (host/packed.cpp) builds them: sets[s] = the number of attributes of
    list s, item_set[j] = the list of user j; scalar (s, y) owns the users of list s in order and user j's results lie at item_row[j] + y"""
    scal_base = offsets(sets)
    users = [[] for _ in sets]
    item_row = [0]
    for j, s in enumerate(item_set):
        users[s].append(j)
        item_row.append(item_row[-1] + sets[s])
    total, n_scal = item_row[-1], scal_base[-1]
    scal_row, row_src, row_dst = [0] * (n_scal + 1), [0] * total, [0] * total
    for s in range(len(sets)):
        for y in range(sets[s]):
            k = scal_base[s] + y
            t = scal_row[k]
            for j in users[s]:
                row_src[t], row_dst[t] = j, item_row[j] + y
                t += 1
            scal_row[k + 1] = t
    return scal_row, row_src, row_dst, item_row


MIXED = ([3, 2, 5], [(0, 2, 2, 0, 2, 0, 0)[j % 7] for j in range(70)])          # ragged item_row; nobody holds list 1: two scalars without rows


@pytest.mark.parametrize("sets,item_set", [([s], [0] * u) for u, s in ((1, 1), (1, 5), (63, 3), (65, 2), (130, 3), (3, 100))] + [MIXED],
                         ids=["1x1", "1x5", "63x3", "65x2", "130x3", "3x100", "mixed"])
def test_fan_out_in_the_callers_shape(eng, grp, sets, item_set):
    """U users x S scalars, scalar-major in and item-major out: 1, 5, 189, 130, 390, 300 and 270 rows -- below, at and across one and two
    blocks of either kernel (G1 256 lanes, G2 128), the larger ones no multiple of a block"""
    rnd = random.Random(sum(sets) * 1000 + len(item_set))
    scal_row, row_src, row_dst, item_row = caller_rows(sets, item_set)
    n_rows = item_row[-1]
    assert n_rows < 128 or n_rows % 128
    pts = Points(grp, A0 + len(item_set), range(1, len(item_set) + 1))
    ks = [rnd.randrange(1, R) for _ in range(sum(sets))]
    got = grp.mul_rows_at(eng)(pts.wire, row_src, scal_row, [le(k) for k in ks], row_dst, fill=FILL)
    assert len(got) == n_rows
    check_rows(grp, got, pts, row_src, scal_row, ks, row_dst)
    base = offsets(sets)
    for j, s in enumerate(item_set):          # said the caller's way: user j's record holds attribute y of its list at position y
        for y in range(sets[s]):
            assert got[item_row[j] + y] == pts.times(j, ks[base[s] + y]), (j, y)


def arbitrary_case(grp):
    """~600 rows (G1) / ~300 (G2) in items of 0 .. 129 rows, an empty first and an empty last item; 40 points read at random with repeats,
    three of them infinity"""
    rnd = random.Random(20261021)
    sizes = [0, 1, 2, 17, 63, 64, 65, 129] + ([129, 65, 64] if grp.name == "g1" else []) + [0]
    off = offsets(sizes)
    n_rows = off[-1]
    assert n_rows % grp.block
    pts = Points(grp, A0 ^ 0x5a5a, [0 if j in (5, 20, 39) else j + 1 for j in range(40)])
    row_src = [rnd.randrange(40) for _ in range(n_rows)]
    assert len(set(row_src)) == 40
    ks = [rnd.randrange(1, R) for _ in sizes]
    return rnd, off, n_rows, pts, row_src, ks


def test_arbitrary_indices(eng, grp):
    rnd, off, n_rows, pts, row_src, ks = arbitrary_case(grp)
    row_dst = list(range(n_rows))
    rnd.shuffle(row_dst)
    got = grp.mul_rows_at(eng)(pts.wire, row_src, off, [le(k) for k in ks], row_dst, fill=FILL)
    check_rows(grp, got, pts, row_src, off, ks, row_dst)
    each = grp.mul_each(eng)([pts.wire[s] for s in row_src], [le(ks[i]) for i in owners(off)])
    assert [got[d] for d in row_dst] == each


def test_slots_no_row_names_keep_their_bytes(eng, grp):
    """the arbitrary case into n_rows + 3 slots of 0xA5: row_dst skips slot 0, a middle slot and the last one"""
    rnd, off, n_rows, pts, row_src, ks = arbitrary_case(grp)
    out_rows = n_rows + 3
    skipped = (0, out_rows // 2, out_rows - 1)
    row_dst = [d for d in range(out_rows) if d not in skipped]
    rnd.shuffle(row_dst)
    got = grp.mul_rows_at(eng)(pts.wire, row_src, off, [le(k) for k in ks], row_dst, out_rows=out_rows, fill=FILL)
    assert len(got) == out_rows
    check_rows(grp, got, pts, row_src, off, ks, row_dst, untouched=skipped)


@pytest.mark.parametrize("last", ["infinity", "scalar 0", "scalar 1 into slot 0"])
def test_degenerate_last_row_under_a_block_of_shadow_lanes(eng, grp, last):
    """n_rows = one block + 1: the second block holds one row and 255 (G1) / 127 (G2) lanes that shadow it -- they read p[row_src[last]], take
    part in the block's inversion and store nothing.  The points are read in reverse order, so a lane that read p[t] would show."""
    rnd = random.Random(len(last))
    n_rows = grp.block + 1
    mult = list(range(1, n_rows + 1))
    row_src = list(range(n_rows))[::-1]          # the last row reads point 0
    if last == "infinity":
        mult[0] = 0
    pts = Points(grp, A0 + 7, mult)
    ks = [rnd.randrange(1, R), {"infinity": rnd.randrange(1, R), "scalar 0": 0, "scalar 1 into slot 0": 1}[last]]
    off = [0, grp.block, n_rows]
    row_dst = list(range(1, n_rows)) + [0] if last == "scalar 1 into slot 0" else list(range(n_rows))
    got = grp.mul_rows_at(eng)(pts.wire, row_src, off, [le(k) for k in ks], row_dst, out_rows=n_rows + 2, fill=FILL)
    check_rows(grp, got, pts, row_src, off, ks, row_dst, untouched=(n_rows, n_rows + 1))
    assert got[row_dst[-1]] == (pts.wire[0] if last == "scalar 1 into slot 0" else grp.inf)


def test_argument_contract(eng, grp):
    g = grp.to_le(grp.gen)
    at = grp.mul_rows_at(eng)
    # no rows: OK, nothing written
    assert at([g], [], [0], [], [], out_rows=2, fill=FILL) == [grp.fill] * 2
    assert at([g], [], [0, 0], [le(3)], [], out_rows=1, fill=FILL) == [grp.fill]
    assert at([], [], [0], [], []) == []
    # a null index array: RHIP_ERR_ARG, nothing written
    fn = getattr(eng.lib, "rhip_%s_mul_rows_at" % grp.name)
    dp, dk, doff, didx = eng.upload(g + g), eng.upload(le(2)), eng.upload_u32([0, 2]), eng.upload_u32([0, 1])
    out = eng.upload(grp.fill * 2)
    n, one = ctypes.c_size_t(2), ctypes.c_size_t(1)
    assert fn(eng.ctx, n, doff.ptr, dp.ptr, None, one, dk.ptr, didx.ptr, out.ptr) == RHIP_ERR_ARG
    assert fn(eng.ctx, n, doff.ptr, dp.ptr, didx.ptr, one, dk.ptr, None, out.ptr) == RHIP_ERR_ARG
    assert fn(eng.ctx, ctypes.c_size_t(0), doff.ptr, dp.ptr, None, one, dk.ptr, None, out.ptr) == 0
    assert eng.download(out) == grp.fill * 2
    assert fn(eng.ctx, n, doff.ptr, dp.ptr, didx.ptr, one, dk.ptr, didx.ptr, out.ptr) == 0
    assert eng.download(out) == grp.multiple(2, 1) * 2
    with pytest.raises(EngineError):
        eng._check(fn(eng.ctx, n, doff.ptr, dp.ptr, None, one, dk.ptr, didx.ptr, out.ptr))
    # the binding's own checks
    for bad in (dict(row_src=[0]),                                  # one index array shorter than the other
                dict(row_dst=[0, 1, 0]),
                dict(row_src=[0, 2]),                               # past the points
                dict(row_dst=[0, 2]),                               # past the output
                dict(row_dst=[1, 2], out_rows=2),
                dict(item_row_off=[0, 1]),                          # the rules of g*_mul_rows
                dict(item_row_off=[1, 2]),
                dict(item_row_off=[0, 2, 1, 2], scalars=[le(1)] * 3),
                dict(scalars=[le(1)] * 2)):
        args = dict(points=[g, g], row_src=[0, 1], item_row_off=[0, 2], scalars=[le(1)], row_dst=[0, 1])
        args.update(bad)
        with pytest.raises(ValueError):
            at(**args)
