"""GPU checks of rhip_ghw11_provision_batch (include/rabe_hip.h) at the device level, independent of the tkgen path: every transform-key row
against oracle.bn254 big-integer arithmetic -- L_z = g2 * (r z^-1 mod R), K_z = g2_alpha * z^-1 + g2_a * (r z^-1), K_x_z = g2 * (h r z^-1) --
and every secret-key row against rhip_ghw11_keygen_batch on the same r.  Shapes: the smallest that reach every edge (one item; a block of the
scalar kernel crossed with a partial block left; a block of the row kernel crossed inside one item; row offsets that are not block-aligned).

The oracle's affine double-and-add takes 70 ms per product, so the reference walks window tables of the three bases built from the oracle's
own additions (the same group elements); it is computed once per shape and shared."""
import random

import pytest

from oracle import bn254 as bn
from rabe_amd.engine import Engine, Ghw11Keys, fr_bytes

pytestmark = pytest.mark.gpu
R = bn.R
INF = bytes(128)


class Windows:
    """k * base as a sum of table entries (d 2^(w i)) * base, every entry and every sum made by the oracle's addition (bn.g2_add; bn.g1_add for
    a base in G1)"""

    def __init__(self, base, w, add=bn.g2_add):
        self.w, self.rows, self.add = w, [], add
        for _ in range((254 + w - 1) // w):
            row, acc = [None], None
            for _d in range(1, 1 << w):
                acc = add(acc, base)
                row.append(acc)
            self.rows.append(row)
            base = add(row[-1], base)

    def mul(self, k):
        k %= R
        acc = None
        for row in self.rows:
            d = k & ((1 << self.w) - 1)
            k >>= self.w
            if d:
                acc = self.add(acc, row[d])
        return acc


def le(pt):
    return INF if pt is None else bn.g2_to_le(pt)


class World:
    def __init__(self):
        rnd = random.Random(2011)
        self.g2 = bn.g2_mul(bn.G2_GEN, rnd.randrange(1, R))
        self.g2_a = bn.g2_mul(self.g2, rnd.randrange(1, R))
        self.g2_alpha = bn.g2_mul(self.g2, rnd.randrange(1, R))
        self.t_g2, self.t_a, self.t_alpha = Windows(self.g2, 8), Windows(self.g2_a, 5), Windows(self.g2_alpha, 5)
        self.eng = Engine(0)
        self.keys = Ghw11Keys(self.eng, le(self.g2), le(self.g2_a), le(self.g2_alpha))
        self.shapes = {}

    def shape(self, name, counts, n_lists):
        """items with counts[i] attributes; items of equal count share one of n_lists hash lists where they can"""
        if name in self.shapes:
            return self.shapes[name]
        rnd = random.Random(name)
        hashes, list_at = [], {}
        item_hash_off, row_off = [], [0]
        for i, c in enumerate(counts):
            key = (c, i % n_lists)
            if key not in list_at:
                list_at[key] = len(hashes)
                hashes += [rnd.randrange(1, R) for _ in range(c)]
            item_hash_off.append(list_at[key])
            row_off.append(row_off[-1] + 2 + c)
        r = [rnd.randrange(1, R) for _ in counts]
        z = [rnd.randrange(2, R) for _ in counts]
        want = []
        for i, c in enumerate(counts):
            u = bn.fr_inv(z[i])
            v = r[i] * u % R
            want.append(le(self.t_g2.mul(v)))
            want.append(le(bn.g2_add(self.t_alpha.mul(u), self.t_a.mul(v))))
            want += [le(self.t_g2.mul(hashes[item_hash_off[i] + y] * v % R)) for y in range(c)]
        s = dict(counts=counts, row_off=row_off, hash_off=item_hash_off, hashes=hashes, r=r, z=z, want=want)
        self.shapes[name] = s
        return s

    def run(self, s, r=None, z=None, want_sk=True):
        fb = lambda xs: [fr_bytes(x) for x in xs]
        return self.eng.ghw11_provision_dev(self.keys, s["row_off"], s["hash_off"], fb(s["hashes"]), fb(r or s["r"]), fb(z or s["z"]), want_sk=want_sk)

    def keygen(self, s, r=None):
        fb = lambda xs: [fr_bytes(x) for x in xs]
        return self.eng.ghw11_keygen_dev(self.keys, s["row_off"], s["hash_off"], fb(s["hashes"]), fb(r or s["r"]))


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.keys.destroy()
    w.eng.close()


SHAPES = {
    "one item, one attribute": ([1], 1),
    "131 one-attribute items": ([1] * 131, 3),                  # the scalar kernel: one whole block of 128 items and 3 more; 393 rows
    "one item, 130 attributes": ([130], 1),                      # the row kernel: 132 rows, a block crossed inside the item, 4 rows more
    "mixed": ([3, 1, 9, 2, 14, 1, 5, 7, 2, 11, 4, 1, 8, 6, 3, 13, 2, 5, 1, 10, 4], 2),          # 154 rows: offsets 5, 8, 19, ... none on 128
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_rows_equal_the_oracle_and_keygen_batch(world, name):
    s = world.shape(name, *SHAPES[name])
    if name == "mixed":
        assert s["row_off"][-1] > 128 and all(o % 128 for o in s["row_off"][1:-1])
    sk, tk, flags = world.run(s)
    assert flags == [0] * len(s["counts"])
    assert len(tk) == s["row_off"][-1]
    bad = [t for t in range(len(tk)) if tk[t] != s["want"][t]]
    assert bad == []
    assert sk == world.keygen(s)
    assert all(row != INF for row in tk)


def test_z_one_gives_the_secret_key_rows(world):
    s = world.shape("mixed", *SHAPES["mixed"])
    sk, tk, flags = world.run(s, z=[1] * len(s["counts"]))
    assert flags == [0] * len(s["counts"]) and tk == sk == world.keygen(s)


def test_a_zero_z_is_flagged_and_its_block_neighbours_stand(world):
    s = world.shape("131 one-attribute items", *SHAPES["131 one-attribute items"])
    for at in (70, 129):                                            # the middle of the whole block; the partial block
        z = list(s["z"])
        z[at] = 0
        sk, tk, flags = world.run(s, z=z)
        assert flags == [1 if i == at else 0 for i in range(131)]
        lo, hi = s["row_off"][at], s["row_off"][at + 1]
        assert tk[:lo] == s["want"][:lo] and tk[hi:] == s["want"][hi:]
        assert tk[lo:hi] == [INF] * (hi - lo)                       # zinv = r zinv = 0: the point at infinity, nothing undefined
        assert sk == world.keygen(s)


def test_without_secret_key_rows_the_transform_key_rows_are_unchanged(world):
    for name in ("one item, one attribute", "mixed"):
        s = world.shape(name, *SHAPES[name])
        sk, tk, flags = world.run(s, want_sk=False)
        assert sk is None and tk == s["want"] and flags == [0] * len(s["counts"])


def test_secret_key_rows_equal_keygen_batch_on_another_r(world):
    s = world.shape("one item, 130 attributes", *SHAPES["one item, 130 attributes"])
    r = [R - 1]
    sk, _tk, _flags = world.run(s, r=r)
    assert sk == world.keygen(s, r=r)
    u = bn.fr_inv(s["z"][0])
    assert _tk[0] == le(world.t_g2.mul((R - 1) * u % R))
