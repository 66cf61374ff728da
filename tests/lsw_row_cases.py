"""Inputs for the fused LSW row routine (bn254/lsw_rows.h: k_lsw_enc_rows on the device, tests/hostsim/lsw_enc_rows.cpp on the CPU) and what
they must give, in integers.

Every base of a test key is a known multiple of the generator, so a row is described by discrete logs alone:
    e3 = g1 * (h secret)      e4 = g1_b * sx      e5 = g1_b2 * (sx h) + h_b * sx
with g1 = G * a, g1_b = G * b, g1_b2 = G * c, h_b = G * d.  Three keys: random logs; c = d (the two halves of e5 walk the SAME table: with h = 1
and a one-digit sx the second walk adds the very point the first one left -- the doubling branch of the mixed addition); d = -c (opposite
tables: with h = 1 the second walk takes the first one apart digit by digit and the last digit cancels).  tests/row_cases.py's `replay` proves
on the logs that those rows meet their branch.

Used by tests/test_gpu_lsw_enc_rows.py (against the four table launches plus the addition) and tests/test_lsw_enc_rows_host.py (against
oracle/bn254.py)."""
import random

from oracle import bn254 as bn
from tests import row_cases as rc

R = bn.R
ROW_COUNTS = (1, 63, 64, 65, 130)          # one lane, a full wave less one, a full wave, a wave plus one lane, three waves with a ragged tail
ITEM_SIZES = (1, 2, 5)
# what a row's scalars are set to; "plain" rows are random
KINDS = ("plain", "sx zero", "secret zero", "sx r-1", "e4 e5 identity", "e3 identity", "all identity")


class Key:
    def __init__(self, name, a, b, c, d):
        self.name, self.logs = name, (a % R, b % R, c % R, d % R)

    def points(self):
        """g1, g1_b, g1_b2, h_b as 64 wire bytes each"""
        return [bn.g1_to_le(bn.g1_mul(bn.G1_GEN, k)) for k in self.logs]


def keys():
    rnd = random.Random("lsw row keys")
    a, b, c, d = (rnd.randrange(1, R) for _ in range(4))
    return [Key("random", a, b, c, d), Key("same", a, b, c, c), Key("opposite", a, b, c, R - c)]


def item_sizes(total, rnd):
    """sizes 1, 2 and 5 mixed so that row_off is ragged, summing to `total`"""
    out = []
    while total:
        s = rnd.choice([x for x in ITEM_SIZES if x <= total])
        out.append(s)
        total -= s
    return out


class Call:
    """one call of the row routine: items (a secret, a list of hashes shared through hash_off) and rows (an sx each)"""

    def __init__(self, key):
        self.key = key
        self.secret, self.row_off, self.hash_off, self.hash, self.sx, self.note = [], [0], [], [], [], []
        self._lists = {}

    def add_item(self, secret, hashes, sxs, note="plain"):
        assert len(hashes) == len(sxs) and hashes
        hk = tuple(hashes)
        if hk not in self._lists:          # items with the same list share their hashes
            self._lists[hk] = len(self.hash)
            self.hash += list(hashes)
        self.secret.append(secret % R)
        self.hash_off.append(self._lists[hk])
        self.sx += [s % R for s in sxs]
        self.note += [note] * len(sxs)
        self.row_off.append(len(self.sx))

    @property
    def n_items(self):
        return len(self.secret)

    @property
    def n_rows(self):
        return len(self.sx)

    def rows(self):
        """(item, h, secret, sx) per row"""
        for i in range(self.n_items):
            for y in range(self.row_off[i + 1] - self.row_off[i]):
                yield i, self.hash[self.hash_off[i] + y], self.secret[i], self.sx[self.row_off[i] + y]

    def host_products(self):
        """the scalars of the existing path: h secret | sx | sx h per row (what lsw::encrypt_packed forms on the host)"""
        ka, kb, kc = [], [], []
        for _i, h, secret, sx in self.rows():
            ka.append(h * secret % R)
            kb.append(sx)
            kc.append(sx * h % R)
        return ka, kb, kc

    def want_logs(self):
        """the discrete logs of e3, e4, e5 per row; 0 is the identity"""
        a, b, c, d = self.key.logs
        return [(a * h * secret % R, b * sx % R, (c * sx * h + d * sx) % R) for _i, h, secret, sx in self.rows()]

    def want_bytes(self):
        return b"".join(bn.g1_to_le(bn.g1_mul(bn.G1_GEN, k)) if k else bytes(64) for row in self.want_logs() for k in row)

    def e5_events(self):
        """the exceptional additions of every row's e5 (tests/row_cases.py: replay), as [(walk, window, kind)]"""
        _a, _b, c, d = self.key.logs
        return [rc.replay([(c, sx * h % R), (d, sx)])[0] for _i, h, _secret, sx in self.rows()]


HASH_LISTS = {s: [random.Random("lsw hashes %d" % s).randrange(1, R) for _ in range(s)] for s in ITEM_SIZES}


def scalar_call(key, total, seed):
    """`total` rows in items of 1, 2 and 5 rows; the scalar cases of KINDS go round the items.  The first row of an item has sx = 0 (what the
    reference's loop leaves a one-attribute list with; here every item's first row, so that a zero sits beside live rows of the same item)."""
    rnd = random.Random("lsw rows %s %d %s" % (key.name, total, seed))
    call = Call(key)
    for n, size in enumerate(item_sizes(total, rnd)):
        kind = KINDS[n % len(KINDS)]
        secret = rnd.randrange(1, R)
        sxs = [0] + [rnd.randrange(1, R) for _ in range(size - 1)]
        if kind == "sx zero":
            sxs = [0] * size
        elif kind in ("secret zero", "e3 identity"):          # h secret = 0 while sx is not (where the item has a second row)
            secret = 0
            if size == 1:
                sxs = [rnd.randrange(1, R)]
        elif kind == "sx r-1":
            sxs = [R - 1] * size
        elif kind == "e4 e5 identity":
            sxs = [0] * size
        elif kind == "all identity":
            secret, sxs = 0, [0] * size
        call.add_item(secret, HASH_LISTS[size], sxs, kind)
    assert call.n_rows == total
    return call


def special_call(key):
    """rows with h = 1 that send the e5 addition into its special cases under the `same` and `opposite` keys: one-digit sx in window 0, a
    middle and the top window (doubling under `same`), full-width sx (cancelling at its top digit under `opposite`), beside ordinary rows"""
    rnd = random.Random("lsw special " + key.name)
    call = Call(key)
    for w in (0, 7, rc.WINDOWS - 1):
        call.add_item(rnd.randrange(1, R), [1], [rnd.randrange(1, 0x3000) << (16 * w)], "one digit w%d" % w)
    call.add_item(rnd.randrange(1, R), [1, 1], [rnd.randrange(1, R), rnd.randrange(1, R)], "full width")
    call.add_item(rnd.randrange(1, R), HASH_LISTS[2], [0, rnd.randrange(1, R)], "plain")
    call.add_item(0, [1], [R - 1], "h secret zero, sx r-1")
    return call


def check_special(call):
    """the proof that special_call meets the branches it is written for"""
    ev = call.e5_events()
    if call.key.name == "same":
        for row, w in enumerate((0, 7, rc.WINDOWS - 1)):
            assert ev[row] == [(1, w, "dbl")], (row, ev[row])
    if call.key.name == "opposite":
        logs = call.want_logs()
        for row in range(call.n_rows):
            if call.note[row] != "plain":          # h = 1: the halves cancel, at the top digit of sx
                assert ev[row] == [(1, rc.top_window(call.sx[row]), "cancel")] and logs[row][2] == 0, (row, ev[row])
            elif call.sx[row]:
                assert ev[row] == [] and logs[row][2] != 0, (row, ev[row])
