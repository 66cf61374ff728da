"""GPU: the fixed-base G1 walks on the Z3 = Z1*H mixed addition (g1_madd_inl, rabe_amd/csrc/bn254/curve.h), byte for byte against
oracle.bn254.  The addition changes the Jacobian representative of every intermediate point and nothing else, so every stored
(affine, canonical) byte has to stay what the oracle says.

One base, three tables: 8-bit and 16-bit windows through the engine's table multiplication, 16-bit and signed 20-bit windows
through the AC17 row kernel (ac17_encrypt_dev).  257 rows: one full block of 256 lanes and one row with 255 shadow lanes.  The
scalars aim at the 13 windows of the signed 20-bit walk: digits at and just above half (the sign flip and its carry), single
non-zero windows, low windows that are zero (the copy into the infinite accumulator and the first real addition, the one with
Z1 = 1, then happen late), 0, 1, r - 1 and a raw word k + r.

The expected points are sums of 8-bit window entries made by the oracle's own addition, computed once per module."""
import random

import pytest

from oracle import bn254 as bn
from oracle import policy as pol
from oracle import schemes as sch
from oracle.tape import SeededRng
from tests import ac17_host as host

pytestmark = pytest.mark.gpu
R = bn.R
W = 20
HALF = 1 << (W - 1)


def word(x):
    """any 256-bit word, not reduced"""
    return int(x).to_bytes(32, "little")


class Oracle:
    """k * base as a sum of (d 2^(8 i)) * base, entries and sums by bn.g1_add; results cached"""

    def __init__(self, base):
        self.rows, self.seen = [], {}
        for _ in range(32):
            row, acc = [None], None
            for _d in range(255):
                acc = bn.g1_add(acc, base)
                row.append(acc)
            self.rows.append(row)
            base = bn.g1_add(row[-1], base)

    def mul(self, k):
        k %= R
        if k not in self.seen:
            acc, x = None, k
            for row in self.rows:
                if x & 255:
                    acc = bn.g1_add(acc, row[x & 255])
                x >>= 8
            self.seen[k] = bn.g1_to_le(acc)
        return self.seen[k]


def edge_scalars():
    """(word, what it is for); the word is what the device reads, its value mod r is what the oracle multiplies by"""
    rnd = random.Random("edge scalars")
    digit = lambda: rnd.randrange(1, HALF)
    out = [(0, "zero: infinity"), (1, "one"), (R - 1, "r - 1"),
           (HALF, "a digit exactly at half: not negated"),
           (HALF + 1, "a negative digit with a carry"),
           (sum((HALF + 1) << (W * i) for i in range(12)) % R, "every digit at half + 1: the carry runs through all 13 windows"),
           (sum(HALF << (W * i) for i in range(12)) % R, "every digit at half")]
    for pos in (0, 1, 12):
        d = digit() if pos < 12 else rnd.randrange(1, 1 << 13)
        out.append((d << (W * pos), "a single non-zero window at position %d" % pos))
    for j in (1, 2, 5):
        k = rnd.randrange(1 << 250, R)
        out.append(((k >> (W * j)) << (W * j), "the low %d windows zero" % j))
    k = rnd.randrange(1, R)
    out.append((k + R, "k + r as a raw word"))
    out.append((2 * R + 5, "5 + 2 r as a raw word"))
    return out


def scalars_257():
    """the edge words first, random ones between, and the lone row of the second block is an edge word too"""
    rnd = random.Random("257 rows")
    edge = [k for k, _why in edge_scalars()]
    ks = edge + [rnd.randrange(R) for _ in range(257 - len(edge) - 1)]
    return ks + [edge[5]]


@pytest.fixture(scope="module")
def env():
    from rabe_amd import Engine
    from rabe_amd import engine as E
    eng = Engine(0)
    pk, _msk = sch.ac17_setup(SeededRng(4242))
    # a key's wide table, once added, is what its launches use: one handle per window width
    dpk = {w: E.Ac17Pk(eng, bn.g1_to_le(pk["g"]), [bn.g2_to_le(x) for x in pk["h_a"]], [bn.gt_to_le(x) for x in pk["e_gh_ka"]]) for w in (16, W)}
    dpk[W].set_g_window(W)
    yield eng, E, pk, dpk, Oracle(pk["g"])
    for h in dpk.values():
        h.destroy()
    eng.close()


def rows_of(raw):
    return [raw[i:i + 64] for i in range(0, len(raw), 64)]


def differing(got, want):
    return [t for t in range(max(len(got), len(want))) if t >= len(got) or t >= len(want) or got[t] != want[t]]


def test_the_edge_scalars_are_what_they_claim():
    """in integers: the signed 20-bit digits of each edge scalar (the recoding of table_mul_g1_wide_inl)"""
    def digits(k):
        out, carry = [], 0
        for i in range(13):
            raw = ((k >> (W * i)) & ((1 << W) - 1)) + carry
            carry = 1 if raw > HALF else 0
            out.append(raw - (1 << W) if carry else raw)
        assert carry == 0 and sum(d << (W * i) for i, d in enumerate(out)) == k
        return out
    by = {why: digits(k % R) for k, why in edge_scalars()}
    assert by["a digit exactly at half: not negated"] == [HALF] + [0] * 12
    assert by["a negative digit with a carry"] == [-(HALF - 1), 1] + [0] * 11
    assert all(d < 0 for d in by["every digit at half + 1: the carry runs through all 13 windows"][:12])
    assert by["every digit at half + 1: the carry runs through all 13 windows"][12] == 1
    for pos in (0, 1, 12):
        d = by["a single non-zero window at position %d" % pos]
        assert d[pos] > 0 and [x for i, x in enumerate(d) if i != pos] == [0] * 12
    for j in (1, 2, 5):
        d = by["the low %d windows zero" % j]
        assert d[:j] == [0] * j and d[j] != 0 and d[j + 1] != 0


def test_table_mul_257_rows_on_8_bit_and_16_bit_windows(env):
    eng, _E, pk, _dpk, ora = env
    ks = scalars_257()
    want = [ora.mul(k) for k in ks]
    tab = eng.g1_table(bn.g1_to_le(pk["g"]))
    try:
        got8 = tab.mul([word(k) for k in ks])
        tab.add_w16()
        got16 = tab.mul([word(k) for k in ks])
    finally:
        tab.destroy()
    assert differing(got8, want) == []
    assert differing(got16, want) == []
    assert want[0] == bytes(64) and want[1] == bn.g1_to_le(pk["g"]) and want[2] == bn.g1_to_le(bn.g1_neg(pk["g"]))


def encrypt_rows(eng, E, dpk, n_items, A, item_A_off, row_off, s_words):
    total = row_off[-1]
    e_one = bn.gt_to_le(bn.FP12_ONE)
    dc0, dc, dcp = eng.alloc(n_items * 384), eng.alloc(total * 192), eng.alloc(n_items * 384)
    E.ac17_encrypt_dev(eng, dpk, n_items, eng.upload(A), eng.upload_u32(item_A_off), eng.upload_u32(row_off), total,
                       eng.upload(b"".join(s_words)), eng.upload(e_one * n_items), dc0, dc, dcp)
    return rows_of(eng.download(dc, total * 192)), eng.download(dc0, n_items * 384), eng.download(dcp, n_items * 384)


def test_row_kernel_257_rows_of_chosen_scalars_on_16_bit_and_signed_20_bit_windows(env):
    """one item of 257 rows whose row scalars s0 a0 + s1 a1 are the chosen ones (a0 solved for); slot l of row t gets scalar t + l"""
    eng, E, _pk, dpk, ora = env
    rnd = random.Random("row kernel scalars")
    ks = scalars_257()
    s0, s1 = rnd.randrange(1, R), rnd.randrange(1, R)
    A, want = [], []
    for t in range(257):
        for l in range(3):
            k = ks[(t + l) % 257]
            a1 = rnd.randrange(R)
            a0 = (k - s1 * a1) * bn.fr_inv(s0) % R
            if k >= R:
                a0 += R                                          # the raw words reach the kernel as raw words
            A += [word(a0), word(a1)]
            want.append(ora.mul(k))
    args = (1, b"".join(A), [0], [0, 257], [word(s0), word(s1)])
    c16, c0_16, cp_16 = encrypt_rows(eng, E, dpk[16], *args)
    assert differing(c16, want) == []
    c20, c0_20, cp_20 = encrypt_rows(eng, E, dpk[W], *args)
    assert differing(c20, want) == []
    assert (c0_20, cp_20) == (c0_16, cp_16)


@pytest.mark.parametrize("n_items", [2, 86])
def test_ac17_rows_of_a_three_row_policy(env, n_items):
    """2 items (6 rows: 250 shadow lanes) and 86 items (258 rows: a full block and two rows) of a 3-row policy, g_window 16 and 20"""
    eng, E, _pk, dpk, ora = env
    policy = r'''{"name": "or", "children": [{"name": "X"}, {"name": "and", "children": [{"name": "A"}, {"name": "B"}]}]}'''
    pi, A = host.policy_table(policy, pol.JSON)
    assert len(pi) == 3
    rnd = random.Random(n_items)
    items = [(rnd.randrange(R), rnd.randrange(R)) for _ in range(n_items)]
    items[-1] = (0, 0)                                           # its rows are infinity: parked with z = 0
    a = [int.from_bytes(A[32 * i:32 * i + 32], "little") for i in range(len(A) // 32)]
    want = [ora.mul(s0 * a[(row * 3 + l) * 2] + s1 * a[(row * 3 + l) * 2 + 1]) for s0, s1 in items for row in range(3) for l in range(3)]
    assert want[-9:] == [bytes(64)] * 9
    args = (n_items, A, [0] * n_items, [3 * i for i in range(n_items + 1)], [word(s) for it in items for s in it])
    got = {}
    for w_bits in (16, W):
        got[w_bits] = encrypt_rows(eng, E, dpk[w_bits], *args)
        assert differing(got[w_bits][0], want) == []
    assert got[16][1:] == got[W][1:]
