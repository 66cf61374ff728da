"""GPU checks of the fused row kernels where a sum over two bases meets the exceptional cases of the mixed addition, and of the bulk entry
points on scalar words that are not canonical.

k_ghw11_enc_rows (rhip_ghw11_encrypt_batch), k_ghw11_keygen_rows / k_ghw11_provision_rows (rhip_ghw11_keygen_batch /
rhip_ghw11_provision_batch) and k_dnf_keygen_g1 / _g2 (rhip_dnf_keygen_batch) each form a sum of two group elements on one Jacobian
accumulator.  With bases related by a discrete log the caller knows -- g1_a = g1 * c, g2_alpha = g2_a * c, a1 = p1 * c -- chosen scalars make
the accumulator equal to the addend (the doubling branch), its opposite (infinity in mid-walk) or leave the finished point at infinity (the
parked z = 0 value, the lane's contribution of one to the block inversion).  tests/row_cases.py builds these inputs and proves in integers
that every row reaches its branch at its window (tests/test_row_kernels_precheck.py runs the proofs without a GPU); here the calls run.

Reference: oracle.bn254 alone.  Every base is a known multiple of one point, so an expected row is that point times a log computed in Python
integers: one exact oracle product for a degenerate row, the window-table sum of oracle additions (test_gpu_ghw11_provision_dev.Windows)
for its ordinary neighbours; bytes(64) / bytes(128) for infinity."""
import json
import os
import random

import pytest

from oracle import bn254 as bn
from rabe_amd import engine as E
from rabe_amd import hostprep as hp
from rabe_amd.engine import DevTreeTables, DnfKeys, Engine, Ghw11Keys, Ghw11Pk, fr_bytes
from tests import row_cases as rc
from tests.test_gpu_ghw11_provision_dev import Windows

pytestmark = pytest.mark.gpu
R = bn.R
HERE = os.path.dirname(os.path.abspath(__file__))
INF1, INF2 = bytes(64), bytes(128)


class Ref:
    """b1 = G1_GEN * x and b2 = G2_GEN * y: every G1 / G2 base of every world is one of them times a known scalar"""

    def __init__(self):
        rnd = random.Random("row kernels")
        self.b1, self.b2 = bn.g1_mul(bn.G1_GEN, rnd.randrange(1, R)), bn.g2_mul(bn.G2_GEN, rnd.randrange(1, R))
        self.y1, self.y2 = rnd.randrange(1 << 200, R), rnd.randrange(1 << 200, R)          # the DNF worlds' g1 = p1 * y1, g2 = p2 * y2
        self.w1, self.w2 = Windows(self.b1, 8, bn.g1_add), Windows(self.b2, 8)
        with open(os.path.join(HERE, "golden", "ghw11.json")) as f:
            self.gt = bytes.fromhex(json.load(f)["pk"]["e_gg_alpha"])                      # some member of Gt: the Gt side is not under test

    def g1(self, log, exact=False):
        log %= R
        return INF1 if not log else bn.g1_to_le(bn.g1_mul(self.b1, log) if exact else self.w1.mul(log))

    def g2(self, log, exact=False):
        log %= R
        return INF2 if not log else bn.g2_to_le(bn.g2_mul(self.b2, log) if exact else self.w2.mul(log))


class Dev:
    """the engine and, per relation, the device tables of the three key handles (built on first use, destroyed with the module)"""

    def __init__(self, ref):
        self.ref, self.eng, self.made = ref, Engine(0), {}

    def _get(self, key, make):
        if key not in self.made:
            self.made[key] = make()
        return self.made[key]

    def enc_pk(self, c):
        return self._get(("pk", c), lambda: Ghw11Pk(self.eng, self.ref.g1(1), self.ref.g1(c, True), self.ref.gt))

    def keys(self, c):
        return self._get(("keys", c), lambda: Ghw11Keys(self.eng, self.ref.g2(1), self.ref.g2(1), self.ref.g2(c, True)))

    def dnf(self, c1, c2):
        r = self.ref
        return self._get(("dnf", c1, c2), lambda: DnfKeys(self.eng, r.g1(1), r.g1(r.y1, True), r.g2(1), r.g2(r.y2, True),
                                                          INF1 if c1 is None else r.g1(c1, True), INF2 if c2 is None else r.g2(c2, True)))

    def close(self):
        for h in self.made.values():
            h.destroy()
        self.eng.close()


@pytest.fixture(scope="module")
def ref():
    return Ref()


@pytest.fixture(scope="module")
def dev(ref):
    d = Dev(ref)
    yield d
    d.close()


def rows_of(raw, size):
    return [raw[i:i + size] for i in range(0, len(raw), size)]


def differing(got, want):
    return [t for t in range(max(len(got), len(want))) if t >= len(got) or t >= len(want) or got[t] != want[t]]


# ---------------------------------------------------------------------------------------------------- k_ghw11_enc_rows
def run_enc(dev, call, secret_words=None, coef_words=None, t_words=None, hash_words=None):
    """rhip_ghw11_encrypt_batch on the call's items; the *_words replace the canonical 32-byte records of an input, in its order"""
    eng = dev.eng
    tt = hp.TreeTables(rc.ENC_TREES, hash_leaf=lambda name: call.H[name])
    assert tt.first_leaf == [call.first_leaf[p] for p in (rc.LEAF, rc.OR3, rc.AND2)]
    dtt = DevTreeTables(eng, tt)
    if hash_words is not None:
        dtt.leaf_hash = eng.upload(b"".join(hash_words))
    n, total = len(call.items), len(call.rows)
    leaf_off, coef_off, coefs = [0], [], []
    for p, _secret, coef in call.items:
        leaf_off.append(leaf_off[-1] + tt.n_leaves(p))
        coef_off.append(len(coefs))
        coefs += coef
    assert leaf_off[-1] == total
    words = lambda given, ints: b"".join(given if given is not None else [fr_bytes(x) for x in ints])
    d_c, d_c1, d_cd = eng.alloc(n * 384), eng.alloc(n * 64), eng.alloc(total * 128)
    E.ghw11_encrypt_dev(eng, dev.enc_pk(call.c), n, total, eng.upload_u32(leaf_off), eng.upload_u32([tt.first_leaf[p] for p, _s, _c in call.items]),
                        eng.upload_u32([tt.first_gate[p] for p, _s, _c in call.items]), dtt, eng.upload(words(secret_words, [s for _p, s, _c in call.items])),
                        eng.upload(words(coef_words, coefs) or bytes(32)), eng.upload_u32(coef_off),
                        eng.upload(words(t_words, [r["t"] for r in call.rows])), eng.upload(dev.ref.gt * n), d_c, d_c1, d_cd)
    return eng.download(d_c, n * 384), rows_of(eng.download(d_c1, n * 64), 64), rows_of(eng.download(d_cd, total * 128), 64)


def enc_want(ref, call):
    """C, D of every row: C an exact product where the row is degenerate"""
    out = []
    for r in call.rows:
        out += [ref.g1(r["c_log"], r["kind"] != "ordinary"), ref.g1(r["d_log"])]
    return out


@pytest.mark.parametrize("c", rc.RELATIONS)
def test_ghw11_encrypt_every_case_on_leaf_or_and_policies(dev, ref, c):
    call = rc.enc_every_case(c)
    _c, c1, cd = run_enc(dev, call)
    assert differing(cd, enc_want(ref, call)) == []
    assert c1 == [ref.g1(secret) for _p, secret, _coef in call.items]
    for t in call.lanes("cancel last", "both zero"):
        assert cd[2 * t] == INF1
    for t in call.lanes("cancel last"):
        assert cd[2 * t + 1] == ref.g1(call.rows[t]["t"], True) != INF1          # C parked with z = 0, D finite


def test_ghw11_encrypt_257_rows_with_infinite_neighbours(dev, ref):
    call = rc.enc_257()
    _c, _c1, cd = run_enc(dev, call)
    want = enc_want(ref, call)
    assert differing(cd, want) == []                                             # the 249 ordinary rows of both blocks included
    assert [t for t in range(257) if cd[2 * t] == INF1] == [63, 64, 256] and [t for t in range(257) if cd[2 * t + 1] == INF1] == [64, 200]


@pytest.mark.parametrize("kind", ["dbl w0", "cancel last", "both zero"])
def test_ghw11_encrypt_one_row(dev, ref, kind):
    call = rc.enc_one_row(1, kind)
    _c, c1, cd = run_enc(dev, call)
    assert cd == enc_want(ref, call) and c1 == [ref.g1(call.items[0][1], True)]


def test_ghw11_encrypt_a_first_block_that_is_all_infinity(dev, ref):
    call = rc.EncCall(1, "all infinity")
    for _ in range(rc.ROWS_BLOCK):
        call.leaf("both zero")
    call.leaf("ordinary").leaf("both zero").leaf("dbl w1").precheck()
    c, c1, cd = run_enc(dev, call)
    assert cd[:2 * rc.ROWS_BLOCK] == [INF1] * (2 * rc.ROWS_BLOCK)           # every lane of the block contributed one to its product
    assert cd == enc_want(ref, call)
    assert c1[:rc.ROWS_BLOCK] == [INF1] * rc.ROWS_BLOCK and c[:384] == ref.gt    # secret = 0: c1 infinite, c = msg


# ---------------------------------------------------------------------------------------------------- k_ghw11_keygen_rows / _provision_rows
def run_keys(dev, call, r_words=None, z_words=None, hash_words=None, z=None):
    words = lambda given, ints: given if given is not None else [fr_bytes(x) for x in ints]
    h, r, zz = words(hash_words, call.hashes), words(r_words, call.r), words(z_words, z if z is not None else call.z)
    keys = dev.keys(call.c)
    sk, tk, flags = dev.eng.ghw11_provision_dev(keys, call.row_off, call.hash_off, h, r, zz)
    return dev.eng.ghw11_keygen_dev(keys, call.row_off, call.hash_off, h, r), sk, tk, flags


def key_want(ref, call):
    deg = set(call.degenerate_rows())
    return [ref.g2(x, t in deg) for t, x in enumerate(call.sk_logs())], [ref.g2(x, t in deg) for t, x in enumerate(call.tk_logs())]


@pytest.mark.parametrize("c", rc.RELATIONS)
def test_ghw11_keygen_and_provision_double_and_cancel_in_row_one(dev, ref, c):
    call = rc.key_small(c)
    kg, sk, tk, flags = run_keys(dev, call)
    want_sk, want_tk = key_want(ref, call)
    assert differing(kg, want_sk) == [] and differing(tk, want_tk) == []
    assert sk == kg and flags == [0] * len(call.counts)
    for i, kind in enumerate(call.kind):
        k_row = call.row_off[i] + 1
        assert (kg[k_row] == INF2) == (tk[k_row] == INF2) == (kind == "cancel")
        if kind == "dbl z one":
            assert tk[k_row] == kg[k_row] == ref.g2(2 * c, True)


def test_ghw11_keygen_and_provision_across_a_block_edge(dev, ref):
    call = rc.key_135()
    kg, sk, tk, flags = run_keys(dev, call)
    want_sk, want_tk = key_want(ref, call)
    assert differing(kg, want_sk) == [] and differing(tk, want_tk) == []
    assert sk == kg and flags == [0] * 45
    assert [t for t in range(135) if kg[t] == INF2] == [t for t in range(135) if tk[t] == INF2] == [64, 130]


def test_ghw11_keygen_r_zero_leaves_one_finite_lane_in_a_block(dev, ref):
    call = rc.key_r_zero_130()
    kg, sk, tk, flags = run_keys(dev, call)
    assert kg == [INF2, ref.g2(call.c, True)] + [INF2] * 130 == sk
    assert tk == [INF2, ref.g2(call.c * rc.inv(call.z[0]), True)] + [INF2] * 130 and flags == [0]


# ---------------------------------------------------------------------------------------------------- k_dnf_keygen_g1 / _g2
def dnf_want(ref, call):
    deg = set(call.degenerate_items())
    g1, g2 = [], []
    for i, r in enumerate(call.r):
        g1 += [ref.g1(r + (call.c1 or 0), i in deg), ref.g1(ref.y1 * r)]           # the sk row of a degenerate item: an exact product
        g2 += [ref.g2(r + (call.c2 or 0), i in deg), ref.g2(ref.y2 * r)]
    return g1, g2


def check_dnf(dev, ref, call):
    g1, g2 = dev.eng.dnf_keygen_dev(dev.dnf(call.c1, call.c2), [fr_bytes(r) for r in call.r])
    want1, want2 = dnf_want(ref, call)
    assert differing(g1, want1) == [] and differing(g2, want2) == []
    return g1, g2


@pytest.mark.parametrize("c1,c2", rc.DNF_RELATIONS)
def test_dnf_keygen_double_cancel_and_zero(dev, ref, c1, c2):
    call = rc.dnf_small(c1, c2)
    g1, g2 = check_dnf(dev, ref, call)
    for i, kind in enumerate(call.kind):
        assert (g1[2 * i] == INF1) == (kind == "cancel g1" or (kind == "cancel g2" and c1 == c2))
        assert (g2[2 * i] == INF2) == (kind == "cancel g2" or (kind == "cancel g1" and c1 == c2))
        assert (g1[2 * i + 1] == INF1) == (g2[2 * i + 1] == INF2) == (kind == "r zero")
        if kind == "r zero":
            assert (g1[2 * i], g2[2 * i]) == (ref.g1(c1, True), ref.g2(c2, True))           # sk = a


def test_dnf_keygen_129_items_across_the_block_edges(dev, ref):
    check_dnf(dev, ref, rc.dnf_129(5, 7))


@pytest.mark.parametrize("kind", ["dbl g1", "cancel g2"])
def test_dnf_keygen_one_item(dev, ref, kind):
    check_dnf(dev, ref, rc.dnf_one_item(5, 7, kind))


def test_dnf_keygen_with_a1_and_a2_at_infinity(dev, ref):
    call = rc.dnf_a_infinity()
    g1, g2 = check_dnf(dev, ref, call)
    assert (g1[2], g1[3], g2[2], g2[3]) == (INF1, INF1, INF2, INF2)
    assert all(g1[2 * i] == ref.g1(r) and g2[2 * i] == ref.g2(r) for i, r in enumerate(call.r))          # sk = p * r


# ---------------------------------------------------------------------------------------------------- raw scalar words
def test_raw_words_in_ghw11_keygen_and_provision(dev, ref):
    """r, z and hash as any 256-bit word: the same bytes as the call on the reduced words, and the oracle's rows"""
    rnd = random.Random("raw keys")
    call = rc.KeyCall(5, [4, 1, 3, 2, 4, 1, 2, 3], {}, "raw")
    hw, rw = rc.raw_words(rnd, len(call.hashes)), rc.raw_words(rnd, len(call.counts))
    zw = [x for x in rc.raw_words(rnd, 2 * len(call.counts)) if x[1]][:len(call.counts)]          # z = R is the flagged zero: its own test
    call.hashes, call.r, call.z = [k for _w, k in hw], [k for _w, k in rw], [k for _w, k in zw]
    for r, z in zip(call.r, call.z):                                             # no row 1 is exceptional: the rows differ by their words alone
        rc.check_row([(1, r)], call.c, [], r + call.c)
        rc.check_row([(call.c, rc.inv(z)), (1, r * rc.inv(z) % R)], None, [], (call.c + r) * rc.inv(z))
    reduced = run_keys(dev, call)
    raw = run_keys(dev, call, r_words=[rc.word_bytes(w) for w, _k in rw], z_words=[rc.word_bytes(w) for w, _k in zw],
                   hash_words=[rc.word_bytes(w) for w, _k in hw])
    assert raw == reduced
    for one in ("r", "z", "hash"):                                               # and each input alone
        kw = {"r": dict(r_words=[rc.word_bytes(w) for w, _k in rw]), "z": dict(z_words=[rc.word_bytes(w) for w, _k in zw]),
              "hash": dict(hash_words=[rc.word_bytes(w) for w, _k in hw])}[one]
        assert run_keys(dev, call, **kw) == reduced
    kg, sk, tk, flags = raw
    want_sk, want_tk = [ref.g2(x) for x in call.sk_logs()], [ref.g2(x) for x in call.tk_logs()]
    assert differing(kg, want_sk) == [] and differing(tk, want_tk) == [] and sk == kg and flags == [0] * len(call.counts)
    assert INF2 in kg and INF2 in tk                                             # the words R among r and hash: rows at infinity


def test_z_equal_to_the_group_order_is_flagged_like_zero(dev, ref):
    call = rc.KeyCall(1, [1] * 131, {}, "z = R").precheck()                      # k_ghw11_tk_scalars: one whole block of 128 items and 3 more
    base = run_keys(dev, call)
    want_tk = [ref.g2(x) for x in call.tk_logs()]
    assert differing(base[2], want_tk) == [] and base[3] == [0] * 131
    for at in (70, 129):
        z0 = list(call.z)
        z0[at] = 0
        zero = run_keys(dev, call, z=z0)
        zw = [fr_bytes(z) for z in call.z]
        zw[at] = rc.word_bytes(R)
        order = run_keys(dev, call, z_words=zw)
        assert order == zero
        _kg, sk, tk, flags = order
        assert flags == [1 if i == at else 0 for i in range(131)]
        lo, hi = call.row_off[at], call.row_off[at + 1]
        assert tk[lo:hi] == [INF2] * 3 and tk[:lo] == want_tk[:lo] and tk[hi:] == want_tk[hi:]
        assert sk == base[1]


def test_raw_words_in_ghw11_encrypt(dev, ref):
    """secret, coef, t and leaf_hash as any 256-bit word"""
    rnd = random.Random("raw enc")
    call = rc.EncCall(5, "raw")
    for _ in range(3):
        call.leaf().or3(["ordinary"] * 3).and2("ordinary", 1).and2("ordinary", 2)
    # put raw words' scalars in: secrets and draws per item, t per row, H per leaf; lam and the logs follow from them
    sw, cw, tw = rc.raw_words(rnd, len(call.items)), rc.raw_words(rnd, 6), rc.raw_words(rnd, len(call.rows))
    hw = [x for x in rc.raw_words(rnd, 12) if x[1]][:6]
    call.H = {n: k for n, (_w, k) in zip(rc.ENC_LEAF_NAMES, hw)}
    coef_at, items = 0, []
    for i, (p, _secret, coef) in enumerate(call.items):
        items.append((p, sw[i][1], [cw[coef_at][1]] if coef else []))
        coef_at += len(coef)
    call.items = items
    names = [n for p, _s, _c in items for n in ("A", "BCD", "EF")[p]]
    call.rows = []
    for t, (lam, name) in enumerate(zip(call.shares(), names)):
        k2 = (R - call.H[name] * tw[t][1]) % R
        call.rows.append(dict(kind="raw", lam=lam, k2=k2, t=tw[t][1], events=[], c_log=(call.c * lam + k2) % R, d_log=tw[t][1]))
    for r in call.rows:
        rc.check_row([(call.c, r["lam"]), (1, r["k2"])], None, [], r["c_log"])
    reduced = run_enc(dev, call)
    given = dict(secret_words=[rc.word_bytes(w) for w, _k in sw], coef_words=[rc.word_bytes(w) for w, _k in cw],
                 t_words=[rc.word_bytes(w) for w, _k in tw], hash_words=[rc.word_bytes(w) for w, _k in hw])
    assert run_enc(dev, call, **given) == reduced
    for one in given:
        assert run_enc(dev, call, **{one: given[one]}) == reduced
    _c, c1, cd = reduced
    assert differing(cd, [x for r in call.rows for x in (ref.g1(r["c_log"]), ref.g1(r["d_log"]))]) == []
    assert c1 == [ref.g1(s) for _p, s, _c in call.items]
    assert INF1 in cd and INF1 in c1


def test_raw_words_in_dnf_keygen(dev, ref):
    rnd = random.Random("raw dnf")
    rw = rc.raw_words(rnd, 12)
    call = rc.DnfCall(5, 7, 12, {}, "raw")
    call.r = [k for _w, k in rw]
    call.kind = ["r zero" if not k else "ordinary" for k in call.r]
    call.precheck()
    keys = dev.dnf(5, 7)
    reduced = dev.eng.dnf_keygen_dev(keys, [fr_bytes(k) for k in call.r])
    assert dev.eng.dnf_keygen_dev(keys, [rc.word_bytes(w) for w, _k in rw]) == reduced
    want1, want2 = dnf_want(ref, call)
    assert differing(reduced[0], want1) == [] and differing(reduced[1], want2) == []
