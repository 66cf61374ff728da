"""GPU checks of the bulk key issuing of BDABE / MKE08 (include/rabe_host.h: rabe_{bdabe,mke08}_keygen_packed,
rabe_bdabe_request_attribute_sk_packed, rabe_mke08_request_authority_sk_packed): the oracle's golden vectors, byte equality with the object
API on one tape, keys built from packed records alone through decrypt and decrypt_packed, failures that stay with their item, call-level
errors, capacities, a bulk call and a device group."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

from oracle import bn254 as bn
from rabe_amd import hostlib as hl
from rabe_amd.schemes import bdabe, mke08

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
R = bn.R
SCHEMES = ["bdabe", "mke08"]


def hb(s):
    return bytes.fromhex(s)


def fri(x):
    return int.from_bytes(hb(x), "little")


def offsets(items):
    return np.concatenate([[0], np.cumsum([len(p) for p in items])]).astype(np.uint64)


def records(blob, off):
    return [bytes(blob[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


def u32(v):
    return int(v).to_bytes(4, "little")


def rows_of(rec):
    """(attribute, au1, au2) rows of an output record, and a check that nothing follows them"""
    n = int.from_bytes(rec[:4], "little")
    at, out = 4, []
    for _ in range(n):
        ln = int.from_bytes(rec[at:at + 4], "little")
        name = rec[at + 4:at + 4 + ln].decode("utf-8")
        at += 4 + ln
        out.append((name, rec[at:at + 64], rec[at + 64:at + 192]))
        at += 192
    assert at == len(rec)
    return out


def row_bytes(rows):
    return b"".join(u32(len(n.encode("utf-8"))) + n.encode("utf-8") + a + b for n, a, b in rows)


class Scheme:
    """the two schemes behind one set of calls"""

    def __init__(self, name):
        self.name = name
        self.mod = bdabe if name == "bdabe" else mke08
        self.uk_kind = name + "_uk"
        self.f1, self.f2 = ("u1", "u2") if name == "bdabe" else ("g1", "g2")
        self.user = "u1" if name == "bdabe" else "user1"

    def authgen(self, host, pk, msk, a):
        return bdabe.authgen(host, pk, msk, a) if self.name == "bdabe" else mke08.authgen(host, a)

    def issuer(self, msk, ska, authority):
        """the second argument of keygen: BDABE's authority key, MKE08's master key"""
        return ska[authority] if self.name == "bdabe" else msk

    def keygen(self, host, pk, issuer, name):
        return self.mod.keygen(host, pk, issuer, name)

    def keygen_packed(self, host, pk, issuer, names):
        return self.mod.keygen_packed(host, pk, issuer, names)

    def request(self, host, uk, ska, attr):
        if self.name == "bdabe":
            bdabe.request_attribute_sk(host, uk, ska, attr)
        else:
            mke08.request_authority_sk(host, uk, attr, ska)

    def request_packed(self, host, ska, sets, item_set, blob, off, trusted=False):
        fn = bdabe.request_attribute_sk_packed if self.name == "bdabe" else mke08.request_authority_sk_packed
        return fn(host, ska, sets, item_set, blob, off, trusted=trusted)

    def raw_request(self, host):
        return host.lib.rabe_bdabe_request_attribute_sk_packed if self.name == "bdabe" else host.lib.rabe_mke08_request_authority_sk_packed

    def raw_keygen(self, host):
        return host.lib.rabe_bdabe_keygen_packed if self.name == "bdabe" else host.lib.rabe_mke08_keygen_packed

    def attr_pk(self, host, pk, ska, attr):
        s = ska[attr.split("::")[0]]
        return bdabe.request_attribute_pk(host, pk, s, attr) if self.name == "bdabe" else mke08.request_authority_pk(host, pk, attr, s)

    def upk(self, rec):
        return self.mod.public_user_key_record(rec)


@pytest.fixture(scope="module")
def host():
    h = hl.Host(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def setups(host):
    out = {}
    for name in SCHEMES:
        s = Scheme(name)
        pk, msk = s.mod.setup(host)
        ska = {a: s.authgen(host, pk, msk, a) for a in ("aa1", "aa2")}
        out[name] = (s, pk, msk, ska)
    return out


NAMES = ["", "u", "user-%d", "a much longer user name, number %d, with some padding behind it .........", "zoë-%d-ü中", "u1"]
SETS = [[], ["aa1::solo"], ["aa1::A", "aa1::B", "aa1::C", "aa1::A"], ["aa1::a%d" % i for i in range(50)]]          # set 2 repeats a name
SETS2 = [["aa2::X", "aa2::Y"], []]


def user_names(n):
    return [NAMES[i % len(NAMES)] % i if "%d" in NAMES[i % len(NAMES)] else NAMES[i % len(NAMES)] for i in range(n)]


# ------------------------------------------------------------------------------------------------ golden vectors
@pytest.mark.parametrize("name", SCHEMES)
def test_golden(host, name):
    s = Scheme(name)
    with open(os.path.join(HERE, "golden", name + ".json")) as f:
        doc = json.load(f)
    host.set_tape([fri(x) for x in doc["setup_tape"]])
    pk, msk = s.mod.setup(host)
    ska = {}
    for a in doc["authorities"]:
        host.set_tape([fri(x) for x in a["tape"]])
        ska[a["name"]] = s.authgen(host, pk, msk, a["name"])
    host.clear_tape()
    for c in doc["cases"]:
        issuer = s.issuer(msk, ska, c.get("key_authority"))
        tape = [fri(x) for x in c["keygen_tape"]]
        host.set_tape(tape)
        blob, off = s.keygen_packed(host, pk, issuer, [s.user])
        host.set_tape(tape)
        uk = s.keygen(host, pk, issuer, s.user)
        host.clear_tape()
        rec = bytes(blob)
        assert off.tolist() == [0, len(rec)] and rec == uk.serialize()
        g = hl.parse_obj(s.uk_kind, rec)
        want = c["uk"]
        assert (g["sk"][s.f1], g["sk"][s.f2]) == (hb(want["sk"][s.f1]), hb(want["sk"][s.f2]))
        assert (g["pk"][s.f1], g["pk"][s.f2]) == (hb(want["pk"][s.f1]), hb(want["pk"][s.f2]))
        assert g["sk_a"] == []
        upk = s.upk(rec)
        by_auth = {}
        for auth in sorted({a.split("::")[0] for a in c["sk_attrs"]}):
            mine = [a for a in c["sk_attrs"] if a.split("::")[0] == auth]
            ob, oo, st = s.request_packed(host, ska[auth], [mine], [0], upk, [0, len(upk)])
            assert st.tolist() == [0] and int(oo[1]) == len(ob)
            rows = rows_of(bytes(ob))
            assert [r_[0] for r_ in rows] == mine
            by_auth[auth] = rows
            for nm, au1, au2 in want["sk_a"]:
                if nm.split("::")[0] == auth:
                    assert (nm, hb(au1), hb(au2)) in rows, nm
        taken = {a: 0 for a in by_auth}
        merged = []
        for a in c["sk_attrs"]:
            auth = a.split("::")[0]
            merged.append(by_auth[auth][taken[auth]])
            taken[auth] += 1
        assert merged == [(nm, hb(x), hb(y)) for nm, x, y in want["sk_a"]]
        for a in c["sk_attrs"]:
            s.request(host, uk, ska[a.split("::")[0]], a)
        assert rec[:-4] + u32(len(merged)) + row_bytes(merged) == uk.serialize()


# ------------------------------------------------------------------------------------------------ byte parity on one tape
@pytest.mark.parametrize("name", SCHEMES)
def test_packed_equals_the_object_api_on_one_tape(host, setups, name):
    s, pk, msk, ska = setups[name]
    issuer = s.issuer(msk, ska, "aa1")
    rnd = random.Random(31)
    n = 30
    names = user_names(n)
    assert "" in names and any(len(x.encode("utf-8")) != len(x) for x in names)
    item_set = [i % 4 for i in range(n)]
    rnd.shuffle(item_set)
    item_set2 = [rnd.randrange(2) for _ in range(n)]
    tape = [rnd.randrange(1, R) for _ in range(n)]
    host.set_tape(tape)
    blob, off = s.keygen_packed(host, pk, issuer, names)
    host.set_tape(tape)
    uks = [s.keygen(host, pk, issuer, nm) for nm in names]
    host.clear_tape()
    recs = records(blob, off)
    assert recs == [uk.serialize() for uk in uks]
    for r_ in recs:
        assert hl.Obj.deserialize(s.uk_kind, r_, host=host).serialize() == r_
    upks = [s.upk(r_) for r_ in recs]
    ublob, uoff = b"".join(upks), offsets(upks)
    for i, uk in enumerate(uks):
        for a in SETS[item_set[i]]:
            s.request(host, uk, ska["aa1"], a)
    first = [uk.serialize() for uk in uks]
    outs = None
    for trusted in (False, True):
        ob, oo, st = s.request_packed(host, ska["aa1"], SETS, item_set, ublob, uoff, trusted=trusted)
        assert (st == 0).all()
        outs = records(ob, oo)
        for i in range(n):
            assert recs[i][:-4] + outs[i] == first[i], i                  # the concatenation identity
            assert len(rows_of(outs[i])) == len(SETS[item_set[i]])
        assert outs[item_set.index(0)] == u32(0)
    # a second authority's rows are appended behind the first's, as the object API appends them
    for i, uk in enumerate(uks):
        for a in SETS2[item_set2[i]]:
            s.request(host, uk, ska["aa2"], a)
    ob2, oo2, st2 = s.request_packed(host, ska["aa2"], SETS2, item_set2, ublob, uoff)
    assert (st2 == 0).all()
    outs2 = records(ob2, oo2)
    for i in range(n):
        r1, r2 = rows_of(outs[i]), rows_of(outs2[i])
        both = recs[i][:-4] + u32(len(r1) + len(r2)) + row_bytes(r1) + row_bytes(r2)
        assert both == uks[i].serialize(), i
        assert hl.Obj.deserialize(s.uk_kind, both, host=host).serialize() == both


# ------------------------------------------------------------------------------------------------ round trip
@pytest.mark.parametrize("name", SCHEMES)
def test_keys_from_packed_records_decrypt(host, setups, name):
    s, pk, msk, ska = setups[name]
    issuer = s.issuer(msk, ska, "aa1")
    attrs1, attrs2 = ["aa1::A", "aa1::B", "aa1::C"], ["aa2::X"]
    pkas = [s.attr_pk(host, pk, ska, a) for a in attrs1 + attrs2 + ["aa2::Y"]]
    lists1, lists2 = [attrs1, ["aa1::A"]], [attrs2, []]
    item_set = [0, 1, 0]
    blob, off = s.keygen_packed(host, pk, issuer, ["alice", "bob", ""])
    recs = records(blob, off)
    upks = [s.upk(r_) for r_ in recs]
    ob1, oo1, st1 = s.request_packed(host, ska["aa1"], lists1, item_set, b"".join(upks), offsets(upks))
    ob2, oo2, st2 = s.request_packed(host, ska["aa2"], lists2, item_set, b"".join(upks), offsets(upks))
    assert (st1 == 0).all() and (st2 == 0).all()
    keys = []
    for i in range(3):
        r1, r2 = rows_of(records(ob1, oo1)[i]), rows_of(records(ob2, oo2)[i])
        keys.append(hl.Obj.deserialize(s.uk_kind, recs[i][:-4] + u32(len(r1) + len(r2)) + row_bytes(r1 + r2), host=host))
    pols = ['{"name": "and", "children": [{"name": "aa1::A"}, {"name": "aa2::X"}]}',
            '{"name": "or", "children": [{"name": "aa1::A"}, {"name": "aa2::Y"}]}',
            '{"name": "and", "children": [{"name": "aa1::B"}, {"name": "aa1::C"}]}']
    item_pol = [0, 1, 2, 1]
    pts = [b"round trip item %d " % i * (i + 1) for i in range(4)]
    cblob, coff = s.mod.encrypt_packed(host, pk, pkas, pols, item_pol, b"".join(pts), offsets(pts))
    cts = records(cblob, coff)
    holds = [set(lists1[item_set[i]]) | set(lists2[item_set[i]]) for i in range(3)]
    opens = [lambda h_: {"aa1::A", "aa2::X"} <= h_, lambda h_: bool({"aa1::A", "aa2::Y"} & h_), lambda h_: {"aa1::B", "aa1::C"} <= h_]
    for u, key in enumerate(keys):
        pt, po, pst = s.mod.decrypt_packed(host, key, cblob, coff)
        for i in range(4):
            if opens[item_pol[i]](holds[u]):
                assert pst[i] == 0 and bytes(pt[int(po[i]):int(po[i + 1])]) == pts[i], (u, i)
                assert s.mod.decrypt(host, key, hl.Obj.deserialize(name + "_ct", cts[i], host=host)) == pts[i]
            else:
                assert pst[i] == -1, (u, i)


# ------------------------------------------------------------------------------------------------ failures
def fp2_pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = bn.fp2_mul(r, a)
        a = bn.fp2_mul(a, a)
        e >>= 1
    return r


def fp2_sqrt(a):
    a1 = fp2_pow(a, (bn.P - 3) // 4)
    alpha = bn.fp2_mul(bn.fp2_mul(a1, a1), a)
    x0 = bn.fp2_mul(a1, a)
    if alpha == (bn.P - 1, 0):
        x = bn.fp2_mul((0, 1), x0)
    else:
        x = bn.fp2_mul(fp2_pow(bn.fp2_add((1, 0), alpha), (bn.P - 1) // 2), x0)
    return x if bn.fp2_mul(x, x) == (a[0] % bn.P, a[1] % bn.P) else None


def twist_point_outside_g2():
    bp = bn.fp2_mul((3, 0), bn.fp2_inv((9, 1)))
    x = (1, 0)
    while True:
        y = fp2_sqrt(bn.fp2_add(bn.fp2_mul(bn.fp2_mul(x, x), x), bp))
        if y is not None:
            q = (x, y)
            assert bn.g2_add(bn.g2_mul(q, bn.R - 1), q) is not None
            return q
        x = (x[0] + 1, 0)


@pytest.mark.parametrize("name", SCHEMES)
def test_failures_stay_with_their_item(host, setups, name):
    s, pk, msk, ska = setups[name]
    issuer = s.issuer(msk, ska, "aa1")
    n = 12
    names = user_names(n)
    item_set = [2, 1, 3, 2, 0, 2, 1, 3, 2, 1, 2, 3]
    blob, off = s.keygen_packed(host, pk, issuer, names)
    upks = [s.upk(r_) for r_ in records(blob, off)]
    ob, oo, st = s.request_packed(host, ska["aa1"], SETS, item_set, b"".join(upks), offsets(upks))
    assert (st == 0).all()
    clean = records(ob, oo)
    bad = list(upks)
    bad[1] = bad[1][:-9]                                                                        # truncated
    bad[3] = bad[3] + b"\x00\x01\x02"                                                           # trailing bytes
    assert (1**3 + 3) % bn.P != 3 * 3
    bad[5] = bad[5][:-192] + bn.g1_to_le((1, 3)) + bad[5][-128:]                                # u1 off the curve
    bad[7] = bad[7][:-128] + bn.g2_to_le(twist_point_outside_g2())                              # u2 on the twist, outside G2
    x = int.from_bytes(bad[9][-192:-160], "little")
    bad[9] = bad[9][:-192] + (x + bn.P).to_bytes(32, "little") + bad[9][-160:]                  # a coordinate >= p (the same point otherwise)
    bblob = np.frombuffer(b"".join(bad), dtype=np.uint8)
    boff = offsets(bad)
    boff2 = boff.copy()
    boff2[11] = boff[10] - 1                                                                    # item 10: offsets not monotone
    boff2[12] = boff[12] + 5                                                                    # item 11: past the end of the blob
    for offs, fails in ((boff, {1, 3, 5, 7, 9}), (boff2, {1, 3, 5, 7, 9, 10, 11})):
        ob, oo, st = s.request_packed(host, ska["aa1"], SETS, item_set, bblob, offs)
        assert [i for i in range(n) if st[i] != 0] == sorted(fails)
        got = records(ob, oo)
        for i in range(n):
            assert got[i] == (b"" if i in fails else clean[i]), i
        assert int(oo[n]) == sum(len(clean[i]) for i in range(n) if i not in fails)
    # trusted: the membership pass is skipped, the non-members are not rejected (their keys are unspecified); the neighbours are unchanged
    ob, oo, st = s.request_packed(host, ska["aa1"], SETS, item_set, bblob, boff, trusted=True)
    assert [i for i in range(n) if st[i] != 0] == [1, 3]
    got = records(ob, oo)
    for i in range(n):
        if i not in (1, 3, 5, 7, 9):
            assert got[i] == clean[i], i
    assert got[1] == b"" and got[3] == b"" and len(got[5]) == len(clean[5])


@pytest.mark.parametrize("name", SCHEMES)
def test_call_level_errors_and_capacity(host, setups, name):
    s, pk, msk, ska = setups[name]
    issuer = s.issuer(msk, ska, "aa1")
    rnd = random.Random(4)
    names = ["a", "", "carol"]
    n = len(names)
    tape = [rnd.randrange(1, R) for _ in range(n)]
    host.set_tape(tape)
    full, uo = s.keygen_packed(host, pk, issuer, names)
    host.clear_tape()
    # uk_cap one byte short: 1, offsets filled, nothing drawn -- the next call on the same tape gives the bytes of a fresh one
    arr, _ = hl._strs(names)
    o2 = np.zeros(n + 1, dtype=np.uint64)
    small = np.zeros(len(full) - 1, dtype=np.uint8)
    host.set_tape(tape)
    rc = s.raw_keygen(host)(host.h, pk.ptr, issuer.ptr, arr, ctypes.c_size_t(n), hl._np_ptr(small), ctypes.c_size_t(small.size), hl._np_ptr(o2))
    assert rc == 1 and o2.tolist() == uo.tolist() and int(o2[n]) == len(full) and not small.any()
    again, _ = s.keygen_packed(host, pk, issuer, names)
    host.clear_tape()
    assert bytes(again) == bytes(full)
    # out_cap one byte short
    upks = [s.upk(r_) for r_ in records(full, uo)]
    ublob, uoff = np.frombuffer(b"".join(upks), dtype=np.uint8), offsets(upks)
    item_set = [2, 0, 1]
    ob, oo, st = s.request_packed(host, ska["aa1"], SETS, item_set, ublob, uoff)
    sarr, _ = hl._strs([a for s_ in SETS for a in s_])
    counts = (ctypes.c_size_t * len(SETS))(*[len(s_) for s_ in SETS])
    it = np.array(item_set, dtype=np.uint32)
    o3 = np.zeros(n + 1, dtype=np.uint64)
    st3 = np.zeros(n, dtype=np.int32)
    small = np.zeros(len(ob) - 1, dtype=np.uint8)
    rc = s.raw_request(host)(host.h, ska["aa1"].ptr, sarr, counts, ctypes.c_size_t(len(SETS)), ctypes.c_size_t(n), hl._np_ptr(it), hl._np_ptr(ublob),
                             ctypes.c_size_t(ublob.size), hl._np_ptr(uoff), ctypes.c_uint32(0), hl._np_ptr(st3), hl._np_ptr(small),
                             ctypes.c_size_t(small.size), hl._np_ptr(o3))
    assert rc == 1 and o3.tolist() == oo.tolist() and int(o3[n]) == len(ob) and not small.any()
    # call-level failures: a message, nothing written
    with pytest.raises(hl.RabeError, match=r"attribute aa2::X is not from_authority\(\) or !is_eligible\(\) \(attribute list 1\)"):
        s.request_packed(host, ska["aa1"], [["aa1::A"], ["aa1::B", "aa2::X"]], [0, 0, 0], ublob, uoff)
    with pytest.raises(hl.RabeError, match=r"attribute aa1::a::b is not from_authority"):
        s.request_packed(host, ska["aa1"], [["aa1::a::b"]], [0, 0, 0], ublob, uoff)
    with pytest.raises(hl.RabeError, match="item_set out of range"):
        s.request_packed(host, ska["aa1"], SETS, [0, len(SETS), 1], ublob, uoff)
    # n_items = 0 succeeds
    b0, o0 = s.keygen_packed(host, pk, issuer, [])
    assert len(b0) == 0 and o0.tolist() == [0]
    r0, ro0, st0 = s.request_packed(host, ska["aa1"], SETS, [], b"", [0])
    assert len(r0) == 0 and ro0.tolist() == [0] and len(st0) == 0


# ------------------------------------------------------------------------------------------------ bulk
@pytest.mark.parametrize("name", SCHEMES)
def test_bulk_4096_users_of_8_attributes(host, setups, name):
    s, pk, msk, ska = setups[name]
    issuer = s.issuer(msk, ska, "aa1")
    n = 4096
    attrs = ["aa1::b%d" % i for i in range(8)]
    rnd = random.Random(99)
    names = ["user%05d" % i for i in range(n)]
    tape = [rnd.randrange(1, R) for _ in range(n)]
    host.set_tape(tape)
    blob, off = s.keygen_packed(host, pk, issuer, names)
    host.clear_tape()
    recs = records(blob, off)
    upks = [s.upk(r_) for r_ in recs]
    ob, oo, st = s.request_packed(host, ska["aa1"], [attrs], [0] * n, b"".join(upks), offsets(upks))
    assert (st == 0).all() and len(oo) == n + 1
    outs = records(ob, oo)
    want_len = 4 + sum(4 + len(a) + 192 for a in attrs)
    for i in range(n):
        assert len(recs[i]) == 192 + 4 + 9 + 192 + 4 and recs[i][192:205] == u32(9) + names[i].encode() and recs[i][-4:] == u32(0), i
        assert len(outs[i]) == want_len and [r_[0] for r_ in rows_of(outs[i])] == attrs, i
    assert len(set(outs)) == n and len(set(recs)) == n
    for i in [0, n - 1] + rnd.sample(range(1, n - 1), 62):
        host.set_tape([tape[i]])                                   # one draw per item: item i's position in the tape is i
        uk = s.keygen(host, pk, issuer, names[i])
        host.clear_tape()
        assert recs[i] == uk.serialize(), i
        for a in attrs:
            s.request(host, uk, ska["aa1"], a)
        assert recs[i][:-4] + outs[i] == uk.serialize(), i


@pytest.mark.parametrize("name", SCHEMES)
def test_device_group_runs_on_its_first_device_with_the_same_bytes(setups, name):
    """like the other keygen_packed functions that are not sharded (ghw11, bsw, ac17): a group host runs the calls on devices[0]"""
    s, pk, msk, ska = setups[name]
    issuer = s.issuer(msk, ska, "aa1")
    rnd = random.Random(3)
    names = user_names(19)
    item_set = [rnd.randrange(len(SETS)) for _ in names]
    tape = [rnd.randrange(1, R) for _ in names]
    got = []
    for devices in ([0], [0, 0]):
        h = hl.Host(0) if len(devices) == 1 else hl.Host(devices=devices)
        try:
            assert h.group_size() == len(devices)
            h.set_tape(tape)
            blob, off = s.keygen_packed(h, pk, issuer, names)
            h.clear_tape()
            upks = [s.upk(r_) for r_ in records(blob, off)]
            ob, oo, st = s.request_packed(h, ska["aa1"], SETS, item_set, b"".join(upks), offsets(upks))
            got.append((bytes(blob), off.tolist(), bytes(ob), oo.tolist(), st.tolist()))
        finally:
            h.close()
    assert got[0] == got[1]


# ------------------------------------------------------------------------------------------------ a user key whose u1 cancels
def test_bdabe_user_key_with_u1_at_infinity(host):
    """the tape draws group elements as generator * fr, so the same draw for g1 and p1 makes p1 = g1; with r_u = R - alpha the sum
    sk.u1 = a1 + p1 * r_u = g1 * alpha - g1 * alpha is the point at infinity (64 zero bytes in the reference's encoding), its neighbours and
    sk.u2 stay finite, and every record equals oracle.schemes on the same tape"""
    from oracle import schemes as sch
    from oracle.tape import ListRng
    rnd = random.Random(2018)
    x1, x2, x4, y, alpha, a3 = (rnd.randrange(1, R) for _ in range(6))
    setup_tape, auth_tape = [x1, x2, x1, x4, y], [alpha, a3]
    host.set_tape(setup_tape)
    pk, msk = bdabe.setup(host)
    host.set_tape(auth_tape)
    ska = bdabe.authgen(host, pk, msk, "aa1")
    opk, omsk = sch.bdabe_setup(ListRng(setup_tape))
    oska = sch.bdabe_authgen(opk, omsk, "aa1", ListRng(auth_tape))
    assert opk["p1"] == opk["g1"]
    names = ["u0", "u1", "u2"]
    tape = [rnd.randrange(1, R), R - alpha, rnd.randrange(1, R)]
    host.set_tape(tape)
    blob, off = bdabe.keygen_packed(host, pk, ska, names)
    host.clear_tape()
    for i, rec in enumerate(records(blob, off)):
        g = hl.parse_obj("bdabe_uk", rec)
        want = sch.bdabe_keygen(opk, oska, names[i], ListRng([tape[i]]))
        assert (g["sk"]["u1"], g["sk"]["u2"]) == (bn.g1_to_le(want["sk"]["u1"]), bn.g2_to_le(want["sk"]["u2"]))
        assert (g["pk"]["u1"], g["pk"]["u2"]) == (bn.g1_to_le(want["pk"]["u1"]), bn.g2_to_le(want["pk"]["u2"]))
        assert (want["sk"]["u1"] is None) == (g["sk"]["u1"] == bytes(64)) == (i == 1)
        assert g["sk"]["u2"] != bytes(128) and g["sk_a"] == []
