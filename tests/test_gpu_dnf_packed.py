"""GPU checks of the packed encrypt of the two DNF schemes (include/rabe_host.h: rabe_bdabe_encrypt_packed, rabe_mke08_encrypt_packed):
the oracle's golden vectors, byte parity with the object API on one tape (policies of 1 to 15 terms, both policy languages, an empty
plaintext, r_j = 0 and r - 1), the round trip through the existing decrypt_packed, the term-table cache under two setups whose keys
share attribute names, the errors, a device group and a bulk call."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

from rabe_amd import hostlib as hl
from rabe_amd.schemes import bdabe, mke08

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PLAINTEXT = b"dance like no one's watching, encrypt like everyone is!"
LANG = {"json": hl.JSON_POLICY, "human": hl.HUMAN_POLICY}
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
ATTRS = ["aa%d::A%d" % (1 + i % 3, i) for i in range(24)]
NOT_DNF = {"bdabe": "Error in bdabe/encrypt: Policy not in DNF.", "mke08": "Error in mke08/encrypt: policy is not in dnf"}
JSON_TO_DNF = "Error in json_to_dnf: could not parse policy as DNF"


def hb(s):
    return bytes.fromhex(s)


def fri(x):
    return int.from_bytes(hb(x), "little")


def offsets(items):
    return np.concatenate([[0], np.cumsum([len(p) for p in items])]).astype(np.uint64)


def records(blob, off):
    return [bytes(blob[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


def policy(terms, language):
    """a flat OR of conjunctions (what json_to_dnf accepts)"""
    def leaf(a):
        return '{"name": "%s"}' % a if language == hl.JSON_POLICY else '"%s"' % a

    def conj(t):
        if len(t) == 1:
            return leaf(t[0])
        if language == hl.JSON_POLICY:
            return '{"name": "and", "children": [%s]}' % ", ".join(leaf(a) for a in t)
        return "(%s)" % " and ".join(leaf(a) for a in t)
    if len(terms) == 1:
        return conj(terms[0])
    if language == hl.JSON_POLICY:
        return '{"name": "or", "children": [%s]}' % ", ".join(conj(t) for t in terms)
    return " or ".join(conj(t) for t in terms)


class Scheme:
    """the two schemes behind one set of calls"""

    def __init__(self, name):
        self.name = name
        self.mod = bdabe if name == "bdabe" else mke08
        self.n_gt = 1 if name == "bdabe" else 2
        self.lead = 2 + (self.n_gt - 1)          # draws in front of the r_j: a, b (, c)

    def setup(self, host, authorities=("aa1", "aa2", "aa3")):
        pk, msk = self.mod.setup(host)
        if self.name == "bdabe":
            ska = {a: bdabe.authgen(host, pk, msk, a) for a in authorities}
        else:
            ska = {a: mke08.authgen(host, a) for a in authorities}
        return pk, msk, ska

    def attr_pk(self, host, pk, ska, attr):
        s = ska[attr.split("::")[0]]
        if self.name == "bdabe":
            return bdabe.request_attribute_pk(host, pk, s, attr)
        return mke08.request_authority_pk(host, pk, attr, s)

    def user_key(self, host, pk, msk, ska, attrs):
        if self.name == "bdabe":
            uk = bdabe.keygen(host, pk, ska[sorted(ska)[0]], "u1")
            for a in attrs:
                bdabe.request_attribute_sk(host, uk, ska[a.split("::")[0]], a)
        else:
            uk = mke08.keygen(host, pk, msk, "user1")
            for a in attrs:
                mke08.request_authority_sk(host, uk, a, ska[a.split("::")[0]])
        return uk

    def ct_kind(self):
        return self.name + "_ct"

    def tuples(self, rec):
        g = hl.parse_obj(self.ct_kind(), rec)
        return g["j"] if self.name == "bdabe" else g["e"]


SCHEMES = ["bdabe", "mke08"]


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
        pk, msk, ska = s.setup(host)
        pkas = [s.attr_pk(host, pk, ska, a) for a in ATTRS]
        out[name] = (s, pk, msk, ska, pkas)
    return out


# ------------------------------------------------------------------------------------------------ golden vectors
@pytest.mark.parametrize("name", SCHEMES)
def test_encrypt_packed_matches_golden(host, name):
    s = Scheme(name)
    with open(os.path.join(HERE, "golden", name + ".json")) as f:
        doc = json.load(f)
    host.set_tape([fri(x) for x in doc["setup_tape"]])
    pk, msk = s.mod.setup(host)
    ska = {}
    for a in doc["authorities"]:
        host.set_tape([fri(x) for x in a["tape"]])
        ska[a["name"]] = bdabe.authgen(host, pk, msk, a["name"]) if name == "bdabe" else mke08.authgen(host, a["name"])
    host.clear_tape()
    for c in doc["cases"]:
        host.set_tape([fri(x) for x in c["keygen_tape"]])
        if name == "bdabe":
            uk = bdabe.keygen(host, pk, ska[c["key_authority"]], "u1")
        else:
            uk = mke08.keygen(host, pk, msk, "user1")
        host.clear_tape()
        for a in c["sk_attrs"]:
            if name == "bdabe":
                bdabe.request_attribute_sk(host, uk, ska[a.split("::")[0]], a)
            else:
                mke08.request_authority_sk(host, uk, a, ska[a.split("::")[0]])
        pkas = [s.attr_pk(host, pk, ska, a) for a in c["pk_attrs"]]
        tape = [fri(x) for x in c["encrypt_tape"]] + [17]
        host.set_tape(tape)
        blob, off = s.mod.encrypt_packed(host, pk, pkas, [c["policy"]], [0], PLAINTEXT, [0, len(PLAINTEXT)], LANG[c["language"]])
        host.clear_tape()
        rec = bytes(blob)
        assert len(off) == 2 and int(off[1]) == len(rec)
        assert s.tuples(rec) == [tuple([t[0]] + [hb(x) for x in t[1:]]) for t in c["ct"]]
        ct = hl.Obj.deserialize(s.ct_kind(), rec)
        assert ct.serialize() == rec
        assert s.mod.decrypt(host, uk, ct) == PLAINTEXT
        host.set_tape(tape)
        assert s.mod.encrypt(host, pk, pkas, c["policy"], LANG[c["language"]], PLAINTEXT).serialize() == rec
        host.clear_tape()


# ------------------------------------------------------------------------------------------------ byte parity on one tape
def parity_policies(language):
    A = ATTRS
    return [policy([[A[0]]], language),                                                  # 1 term
            policy([[A[0], A[1]], [A[2]]], language),                                    # 2 terms
            policy([[A[3]], [A[4]], [A[5]]], language),                                  # 3 terms
            policy([[A[i], A[i + 8]] for i in range(8)], language),                      # 15 terms (json_to_dnf's index rule splits ANDs)
            policy([[A[6], A[7]]], language),                                            # 1 term of 2 attributes
            policy([["aa1::NOPE"]], language)]                                           # no attribute key: no terms


@pytest.mark.parametrize("name", SCHEMES)
@pytest.mark.parametrize("language", [hl.JSON_POLICY, hl.HUMAN_POLICY])
def test_encrypt_packed_equals_object_api_on_one_tape(host, setups, name, language):
    s, pk, _msk, _ska, pkas = setups[name]
    rnd = random.Random(7 + language + 10 * s.n_gt)
    pols = parity_policies(language)
    assert [len(hl.policy_dnf_terms(p, ATTRS, language)) for p in pols] == [1, 2, 3, 15, 1, 0]
    n = 16
    item_pol = [i % len(pols) for i in range(n)]
    pts = [b"" if i == 5 else bytes(rnd.randrange(256) for _ in range(rnd.randrange(1, 300))) for i in range(n)]
    tape = [rnd.randrange(1, R) for _ in range(n * 20)]
    host.set_tape(tape)
    blob, off = s.mod.encrypt_packed(host, pk, pkas, pols, item_pol, b"".join(pts), offsets(pts), language)
    host.set_tape(tape)
    objs = [s.mod.encrypt(host, pk, pkas, pols[item_pol[i]], language, pts[i]).serialize() for i in range(n)]
    host.clear_tape()
    assert records(blob, off) == objs


@pytest.mark.parametrize("name", SCHEMES)
def test_edge_draws(host, setups, name):
    """r_j = 0 (infinity in every group element of the term, e1 = msg) and r_j = r - 1, as the object API makes them"""
    s, pk, _msk, _ska, pkas = setups[name]
    pol = policy([[ATTRS[0]], [ATTRS[1]], [ATTRS[2]]], hl.JSON_POLICY)
    lead = [123456789 + k for k in range(s.lead)]
    tape = lead + [0, R - 1, 5] + [9]
    res = []
    for packed in (True, False):
        host.set_tape(tape)
        try:
            if packed:
                blob, _off = s.mod.encrypt_packed(host, pk, pkas, [pol], [0], PLAINTEXT, [0, len(PLAINTEXT)])
                res.append(("ok", bytes(blob)))
            else:
                res.append(("ok", s.mod.encrypt(host, pk, pkas, pol, hl.JSON_POLICY, PLAINTEXT).serialize()))
        except (hl.RabeError, hl.RabePanic) as e:
            res.append((type(e).__name__, str(e)))
        finally:
            host.clear_tape()
    if res[1][0] == "ok":
        assert res[0] == res[1]
        t = s.tuples(res[0][1])
        assert len(t) == 3
        zero = t[0]
        assert all(not any(x) for x in zero[1 + s.n_gt:])            # p1 * 0, p2 * 0, T1 * 0, T2 * 0: the encoding of infinity
    else:
        assert res[0][0] == res[1][0] and res[0][1].startswith(res[1][1])


# ------------------------------------------------------------------------------------------------ round trip
@pytest.mark.parametrize("name", SCHEMES)
def test_round_trip_through_decrypt_packed(host, setups, name):
    s, pk, msk, ska, pkas = setups[name]
    A = ATTRS
    uk = s.user_key(host, pk, msk, ska, [A[0], A[1], A[9], A[12]])
    pols = [policy([[A[0]]], hl.JSON_POLICY),                                  # satisfied
            policy([[A[2]], [A[0], A[1]]], hl.JSON_POLICY),                    # satisfied by its second term
            policy([[A[3]], [A[4]]], hl.JSON_POLICY),                          # not satisfied
            policy([[A[i], A[i + 8]] for i in range(8)], hl.HUMAN_POLICY)]     # satisfied by a late term
    langs = [hl.JSON_POLICY] * 3 + [hl.HUMAN_POLICY]
    n = 14
    item_pol = [i % 4 for i in range(n)]
    pts = [b"round trip %d " % i * (i + 1) for i in range(n)]
    pts[5] = b""
    recs = [None] * n
    for lang in (hl.JSON_POLICY, hl.HUMAN_POLICY):          # one language per call: split the items by their policy's language
        idx = [i for i in range(n) if langs[item_pol[i]] == lang]
        sub = [p for p in range(4) if langs[p] == lang]
        blob, off = s.mod.encrypt_packed(host, pk, pkas, [pols[p] for p in sub], [sub.index(item_pol[i]) for i in idx],
                                         b"".join(pts[i] for i in idx), offsets([pts[i] for i in idx]), lang)
        for j, r in zip(idx, records(blob, off)):
            recs[j] = r
    out, po, st = s.mod.decrypt_packed(host, uk, b"".join(recs), offsets(recs))
    for i in range(n):
        if item_pol[i] == 2:
            assert st[i] == -1 and int(po[i + 1]) == int(po[i])
        else:
            assert st[i] == 0 and bytes(out[int(po[i]):int(po[i + 1])]) == pts[i]
    for i in (0, 1, 3, 5):
        assert s.mod.decrypt(host, uk, hl.Obj.deserialize(s.ct_kind(), recs[i])) == pts[i]


# ------------------------------------------------------------------------------------------------ the term-table cache
@pytest.mark.parametrize("name", SCHEMES)
def test_same_policy_text_under_two_setups(host, name):
    s = Scheme(name)
    names = ["aa1::X", "aa1::Y"]
    pol = policy([["aa1::X", "aa1::Y"], ["aa1::Y"]], hl.JSON_POLICY)
    made = []
    for _ in range(2):
        pk, msk, ska = s.setup(host, ("aa1",))
        pkas = [s.attr_pk(host, pk, ska, a) for a in names]
        uk = s.user_key(host, pk, msk, ska, names)
        pts = [b"setup %d item %d" % (len(made), i) for i in range(3)]
        blob, off = s.mod.encrypt_packed(host, pk, pkas, [pol], [0, 0, 0], b"".join(pts), offsets(pts))
        made.append((uk, bytes(blob), off, pts))
    for k, (_uk, blob, off, pts) in enumerate(made):
        for j, (uk, _b, _o, _p) in enumerate(made):
            out, po, st = s.mod.decrypt_packed(host, uk, blob, off)
            if j == k:
                assert (st == 0).all() and records(out, po) == pts
            else:
                assert (st == -1).all()


# ------------------------------------------------------------------------------------------------ errors
@pytest.mark.parametrize("name", SCHEMES)
def test_errors_fail_the_call(host, setups, name):
    s, pk, _msk, _ska, pkas = setups[name]
    A = ATTRS
    good = policy([[A[0]]], hl.JSON_POLICY)
    pt, po = b"abc", [0, 3]
    not_dnf = '{"name": "and", "children": [{"name": "or", "children": [{"name": "%s"}, {"name": "%s"}]}, {"name": "%s"}]}' % (A[0], A[1], A[2])
    with pytest.raises(hl.RabeError) as e:
        s.mod.encrypt(host, pk, pkas, not_dnf, hl.JSON_POLICY, pt)
    assert str(e.value) == NOT_DNF[name]
    with pytest.raises(hl.RabeError) as e:
        s.mod.encrypt_packed(host, pk, pkas, [good, not_dnf], [0], pt, po)
    assert str(e.value).startswith(NOT_DNF[name]) and "policies[1]" in str(e.value)
    # an OR below an OR passes the DNF test and fails json_to_dnf: the object API's panic
    nested = '{"name": "or", "children": [{"name": "or", "children": [{"name": "%s"}, {"name": "%s"}]}, {"name": "%s"}]}' % (A[0], A[1], A[2])
    with pytest.raises(hl.RabePanic) as e:
        s.mod.encrypt(host, pk, pkas, nested, hl.JSON_POLICY, pt)
    assert JSON_TO_DNF in str(e.value)
    with pytest.raises(hl.RabePanic) as e:
        s.mod.encrypt_packed(host, pk, pkas, [nested, good], [1], pt, po)
    assert JSON_TO_DNF in str(e.value) and "policies[0]" in str(e.value)
    with pytest.raises(hl.RabeError) as e:
        s.mod.encrypt_packed(host, pk, pkas, [good], [0, 1], pt + pt, [0, 3, 6])
    assert "item_policy out of range" in str(e.value)
    # an attribute without a public key is dropped from its conjunction by the object API (json_to_dnf finds no key for it); the packed
    # call does the same
    host.set_tape(list(range(1, 40)))
    missing = policy([[A[0], "aa2::MISSING"], ["aa3::MISSING"]], hl.JSON_POLICY)
    blob, _off = s.mod.encrypt_packed(host, pk, pkas, [missing], [0], pt, po)
    host.set_tape(list(range(1, 40)))
    assert bytes(blob) == s.mod.encrypt(host, pk, pkas, missing, hl.JSON_POLICY, pt).serialize()
    host.clear_tape()


@pytest.mark.parametrize("name", SCHEMES)
def test_buffer_too_small_reports_the_size_needed(host, setups, name):
    s, pk, _msk, _ska, pkas = setups[name]
    pols = [policy([[ATTRS[0]], [ATTRS[1]]], hl.JSON_POLICY)]
    pol = (ctypes.c_char_p * 1)(pols[0].encode())
    arr = (ctypes.c_void_p * len(pkas))(*[p.ptr for p in pkas])
    pts = [b"abc", b"defgh"]
    pt_blob = np.frombuffer(b"".join(pts), dtype=np.uint8)
    pt_off = offsets(pts)
    ip = np.zeros(2, dtype=np.uint32)
    co = np.zeros(3, dtype=np.uint64)
    small = np.zeros(16, dtype=np.uint8)
    rc = getattr(host.lib, "rabe_%s_encrypt_packed" % name)(host.h, pk.ptr, arr, ctypes.c_size_t(len(pkas)), pol, ctypes.c_size_t(1), hl.JSON_POLICY,
                                                             ctypes.c_size_t(2), hl._np_ptr(ip), hl._np_ptr(pt_blob), hl._np_ptr(pt_off),
                                                             hl._np_ptr(small), ctypes.c_size_t(small.size), hl._np_ptr(co))
    assert rc == 1
    full, full_off = s.mod.encrypt_packed(host, pk, pkas, pols, [0, 0], b"".join(pts), pt_off)
    assert int(co[2]) == int(full_off[2]) == len(full)


# ------------------------------------------------------------------------------------------------ device group, bulk
@pytest.mark.parametrize("name", SCHEMES)
def test_device_group_equals_single_engine(setups, name):
    s, pk, _msk, _ska, pkas = setups[name]
    rnd = random.Random(3)
    pols = parity_policies(hl.HUMAN_POLICY)
    n = 21
    item_pol = [i % len(pols) for i in range(n)]
    pts = [b"group-%d " % i * (i % 4 + 1) for i in range(n)]
    tape = [rnd.randrange(1, R) for _ in range(n * 20)]
    got = []
    for devices in ([0], [0, 0]):
        h = hl.Host(0) if len(devices) == 1 else hl.Host(devices=devices)
        try:
            assert h.group_size() == len(devices)
            h.set_tape(tape)
            blob, off = s.mod.encrypt_packed(h, pk, pkas, pols, item_pol, b"".join(pts), offsets(pts), hl.HUMAN_POLICY)
            got.append((bytes(blob), off.tolist()))
        finally:
            h.close()
    assert got[0] == got[1]


@pytest.mark.parametrize("name", SCHEMES)
def test_bulk_on_os_randomness(host, setups, name):
    s, pk, msk, ska, pkas = setups[name]
    A = ATTRS
    pols = [policy([[A[i]] for i in range(8)], hl.JSON_POLICY), policy([[A[9]], [A[10]], [A[11]]], hl.JSON_POLICY)]
    uk = s.user_key(host, pk, msk, ska, [A[7], A[11]])
    n = 4096
    item_pol = [i % 2 for i in range(n)]
    pts = [b"bulk item %05d" % i for i in range(n)]
    blob, off = s.mod.encrypt_packed(host, pk, pkas, pols, item_pol, b"".join(pts), offsets(pts))
    assert len(off) == n + 1
    recs = records(blob, off)
    pick = [0, 1, 1337, 2900, n - 2, n - 1]
    sub = [recs[i] for i in pick]
    out, po, st = s.mod.decrypt_packed(host, uk, b"".join(sub), offsets(sub))
    assert (st == 0).all()
    assert records(out, po) == [pts[i] for i in pick]
    for i in pick[:2]:
        assert s.mod.decrypt(host, uk, hl.Obj.deserialize(s.ct_kind(), recs[i])) == pts[i]
