"""GPU checks of GHW11's packed service path (include/rabe_host.h: rabe_ghw11_encrypt_packed, rabe_ghw11_decrypt_out_packed):
encrypt_packed against the oracle's golden vectors and byte for byte against the object API on one tape, the whole chain
encrypt_packed -> transform_packed -> decrypt_out_packed, failures that stay with their item, a device group, and a bulk call."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

from rabe_amd import hostlib as hl
from rabe_amd.schemes import ghw11

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PLAINTEXT = b"dance like no one's watching, encrypt like everyone is!"
LANG = {"json": hl.JSON_POLICY, "human": hl.HUMAN_POLICY}
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
ATTRS = ["a%d" % i for i in range(50)]


def hb(s):
    return bytes.fromhex(s)


def fri(x):
    return int.from_bytes(hb(x), "little")


def offsets(items):
    return np.concatenate([[0], np.cumsum([len(p) for p in items])]).astype(np.uint64)


def records(blob, off):
    return [bytes(blob[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


def tree50(rnd, language):
    """a random AND/OR tree over the 50 attributes: every leaf once, so a key holding all of them satisfies it"""
    names = ATTRS[:]
    rnd.shuffle(names)

    def node(ns):
        if len(ns) == 1:
            return '{"name": "%s"}' % ns[0] if language == hl.JSON_POLICY else '"%s"' % ns[0]
        h = rnd.randrange(1, len(ns))
        op = rnd.choice(["and", "or"])
        if language == hl.JSON_POLICY:
            return '{"name": "%s", "children": [%s, %s]}' % (op, node(ns[:h]), node(ns[h:]))
        return "(%s %s %s)" % (node(ns[:h]), op, node(ns[h:]))
    return node(names)


@pytest.fixture(scope="module")
def host():
    h = hl.Host(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def keys(host):
    pk, msk = ghw11.setup(host)
    tk, rk = ghw11.tkgen(host, ghw11.keygen(host, pk, msk, ATTRS + ["A", "B", "C", "D"]))
    return pk, msk, tk, rk


def test_encrypt_packed_matches_golden(host):
    with open(os.path.join(HERE, "golden", "ghw11.json")) as f:
        doc = json.load(f)
    p = doc["pk"]
    pk = hl.Obj.deserialize("ghw11_pk", hb(p["g1"]) + hb(p["g2"]) + hb(p["g1_a"]) + hb(p["g2_a"]) + hb(p["e_gg_alpha"]))
    for c in doc["cases"]:
        et = [fri(x) for x in c["encrypt_tape"]]
        tape = [et[0], fri(c["msg_rho"])] + et[1:] + [13]          # secret, msg, gate coefficients, t_i.., nonce
        host.set_tape(tape)
        blob, off = ghw11.encrypt_packed(host, pk, [c["policy"]], [0], PLAINTEXT, [0, len(PLAINTEXT)], LANG[c["language"]])
        host.clear_tape()
        rec = bytes(blob)
        assert len(off) == 2 and int(off[1]) == len(rec)
        g = hl.parse_obj("ghw11_ct", rec)
        assert (g["c"], g["c1"]) == (hb(c["ct"]["c"]), hb(c["ct"]["c1"]))
        assert g["ci_di"] == [(n, hb(a), hb(b)) for n, a, b in c["ct"]["ci_di"]]
        assert hl.Obj.deserialize("ghw11_ct", rec).serialize() == rec
        host.set_tape(tape)
        assert ghw11.encrypt(host, pk, c["policy"], LANG[c["language"]], PLAINTEXT).serialize() == rec
        host.clear_tape()


@pytest.mark.parametrize("language", [hl.JSON_POLICY, hl.HUMAN_POLICY])
def test_encrypt_packed_equals_object_api_on_one_tape(host, keys, language):
    pk = keys[0]
    rnd = random.Random(11 + language)
    if language == hl.JSON_POLICY:
        pols = ['{"name": "A"}',
                '{"name": "and", "children": [{"name": "A"}, {"name": "or", "children": [{"name": "D"}, {"name": "and", "children": [{"name": "B"}, {"name": "C"}]}]}]}']
    else:
        pols = ['"A" or "B"', '("A" or "D") and ("B" or ("C" and "D"))']
    pols.append(tree50(rnd, language))
    n = 12
    item_pol = [i % 3 for i in range(n)]
    pts = [b"" if i == 4 else bytes(rnd.randrange(256) for _ in range(rnd.randrange(1, 300))) for i in range(n)]
    tape = [rnd.randrange(1, R) for _ in range(n * 110)]
    host.set_tape(tape)
    blob, off = ghw11.encrypt_packed(host, pk, pols, item_pol, b"".join(pts), offsets(pts), language)
    host.set_tape(tape)
    objs = [ghw11.encrypt(host, pk, pols[item_pol[i]], language, pts[i]).serialize() for i in range(n)]
    host.clear_tape()
    assert records(blob, off) == objs


@pytest.fixture(scope="module")
def chain(host, keys):
    """12 items over three policies, one of them unsatisfiable by the key (item 5 and 8: policy 2)"""
    pk, _msk, tk, _rk = keys
    rnd = random.Random(5)
    pols = [tree50(rnd, hl.JSON_POLICY), '{"name": "or", "children": [{"name": "A"}, {"name": "B"}]}',
            '{"name": "and", "children": [{"name": "A"}, {"name": "Z"}]}']
    item_pol = [0, 1, 0, 1, 0, 2, 1, 0, 2, 1, 0, 1]
    pts = [b"item %d " % i * (i + 1) for i in range(len(item_pol))]
    pts[3] = b""
    blob, off = ghw11.encrypt_packed(host, pk, pols, item_pol, b"".join(pts), offsets(pts))
    tct, st = ghw11.transform_packed(host, tk, blob, off)
    return pols, item_pol, pts, blob, off, tct, st


def test_round_trip_through_the_service(host, keys, chain):
    _pk, _msk, _tk, rk = keys
    _pols, item_pol, pts, blob, off, tct, st = chain
    bad = [i for i, p in enumerate(item_pol) if p == 2]
    assert [i for i in range(len(item_pol)) if st[i] != 0] == bad
    for i in bad:
        assert not tct[i].any()                                       # transform_packed's failure mark
    for trusted in (False, True):
        pt, po, status = ghw11.decrypt_out_packed(host, rk, tct, blob, off, trusted=trusted)
        for i in range(len(item_pol)):
            if i in bad:
                assert status[i] == -1 and int(po[i + 1]) == int(po[i])
            else:
                assert status[i] == 0 and bytes(pt[int(po[i]):int(po[i + 1])]) == pts[i]
    recs = records(blob, off)
    for i in (0, 3, 7, 11):                                           # against the object decrypt_out
        tobj = hl.Obj.deserialize("ghw11_tct", tct[i].tobytes())
        assert ghw11.decrypt_out(host, tobj, rk, hl.Obj.deserialize("ghw11_ct", recs[i])) == pts[i]


def test_failures_stay_with_their_item(host, keys, chain):
    pk, msk, _tk, rk = keys
    _pols, item_pol, pts, blob, off, tct, st = chain
    good = [i for i in range(len(item_pol)) if st[i] == 0]

    def opened(res, skip):
        pt, po, status = res
        for i in good:
            if i not in skip:
                assert status[i] == 0 and bytes(pt[int(po[i]):int(po[i + 1])]) == pts[i]
    # t not in Gt: rejected in checked mode
    t2 = tct.copy()
    t2[2, 384 + 7] ^= 0x40
    res = ghw11.decrypt_out_packed(host, rk, t2, blob, off)
    assert res[2][2] == -1
    opened(res, {2})
    assert res[2][5] == -1 and res[2][8] == -1
    # a wrong retrieve key: every item fails, the call succeeds
    _tk2, rk2 = ghw11.tkgen(host, ghw11.keygen(host, pk, msk, ATTRS + ["A", "B"]))
    _pt, _po, status = ghw11.decrypt_out_packed(host, rk2, tct, blob, off)
    assert (status == -1).all()
    # a truncated ciphertext record
    recs = records(blob, off)
    recs[6] = recs[6][:-9]
    res = ghw11.decrypt_out_packed(host, rk, tct, b"".join(recs), offsets(recs))
    assert res[2][6] == -1
    opened(res, {6})


def test_buffers_too_small_report_the_size_needed(host, keys, chain):
    pk, _msk, _tk, rk = keys
    _pols, _item_pol, _pts, blob, off, tct, _st = chain
    lib = host.lib
    pol = (ctypes.c_char_p * 1)(b'{"name": "A"}')
    pts = [b"abc", b"defgh"]
    pt_blob = np.frombuffer(b"".join(pts), dtype=np.uint8)
    pt_off = offsets(pts)
    ip = np.zeros(2, dtype=np.uint32)
    co = np.zeros(3, dtype=np.uint64)
    small = np.zeros(16, dtype=np.uint8)
    rc = lib.rabe_ghw11_encrypt_packed(host.h, pk.ptr, pol, ctypes.c_size_t(1), hl.JSON_POLICY, ctypes.c_size_t(2), hl._np_ptr(ip), hl._np_ptr(pt_blob),
                                       hl._np_ptr(pt_off), hl._np_ptr(small), ctypes.c_size_t(small.size), hl._np_ptr(co))
    assert rc == 1
    full, full_off = ghw11.encrypt_packed(host, pk, ['{"name": "A"}'], [0, 0], b"".join(pts), pt_off)
    assert int(co[2]) == int(full_off[2]) == len(full)
    n = len(off) - 1
    t = np.ascontiguousarray(tct, dtype=np.uint8)
    co = np.ascontiguousarray(off, dtype=np.uint64)
    po = np.zeros(n + 1, dtype=np.uint64)
    status = np.zeros(n, dtype=np.int32)
    rc = lib.rabe_ghw11_decrypt_out_packed(host.h, rk.ptr, ctypes.c_size_t(n), hl._np_ptr(t), hl._np_ptr(blob), ctypes.c_size_t(blob.size),
                                           hl._np_ptr(co), ctypes.c_uint32(0), hl._np_ptr(status), hl._np_ptr(small), ctypes.c_size_t(small.size),
                                           hl._np_ptr(po))
    assert rc == 1 and int(po[n]) == blob.size


def test_device_group_equals_single_engine(keys):
    pk = keys[0]
    rnd = random.Random(3)
    pols = [tree50(rnd, hl.HUMAN_POLICY), '"A" and ("B" or "C")', '"D" or "A"']
    n = 21
    item_pol = [i % 3 for i in range(n)]
    pts = [b"group-%d " % i * (i % 4 + 1) for i in range(n)]
    tape = [rnd.randrange(1, R) for _ in range(n * 110)]
    got = []
    for devices in ([0], [0, 0]):
        h = hl.Host(0) if len(devices) == 1 else hl.Host(devices=devices)
        try:
            assert h.group_size() == len(devices)
            h.set_tape(tape)
            blob, off = ghw11.encrypt_packed(h, pk, pols, item_pol, b"".join(pts), offsets(pts), hl.HUMAN_POLICY)
            got.append((bytes(blob), off.tolist()))
        finally:
            h.close()
    assert got[0] == got[1]


def test_bulk_on_os_randomness(host, keys):
    pk, _msk, tk, rk = keys
    pol = tree50(random.Random(50), hl.JSON_POLICY)
    n = 4096
    pts = [b"bulk item %05d" % i for i in range(n)]
    blob, off = ghw11.encrypt_packed(host, pk, [pol], [0] * n, b"".join(pts), offsets(pts))
    assert len(off) == n + 1
    recs = records(blob, off)
    pick = [0, 1337, 2900, n - 1]
    sub = [recs[i] for i in pick]
    sblob, soff = b"".join(sub), offsets(sub)
    tct, st = ghw11.transform_packed(host, tk, sblob, soff)
    assert (st == 0).all()
    pt, po, status = ghw11.decrypt_out_packed(host, rk, tct, sblob, soff)
    assert (status == 0).all()
    assert [bytes(pt[int(po[j]):int(po[j + 1])]) for j in range(len(pick))] == [pts[i] for i in pick]


def test_a_row_whose_c_cancels_carries_the_encoding_of_infinity(host):
    """a = 1 in the setup tape makes g1_a = g1, so on a one-leaf policy C = g1 * (secret - H t): the t of item 1 is secret / H, its C is the
    point at infinity (64 zero bytes in the reference's encoding) and its D finite; the records equal oracle.schemes on the same tape"""
    from oracle import bn254 as bn
    from oracle import policy as opol
    from oracle import schemes as sch
    from oracle.tape import ListRng
    rnd = random.Random(2011)
    setup_tape = [rnd.randrange(1, R), rnd.randrange(1, R), 1, rnd.randrange(1, R)]
    host.set_tape(setup_tape)
    pk, _msk = ghw11.setup(host)
    host.clear_tape()
    opk, _omsk = sch.ghw11_setup(ListRng(setup_tape))
    assert opk["g1_a"] == opk["g1"]
    policy = '{"name": "A"}'
    h = sch.sha3_hash_fr("A")
    n = 3
    secrets, rhos = [rnd.randrange(1, R) for _ in range(n)], [rnd.randrange(1, R) for _ in range(n)]
    ts = [rnd.randrange(1, R), secrets[1] * bn.fr_inv(h) % R, rnd.randrange(1, R)]
    assert (secrets[1] - h * ts[1]) % R == 0
    tape = [x for i in range(n) for x in (secrets[i], rhos[i], ts[i], 13 + i)]          # secret, msg, t, nonce per item
    host.set_tape(tape)
    blob, off = ghw11.encrypt_packed(host, pk, [policy], [0] * n, PLAINTEXT * n, [len(PLAINTEXT) * i for i in range(n + 1)], hl.JSON_POLICY)
    host.clear_tape()
    e_gen = bn.pairing(bn.G1_GEN, bn.G2_GEN)
    for i, rec in enumerate(records(blob, off)):
        g = hl.parse_obj("ghw11_ct", rec)
        ct = sch.ghw11_encrypt(opk, policy, opol.JSON, ListRng([secrets[i], ts[i]]), bn.gt_pow(e_gen, rhos[i]))
        assert (g["c"], g["c1"]) == (bn.gt_to_le(ct["c"]), bn.g1_to_le(ct["c1"]))
        assert g["ci_di"] == [(node, bn.g1_to_le(ci), bn.g1_to_le(di)) for node, ci, di in ct["ci_di"]]
        assert (ct["ci_di"][0][1] is None) == (g["ci_di"][0][1] == bytes(64)) == (i == 1)
        assert g["ci_di"][0][2] != bytes(64)
