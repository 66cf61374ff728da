"""GPU checks of GHW11's decrypt for a key holder without a proxy (include/rabe_host.h: rabe_ghw11_decrypt_packed, rabe_ghw11_decrypt,
rabe_ghw11_decrypt_gt).  Its definition is the chain tkgen -> transform_packed -> decrypt_out_packed for any z, so that chain is the
reference here; decrypt_gt is held to the oracle's c * t_1^-1 on the golden vectors.  The suite's pairing mode (99, tests/conftest.py) runs
every launch as the automatic selection would and again with each kernel family forced, and compares the final bytes -- msg, not t."""
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
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
LANG = {"json": hl.JSON_POLICY, "human": hl.HUMAN_POLICY}
KEY_ATTRS = ["A", "B", "C", "D", "E"]
P_AND2 = '{"name": "and", "children": [{"name": "A"}, {"name": "B"}]}'
# five leaves; the key holds none of X, Y, W and satisfies through the second child of the OR
P_MIXED5 = ('{"name": "or", "children": [{"name": "and", "children": [{"name": "X"}, {"name": "Y"}, {"name": "W"}]}, '
            '{"name": "and", "children": [{"name": "C"}, {"name": "D"}]}]}')
P_LEAF = '{"name": "E"}'          # one leaf: m + 2 = 3 pairs, the smallest count
P_UNSAT = '{"name": "and", "children": [{"name": "A"}, {"name": "Z"}]}'
# one more than the six-lane Miller kernel takes on its own: ten groups per wave, one wave per SIMD, 4 SIMDs on each of the MI355X's 256 CUs
# (engine_coop.hip: rhip_use_c6) -- from here on the automatic selection runs the reduced-radix Miller loops (docs/rr29.md)
N_BIG = 256 * 4 * 10 + 1


def hb(s):
    return bytes.fromhex(s)


def offsets(items):
    return np.concatenate([[0], np.cumsum([len(p) for p in items])]).astype(np.uint64)


def records(blob, off):
    return [bytes(blob[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


def slots(res):
    pt, po, _status = res
    return [bytes(pt[int(po[i]):int(po[i + 1])]) for i in range(len(po) - 1)]


def u32(v):
    return int(v).to_bytes(4, "little")


def build_ct(g):
    """the record of a parsed Ghw11Ciphertext (hostlib.parse_obj), so that a test can reorder or damage its fields"""
    out = u32(len(g["policy"][0].encode())) + g["policy"][0].encode() + bytes([g["policy"][1]]) + g["c"] + g["c1"] + u32(len(g["ci_di"]))
    for name, ci, di in g["ci_di"]:
        out += u32(len(name.encode())) + name.encode() + ci + di
    return out + u32(len(g["data"])) + g["data"]


@pytest.fixture(scope="module")
def host():
    h = hl.Host(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def keys(host):
    pk, msk = ghw11.setup(host)
    return pk, msk, ghw11.keygen(host, pk, msk, KEY_ATTRS)


def tkgen_with(host, sk, z):
    host.set_tape([z])
    tk, rk = ghw11.tkgen(host, sk)
    host.clear_tape()
    assert rk.serialize() == int(z).to_bytes(32, "little")
    return tk, rk


def chain(host, sk, z, blob, off):
    tk, rk = tkgen_with(host, sk, z)
    tct, _st = ghw11.transform_packed(host, tk, blob, off)
    return ghw11.decrypt_out_packed(host, rk, tct, blob, off)


@pytest.fixture(scope="module")
def batch(host, keys):
    """67 items over the three policies: a wave of items plus a tail, ragged pair counts (4, 4, 3), encrypted on a tape"""
    pk = keys[0]
    rnd = random.Random(67)
    pols = [P_AND2, P_MIXED5, P_LEAF]
    n = 67
    item_pol = [i % 3 for i in range(n)]
    pts = [b"" if i == 9 else bytes(rnd.randrange(256) for _ in range(rnd.randrange(1, 90))) for i in range(n)]
    host.set_tape([rnd.randrange(1, R) for _ in range(n * 16)])
    blob, off = ghw11.encrypt_packed(host, pk, pols, item_pol, b"".join(pts), offsets(pts))
    host.clear_tape()
    return pts, blob, off


def test_equals_the_chain_for_two_z(host, keys, batch):
    sk = keys[2]
    pts, blob, off = batch
    for trusted in (False, True):
        res = ghw11.decrypt_packed(host, sk, blob, off, trusted=trusted)
        assert (res[2] == 0).all()
        assert slots(res) == pts
    rnd = random.Random(2)
    for _ in range(2):
        ref = chain(host, sk, rnd.randrange(2, R), blob, off)
        assert res[2].tolist() == ref[2].tolist()
        assert res[1].tolist() == ref[1].tolist()
        assert bytes(res[0]) == bytes(ref[0])


def test_equals_the_chain_where_the_reduced_radix_miller_loops_run(host, keys):
    pk, _msk, sk = keys
    pts = [b"%05d" % i for i in range(N_BIG)]
    blob, off = ghw11.encrypt_packed(host, pk, [P_AND2], [0] * N_BIG, b"".join(pts), offsets(pts))
    res = ghw11.decrypt_packed(host, sk, blob, off)
    assert (res[2] == 0).all()
    assert bytes(res[0]) == b"".join(pts) and res[1].tolist() == offsets(pts).tolist()
    ref = chain(host, sk, 0x5EED5EED5EED, blob, off)
    assert res[2].tolist() == ref[2].tolist() and res[1].tolist() == ref[1].tolist() and bytes(res[0]) == bytes(ref[0])


def test_object_decrypt_and_decrypt_gt_match_the_golden_vectors(host):
    with open(os.path.join(HERE, "golden", "ghw11.json")) as f:
        doc = json.load(f)
    for c in doc["cases"]:
        sk = hl.Obj.deserialize("ghw11_sk", hb(c["sk"]["k"]) + hb(c["sk"]["l"]) + u32(len(c["sk"]["attr_key"]))
                                + b"".join(u32(len(n.encode())) + n.encode() + hb(k) for n, k in c["sk"]["attr_key"]))
        msg = hb(c["msg"])          # = the oracle's c * t_1^-1 (tests/test_ghw11_decrypt_surface.py holds the oracle to it)
        sealed = hl.encrypt_symmetric(msg, b"golden plaintext", bytes(range(12)))
        rec = build_ct({"policy": (c["policy"], LANG[c["language"]]), "c": hb(c["ct"]["c"]), "c1": hb(c["ct"]["c1"]),
                        "ci_di": [(n, hb(a), hb(b)) for n, a, b in c["ct"]["ci_di"]], "data": sealed})
        ct = hl.Obj.deserialize("ghw11_ct", rec)
        assert ghw11.decrypt_gt(host, sk, ct) == msg == hb(c["decrypted"])
        assert ghw11.decrypt(host, sk, ct) == b"golden plaintext"
        res = ghw11.decrypt_packed(host, sk, rec, [0, len(rec)])
        assert res[2].tolist() == [0] and slots(res) == [b"golden plaintext"]


def test_object_decrypt_refuses_a_policy_the_key_does_not_satisfy(host, keys):
    pk, _msk, sk = keys
    ct = ghw11.encrypt(host, pk, P_UNSAT, hl.JSON_POLICY, b"x")
    with pytest.raises(hl.RabeError):
        ghw11.decrypt(host, sk, ct)


def test_failures_stay_with_their_item(host, keys, batch):
    pk, _msk, sk = keys
    pts, blob, off = batch
    recs = records(blob, off)[:9]
    want = list(pts[:9])
    bad = {}
    bad[1] = ghw11.encrypt(host, pk, P_UNSAT, hl.JSON_POLICY, b"never").serialize()          # the key does not satisfy the policy
    bad[2] = recs[2][:-9]                                                                       # a truncated record
    g = hl.parse_obj("ghw11_ct", recs[4])
    ci = bytearray(g["ci_di"][0][1]); ci[0] ^= 1                                                # C_0 moved off the curve (x + 1: still canonical)
    bad[4] = build_ct(dict(g, ci_di=[(g["ci_di"][0][0], bytes(ci), g["ci_di"][0][2])] + g["ci_di"][1:]))
    g = hl.parse_obj("ghw11_ct", recs[5])
    c = bytearray(g["c"]); c[40] ^= 2                                                           # c: canonical coordinates, not in Gt
    bad[5] = build_ct(dict(g, c=bytes(c)))
    g = hl.parse_obj("ghw11_ct", recs[7])
    d = bytearray(g["data"]); d[14] ^= 0x80                                                     # a flipped ciphertext byte: the tag fails
    bad[7] = build_ct(dict(g, data=bytes(d)))
    for i, r in bad.items():
        recs[i] = r
    blob9 = np.frombuffer(b"".join(recs), dtype=np.uint8)
    off9 = offsets(recs)
    off9[9] += 5                                                                                # item 8's bounds run past ct_len
    res = ghw11.decrypt_packed(host, sk, blob9, off9)
    first_error = (host.lib.rabe_host_last_error(None) or b"").decode()
    assert first_error == "Error: attributes in tk do not match policy in ct."          # item 1's, in transform_packed's words
    failed = sorted(list(bad) + [8])
    assert len(failed) == 6
    got = slots(res)
    for i in range(9):
        if i in failed:
            assert res[2][i] == -1 and got[i] == b"", i
        else:
            assert res[2][i] == 0 and got[i] == want[i], i
    po = res[1].tolist()
    assert po[0] == 0 and all(a <= b for a, b in zip(po, po[1:])) and po[9] == len(res[0]) == sum(len(want[i]) for i in (0, 3, 6))
    # the chain fails the same items (its own tag failure leaves a zeroed slot behind where this call leaves an empty one)
    ref = chain(host, sk, 77, blob9, off9)
    assert ref[2].tolist() == res[2].tolist()


def test_rows_in_another_order_take_the_row_lookup(host, keys, batch):
    sk = keys[2]
    pts, blob, off = batch
    recs = records(blob, off)
    i = 1                                                                                       # the five-leaf policy
    g = hl.parse_obj("ghw11_ct", recs[i])
    assert len(g["ci_di"]) == 5
    rows = [g["ci_di"][k] for k in (3, 0, 4, 2, 1)]
    swapped = build_ct(dict(g, ci_di=rows))
    assert swapped != recs[i] and len(swapped) == len(recs[i])
    mix = [recs[0], swapped, recs[i], recs[2]]
    res = ghw11.decrypt_packed(host, sk, b"".join(mix), offsets(mix))
    assert res[2].tolist() == [0, 0, 0, 0]
    assert slots(res) == [pts[0], pts[i], pts[i], pts[2]]
    # a row the selection needs is missing from the record: that item alone
    short = build_ct(dict(g, ci_di=[r for r in g["ci_di"] if not r[0].startswith("C")]))
    mix = [recs[0], short, recs[2]]
    res = ghw11.decrypt_packed(host, sk, b"".join(mix), offsets(mix))
    assert res[2].tolist() == [0, -1, 0] and slots(res) == [pts[0], b"", pts[2]]


def test_sizing(host, keys, batch):
    sk = keys[2]
    pts, blob, off = batch
    n = 5
    sub = records(blob, off)[:n]
    sblob, soff = np.frombuffer(b"".join(sub), dtype=np.uint8), offsets(sub)
    need = sum(len(p) + 28 for p in pts[:n])          # nonce and tag ride with every sealed part
    po = np.zeros(n + 1, dtype=np.uint64)
    status = np.full(n, 7, dtype=np.int32)
    buf = np.full(need, 0xAB, dtype=np.uint8)

    def call(cap, count=n):
        return host.lib.rabe_ghw11_decrypt_packed(host.h, sk.ptr, ctypes.c_size_t(count), hl._np_ptr(sblob), ctypes.c_size_t(sblob.size), hl._np_ptr(soff),
                                                  ctypes.c_uint32(0), hl._np_ptr(status), hl._np_ptr(buf), ctypes.c_size_t(cap), hl._np_ptr(po))
    assert call(need - 1) == 1
    assert int(po[n]) == need and (buf == 0xAB).all() and (status == 7).all()
    assert call(need) == 0
    assert (status == 0).all() and bytes(buf[:int(po[n])]) == b"".join(pts[:n])
    po[:] = 99
    assert call(0, 0) == 0 and int(po[0]) == 0


def test_no_randomness_is_drawn(host, keys, batch):
    sk = keys[2]
    pts, blob, off = batch
    z1, z2 = 0x1234567, 0x7654321
    host.set_tape([z1, z2])
    res = ghw11.decrypt_packed(host, sk, blob, off)
    ct = hl.Obj.deserialize("ghw11_ct", records(blob, off)[0])
    assert ghw11.decrypt(host, sk, ct) == pts[0]
    _tk, rk = ghw11.tkgen(host, sk)          # the tape's first value is still the next draw
    _tk, rk2 = ghw11.tkgen(host, sk)
    host.clear_tape()
    assert (res[2] == 0).all()
    assert rk.serialize() == z1.to_bytes(32, "little") and rk2.serialize() == z2.to_bytes(32, "little")


def test_two_keys_in_alternation_keep_their_own_lines(host, keys, batch):
    pk, msk, sk = keys
    pts, blob, off = batch
    other = ghw11.keygen(host, pk, msk, ["E", "A"])          # satisfies the one-leaf policy only; its k, l, k_x differ from sk's
    n = len(pts)
    for _ in range(2):
        res = ghw11.decrypt_packed(host, sk, blob, off)
        assert (res[2] == 0).all() and slots(res) == pts
        res = ghw11.decrypt_packed(host, other, blob, off)
        assert res[2].tolist() == [0 if i % 3 == 2 else -1 for i in range(n)]
        assert slots(res) == [pts[i] if i % 3 == 2 else b"" for i in range(n)]
