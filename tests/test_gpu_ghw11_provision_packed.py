"""GPU checks of GHW11's bulk provisioning (include/rabe_host.h: rabe_ghw11_provision_packed): the oracle's golden vectors on the tape
keygen_tape + tkgen_tape, byte equality with rabe_ghw11_keygen_packed followed by rabe_ghw11_tkgen_packed on the same draws, the chain
provision_packed -> encrypt_packed -> transform_packed -> decrypt_out_packed, call-level failures and capacities, the lazily built table
of g2_alpha leaving keygen_packed alone, and a device group."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

from oracle import bn254 as bn
from rabe_amd import hostlib as hl
from rabe_amd.schemes import ghw11

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
R = bn.R
SETS = [["solo"], ["A", "B", "C", "A"], ["a%d" % i for i in range(100)], ["B", "D"]]          # set 1 repeats a name


def hb(s):
    return bytes.fromhex(s)


def fri(x):
    return int.from_bytes(hb(x), "little")


def offsets(items):
    return np.concatenate([[0], np.cumsum([len(p) for p in items])]).astype(np.uint64)


def records(blob, off):
    return [bytes(blob[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


@pytest.fixture(scope="module")
def host():
    h = hl.Host(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def authority(host):
    return ghw11.setup(host)


def raw_call(host, pk, msk, sets, item_set, sk_buf, sk_off, tk_buf, tk_off, rk):
    """rabe_ghw11_provision_packed itself, on the caller's buffers (sk_off None: NULL); returns its return code"""
    arr, _ = hl._strs([a for s_ in sets for a in s_])
    counts = (ctypes.c_size_t * max(len(sets), 1))(*[len(s_) for s_ in sets])
    it = np.array(item_set, dtype=np.uint32)
    return host.lib.rabe_ghw11_provision_packed(host.h, pk.ptr, msk.ptr, arr, counts, ctypes.c_size_t(len(sets)), ctypes.c_size_t(len(item_set)),
                                                hl._np_ptr(it), hl._np_ptr(sk_buf), ctypes.c_size_t(sk_buf.size),
                                                hl._np_ptr(sk_off) if sk_off is not None else None, hl._np_ptr(tk_buf), ctypes.c_size_t(tk_buf.size),
                                                hl._np_ptr(tk_off), hl._np_ptr(rk))


def test_golden(host):
    with open(os.path.join(HERE, "golden", "ghw11.json")) as f:
        doc = json.load(f)
    p = doc["pk"]
    pkb = hb(p["g1"]) + hb(p["g2"]) + hb(p["g1_a"]) + hb(p["g2_a"]) + hb(p["e_gg_alpha"])
    pk = hl.Obj.deserialize("ghw11_pk", pkb)
    msk = hl.Obj.deserialize("ghw11_msk", hb(doc["msk"]["g2_alpha"]) + pkb)
    assert doc["cases"]
    for c in doc["cases"]:
        host.set_tape([fri(x) for x in c["keygen_tape"]] + [fri(x) for x in c["tkgen_tape"]])
        skb, so, tkb, to, rk = ghw11.provision_packed(host, pk, msk, [c["attrs"]], [0])
        host.clear_tape()
        g = hl.parse_obj("ghw11_sk", bytes(skb))
        assert (g["k"], g["l"]) == (hb(c["sk"]["k"]), hb(c["sk"]["l"]))
        assert g["attr_key"] == [(n, hb(x)) for n, x in c["sk"]["attr_key"]]
        t = hl.parse_obj("ghw11_tk", bytes(tkb))
        assert (t["k_z"], t["l_z"]) == (hb(c["tk"]["k_z"]), hb(c["tk"]["l_z"]))
        assert t["attr_key_z"] == [(n, hb(x)) for n, x in c["tk"]["attr_key_z"]]
        assert rk.shape == (1, 32) and rk[0].tobytes() == hb(c["tkgen_tape"][0])
        assert so.tolist() == [0, len(skb)] and to.tolist() == [0, len(tkb)]


def test_equals_keygen_packed_then_tkgen_packed_on_the_same_draws(host, authority):
    pk, msk = authority
    rnd = random.Random(77)
    item_set = [i % 3 for i in range(24)] + [3, 1, 2]
    rnd.shuffle(item_set)
    n = len(item_set)
    ktape = [rnd.randrange(1, R) for _ in range(n)]
    ztape = [rnd.randrange(1, R) for _ in range(n)]
    host.set_tape(ktape + ztape)
    skb, so, tkb, to, rk = ghw11.provision_packed(host, pk, msk, SETS, item_set)
    host.set_tape(ktape + ztape)
    none_b, none_o, tkb2, to2, rk2 = ghw11.provision_packed(host, pk, msk, SETS, item_set, want_sk=False)
    host.set_tape(ktape)
    blob, off = ghw11.keygen_packed(host, pk, msk, SETS, item_set)
    host.clear_tape()
    assert so.tolist() == off.tolist() and bytes(skb) == bytes(blob)
    for trusted in (False, True):
        host.set_tape(ztape)
        ref_tk, ref_to, ref_rk, st = ghw11.tkgen_packed(host, blob, off, trusted=trusted)
        host.clear_tape()
        assert (st == 0).all()
        assert to.tolist() == ref_to.tolist() and bytes(tkb) == bytes(ref_tk) and rk.tobytes() == ref_rk.tobytes()
    assert rk.tobytes() == b"".join(z.to_bytes(32, "little") for z in ztape)
    assert none_b is None and none_o is None
    assert to2.tolist() == to.tolist() and bytes(tkb2) == bytes(tkb) and rk2.tobytes() == rk.tobytes()
    for r_ in records(skb, so):
        assert hl.Obj.deserialize("ghw11_sk", r_, host=host).serialize() == r_
    for t_ in records(tkb, to):
        assert hl.Obj.deserialize("ghw11_tk", t_, host=host).serialize() == t_
    for i in range(n):
        assert hl.Obj.deserialize("ghw11_rk", rk[i].tobytes()).serialize() == rk[i].tobytes()


def test_the_keys_work_through_the_service(host, authority):
    pk, msk = authority
    item_set = [1, 3, 1, 2, 3, 1]                  # users 1 and 4 hold {B, D}: no "A"
    _skb, _so, tkb, to, rk = ghw11.provision_packed(host, pk, msk, SETS, item_set, want_sk=False)
    tks = records(tkb, to)
    pols = ['{"name": "and", "children": [{"name": "A"}, {"name": "B"}]}', '{"name": "or", "children": [{"name": "B"}, {"name": "a7"}]}']
    item_pol = [0, 1, 0, 1]
    pts = [b"provisioned item %d " % i * (i + 1) for i in range(4)]
    cblob, coff = ghw11.encrypt_packed(host, pk, pols, item_pol, b"".join(pts), offsets(pts))
    seen = set()
    for u in (0, 1, 3):                             # one transform call per distinct key: lists {A, B, C}, {B, D}, a0 .. a99
        tk = hl.Obj.deserialize("ghw11_tk", tks[u], host=host)
        rko = hl.Obj.deserialize("ghw11_rk", rk[u].tobytes())
        tct, tst = ghw11.transform_packed(host, tk, cblob, coff)
        attrs = SETS[item_set[u]]
        want = [0 if ("A" in attrs and "B" in attrs) else -1, 0 if ("B" in attrs or "a7" in attrs) else -1] * 2
        assert tst.tolist() == want, u
        pt, po, pst = ghw11.decrypt_out_packed(host, rko, tct, cblob, coff)
        for i in range(4):
            if want[i] == 0:
                assert pst[i] == 0 and bytes(pt[int(po[i]):int(po[i + 1])]) == pts[i]
                seen.add(True)
            else:
                assert pst[i] == -1
                seen.add(False)
    assert seen == {True, False}


def test_capacity_and_call_level_errors(host, authority):
    pk, msk = authority
    rnd = random.Random(4)
    item_set = [1, 0, 3]
    n = len(item_set)
    tape = [rnd.randrange(1, R) for _ in range(2 * n)]
    host.set_tape(tape)
    skb, so, tkb, to, rk = ghw11.provision_packed(host, pk, msk, SETS, item_set)
    host.clear_tape()
    full = (bytes(skb), so.tolist(), bytes(tkb), to.tolist(), rk.tobytes())

    def attempt(sk_size, tk_size, with_sk=True, sets=SETS, items=item_set):
        sk_buf, tk_buf = np.full(sk_size, 0xAB, dtype=np.uint8), np.full(tk_size, 0xAB, dtype=np.uint8)
        o1, o2 = (np.zeros(len(items) + 1, dtype=np.uint64) if with_sk else None), np.zeros(len(items) + 1, dtype=np.uint64)
        rk2 = np.full((max(len(items), 1), 32), 0xAB, dtype=np.uint8)
        rc = raw_call(host, pk, msk, sets, items, sk_buf, o1, tk_buf, o2, rk2)
        untouched = (sk_buf == 0xAB).all() and (tk_buf == 0xAB).all() and (rk2 == 0xAB).all()
        return rc, sk_buf, o1, tk_buf, o2, rk2, untouched

    # either capacity one byte short: 1, the offsets filled, nothing written and nothing drawn -- the tape set ONCE serves the refused
    # calls and then the one with room, which gives the bytes of the first call
    host.set_tape(tape)
    rc, _s, o1, _t, o2, _r, untouched = attempt(len(skb), len(tkb) - 1)
    assert rc == 1 and untouched and o1.tolist() == so.tolist() and o2.tolist() == to.tolist()
    rc, _s, o1, _t, o2, _r, untouched = attempt(len(skb) - 1, len(tkb))
    assert rc == 1 and untouched and o1.tolist() == so.tolist() and o2.tolist() == to.tolist()
    rc, _s, o1, _t, o2, _r, untouched = attempt(0, len(tkb) - 1, with_sk=False)
    assert rc == 1 and untouched and o2.tolist() == to.tolist()
    # an empty list and an item_set out of range fail before any draw, at the C level too (the Python wrapper refuses them itself)
    rc, *_x, untouched = attempt(len(skb), len(tkb), sets=[["A"], []], items=[0, 0, 0])
    assert rc not in (0, 1) and untouched and b"empty attribute list" in host.lib.rabe_host_last_error(None)
    rc, *_x, untouched = attempt(len(skb), len(tkb), items=[0, len(SETS), 1])
    assert rc not in (0, 1) and untouched and b"item_set out of range" in host.lib.rabe_host_last_error(None)
    rc, sk_buf, o1, tk_buf, o2, rk2, _u = attempt(len(skb), len(tkb))
    host.clear_tape()
    assert rc == 0 and (sk_buf.tobytes(), o1.tolist(), tk_buf.tobytes(), o2.tolist(), rk2.tobytes()) == full
    # z = 0 fails the whole call as tkgen's inverse().unwrap() does, and leaves the buffers as they were
    for with_sk in (True, False):
        host.set_tape(tape[:n] + [tape[n], 0, tape[n + 2]])
        rc, *_x, untouched = attempt(len(skb) if with_sk else 0, len(tkb), with_sk=with_sk)
        host.clear_tape()
        assert rc not in (0, 1) and untouched and b"inverse of zero" in host.lib.rabe_host_last_error(None)
    host.set_tape(tape[:n] + [tape[n], 0, tape[n + 2]])
    with pytest.raises((hl.RabeError, hl.RabePanic), match="inverse of zero"):
        ghw11.provision_packed(host, pk, msk, SETS, item_set)
    host.clear_tape()
    with pytest.raises(ValueError, match="empty attribute list"):
        ghw11.provision_packed(host, pk, msk, [["A"], []], [0, 0])
    with pytest.raises(ValueError, match="item_set out of range"):
        ghw11.provision_packed(host, pk, msk, SETS, [0, len(SETS)])
    # n_items = 0 succeeds
    for want_sk in (True, False):
        b0, o0, t0, to0, rk0 = ghw11.provision_packed(host, pk, msk, SETS, [], want_sk=want_sk)
        assert len(t0) == 0 and to0.tolist() == [0] and len(rk0) == 0
        assert (b0 is None and o0 is None) if not want_sk else (len(b0) == 0 and o0.tolist() == [0])


def test_the_lazy_table_leaves_keygen_packed_alone():
    """a fresh host (its own key handle): keygen_packed before the first provision call, which adds the window table of g2_alpha to the
    handle, and after it -- the same bytes on one tape; and the provision call that built the table equals the two calls it is defined by"""
    h = hl.Host(0)
    try:
        pk, msk = ghw11.setup(h)
        rnd = random.Random(12)
        item_set = [3, 0, 1, 3, 2]
        n = len(item_set)
        tape = [rnd.randrange(1, R) for _ in range(2 * n)]
        h.set_tape(tape)
        before, off0 = ghw11.keygen_packed(h, pk, msk, SETS, item_set)
        before = bytes(before)
        h.set_tape(tape)
        skb, so, tkb, to, rk = ghw11.provision_packed(h, pk, msk, SETS, item_set)
        h.set_tape(tape)
        after, off1 = ghw11.keygen_packed(h, pk, msk, SETS, item_set)
        ref_tk, ref_to, ref_rk, st = ghw11.tkgen_packed(h, after, off1)
        h.clear_tape()
        assert bytes(after) == before == bytes(skb) and off0.tolist() == off1.tolist() == so.tolist()
        assert (st == 0).all() and bytes(tkb) == bytes(ref_tk) and to.tolist() == ref_to.tolist() and rk.tobytes() == ref_rk.tobytes()
    finally:
        h.close()


def test_device_group_runs_on_its_first_device_with_the_same_bytes(authority):
    """as keygen_packed: a group host runs the call on devices[0]"""
    pk, msk = authority
    rnd = random.Random(3)
    item_set = [rnd.randrange(len(SETS)) for _ in range(19)]
    tape = [rnd.randrange(1, R) for _ in range(2 * len(item_set))]
    got = []
    for devices in ([0], [0, 0]):
        h = hl.Host(0) if len(devices) == 1 else hl.Host(devices=devices)
        try:
            assert h.group_size() == len(devices)
            h.set_tape(tape)
            skb, so, tkb, to, rk = ghw11.provision_packed(h, pk, msk, SETS, item_set)
            h.clear_tape()
            got.append((bytes(skb), so.tolist(), bytes(tkb), to.tolist(), rk.tobytes()))
        finally:
            h.close()
    assert got[0] == got[1]
