"""GPU checks of GHW11's bulk key issuing (include/rabe_host.h: rabe_ghw11_keygen_packed, rabe_ghw11_tkgen_packed): the oracle's golden
vectors, byte equality with the object API on one tape, the chain keygen_packed -> tkgen_packed -> transform_packed -> decrypt_out_packed,
failures that stay with their item, capacities, a bulk call and a device group."""
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
LANG = {"json": hl.JSON_POLICY, "human": hl.HUMAN_POLICY}


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


SETS = [["solo"], ["A", "B", "C", "A"], ["a%d" % i for i in range(100)], ["B", "D"]]          # set 1 repeats a name


def object_keys(host, pk, msk, item_set, tape):
    host.set_tape(tape)
    sks = [ghw11.keygen(host, pk, msk, SETS[s]) for s in item_set]
    host.clear_tape()
    return sks


def object_tks(host, sks, tape):
    host.set_tape(tape)
    out = [ghw11.tkgen(host, sk) for sk in sks]
    host.clear_tape()
    return [(tk.serialize(), rk.serialize()) for tk, rk in out]


def test_golden(host):
    with open(os.path.join(HERE, "golden", "ghw11.json")) as f:
        doc = json.load(f)
    p = doc["pk"]
    pkb = hb(p["g1"]) + hb(p["g2"]) + hb(p["g1_a"]) + hb(p["g2_a"]) + hb(p["e_gg_alpha"])
    pk = hl.Obj.deserialize("ghw11_pk", pkb)
    msk = hl.Obj.deserialize("ghw11_msk", hb(doc["msk"]["g2_alpha"]) + pkb)
    for c in doc["cases"]:
        kt, tt = [fri(x) for x in c["keygen_tape"]], [fri(x) for x in c["tkgen_tape"]]
        host.set_tape(kt)
        blob, off = ghw11.keygen_packed(host, pk, msk, [c["attrs"]], [0])
        host.set_tape(kt)
        sk_obj = ghw11.keygen(host, pk, msk, c["attrs"])
        host.clear_tape()
        rec = bytes(blob)
        g = hl.parse_obj("ghw11_sk", rec)
        assert (g["k"], g["l"]) == (hb(c["sk"]["k"]), hb(c["sk"]["l"]))
        assert g["attr_key"] == [(n, hb(x)) for n, x in c["sk"]["attr_key"]]
        assert rec == sk_obj.serialize()
        host.set_tape(tt)
        tkb, to, rk, st = ghw11.tkgen_packed(host, rec, off)
        host.set_tape(tt)
        tk_obj, rk_obj = ghw11.tkgen(host, sk_obj)
        host.clear_tape()
        assert st.tolist() == [0]
        t = hl.parse_obj("ghw11_tk", bytes(tkb))
        assert (t["k_z"], t["l_z"]) == (hb(c["tk"]["k_z"]), hb(c["tk"]["l_z"]))
        assert t["attr_key_z"] == [(n, hb(x)) for n, x in c["tk"]["attr_key_z"]]
        assert rk[0].tobytes() == hb(c["tkgen_tape"][0])
        assert bytes(tkb) == tk_obj.serialize() and rk[0].tobytes() == rk_obj.serialize()


def test_mixed_shapes_equal_the_object_api_on_one_tape(host, authority):
    pk, msk = authority
    rnd = random.Random(77)
    item_set = [i % 3 for i in range(24)] + [3, 1, 2]
    rnd.shuffle(item_set)
    n = len(item_set)
    ktape = [rnd.randrange(1, R) for _ in range(n)]
    ztape = [rnd.randrange(1, R) for _ in range(n)]
    host.set_tape(ktape)
    blob, off = ghw11.keygen_packed(host, pk, msk, SETS, item_set)
    host.clear_tape()
    sks = object_keys(host, pk, msk, item_set, ktape)
    recs = records(blob, off)
    assert recs == [sk.serialize() for sk in sks]
    for r_ in recs:
        assert hl.Obj.deserialize("ghw11_sk", r_, host=host).serialize() == r_
    for trusted in (False, True):
        host.set_tape(ztape)
        tkb, to, rk, st = ghw11.tkgen_packed(host, blob, off, trusted=trusted)
        host.clear_tape()
        assert (st == 0).all()
        ref = object_tks(host, sks, ztape)
        tks = records(tkb, to)
        assert tks == [t for t, _ in ref]
        assert [rk[i].tobytes() for i in range(n)] == [z for _, z in ref]
    for t_ in tks:
        assert hl.Obj.deserialize("ghw11_tk", t_, host=host).serialize() == t_
    for i in range(n):
        assert hl.Obj.deserialize("ghw11_rk", rk[i].tobytes()).serialize() == rk[i].tobytes()


def test_chain_through_the_service(host, authority):
    pk, msk = authority
    item_set = [1, 3, 1, 2, 3, 1]                  # users 1 and 4 hold {B, D}: no "A"
    blob, off = ghw11.keygen_packed(host, pk, msk, SETS, item_set)
    tkb, to, rk, st = ghw11.tkgen_packed(host, blob, off)
    assert (st == 0).all()
    tks = records(tkb, to)
    pols = ['{"name": "and", "children": [{"name": "A"}, {"name": "B"}]}', '{"name": "or", "children": [{"name": "B"}, {"name": "a7"}]}']
    item_pol = [0, 1, 0, 1]
    pts = [b"chain item %d " % i * (i + 1) for i in range(4)]
    cblob, coff = ghw11.encrypt_packed(host, pk, pols, item_pol, b"".join(pts), offsets(pts))
    for u in (0, 1, 2, 3, 4):
        tk = hl.Obj.deserialize("ghw11_tk", tks[u], host=host)
        rko = hl.Obj.deserialize("ghw11_rk", rk[u].tobytes())
        tct, tst = ghw11.transform_packed(host, tk, cblob, coff)
        has_a = "A" in SETS[item_set[u]]
        has_b_or_a7 = "B" in SETS[item_set[u]] or "a7" in SETS[item_set[u]]
        want = [0 if (has_a and "B" in SETS[item_set[u]]) else -1, 0 if has_b_or_a7 else -1] * 2
        assert tst.tolist() == want, u
        pt, po, pst = ghw11.decrypt_out_packed(host, rko, tct, cblob, coff)
        for i in range(4):
            if want[i] == 0:
                assert pst[i] == 0 and bytes(pt[int(po[i]):int(po[i + 1])]) == pts[i]
            else:
                assert pst[i] == -1


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


def test_failures_stay_with_their_item(host, authority):
    pk, msk = authority
    rnd = random.Random(8)
    item_set = [1, 3, 0, 1, 3, 1, 0, 3]
    n = len(item_set)
    ktape = [rnd.randrange(1, R) for _ in range(n)]
    sks = object_keys(host, pk, msk, item_set, ktape)
    recs = [sk.serialize() for sk in sks]
    bad = list(recs)
    bad[1] = bad[1][:-9]                                                           # truncated: fails on the host, draws nothing
    bad[3] = bad[3][:32] + (bn.P + 5).to_bytes(32, "little") + bad[3][64:]         # a coordinate >= p: decodes, fails the membership pass
    q = bn.g2_to_le(twist_point_outside_g2())
    bad[5] = bad[5][:128] + q + bad[5][256:]                                       # l on the twist, outside the r-torsion
    blob = np.frombuffer(b"".join(bad), dtype=np.uint8)
    off = offsets(bad)
    off2 = off.copy()
    off2[7] = off[6] - 1                                                           # item 6: offsets not monotone
    off2[8] = off[8] + 5                                                           # item 7: past the end of the blob
    ztape = [rnd.randrange(1, R) for _ in range(n)]
    # items that decode on the host draw: all but 1 (and 6, 7 with the broken offsets)
    for offs, host_bad in ((off, {1}), (off2, {1, 6, 7})):
        host.set_tape(ztape)
        tkb, to, rk, st = ghw11.tkgen_packed(host, blob, offs)
        host.clear_tape()
        fails = host_bad | {3, 5}
        assert [i for i in range(n) if st[i] != 0] == sorted(fails)
        drawing = [i for i in range(n) if i not in host_bad]
        ref = {}
        for d, i in enumerate(drawing):                                           # one z per item that decodes on the host, in item order
            if i in fails:
                continue                                                          # a non-member's z is spent
            host.set_tape([ztape[d]])
            tk, rko = ghw11.tkgen(host, sks[i])
            host.clear_tape()
            ref[i] = (tk.serialize(), rko.serialize())
        tks = records(tkb, to)
        for i in range(n):
            if i in fails:
                assert tks[i] == b"" and not rk[i].any()
            else:
                assert (tks[i], rk[i].tobytes()) == ref[i], i
    # trusted: the membership pass is skipped, the non-members are not rejected (their transform keys are unspecified)
    host.set_tape(ztape)
    _tkb, _to, _rk, st = ghw11.tkgen_packed(host, blob, off, trusted=True)
    host.clear_tape()
    assert [i for i in range(n) if st[i] != 0] == [1]


def test_capacity_and_call_level_errors(host, authority):
    pk, msk = authority
    lib = host.lib
    rnd = random.Random(4)
    item_set = [1, 0, 3]
    n = len(item_set)
    tape = [rnd.randrange(1, R) for _ in range(2 * n)]
    host.set_tape(tape)
    full, so = ghw11.keygen_packed(host, pk, msk, SETS, item_set)
    host.clear_tape()
    # sk_cap one byte short: 1, offsets filled, nothing drawn (the next call on the same tape gives the same bytes)
    arr, _ = hl._strs([a for s_ in SETS for a in s_])
    counts = (ctypes.c_size_t * len(SETS))(*[len(s_) for s_ in SETS])
    it = np.array(item_set, dtype=np.uint32)
    o2 = np.zeros(n + 1, dtype=np.uint64)
    small = np.zeros(len(full) - 1, dtype=np.uint8)
    host.set_tape(tape)
    rc = lib.rabe_ghw11_keygen_packed(host.h, pk.ptr, msk.ptr, arr, counts, ctypes.c_size_t(len(SETS)), ctypes.c_size_t(n), hl._np_ptr(it),
                                      hl._np_ptr(small), ctypes.c_size_t(small.size), hl._np_ptr(o2))
    assert rc == 1 and o2.tolist() == so.tolist() and not small.any()
    again, _ = ghw11.keygen_packed(host, pk, msk, SETS, item_set)
    host.clear_tape()
    assert bytes(again) == bytes(full)
    # tk_cap one byte short
    ztape = tape[n:]
    host.set_tape(ztape)
    tkb, to, rk, st = ghw11.tkgen_packed(host, full, so)
    sk = np.ascontiguousarray(full)
    to2 = np.zeros(n + 1, dtype=np.uint64)
    rk2 = np.zeros((n, 32), dtype=np.uint8)
    st2 = np.zeros(n, dtype=np.int32)
    small = np.zeros(len(tkb) - 1, dtype=np.uint8)
    host.set_tape(ztape)
    rc = lib.rabe_ghw11_tkgen_packed(host.h, ctypes.c_size_t(n), hl._np_ptr(sk), ctypes.c_size_t(sk.size), hl._np_ptr(so), ctypes.c_uint32(0),
                                     hl._np_ptr(st2), hl._np_ptr(small), ctypes.c_size_t(small.size), hl._np_ptr(to2), hl._np_ptr(rk2))
    assert rc == 1 and int(to2[n]) == len(tkb) and not small.any() and not rk2.any()
    tkb2, _to, rk3, _st = ghw11.tkgen_packed(host, full, so)
    host.clear_tape()
    assert bytes(tkb2) == bytes(tkb) and rk3.tobytes() == rk.tobytes()
    # call-level failures: a message, nothing written
    with pytest.raises(hl.RabeError, match="empty attribute list"):
        ghw11.keygen_packed(host, pk, msk, [["A"], []], [0, 0])
    with pytest.raises(hl.RabeError, match="item_set out of range"):
        ghw11.keygen_packed(host, pk, msk, SETS, [0, len(SETS)])
    host.set_tape([5, 0, 7])
    with pytest.raises((hl.RabeError, hl.RabePanic), match="inverse of zero"):
        ghw11.tkgen_packed(host, full, so)
    host.clear_tape()
    # n_items = 0 succeeds
    b0, o0 = ghw11.keygen_packed(host, pk, msk, SETS, [])
    assert len(b0) == 0 and o0.tolist() == [0]
    t0, to0, rk0, st0 = ghw11.tkgen_packed(host, b"", [0])
    assert len(t0) == 0 and to0.tolist() == [0] and len(rk0) == 0 and len(st0) == 0


def test_bulk_8192_keys_of_50_attributes(host, authority):
    pk, msk = authority
    n = 8192
    attrs = ["a%d" % i for i in range(50)]
    rnd = random.Random(99)
    ktape = [rnd.randrange(1, R) for _ in range(n)]
    ztape = [rnd.randrange(1, R) for _ in range(n)]
    host.set_tape(ktape)
    blob, off = ghw11.keygen_packed(host, pk, msk, [attrs], [0] * n)
    host.set_tape(ztape)
    tkb, to, rk, st = ghw11.tkgen_packed(host, blob, off)
    host.clear_tape()
    assert (st == 0).all() and len(off) == n + 1
    for i in [0, n - 1] + rnd.sample(range(1, n - 1), 16):
        host.set_tape([ktape[i], ztape[i]])                    # one draw per item and call: item i's position in each tape is i
        sk = ghw11.keygen(host, pk, msk, attrs)
        tk, rko = ghw11.tkgen(host, sk)
        host.clear_tape()
        assert bytes(blob[int(off[i]):int(off[i + 1])]) == sk.serialize(), i
        assert bytes(tkb[int(to[i]):int(to[i + 1])]) == tk.serialize(), i
        assert rk[i].tobytes() == rko.serialize(), i


def test_device_group_runs_on_its_first_device_with_the_same_bytes(authority):
    """like the other keygen_packed functions that are not sharded (bsw, ac17): a group host runs the call on devices[0]"""
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
            blob, off = ghw11.keygen_packed(h, pk, msk, SETS, item_set)
            tkb, to, rk, st = ghw11.tkgen_packed(h, blob, off)
            h.clear_tape()
            got.append((bytes(blob), off.tolist(), bytes(tkb), to.tolist(), rk.tobytes(), st.tolist()))
        finally:
            h.close()
    assert got[0] == got[1]
