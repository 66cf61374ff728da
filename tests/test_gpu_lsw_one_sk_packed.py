"""rabe_lsw_decrypt_one_sk_packed: ONE key against a blob of KpAbeCiphertext records (what rabe_lsw_encrypt_packed writes).  Every
plaintext equals lsw::decrypt of the same record through the object API; every failure -- attributes that do not satisfy the key, a
malformed record, an element outside its group, a tag that does not verify -- stays with its item."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import bn254 as bn
from rabe_amd import hostlib as hl
from rabe_amd.schemes import lsw

pytestmark = pytest.mark.gpu

POLICY = '{"name": "or", "children": [{"name": "and", "children": [{"name": "A"}, {"name": "B"}, {"name": "C"}]}, ' \
         '{"name": "and", "children": [{"name": "D"}, {"name": "E"}]}]}'
NO_MATCH = "Error in lsw/decrypt: attributes do not match policy."
SETS = [["C", "A", "B", "X"], ["A", "D"], ["E", "Y", "D"]]             # list 1 does not satisfy the key


def offsets(items):
    return np.concatenate([[0], np.cumsum([len(p) for p in items])]).astype(np.uint64)


def split(blob, off):
    b = np.asarray(blob).tobytes()
    return [b[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def last_error(host):
    return (host.lib.rabe_host_last_error(host.h) or b"").decode()


def object_decrypt(host, sk, rec):
    """lsw::decrypt of one record through the object API: the plaintext, or the error text"""
    try:
        return lsw.decrypt(host, sk, hl.Obj.deserialize("lsw_ct", rec))
    except (hl.RabeError, hl.RabePanic) as ex:
        return "error: " + str(ex)


def row_at(rec, row):
    """offset of row `row`'s first element (E1) in a KpAbeCiphertext record: e1 | e2 | u32 rows | (name, e1, e2, e3)*"""
    at = 384 + 128
    rows = int.from_bytes(rec[at:at + 4], "little")
    assert row < rows
    at += 4
    for _ in range(row):
        at += 4 + int.from_bytes(rec[at:at + 4], "little") + 192
    return at + 4 + int.from_bytes(rec[at:at + 4], "little")


def record(rows, e1, e2, sealed):
    out = e1 + e2 + len(rows).to_bytes(4, "little")
    for name, elems in rows:
        out += len(name).to_bytes(4, "little") + name.encode() + elems
    return out + len(sealed).to_bytes(4, "little") + sealed


def parse(rec):
    at = 384 + 128
    rows = []
    n = int.from_bytes(rec[at:at + 4], "little")
    at += 4
    for _ in range(n):
        ln = int.from_bytes(rec[at:at + 4], "little")
        rows.append((rec[at + 4:at + 4 + ln].decode(), rec[at + 4 + ln:at + 4 + ln + 192]))
        at += 4 + ln + 192
    ln = int.from_bytes(rec[at:at + 4], "little")
    return rows, rec[:384], rec[384:512], rec[at + 4:at + 4 + ln]


@pytest.fixture(scope="module")
def host():
    h = hl.Host(0)
    yield h
    h.close()


def make_world(host):
    """the key and 70 ciphertexts over three attribute lists, written by the packed encrypt"""
    pk, msk = lsw.setup(host)
    sk = lsw.keygen(host, pk, msk, POLICY, hl.JSON_POLICY)
    n = 70
    item_set = [i % 3 for i in range(n)]
    pts = [b"lsw one key, item %d " % i * (i % 3 + 1) for i in range(n)]
    blob, off = lsw.encrypt_packed(host, pk, SETS, item_set, b"".join(pts), offsets(pts))
    return pk, msk, sk, item_set, pts, np.array(blob, copy=True), np.array(off, copy=True)


@pytest.fixture(scope="module")
def world(host):
    """computed once, shared by the tests, never modified"""
    return make_world(host)


def test_round_trip_equals_the_object_api(host, world):
    pk, msk, sk, item_set, pts, blob, off = world
    n = len(pts)
    recs = split(blob, off)
    out, oo, st = lsw.decrypt_one_sk_packed(host, sk, blob, off)
    got = split(out, oo)
    assert last_error(host) == NO_MATCH
    for i in range(n):
        want = object_decrypt(host, sk, recs[i])
        if item_set[i] == 1:
            assert want == "error: " + NO_MATCH and st[i] == -1 and got[i] == b"", i
        else:
            assert want == pts[i] and st[i] == 0 and got[i] == pts[i], i
    t_out, t_oo, t_st = lsw.decrypt_one_sk_packed(host, sk, blob, off, trusted=True)
    assert np.array_equal(t_out, out) and np.array_equal(t_oo, oo) and np.array_equal(t_st, st)


def test_odd_record_layouts_keep_first_row_semantics(host, world):
    pk, msk, sk, item_set, pts, blob, off = world
    recs = split(blob, off)
    rows, e1, e2, sealed = parse(recs[0])                                    # C, A, B, X
    reordered = record([rows[3], rows[2], rows[0], rows[1]], e1, e2, sealed)
    # a duplicated name whose FIRST row holds another ciphertext's elements: the lookups of lsw::decrypt take that row, the tag fails
    other = parse(recs[3])[0]
    dup_ok = record(rows + [("A", other[1][1])], e1, e2, sealed)
    dup_bad = record([("A", other[1][1])] + rows, e1, e2, sealed)
    batch = [recs[0], reordered, dup_ok, dup_bad, recs[2]]
    out, oo, st = lsw.decrypt_one_sk_packed(host, sk, b"".join(batch), offsets(batch))
    got = split(out, oo)
    for i, rec in enumerate(batch):
        want = object_decrypt(host, sk, rec)
        if isinstance(want, bytes):
            assert st[i] == 0 and got[i] == want, i
        else:
            assert st[i] == -1 and not any(got[i]), i
    assert [int(s) for s in st] == [0, 0, 0, -1, 0]


def twist_point_outside_g2():
    from tests.test_gpu_ghw11_keys_packed import twist_point_outside_g2 as helper
    return bn.g2_to_le(helper())


def untrusted_cases(host, world):
    """each damaged record fails its own item and nothing else"""
    pk, msk, sk, item_set, pts, blob, off = world
    good = [i for i in range(12) if item_set[i] != 1]
    recs = [split(blob, off)[i] for i in good]
    want = [pts[i] for i in good]
    n = len(recs)

    def expect(batch, off_, victim, needle):
        out, oo, st = lsw.decrypt_one_sk_packed(host, sk, b"".join(batch), off_)
        got = split(out, oo)
        assert [int(s) for s in st] == [-1 if i == victim else 0 for i in range(n)], (needle, list(st))
        # no plaintext byte of the failed item comes out: its slot is empty, or zeroed where the verdict came after the open
        assert not any(got[victim]) and all(got[i] == want[i] for i in range(n) if i != victim), needle
        assert needle in last_error(host), (needle, last_error(host))

    def replaced(victim, rec):
        return recs[:victim] + [rec] + recs[victim + 1:]

    # a truncated record (its neighbours keep their offsets: the blob is simply shorter there)
    cut = replaced(2, recs[2][:-40 - len(want[2])])
    expect(cut, offsets(cut), 2, "truncated")
    # overlapping offsets: item 3 ends before it starts
    o = offsets(recs)
    o[4] = o[3] - 8
    out, oo, st = lsw.decrypt_one_sk_packed(host, sk, b"".join(recs), o)
    assert st[3] == -1 and "offsets" in last_error(host)
    assert all(st[i] == 0 and split(out, oo)[i] == want[i] for i in range(n) if i not in (3, 4))
    # a flipped tag byte
    r = bytearray(recs[1])
    r[-1] ^= 1
    expect(replaced(1, bytes(r)), offsets(recs), 1, "aead")
    # a selected E1 row off the curve
    r = bytearray(recs[4])
    r[row_at(r, 1) + 33] ^= 1
    expect(replaced(4, bytes(r)), offsets(recs), 4, "not a point of G1")
    # e2 on the twist, outside the r-torsion: only a subgroup test -- the item's own walk, or the stand-alone one -- can see it
    r = bytearray(recs[5])
    r[384:512] = twist_point_outside_g2()
    expect(replaced(5, bytes(r)), offsets(recs), 5, "not a member of G2")
    # e1 outside the order-r subgroup (an arbitrary Fq12 element)
    r = bytearray(recs[0])
    r[:384] = b"".join((i + 2).to_bytes(32, "little") for i in range(12))
    expect(replaced(0, bytes(r)), offsets(recs), 0, "not a member of Gt")


def test_untrusted_input_fails_its_item_only(host, world):
    untrusted_cases(host, world)


CHILD = """
import sys
sys.path.insert(0, %r)
import tests.test_gpu_lsw_one_sk_packed as T
from rabe_amd import hostlib as hl
h = hl.Host(0)
T.untrusted_cases(h, T.make_world(h))
h.close()
print("untrusted cases ok")
"""


def test_untrusted_input_without_walk_checks():
    """the same outcomes with e2's verdict from the stand-alone test (RABE_NO_WALK_CHECKS is read once per process: a child)"""
    env = dict(os.environ, RABE_NO_WALK_CHECKS="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pr = subprocess.run([sys.executable, "-c", CHILD % root], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert pr.returncode == 0 and b"untrusted cases ok" in pr.stdout, pr.stdout.decode()[-3000:]


def raw_call(host, sk, blob, off, cap):
    n = len(off) - 1
    ct = np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, bytes) else np.ascontiguousarray(blob)
    co = np.ascontiguousarray(off, dtype=np.uint64)
    po = np.zeros(n + 1, dtype=np.uint64)
    st = np.zeros(max(n, 1), dtype=np.int32)
    buf = np.zeros(max(cap, 1), dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = host.lib.rabe_lsw_decrypt_one_sk_packed(host.h, sk.ptr, ctypes.c_size_t(n), p(ct), ctypes.c_size_t(ct.size), p(co), ctypes.c_uint32(0), p(st), p(buf),
                                                 ctypes.c_size_t(cap), p(po))
    return rc, po, st[:n], buf


def test_capacity_and_edge_sizes(host, world):
    pk, msk, sk, item_set, pts, blob, off = world
    recs = split(blob, off)[:7]
    need = sum(len(parse(r)[3]) for r in recs)                               # the sealed lengths: plaintext + nonce + tag
    b, o = b"".join(recs), offsets(recs)
    rc, po, st, buf = raw_call(host, sk, b, o, need - 1)
    assert rc == 1 and int(po[len(recs)]) == need
    rc, po, st, buf = raw_call(host, sk, b, o, need)
    assert rc == 0 and [int(s) for s in st] == [-1 if item_set[i] == 1 else 0 for i in range(7)]
    assert buf[:int(po[7])].tobytes() == b"".join(pts[i] for i in range(7) if item_set[i] != 1)
    out, oo, st = lsw.decrypt_one_sk_packed(host, sk, b"", np.zeros(1, dtype=np.uint64))
    assert len(out) == 0 and list(oo) == [0] and len(st) == 0
    out, oo, st = lsw.decrypt_one_sk_packed(host, sk, recs[0], offsets(recs[:1]))
    assert list(st) == [0] and np.asarray(out).tobytes() == pts[0]


def test_key_with_a_negative_leaf(host, world):
    pk, msk = world[0], world[1]
    pol = '{"name": "or", "children": [{"name": "and", "children": [{"name": "A"}, {"name": "B"}]}, {"name": "!N"}]}'
    sk = lsw.keygen(host, pk, msk, pol, hl.JSON_POLICY)
    pts = [b"positive rows select", b"the negative leaf selects", b"positive again"]
    sets = [["A", "B"], ["!N", "A"]]
    blob, off = lsw.encrypt_packed(host, pk, sets, [0, 1, 0], b"".join(pts), offsets(pts))
    out, oo, st = lsw.decrypt_one_sk_packed(host, sk, blob, off)
    assert [int(s) for s in st] == [0, -1, 0] and split(out, oo) == [pts[0], b"", pts[2]]
    assert "a negative attribute is selected" in last_error(host)


def test_device_group_equals_single_engine(host, world):
    pk, msk, sk, item_set, pts, blob, off = world
    ref = lsw.decrypt_one_sk_packed(host, sk, blob, off)
    group = hl.Host(devices=[0, 0])
    try:
        assert group.group_size() == 2
        got = lsw.decrypt_one_sk_packed(group, sk, blob, off)
        assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(ref, got))
        got = lsw.decrypt_one_sk_packed(group, sk, blob, off, trusted=True)
        assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(ref, got))
    finally:
        group.close()
