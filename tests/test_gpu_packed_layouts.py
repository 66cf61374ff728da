"""Record layouts other than the one the packed encrypt / keygen writes, through bsw::decrypt_packed, lsw::decrypt_packed,
aw11::decrypt_packed and ghw11::transform_packed: rows in another order, a duplicated row name after or before the originals, a renamed
row.  Such records leave the shared selection of their policy and go through the name lookups of the reference's decrypt (the FIRST row
of a name counts); what comes out per item is what the object API gives for the same bytes.  In checked mode the G2 elements of such a
record get their subgroup verdict from the decrypt's own walks where the selection names their row, and from the stand-alone test where
it does not: an element outside G2 fails its item in either place."""
import numpy as np
import pytest

from oracle import bn254 as bn
from rabe_amd import hostlib as hl
from rabe_amd.schemes import aw11, bsw, ghw11, lsw

pytestmark = pytest.mark.gpu

ITEM_POL = [0, 1, 0, 1, 1, 0]


def js(name, *children):
    return '{"name": "%s", "children": [%s]}' % (name, ", ".join(children)) if children else '{"name": "%s"}' % name


# policy 0 selects every row; of policy 1 a key (ciphertext, for lsw) that holds A alone selects row 0 and leaves rows 1 and 2 out
HUMAN_POLS = ['"A" and "B" and "C"', '"A" or ("B" and "D")']
JSON_POLS = [js("and", js("A"), js("B"), js("C")), js("or", js("A"), js("and", js("B"), js("D")))]
AW11_POLS = [js("and", js("A"), js("and", js("B"), js("C"))), JSON_POLS[1]]          # aw11's MSP takes two children under an AND


def offsets(items):
    return np.concatenate([[0], np.cumsum([len(p) for p in items])]).astype(np.uint64)


def split(blob, off):
    b = np.asarray(blob).tobytes()
    return [b[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def last_error(host):
    return (host.lib.rabe_host_last_error(host.h) or b"").decode()


def twist_point_outside_g2():
    from tests.test_gpu_ghw11_keys_packed import twist_point_outside_g2 as helper
    return bn.g2_to_le(helper())


class Codec:
    """policy text | language | `head` bytes | u32 rows | (name, `elem` bytes)* | tail (u32 length + sealed data, or nothing)"""

    def __init__(self, head, elem, walked_at=None):
        self.head, self.elem, self.walked_at = head, elem, walked_at

    def parse(self, rec):
        at = 4 + int.from_bytes(rec[:4], "little") + 1 + self.head
        n = int.from_bytes(rec[at:at + 4], "little")
        prefix, at, rows = rec[:at], at + 4, []
        for _ in range(n):
            ln = int.from_bytes(rec[at:at + 4], "little")
            rows.append((rec[at + 4:at + 4 + ln], rec[at + 4 + ln:at + 4 + ln + self.elem]))
            at += 4 + ln + self.elem
        return prefix, rows, rec[at:]

    @staticmethod
    def build(prefix, rows, tail):
        return prefix + len(rows).to_bytes(4, "little") + b"".join(len(nm).to_bytes(4, "little") + nm + el for nm, el in rows) + tail

    def with_walked(self, row, point):
        """the row with its element of the walked array (bsw: the leaf's g2, lsw: d2, aw11: c2) replaced"""
        nm, el = row
        return nm, el[:self.walked_at] + point + el[self.walked_at + 128:]


BSW = Codec(64 + 384, 64 + 128, walked_at=64)
LSW = Codec(0, 64 + 128 + 192, walked_at=64)
AW11 = Codec(384, 384 + 128 + 128, walked_at=384)
GHW11 = Codec(384 + 64, 64 + 64)


def odd_layouts(codec, recs, renamed=False):
    """recs: the records of ITEM_POL.  Two untouched ones, then record 0 (policy 0: three rows, all selected) in other layouts"""
    prefix, rows, tail = codec.parse(recs[0])
    other = codec.parse(recs[2])[1]                                           # the same policy, other elements
    assert len(rows) == 3 and [nm for nm, _ in other] == [nm for nm, _ in rows]
    batch = [recs[0], recs[1],
             codec.build(prefix, [rows[2], rows[0], rows[1]], tail),              # another order
             codec.build(prefix, rows + [(rows[0][0], other[0][1])], tail),       # a second row of a name: the first one counts
             codec.build(prefix, [(rows[1][0], other[1][1])] + rows, tail)]       # ... and here the first one holds the wrong elements
    if renamed:
        batch.append(codec.build(prefix, [(b"ZZ", rows[0][1])] + rows[1:], tail))  # bsw: no row of the entry's name -> the entry is skipped
    return batch + [recs[3], recs[5]]


def check_decrypt(host, batch, packed, single):
    """packed(blob, off, trusted) -> (out, out_off, status); single(rec) -> the object API's plaintext, or raises"""
    res = [packed(b"".join(batch), offsets(batch), trusted) for trusted in (False, True)]
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(*res))
    out, oo, st = res[0]
    got = split(out, oo)
    for i, rec in enumerate(batch):
        try:
            want = single(rec)
        except (hl.RabeError, hl.RabePanic):
            want = None
        if want is None:
            assert st[i] == -1 and not any(got[i]), i
        else:
            assert st[i] == 0 and got[i] == want, i
    return [int(s) for s in st]


def check_walked_array(host, codec, recs, packed, want):
    """recs: three records of policy 1 for a key that selects row 0 alone.  The middle one, its rows reversed, with a twist point outside
    G2 in an unselected row (the stand-alone test has to see it), then in the selected row (the walk's verdict has to)."""
    prefix, rows, tail = codec.parse(recs[1])
    assert len(rows) == 3
    point = twist_point_outside_g2()
    for bad_row in (1, 0):
        damaged = [codec.with_walked(r, point) if y == bad_row else r for y, r in enumerate(rows)]
        batch = [recs[0], codec.build(prefix, damaged[::-1], tail), recs[2]]
        out, oo, st = packed(b"".join(batch), offsets(batch), False)
        got = split(out, oo)
        assert [int(s) for s in st] == [0, -1, 0], (bad_row, list(st))
        assert not any(got[1]) and got[0] == want[0] and got[2] == want[2], bad_row
        assert "not a group member" in last_error(host), (bad_row, last_error(host))
    # the reversed record itself is sound
    batch = [recs[0], codec.build(prefix, rows[::-1], tail), recs[2]]
    out, oo, st = packed(b"".join(batch), offsets(batch), False)
    assert not st.any() and split(out, oo) == want


@pytest.fixture(scope="module")
def host():
    h = hl.Host(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def pts():
    return [b"layouts, item %d " % i * (i % 3 + 1) for i in range(len(ITEM_POL))]


@pytest.fixture(scope="module")
def bsw_world(host, pts):
    pk, msk = bsw.setup(host)
    blob, off = bsw.encrypt_packed(host, pk, HUMAN_POLS, ITEM_POL, b"".join(pts), offsets(pts), hl.HUMAN_POLICY)
    return pk, msk, split(blob, off)


def test_bsw_layouts_equal_the_object_api(host, bsw_world, pts):
    pk, msk, recs = bsw_world
    sk = bsw.keygen(host, pk, msk, ["A", "B", "C", "D"])
    st = check_decrypt(host, odd_layouts(BSW, recs, renamed=True), lambda b, o, t: bsw.decrypt_packed(host, sk, b, o, trusted=t),
                       lambda rec: bsw.decrypt(host, sk, hl.Obj.deserialize("bsw_ct", rec)))
    assert st == [0, 0, 0, 0, -1, -1, 0, 0]


def test_bsw_walked_array_of_a_reordered_record(host, bsw_world, pts):
    pk, msk, recs = bsw_world
    sk = bsw.keygen(host, pk, msk, ["A"])
    check_walked_array(host, BSW, [recs[1], recs[3], recs[4]], lambda b, o, t: bsw.decrypt_packed(host, sk, b, o, trusted=t), [pts[1], pts[3], pts[4]])


@pytest.fixture(scope="module")
def lsw_world(host):
    pk, msk = lsw.setup(host)
    blob, off = lsw.keygen_packed(host, pk, msk, JSON_POLS, ITEM_POL, hl.JSON_POLICY)
    return pk, msk, split(blob, off)


def test_lsw_layouts_equal_the_object_api(host, lsw_world):
    pk, msk, recs = lsw_world
    pt = b"one ciphertext, keys in odd layouts"
    ct = lsw.encrypt(host, pk, ["A", "B", "C", "D"], pt)
    st = check_decrypt(host, odd_layouts(LSW, recs), lambda b, o, t: lsw.decrypt_packed(host, ct, b, o, trusted=t),
                       lambda rec: lsw.decrypt(host, hl.Obj.deserialize("lsw_sk", rec), ct))
    assert st == [0, 0, 0, 0, -1, 0, 0]


def test_lsw_walked_array_of_a_reordered_key(host, lsw_world):
    pk, msk, recs = lsw_world
    pt = b"attribute A alone"
    ct = lsw.encrypt(host, pk, ["A"], pt)
    check_walked_array(host, LSW, [recs[1], recs[3], recs[4]], lambda b, o, t: lsw.decrypt_packed(host, ct, b, o, trusted=t), [pt, pt, pt])


def test_lsw_key_policy_that_names_an_attribute_twice(host, lsw_world):
    """`A and A`: both selection entries resolve to the first row named A, so the second row is walked by no pairing.  An element outside
    G2 there fails the item and leaves its neighbours alone.  (Which error the item reports is not asserted: the same share counted twice
    fails the tag as well.)"""
    pk, msk, _ = lsw_world
    pols = [js("and", js("A"), js("A")), js("or", js("A"), js("B"))]
    blob, off = lsw.keygen_packed(host, pk, msk, pols, [1, 0, 1], hl.JSON_POLICY)
    recs = split(blob, off)
    prefix, rows, tail = LSW.parse(recs[1])
    assert [nm for nm, _ in rows] == [b"A", b"A"]
    recs[1] = LSW.build(prefix, [rows[0], LSW.with_walked(rows[1], twist_point_outside_g2())], tail)
    pt = b"repeated attribute"
    ct = lsw.encrypt(host, pk, ["A"], pt)
    out, oo, st = lsw.decrypt_packed(host, ct, b"".join(recs), offsets(recs))
    got = split(out, oo)
    print("lsw `A and A`, second row's d2 outside G2: status", list(st), "last error:", last_error(host))
    assert [int(s) for s in st] == [0, -1, 0] and got[0] == pt and got[2] == pt and not any(got[1])


@pytest.fixture(scope="module")
def aw11_world(host, pts):
    gk = aw11.setup(host)
    pk, msk = aw11.authgen(host, gk, ["A", "B", "C", "D"])
    blob, off = aw11.encrypt_packed(host, gk, [pk], AW11_POLS, ITEM_POL, b"".join(pts), offsets(pts), hl.JSON_POLICY)
    return gk, msk, split(blob, off)


def test_aw11_layouts_equal_the_object_api(host, aw11_world, pts):
    gk, msk, recs = aw11_world
    sk = aw11.keygen(host, gk, msk, "alice", ["A", "B", "C", "D"])
    st = check_decrypt(host, odd_layouts(AW11, recs), lambda b, o, t: aw11.decrypt_packed(host, gk, sk, b, o, trusted=t),
                       lambda rec: aw11.decrypt(host, gk, sk, hl.Obj.deserialize("aw11_ct", rec)))
    assert st == [0, 0, 0, 0, -1, 0, 0]


def test_aw11_walked_array_of_a_reordered_record(host, aw11_world, pts):
    gk, msk, recs = aw11_world
    sk = aw11.keygen(host, gk, msk, "bob", ["A"])
    check_walked_array(host, AW11, [recs[1], recs[3], recs[4]], lambda b, o, t: aw11.decrypt_packed(host, gk, sk, b, o, trusted=t),
                       [pts[1], pts[3], pts[4]])


def test_ghw11_transform_layouts_equal_the_object_api(host, pts):
    pk, msk = ghw11.setup(host)
    recs = [ghw11.encrypt(host, pk, HUMAN_POLS[p], hl.HUMAN_POLICY, pts[i]).serialize() for i, p in enumerate(ITEM_POL)]
    tk, _ = ghw11.tkgen(host, ghw11.keygen(host, pk, msk, ["A", "B", "C", "D"]))
    batch = odd_layouts(GHW11, recs)
    res = [ghw11.transform_packed(host, tk, b"".join(batch), offsets(batch), trusted=t) for t in (False, True)]
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    out, st = res[0]
    for i, rec in enumerate(batch):
        try:
            want = ghw11.transform(host, hl.Obj.deserialize("ghw11_ct", rec), tk).serialize()
        except (hl.RabeError, hl.RabePanic):
            want = None
        if want is None:
            assert st[i] == -1 and not out[i].any(), i
        else:
            assert st[i] == 0 and out[i].tobytes() == want, i
    assert [int(s) for s in st] == [0] * len(batch)
    # the first row of the duplicated name holds another record's elements: another t than the untouched record's
    assert out[3].tobytes() == out[0].tobytes() and out[4].tobytes() != out[0].tobytes()
