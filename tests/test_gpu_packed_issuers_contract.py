"""What the packed issuers (rabe_*_{encrypt,encaps,keygen,delegate,provision,request_*_sk}_packed) promise around their share trees and their output
sizing, frozen per entry point:
(a) one call over three policies used out of order -- a lone leaf (no gate, no coefficient draw) between policies that draw one and two -- gives
    the object API's bytes on the same tape (bsw encrypt and encaps, ghw11 encrypt, aw11 encrypt, lsw keygen without and with a negated leaf).
    The policy language has AND and OR gates only (binary ANDs where a scheme also builds the MSP), so the widest tree is two nested ANDs
    (a coefficient each) over an OR: three gates whose coefficient offsets follow the lone leaf's none;
(b) a capacity one byte short returns 1 with the size in off[n], writes nothing and draws nothing; the exact size succeeds;
(c) an index out of range fails the call with that entry point's message before anything is drawn or written;
(d) n = 0 with a null output buffer: the return code and off[0] of each entry point as they are -- they differ, on purpose."""
import ctypes

import numpy as np
import pytest

from rabe_amd import hostlib as hl
from rabe_amd.schemes import ac17, aw11, bdabe, bsw, ghw11, lsw, mke08

pytestmark = pytest.mark.gpu
ITEMS = [2, 0, 1, 0, 2]
TAPE = [1000003 * (i + 7) + 19 for i in range(400)]


def leaf(a):
    return '{"name": "%s"}' % a


def gate(kind, *kids):
    return '{"name": "%s", "children": [%s]}' % (kind, ", ".join(kids))


def trees(b="B"):
    return [leaf("A"), gate("and", leaf(b), leaf("C")), gate("and", leaf("A"), gate("and", gate("or", leaf(b), leaf("D")), leaf("C")))]


COEFS = [0, 1, 2]          # coefficient draws of the three trees
PTS = [b"issuer contract %d " % i * (i + 1) for i in range(len(ITEMS))]


def offsets(items):
    return np.concatenate([[0], np.cumsum([len(p) for p in items])]).astype(np.uint64)


def records(blob, off):
    return [bytes(blob[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


@pytest.fixture(scope="module")
def host():
    h = hl.Host(0)
    yield h
    h.close()


# ------------------------------------------------------------------------------------------------ (a) interleaved share-tree batches
def test_bsw_encrypt_and_encaps_interleaved_trees_equal_the_object_api(host):
    pk, _msk = bsw.setup(host)
    pols = trees()
    host.set_tape(TAPE)
    objs = bsw.encrypt_batch(host, pk, [pols[p] for p in ITEMS], hl.JSON_POLICY, PTS)
    host.set_tape(TAPE)
    blob, off = bsw.encrypt_packed(host, pk, pols, ITEMS, b"".join(PTS), offsets(PTS))
    want = [o.serialize() for o in objs]
    assert records(blob, off) == want
    # encaps: the same draws without the nonce that follows every item's (secret, msg, coefficients)
    kem_tape, at = [], 0
    for p in ITEMS:
        kem_tape += TAPE[at:at + 2 + COEFS[p]]
        at += 2 + COEFS[p] + 1
    host.set_tape(kem_tape)
    hdr, ho, _keys = bsw.encaps_packed(host, pk, pols, ITEMS)
    host.clear_tape()
    assert records(hdr, ho) == [w[:-(4 + len(PTS[i]) + 28)] + bytes(4) for i, w in enumerate(want)]


def test_ghw11_encrypt_interleaved_trees_equal_the_object_api(host):
    pk, _msk = ghw11.setup(host)
    pols = trees()
    host.set_tape(TAPE)
    want = [ghw11.encrypt(host, pk, pols[p], hl.JSON_POLICY, PTS[i]).serialize() for i, p in enumerate(ITEMS)]
    host.set_tape(TAPE)
    blob, off = ghw11.encrypt_packed(host, pk, pols, ITEMS, b"".join(PTS), offsets(PTS))
    host.clear_tape()
    assert records(blob, off) == want


def test_aw11_encrypt_interleaved_trees_equal_the_object_api(host):
    gk = aw11.setup(host)
    pk1, _m1 = aw11.authgen(host, gk, ["A", "B", "C"])
    pk2, _m2 = aw11.authgen(host, gk, ["D"])
    pols = trees()
    host.set_tape(TAPE)
    objs = aw11.encrypt_batch(host, gk, [pk1, pk2], [pols[p] for p in ITEMS], hl.JSON_POLICY, PTS)
    host.set_tape(TAPE)
    blob, off = aw11.encrypt_packed(host, gk, [pk1, pk2], pols, ITEMS, b"".join(PTS), offsets(PTS))
    host.clear_tape()
    assert records(blob, off) == [o.serialize() for o in objs]


@pytest.mark.parametrize("b", ["B", "!B"], ids=["positive", "negated-leaf"])
def test_lsw_keygen_interleaved_trees_equal_the_object_api(host, b):
    pk, msk = lsw.setup(host)
    pols = trees(b)
    host.set_tape(TAPE)
    objs = lsw.keygen_batch(host, pk, msk, [pols[p] for p in ITEMS], hl.JSON_POLICY)
    host.set_tape(TAPE)
    blob, off = lsw.keygen_packed(host, pk, msk, pols, ITEMS)
    host.clear_tape()
    assert records(blob, off) == [o.serialize() for o in objs]


# ------------------------------------------------------------------------------------------------ (b) (c) (d) through the C entry points
SETS = [["A", "B"], ["C"], ["A", "C", "D"]]


class Site:
    """one C entry point: fn(h, *head(n), kinds, n, item index, [pt_blob, pt_off], *before_out(n), out_buf, out_cap, out_off, *after_out(n))"""

    def __init__(self, fn, form, kinds, head, message, empty, pts=False, before_out=None, after_out=None):
        self.fn, self.form, self.kinds, self.head, self.message, self.empty, self.pts = fn, form, kinds, head, message, empty, pts
        self.before_out, self.after_out = before_out or (lambda n: []), after_out or (lambda n: [])

    def call(self, host, items, buf, cap, off):
        n = len(items)
        it = np.array(items, dtype=np.uint32)
        if self.form == "policies":
            arr, cnt = hl._strs(self.kinds)
            mid = [arr, cnt, hl.JSON_POLICY]
        else:
            arr, _ = hl._strs([a for s in self.kinds for a in s])
            mid = [arr, (ctypes.c_size_t * len(self.kinds))(*[len(s) for s in self.kinds]), ctypes.c_size_t(len(self.kinds))]
        args = list(self.head(n)) + mid + [ctypes.c_size_t(n), hl._np_ptr(it)]
        keep = [it]
        if self.pts:
            pts = [b"payload %d" % i for i in range(n)]
            blob, po = np.frombuffer(b"".join(pts) or b"\0", dtype=np.uint8), offsets(pts)
            keep += [blob, po]
            args += [hl._np_ptr(blob), hl._np_ptr(po)]
        args += list(self.before_out(n)) + [hl._np_ptr(buf) if buf is not None else None, ctypes.c_size_t(cap), hl._np_ptr(off)] + list(self.after_out(n))
        return getattr(host.lib, self.fn)(host.h, *args)


def scratch(n, size=32):
    return hl._np_ptr(np.zeros((max(n, 1), size), dtype=np.uint8))


@pytest.fixture(scope="module")
def sites(host):
    out = {}
    keep = []          # the key objects live as long as the sites that hold their pointers

    def add(name, *a, **kw):
        out[name] = Site(*a, **kw)

    pk, msk = ac17.setup(host)
    keep += [pk, msk]
    add("ac17_cp_keygen", "rabe_ac17_cp_keygen_packed", "sets", SETS, lambda n, m=msk: [m.ptr], b"cp_keygen_packed: item_set out of range", (1, 0))
    add("ac17_kp_keygen", "rabe_ac17_kp_keygen_packed", "policies", trees(), lambda n, m=msk: [m.ptr], b"kp_keygen_packed: item_policy out of range", (1, 0))
    add("ac17_cp_encrypt", "rabe_ac17_cp_encrypt_packed", "policies", trees(), lambda n, p=pk: [p.ptr], b"encrypt_packed: item_policy out of range", (1, 0),
        pts=True)
    add("ac17_kp_encrypt", "rabe_ac17_kp_encrypt_packed", "sets", SETS, lambda n, p=pk: [p.ptr], b"encrypt_packed: item_policy out of range", (1, 0), pts=True)
    add("ac17_cp_encaps", "rabe_ac17_cp_encaps_packed", "policies", trees(), lambda n, p=pk: [p.ptr], b"encrypt_packed: item_policy out of range", (0, 0),
        after_out=lambda n: [scratch(n)])
    pk, msk = bsw.setup(host)
    sk = bsw.keygen(host, pk, msk, ["A", "B", "C", "D"])
    keep += [pk, msk, sk]
    add("bsw_keygen", "rabe_bsw_keygen_packed", "sets", SETS, lambda n, p=pk, m=msk: [p.ptr, m.ptr], b"bsw::keygen_packed: item_set out of range", (1, 0))
    add("bsw_delegate", "rabe_bsw_delegate_packed", "sets", SETS, lambda n, p=pk, s=sk: [p.ptr, s.ptr], b"bsw::delegate_packed: item_subset out of range", (1, 0))
    add("bsw_encrypt", "rabe_bsw_encrypt_packed", "policies", trees(), lambda n, p=pk: [p.ptr], b"bsw::encrypt_packed: item_policy out of range", (1, 0), pts=True)
    add("bsw_encaps", "rabe_bsw_encaps_packed", "policies", trees(), lambda n, p=pk: [p.ptr], b"bsw::encrypt_packed: item_policy out of range", (0, 0),
        after_out=lambda n: [scratch(n)])
    pk, msk = lsw.setup(host)
    keep += [pk, msk]
    add("lsw_encrypt", "rabe_lsw_encrypt_packed", "sets", SETS, lambda n, p=pk: [p.ptr], b"lsw::encrypt_packed: item_set out of range", (1, 0), pts=True)
    add("lsw_keygen", "rabe_lsw_keygen_packed", "policies", trees(), lambda n, p=pk, m=msk: [p.ptr, m.ptr], b"lsw::keygen_packed: item_policy out of range", (1, 0))
    gk = aw11.setup(host)
    apk, amsk = aw11.authgen(host, gk, ["A", "B", "C", "D"])
    pks = (ctypes.c_void_p * 1)(apk.ptr)
    keep += [gk, apk, amsk, pks]
    add("aw11_encrypt", "rabe_aw11_encrypt_packed", "policies", trees(), lambda n, g=gk: [g.ptr, pks, ctypes.c_size_t(1)],
        b"aw11::encrypt_packed: item_policy out of range", (1, 0), pts=True)
    add("aw11_keygen", "rabe_aw11_keygen_packed", "sets", SETS, lambda n, g=gk, m=amsk: [g.ptr, m.ptr, hl._strs(["user-%d" % i for i in range(n)])[0]],
        b"aw11::keygen_packed: item_set out of range", (1, 0))
    pk, msk = ghw11.setup(host)
    keep += [pk, msk]
    add("ghw11_encrypt", "rabe_ghw11_encrypt_packed", "policies", trees(), lambda n, p=pk: [p.ptr], b"ghw11::encrypt_packed: item_policy out of range", (1, 0),
        pts=True)
    add("ghw11_keygen", "rabe_ghw11_keygen_packed", "sets", SETS, lambda n, p=pk, m=msk: [p.ptr, m.ptr], b"ghw11::keygen_packed: item_set out of range", (0, 0))
    add("ghw11_provision", "rabe_ghw11_provision_packed", "sets", SETS, lambda n, p=pk, m=msk: [p.ptr, m.ptr], b"ghw11::provision_packed: item_set out of range",
        (0, 0), before_out=lambda n: [None, ctypes.c_size_t(0), None], after_out=lambda n: [scratch(n)])
    for name, mod in (("bdabe", bdabe), ("mke08", mke08)):
        pk, msk = mod.setup(host)
        ska = bdabe.authgen(host, pk, msk, "aa1") if name == "bdabe" else mke08.authgen(host, "aa1")
        attr_pk = (lambda a: bdabe.request_attribute_pk(host, pk, ska, a)) if name == "bdabe" else (lambda a: mke08.request_authority_pk(host, pk, a, ska))
        apks = [attr_pk("aa1::" + a) for a in "ABCD"]
        arr = (ctypes.c_void_p * len(apks))(*[p.ptr for p in apks])
        keep += [pk, msk, ska, apks, arr]
        dnf = [leaf("aa1::A"), gate("and", leaf("aa1::B"), leaf("aa1::C")), gate("or", leaf("aa1::A"), gate("and", leaf("aa1::B"), leaf("aa1::D")))]
        add(name + "_encrypt", "rabe_%s_encrypt_packed" % name, "policies", dnf, lambda n, p=pk, a=arr, k=len(apks): [p.ptr, a, ctypes.c_size_t(k)],
            b"%s::encrypt_packed: item_policy out of range" % name.encode(), (1, 0), pts=True)
        users, uo = mod.keygen_packed(host, pk, ska if name == "bdabe" else msk, ["user-%d" % i for i in range(4)])
        upks = [mod.public_user_key_record(r) for r in records(users, uo)]
        request = "request_attribute_sk_packed" if name == "bdabe" else "request_authority_sk_packed"

        def before(n, upks=upks):
            blob, off, status = np.frombuffer(b"".join(upks[:n]) or b"\0", dtype=np.uint8), offsets(upks[:n]), np.zeros(max(n, 1), dtype=np.int32)
            keep.append((blob, off, status))
            return [hl._np_ptr(blob), ctypes.c_size_t(blob.size if n else 0), hl._np_ptr(off), ctypes.c_uint32(0), hl._np_ptr(status)]
        add(name + "_request_sk", "rabe_%s_%s" % (name, request), "sets", [["aa1::" + a for a in s] for s in SETS], lambda n, s=ska: [s.ptr],
            b"%s::%s: item_set out of range" % (name.encode(), request.encode()), (0, 0), before_out=before)
    out["_keep"] = keep
    return out


SITE_NAMES = ["ac17_cp_keygen", "ac17_kp_keygen", "ac17_cp_encrypt", "ac17_kp_encrypt", "ac17_cp_encaps", "bsw_keygen", "bsw_delegate", "bsw_encrypt",
              "bsw_encaps", "lsw_encrypt", "lsw_keygen", "aw11_encrypt", "aw11_keygen", "ghw11_encrypt", "ghw11_keygen", "ghw11_provision",
              "bdabe_encrypt", "bdabe_request_sk", "mke08_encrypt", "mke08_request_sk"]


def reference(host, site, items):
    """the records of a call with room to spare, on TAPE"""
    buf, off = np.full(1 << 16, 0xAB, dtype=np.uint8), np.zeros(len(items) + 1, dtype=np.uint64)
    host.set_tape(TAPE)
    rc = site.call(host, items, buf, buf.size, off)
    host.clear_tape()
    assert rc == 0, host.lib.rabe_host_last_error(None)
    need = int(off[len(items)])
    assert 0 < need < buf.size
    return bytes(buf[:need]), off.tolist()


@pytest.mark.parametrize("name", SITE_NAMES)
def test_one_byte_short_then_exact(host, sites, name):
    site = sites[name]
    items = [2, 0, 1]
    want, want_off = reference(host, site, items)
    need = len(want)
    buf, off = np.full(need, 0xAB, dtype=np.uint8), np.full(len(items) + 1, 99, dtype=np.uint64)
    host.set_tape(TAPE)          # set once: a refused call that drew anything would shift the draws of the one that follows
    rc = site.call(host, items, buf, need - 1, off)
    print(name, "short: rc", rc, "off", off.tolist(), "need", need)
    assert rc == 1 and int(off[len(items)]) == need and off.tolist() == want_off and (buf == 0xAB).all()
    rc = site.call(host, items, buf, need, off)
    host.clear_tape()
    assert rc == 0 and bytes(buf) == want and off.tolist() == want_off


@pytest.mark.parametrize("name", SITE_NAMES)
def test_index_out_of_range_fails_before_any_draw(host, sites, name):
    site = sites[name]
    want, want_off = reference(host, site, [1, 0])
    buf, off = np.full(len(want), 0xAB, dtype=np.uint8), np.zeros(3, dtype=np.uint64)
    host.set_tape(TAPE)
    rc = site.call(host, [1, len(site.kinds)], buf, buf.size, off)
    msg = host.lib.rabe_host_last_error(None)
    print(name, "out of range: rc", rc, msg)
    assert rc not in (0, 1) and site.message in msg and (buf == 0xAB).all()
    rc = site.call(host, [1, 0], buf, buf.size, off)          # the tape is where it was: the bytes of the fresh run
    host.clear_tape()
    assert rc == 0 and bytes(buf) == want and off.tolist() == want_off


@pytest.mark.parametrize("name", SITE_NAMES)
def test_empty_call_with_a_null_buffer(host, sites, name):
    site = sites[name]
    off = np.full(1, 99, dtype=np.uint64)
    rc = site.call(host, [], None, 0, off)
    print(name, "n = 0: rc", rc, "off[0]", int(off[0]))
    assert (rc, int(off[0])) == site.empty
