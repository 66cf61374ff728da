"""The table behind tests/test_gpu_encrypt_tail_contract.py and tools/record_encrypt_tail_contract.py: the packed encrypt and encaps entry of
every scheme (both AC17 flavours) and every issuer that hands a source table to the record writer (host/record_layout.h: RecordSources), run at a
shape wide enough to show a wrong index array, a wrong stride or a misplaced seal.

Shape: 5 items over 3 policies / attribute lists / subsets of 1, 2 and 3 rows, in the order [2, 0, 1, 2, 0], payloads of 1, 15, 16, 17 and
33 bytes -- below, at and past an AES block and past two.  The DNF issuer gets names of five lengths (its names are a source with explicit
byte offsets), LSW's key issuer also runs with negative leaves (five sources instead of two).  Every draw comes from a tape.

The argument descriptors and the key setup follow tests/packed_abi_cases.py, which freezes the same entry points at 3 items with their
sizing, short, empty and null calls; here there is the full call alone."""
import ctypes
import hashlib

import numpy as np

from rabe_amd import hostlib as hl
from rabe_amd.schemes import ac17, aw11, bdabe, bsw, ghw11, lsw, mke08
from tests.packed_abi_cases import FLAGS, U8, blob, buf, buf2, count, gate, inp, leaf, marker, offsets, policies, ptrs, sets, u8, val

N = 5
ITEMS = [2, 0, 1, 2, 0]
TAPE = [1000003 * (i + 11) + 23 for i in range(4000)]
PTS = [b"\x01", bytes(range(15)), bytes(range(16)), bytes(range(17)), bytes(range(33))]
NAMES = ["u", "user-1", "user-22", "ab", "user-4444"]
ROOM = 1 << 16
OFF, STATUS, FIXED = 0x9999999999999999, 7, 0xCD


def node(op, *names):
    """`op` over the names as a chain of two-child gates, the right child nested (the MSP of AC17 takes no wider gate)"""
    rest = leaf(names[-1])
    for a in reversed(names[:-1]):
        rest = '{"name": "%s", "children": [%s, %s]}' % (op, leaf(a), rest)
    return rest


def off(name):
    return ("off", name, N + 1)


def status(name="status"):
    return ("status", name, N)


def fixed(name, stride):
    return ("fixed", name, stride * N)


def build_entries(host):
    """{name: (entry point, argument list)}, and what has to stay alive while the table is used"""
    keep, E = [], {}
    pols, lists = [leaf("A"), gate("A", "B"), node("and", "A", "B", "C")], [["A"], ["A", "B"], ["A", "B", "C"]]
    pt_blob, pt_off = b"".join(PTS), offsets(PTS)
    pt = [inp("pt_blob", u8(pt_blob)), inp("pt_off", pt_off)]
    item = inp("item", np.array(ITEMS, dtype=np.uint32))
    host.set_tape(TAPE)

    def encrypt_pair(scheme, head, kinds, flavour=""):
        E["%s%s_encrypt" % (scheme, flavour)] = ("rabe_%s%s_encrypt_packed" % (scheme, flavour), head + kinds + [count(), item] + pt + [buf(), off("off")])
        E["%s%s_encaps" % (scheme, flavour)] = ("rabe_%s_kem_encaps" % scheme if scheme in ("bdabe", "mke08") else "rabe_%s%s_encaps_packed" % (scheme, flavour), head + kinds + [count(), item, buf(), off("off"), fixed("keys", 32)])

    def issue(name, fn, head, kinds):
        E[name] = (fn, head + kinds + [count(), item, buf(), off("off")])

    # ---- ac17
    pk, msk = ac17.setup(host)
    keep += [pk, msk]
    encrypt_pair("ac17", [val(pk.ptr)], policies(pols), "_cp")
    encrypt_pair("ac17", [val(pk.ptr)], sets(lists), "_kp")
    issue("ac17_kp_keygen", "rabe_ac17_kp_keygen_packed", [val(msk.ptr)], policies(pols))
    # ---- bsw
    pk, msk = bsw.setup(host)
    sk = bsw.keygen(host, pk, msk, ["A", "B", "C"])
    keep += [pk, msk, sk]
    encrypt_pair("bsw", [val(pk.ptr)], policies(pols))
    issue("bsw_delegate", "rabe_bsw_delegate_packed", [val(pk.ptr), val(sk.ptr)], sets(lists))
    # ---- lsw
    pk, msk = lsw.setup(host)
    keep += [pk, msk]
    encrypt_pair("lsw", [val(pk.ptr)], sets(lists))
    issue("lsw_keygen", "rabe_lsw_keygen_packed", [val(pk.ptr), val(msk.ptr)], policies(pols))
    issue("lsw_keygen_negative", "rabe_lsw_keygen_packed", [val(pk.ptr), val(msk.ptr)], policies([leaf("!A"), node("and", "A", "!B"), node("and", "!A", "B", "C")]))
    # ---- aw11
    gk = aw11.setup(host)
    apk, amsk = aw11.authgen(host, gk, ["A", "B", "C"])
    keep += [gk, apk, amsk]
    encrypt_pair("aw11", [val(gk.ptr)] + ptrs([apk]), policies(pols))
    # ---- ghw11
    pk, msk = ghw11.setup(host)
    keep += [pk, msk]
    encrypt_pair("ghw11", [val(pk.ptr)], policies(pols))
    issue("ghw11_keygen", "rabe_ghw11_keygen_packed", [val(pk.ptr), val(msk.ptr)], sets(lists))
    E["ghw11_provision"] = ("rabe_ghw11_provision_packed", [val(pk.ptr), val(msk.ptr)] + sets(lists) + [count(), item, buf2("sk_buf", ROOM), off("sk_off"), buf(),
                                                                                                    off("tk_off"), fixed("rk", 32)])
    # ---- bdabe, mke08: one row per DNF term
    attrs = ["aa1::A", "aa1::B", "aa1::C"]
    dnf = [leaf(attrs[0]), node("or", *attrs[:2]), '{"name": "or", "children": [%s]}' % ", ".join(leaf(a) for a in attrs)]          # json_to_dnf: one flat OR
    dnf_lists = [attrs[:1], attrs[:2], attrs]
    names, _ = hl._strs(NAMES)
    for name, mod in (("bdabe", bdabe), ("mke08", mke08)):
        pk, msk = mod.setup(host)
        if name == "bdabe":
            ska = bdabe.authgen(host, pk, msk, "aa1")
            apks = [bdabe.request_attribute_pk(host, pk, ska, a) for a in attrs]
            issuer, request = ska, "rabe_bdabe_request_attribute_sk_packed"
        else:
            ska = mke08.authgen(host, "aa1")
            apks = [mke08.request_authority_pk(host, pk, a, ska) for a in attrs]
            issuer, request = msk, "rabe_mke08_request_authority_sk_packed"
        keep += [pk, msk, ska, apks]
        encrypt_pair(name, [val(pk.ptr)] + ptrs(apks), policies(dnf))
        E[name + "_keygen"] = ("rabe_%s_keygen_packed" % name, [val(pk.ptr), val(issuer.ptr), val(names), count(), buf(), off("off")])
        host.set_tape(TAPE)
        users, uo = mod.keygen_packed(host, pk, issuer, NAMES)[:2]
        users = bytes(users)
        upks = [mod.public_user_key_record(users[int(uo[i]):int(uo[i + 1])]) for i in range(N)]
        E[name + "_request_sk"] = (request, [val(ska.ptr)] + sets(dnf_lists) + [count(), item] + blob("upk", b"".join(upks), offsets(upks)) +
                                   [FLAGS, status(), buf(), off("off")])
    host.clear_tape()
    return E, keep


def run(host, entry):
    """the full call of one entry: return code, error text, the offsets arrays, and a SHA-256 per written array -- `buf` up to the extent its
    offsets announce (what lies behind must be untouched)"""
    fn, arglist = entry
    outs, args, keep = [], [], []
    for kind, name, v in arglist:
        if kind == "val":
            args.append(v)
        elif kind == "n":
            args.append(ctypes.c_size_t(N))
        elif kind == "in":
            keep.append(v)
            args.append(hl._np_ptr(v))
        elif kind in ("buf", "buf2"):
            a = np.full(ROOM, U8, dtype=np.uint8)
            outs.append((name, a))
            args += [hl._np_ptr(a), ctypes.c_size_t(ROOM)]
        else:
            a = np.full(v, {"off": OFF, "status": STATUS, "fixed": FIXED}[kind], dtype={"off": np.uint64, "status": np.int32, "fixed": np.uint8}[kind])
            outs.append((name, a))
            args.append(hl._np_ptr(a))
    quiet = marker(host.lib)
    host.set_tape(TAPE)
    rc = getattr(host.lib, fn)(host.h, *args)
    host.clear_tape()
    err = host.lib.rabe_host_last_error(None)
    rec = {"rc": int(rc), "err": "" if err == quiet else (err or b"").decode("utf-8", "replace")}
    arrays = dict(outs)
    rec["off"] = {name: [int(x) for x in a] for name, a in outs if a.dtype == np.uint64}
    rec["sha256"] = {}
    for name, a in outs:
        if a.dtype == np.uint64:
            continue
        if name in ("buf", "sk_buf") and rc == 0:
            extent = int(arrays[{"buf": [n for n in ("tk_off", "off") if n in arrays][0], "sk_buf": "sk_off"}[name]][N])
            assert extent <= a.size and (a[extent:] == U8).all(), (fn, name, "bytes written behind the last record")
            a = a[:extent]
        rec["sha256"][name] = hashlib.sha256(a.tobytes()).hexdigest()
    return rec
