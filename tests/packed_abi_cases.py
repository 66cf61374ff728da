"""The table behind tests/test_gpu_packed_abi_contract.py and tools/record_packed_abi_contract.py: every rabe_*_packed entry point of
include/rabe_host.h with its argument list, and the cases each one is run through.

Shapes: 3 items over 2 policies / attribute lists (a single leaf and one AND gate over the attributes A, B), payloads of 1 and 17 bytes, every
draw -- the keys' included -- from a tape, so a record is a pure function of the library.

An argument is in an entry's `nullable` list only where the code refuses it in plain sight: a `null input` throw in the entry point, an
`engines_if(...)` guard in front of a check of the scheme's function, or that check at the top of the scheme's function (host/schemes.cpp,
host/packed.cpp).  Everything else is never handed over as null: the library would dereference it."""
import ctypes
import hashlib

import numpy as np

from rabe_amd import hostlib as hl
from rabe_amd.schemes import ac17, aw11, bdabe, bsw, ghw11, lsw, mke08

N = 3
ITEMS = [0, 1, 0]
TAPE = [1000003 * (i + 7) + 19 for i in range(1500)]
PTS = [b"\x01", bytes(range(17)), b"\x02"]
ROOM = 1 << 15          # capacity of the full call: the records of three items are a few kilobytes
U8, OFF, STATUS, FIXED = 0xAB, 0x9999999999999999, 7, 0xCD          # sentinels of the output arrays


def leaf(a):
    return '{"name": "%s"}' % a


def gate(a, b):
    return '{"name": "and", "children": [%s, %s]}' % (leaf(a), leaf(b))


def offsets(items):
    return np.concatenate([[0], np.cumsum([len(p) for p in items])]).astype(np.uint64)


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


# ---- argument descriptors: what an entry point takes, in the header's order
def val(v):
    return ("val", None, v)


def count():
    return ("n", None, None)          # n_items: 3, or 0 in the `n0` case


def inp(name, array):
    return ("in", name, array)


def buf(name="buf"):
    return ("buf", name, None)          # the output buffer, followed by its capacity


def buf2(name, size):
    return ("buf2", name, size)          # a second sized output (provision's secret keys), followed by its capacity


def off(name):
    return ("off", name, N + 1)


def status(name="status"):
    return ("status", name, N)


def fixed(name, stride):
    return ("fixed", name, stride * N)


def policies(texts):
    arr, n = hl._strs(texts)
    return [val(arr), val(n), val(hl.JSON_POLICY)]


def sets(lists):
    arr, _ = hl._strs([a for s in lists for a in s])
    return [val(arr), val((ctypes.c_size_t * len(lists))(*[len(s) for s in lists])), val(ctypes.c_size_t(len(lists)))]


def ptrs(objs):
    return [val((ctypes.c_void_p * len(objs))(*[o.ptr for o in objs])), val(ctypes.c_size_t(len(objs)))]


def blob(name, data, offs):
    """records in: blob, its length, the offsets"""
    return [inp(name + "_blob", u8(data)), val(ctypes.c_size_t(len(bytes(data)))), inp(name + "_off", np.ascontiguousarray(offs, dtype=np.uint64))]


FLAGS = val(ctypes.c_uint32(0))


class Entry:
    def __init__(self, fn, args, need, nullable):
        """need: what `short` is one byte short of -- ("out", name): the last offset the full call wrote; ("const", bytes); ("span", name), the
        decrypt shape: `short` is one byte short of the plaintexts the full call wrote (pt_off[n], which no call can do with less than), and
        `short_span` one byte short of the records of that input offsets array -- what the cut call and some uncut ones ask for"""
        self.fn, self.args, self.need, self.nullable = fn, args, need, nullable
        names = [a[1] for a in args if a[1]]
        assert all(n in names for n in nullable), (fn, nullable, names)
        # where the records in `buf` end: the last entry of the offsets array that describes them, or a fixed size
        self.extent = "pt_off" if "pt_off" in names else need[1] if need else None

    def cases(self):
        out = ["full", "n0"]
        if any(a[0] == "buf" for a in self.args):
            out += ["sizing", "short"] + (["short_span"] if self.need[0] == "span" else [])
        return out + ["null:" + n for n in self.nullable]


def build_entries(host):
    """the keys (module scope in the test), the inputs of the decrypt-shaped calls, the table.  Returns (entries, keep-alive list)."""
    keep = []
    E = {}

    def add(fn, args, need, nullable):
        E[fn] = Entry(fn, args, need, nullable)

    pols, lists = [leaf("A"), gate("A", "B")], [["A", "B"], ["A"]]
    pt_blob, pt_off = b"".join(PTS), offsets(PTS)
    pt = [inp("pt_blob", u8(pt_blob)), inp("pt_off", pt_off)]
    item = inp("item", np.array(ITEMS, dtype=np.uint32))
    host.set_tape(TAPE)

    def records(fn, *a, **kw):
        """the inputs of a decrypt-shaped call: what the matching issuer writes on the tape"""
        host.set_tape(TAPE)
        r = fn(host, *a, **kw)
        return bytes(r[0]), np.array(r[1], dtype=np.uint64)

    def encrypt_shape(fn, head, kinds, tail=()):
        add(fn, head + kinds + [count(), item] + pt + [buf(), off("off")] + list(tail), ("out", "off"), ["item", "pt_off", "off"])

    def issue_shape(fn, head, kinds, nullable):
        add(fn, head + kinds + [count(), item, buf(), off("off")], ("out", "off"), nullable)

    def encaps_shape(fn, head, kinds):
        add(fn, head + kinds + [count(), item, buf(), off("off"), fixed("keys", 32)], ("out", "off"), ["item", "off", "keys"])

    def decrypt_shape(fn, head, data, offs, nullable, before=()):
        add(fn, head + [count()] + list(before) + blob("ct", data, offs) + [FLAGS, status(), buf(), off("pt_off")], ("span", "ct_off"), nullable)

    def decaps_shape(fn, head, data, offs):
        add(fn, head + [count()] + blob("ct", data, offs) + [FLAGS, status(), fixed("keys", 32)], None, ["ct_blob", "ct_off", "status", "keys"])

    # ---- ac17
    pk, msk = ac17.setup(host)
    cp_sk, kp_sk = ac17.cp_keygen(host, msk, ["A", "B"]), ac17.kp_keygen(host, msk, gate("A", "B"))
    keep += [pk, msk, cp_sk, kp_sk]
    encrypt_shape("rabe_ac17_cp_encrypt_packed", [val(pk.ptr)], policies(pols))
    encrypt_shape("rabe_ac17_kp_encrypt_packed", [val(pk.ptr)], sets(lists))
    issue_shape("rabe_ac17_cp_keygen_packed", [val(msk.ptr)], sets(lists), ["item", "off"])
    issue_shape("rabe_ac17_kp_keygen_packed", [val(msk.ptr)], policies(pols), ["item", "off"])
    encaps_shape("rabe_ac17_cp_encaps_packed", [val(pk.ptr)], policies(pols))
    encaps_shape("rabe_ac17_kp_encaps_packed", [val(pk.ptr)], sets(lists))
    cp_ct = records(ac17.cp_encrypt_packed, pk, pols, ITEMS, pt_blob, pt_off)
    kp_ct = records(ac17.kp_encrypt_packed, pk, lists, ITEMS, pt_blob, pt_off)
    decrypt_shape("rabe_ac17_cp_decrypt_packed", [val(cp_sk.ptr)], *cp_ct, ["ct_blob", "ct_off"])
    decrypt_shape("rabe_ac17_kp_decrypt_packed", [val(kp_sk.ptr)], *kp_ct, ["ct_blob", "ct_off"])          # the list [A] fails its item alone
    decaps_shape("rabe_ac17_cp_decaps_packed", [val(cp_sk.ptr)], *cp_ct)
    decaps_shape("rabe_ac17_kp_decaps_packed", [val(kp_sk.ptr)], *kp_ct)
    # ---- bsw
    pk, msk = bsw.setup(host)
    sk = bsw.keygen(host, pk, msk, ["A", "B"])
    keep += [pk, msk, sk]
    encrypt_shape("rabe_bsw_encrypt_packed", [val(pk.ptr)], policies(pols))
    encaps_shape("rabe_bsw_encaps_packed", [val(pk.ptr)], policies(pols))
    issue_shape("rabe_bsw_keygen_packed", [val(pk.ptr), val(msk.ptr)], sets(lists), ["item", "off"])
    issue_shape("rabe_bsw_delegate_packed", [val(pk.ptr), val(sk.ptr)], sets(lists), ["item", "off"])
    ct = records(bsw.encrypt_packed, pk, pols, ITEMS, pt_blob, pt_off)
    decrypt_shape("rabe_bsw_decrypt_packed", [val(sk.ptr)], *ct, ["ct_blob", "ct_off"])
    decaps_shape("rabe_bsw_decaps_packed", [val(sk.ptr)], *ct)
    # ---- lsw
    pk, msk = lsw.setup(host)
    sk = lsw.keygen(host, pk, msk, gate("A", "B"))
    one_ct = lsw.encrypt(host, pk, ["A", "B"], PTS[1])
    keep += [pk, msk, sk, one_ct]
    encrypt_shape("rabe_lsw_encrypt_packed", [val(pk.ptr)], sets(lists))
    encaps_shape("rabe_lsw_encaps_packed", [val(pk.ptr)], sets(lists))
    issue_shape("rabe_lsw_keygen_packed", [val(pk.ptr), val(msk.ptr)], policies(pols), ["item", "off"])
    sks = records(lsw.keygen_packed, pk, msk, pols, ITEMS)
    ct = records(lsw.encrypt_packed, pk, lists, ITEMS, pt_blob, pt_off)
    add("rabe_lsw_decrypt_packed", [val(one_ct.ptr), count()] + blob("sk", *sks) + [FLAGS, status(), buf(), off("pt_off")], ("span", "sk_off"), ["sk_blob", "sk_off"])
    decrypt_shape("rabe_lsw_decrypt_one_sk_packed", [val(sk.ptr)], *ct, ["ct_blob", "ct_off", "pt_off"])
    decaps_shape("rabe_lsw_decaps_packed", [val(sk.ptr)], *ct)
    # ---- aw11
    gk = aw11.setup(host)
    apk, amsk = aw11.authgen(host, gk, ["A", "B"])
    sk = aw11.keygen(host, gk, amsk, "user", ["A", "B"])
    keep += [gk, apk, amsk, sk]
    gids, _ = hl._strs(["user-%d" % i for i in range(N)])
    issue_shape("rabe_aw11_keygen_packed", [val(gk.ptr), val(amsk.ptr), val(gids)], sets(lists), ["item", "off"])
    encrypt_shape("rabe_aw11_encrypt_packed", [val(gk.ptr)] + ptrs([apk]), policies(pols))
    encaps_shape("rabe_aw11_encaps_packed", [val(gk.ptr)] + ptrs([apk]), policies(pols))
    ct = records(aw11.encrypt_packed, gk, [apk], pols, ITEMS, pt_blob, pt_off)
    decrypt_shape("rabe_aw11_decrypt_packed", [val(gk.ptr), val(sk.ptr)], *ct, ["ct_blob", "ct_off"])
    decaps_shape("rabe_aw11_decaps_packed", [val(gk.ptr), val(sk.ptr)], *ct)
    # ---- ghw11
    pk, msk = ghw11.setup(host)
    sk = ghw11.keygen(host, pk, msk, ["A", "B"])
    tk, rk = ghw11.tkgen(host, sk)
    keep += [pk, msk, sk, tk, rk]
    encrypt_shape("rabe_ghw11_encrypt_packed", [val(pk.ptr)], policies(pols))
    encaps_shape("rabe_ghw11_encaps_packed", [val(pk.ptr)], policies(pols))
    issue_shape("rabe_ghw11_keygen_packed", [val(pk.ptr), val(msk.ptr)], sets(lists), ["item", "off"])
    ct = records(ghw11.encrypt_packed, pk, pols, ITEMS, pt_blob, pt_off)
    tct, _st = ghw11.transform_packed(host, tk, *ct)
    tct = np.ascontiguousarray(tct, dtype=np.uint8).reshape(-1).copy()
    sks = records(ghw11.keygen_packed, pk, msk, lists, ITEMS)
    add("rabe_ghw11_transform_packed", [val(tk.ptr), count()] + blob("ct", *ct) + [FLAGS, status(), buf()], ("const", 768 * N), ["ct_blob", "ct_off", "status"])
    decrypt_shape("rabe_ghw11_decrypt_out_packed", [val(rk.ptr)], *ct, ["tct", "ct_blob", "ct_off", "status", "pt_off"], before=[inp("tct", tct)])
    decrypt_shape("rabe_ghw11_decrypt_packed", [val(sk.ptr)], *ct, ["ct_blob", "ct_off", "status", "pt_off"])
    add("rabe_ghw11_decaps_out_packed", [val(rk.ptr), count(), inp("tct", tct), FLAGS, status(), fixed("keys", 32)], None, ["tct", "status", "keys"])
    decaps_shape("rabe_ghw11_decaps_packed", [val(sk.ptr)], *ct)
    add("rabe_ghw11_tkgen_packed", [count()] + blob("sk", *sks) + [FLAGS, status(), buf(), off("tk_off"), fixed("rk", 32)], ("out", "tk_off"),
        ["sk_blob", "sk_off", "status", "tk_off", "rk"])
    add("rabe_ghw11_provision_packed", [val(pk.ptr), val(msk.ptr)] + sets(lists) + [count(), item, buf2("sk_buf", ROOM), off("sk_off"), buf(), off("tk_off"),
                                                                                    fixed("rk", 32)], ("out", "tk_off"), ["item", "tk_off", "rk"])
    # ---- bdabe, mke08
    dnf = [leaf("aa1::A"), gate("aa1::A", "aa1::B")]
    dnf_lists = [["aa1::A", "aa1::B"], ["aa1::A"]]
    names, _ = hl._strs(["user-%d" % i for i in range(N)])
    for name, mod in (("bdabe", bdabe), ("mke08", mke08)):
        pk, msk = mod.setup(host)
        if name == "bdabe":
            ska = bdabe.authgen(host, pk, msk, "aa1")
            apks = [bdabe.request_attribute_pk(host, pk, ska, a) for a in dnf_lists[0]]
            uk = bdabe.keygen(host, pk, ska, "user")
            for a in dnf_lists[0]:
                bdabe.request_attribute_sk(host, uk, ska, a)
            issuer, request = ska, "rabe_bdabe_request_attribute_sk_packed"
        else:
            ska = mke08.authgen(host, "aa1")
            apks = [mke08.request_authority_pk(host, pk, a, ska) for a in dnf_lists[0]]
            uk = mke08.keygen(host, pk, msk, "user")
            for a in dnf_lists[0]:
                mke08.request_authority_sk(host, uk, a, ska)
            issuer, request = msk, "rabe_mke08_request_authority_sk_packed"
        keep += [pk, msk, ska, apks, uk]
        encrypt_shape("rabe_%s_encrypt_packed" % name, [val(pk.ptr)] + ptrs(apks), policies(dnf))
        ct = records(mod.encrypt_packed, pk, apks, dnf, ITEMS, pt_blob, pt_off)
        decrypt_shape("rabe_%s_decrypt_packed" % name, [val(uk.ptr)], *ct, [])
        add("rabe_%s_keygen_packed" % name, [val(pk.ptr), val(issuer.ptr), val(names), count(), buf(), off("off")], ("out", "off"), ["off"])
        users, uo = records(mod.keygen_packed, pk, issuer, ["user-%d" % i for i in range(N)])
        upks = [mod.public_user_key_record(users[int(uo[i]):int(uo[i + 1])]) for i in range(N)]
        add(request, [val(ska.ptr)] + sets(dnf_lists) + [count(), item] + blob("upk", b"".join(upks), offsets(upks)) + [FLAGS, status(), buf(), off("off")],
            ("out", "off"), ["item", "upk_blob", "upk_off", "status", "off"])
    host.clear_tape()
    return E, keep


def marker(lib):
    """leaves a known text in the calling thread's last error, so that a call which sets none can be told from one that repeats the last one"""
    p = ctypes.c_void_p()
    rc = lib.rabe_policy_parse(b"not a policy", hl.JSON_POLICY, hl.JSON_POLICY, ctypes.byref(p))
    assert rc != 0
    return lib.rabe_host_last_error(None)


def run_case(host, entry, case, need=None):
    """one call.  Returns (record, need): the record is what the golden file holds; need = {case: the size that `short` case is measured against}."""
    n = 0 if case == "n0" else N
    null = case[5:] if case.startswith("null:") else None
    short = need.get(case) if need else None
    assert not case.startswith("short") or short, (entry.fn, case, "the full call reported no size")
    outs, args, keep = [], [], []
    for kind, name, v in entry.args:
        if kind == "val":
            args.append(v)
        elif kind == "n":
            args.append(ctypes.c_size_t(n))
        elif kind == "in":
            keep.append(v)
            args.append(None if name == null else hl._np_ptr(v))
        elif kind in ("buf", "buf2"):
            size = v if kind == "buf2" else short if short else ROOM
            a = np.full(size, U8, dtype=np.uint8)
            outs.append((name, a, U8))
            if kind == "buf" and case == "sizing":
                args += [None, ctypes.c_size_t(0)]
            else:
                args += [hl._np_ptr(a), ctypes.c_size_t(size - 1 if kind == "buf" and short else size)]
        else:
            a = np.full(v, {"off": OFF, "status": STATUS, "fixed": FIXED}[kind], dtype={"off": np.uint64, "status": np.int32, "fixed": np.uint8}[kind])
            outs.append((name, a, a[0].copy()))
            args.append(None if name == null else hl._np_ptr(a))
    quiet = marker(host.lib)
    host.set_tape(TAPE)
    rc = getattr(host.lib, entry.fn)(host.h, *args)
    host.clear_tape()
    err = host.lib.rabe_host_last_error(None)
    rec = {"rc": int(rc), "err": "" if err == quiet else (err or b"").decode("utf-8", "replace")}
    touched = dict((name, a) for name, a, fill in outs if not (a == fill).all())
    rec["touched"] = list(touched)
    rec["off"] = {name: [int(x) for x in a] for name, a in touched.items() if a.dtype == np.uint64}
    # the records: the buffer up to the extent its offsets array announces (a call cut over a group closes its blocks' slices up and may leave
    # their first copies behind the last record: `tail_clean` says whether it did), every other written array whole
    extent = entry.extent if isinstance(entry.extent, int) else int(touched[entry.extent][n]) if entry.extent in touched else None
    rec["tail_clean"] = True
    parts = []
    for name, a in touched.items():
        if name == "buf" and extent is not None and extent <= a.size:
            rec["tail_clean"] = bool((a[extent:] == U8).all())
            a = a[:extent]
        parts.append(a.tobytes())
    rec["sha256"] = hashlib.sha256(b"".join(parts)).hexdigest() if touched else ""
    if case == "full" and entry.need and rc == 0:
        how, what = entry.need
        arrays = dict((name, a) for name, a, _ in outs)
        arrays.update((name, v) for kind, name, v in entry.args if kind == "in")
        if how == "span":
            need = {"short": int(arrays["pt_off"][N]), "short_span": int(arrays[what][N] - arrays[what][0])}
        else:
            need = {"short": what if how == "const" else int(arrays[what][N])}
    return rec, need


def run_entry(host, entry):
    """{case: record} of one entry point on one host; `short` is cut to the size the full call reported"""
    out, need = {}, None
    for case in entry.cases():
        out[case], need = run_case(host, entry, case, need)
    return out
