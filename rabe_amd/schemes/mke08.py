"""rabe::schemes::mke08 (src/schemes/mke08/mod.rs:130-380) over the host layer."""
import ctypes

from ..hostlib import JSON_POLICY, Obj, batch_decrypt


def setup(host):
    pk, msk = ctypes.c_void_p(), ctypes.c_void_p()
    host.call("rabe_mke08_setup", ctypes.byref(pk), ctypes.byref(msk))
    return Obj("mke08_pk", pk), Obj("mke08_msk", msk)


def keygen(host, pk, msk, name):
    uk = ctypes.c_void_p()
    host.call("rabe_mke08_keygen", pk.ptr, msk.ptr, name.encode("utf-8"), ctypes.byref(uk))
    return Obj("mke08_uk", uk)


def authgen(host, name):
    ska = ctypes.c_void_p()
    host.call("rabe_mke08_authgen", name.encode("utf-8"), ctypes.byref(ska))
    return Obj("mke08_ska", ska)


def request_authority_pk(host, pk, attribute, ska):
    pka = ctypes.c_void_p()
    host.call("rabe_mke08_request_authority_pk", pk.ptr, attribute.encode("utf-8"), ska.ptr, ctypes.byref(pka))
    return Obj("mke08_pka", pka)


def request_authority_sk(host, uk, attribute, ska):
    """the reference returns the Mke08SecretAttributeKey and its callers push it onto `sk.sk_a`; here it is appended"""
    host.call("rabe_mke08_request_authority_sk", uk.ptr, attribute.encode("utf-8"), ska.ptr)


def encrypt(host, pk, attr_pks, policy, language, data):
    arr = (ctypes.c_void_p * max(1, len(attr_pks)))(*[p.ptr for p in attr_pks])
    ct = ctypes.c_void_p()
    host.call("rabe_mke08_encrypt", pk.ptr, arr, ctypes.c_size_t(len(attr_pks)), policy.encode("utf-8"), language, bytes(data),
              ctypes.c_size_t(len(data)), ctypes.byref(ct))
    return Obj("mke08_ct", ct)


def decrypt(host, uk, ct):
    return host.out_bytes("rabe_mke08_decrypt", uk.ptr, ct.ptr)


def decrypt_gt(host, uk, ct):
    return host.out_gt("rabe_mke08_decrypt_gt", uk.ptr, ct.ptr)


def decrypt_batch(host, uks, cts):
    return batch_decrypt(host, "rabe_mke08_decrypt_batch", (), uks, cts)


def decrypt_packed(host, uk, ct_blob, ct_off, out=None, trusted=False):
    """n serialized Mke08Ciphertext records under ONE user key (rabe_mke08_decrypt_packed).
    Returns (pt_blob view, pt_off uint64 [n+1], status int32 [n])."""
    from ..hostlib import packed_decrypt
    return packed_decrypt(host, "rabe_mke08_decrypt_packed", (uk.ptr,), ct_blob, ct_off, out, trusted)


def encrypt_packed(host, pk, attr_pks, policies, item_policy, pt_blob, pt_off, language=JSON_POLICY, out=None):
    """n encryptions in one call (rabe_mke08_encrypt_packed): item i encrypts pt_blob[pt_off[i]:pt_off[i+1]] under
    policies[item_policy[i]] with the public attribute keys attr_pks -> (ct_blob, ct_off), the serialized Mke08Ciphertext records"""
    import numpy as np
    from ..hostlib import _as_u8, packed_produce
    arr = (ctypes.c_void_p * max(1, len(attr_pks)))(*[p.ptr for p in attr_pks])
    return packed_produce(host, "rabe_mke08_encrypt_packed", (pk.ptr, arr, ctypes.c_size_t(len(attr_pks))), policies, item_policy, language,
                          (_as_u8(pt_blob), np.ascontiguousarray(pt_off, dtype=np.uint64)), out)


# ---- key encapsulation (rabe_mke08_kem_encaps / rabe_mke08_kem_decaps): the packed pair without payloads
def encaps_packed(host, pk, attr_pks, policies, item_policy, language=JSON_POLICY, out=None):
    """n headers (Mke08Ciphertext records with an empty sealed part: encrypt_packed's for the same draws minus the nonce) + n 32-byte content
    keys SHA3-256(bytes(msg1 * msg2)).  Returns (hdr_blob view, hdr_off uint64 [n+1], keys uint8 [n, 32])."""
    from ..hostlib import packed_encaps
    arr = (ctypes.c_void_p * max(1, len(attr_pks)))(*[p.ptr for p in attr_pks])
    return packed_encaps(host, "rabe_mke08_kem_encaps", (pk.ptr, arr, ctypes.c_size_t(len(attr_pks))), policies, item_policy, language, out)


def decaps_packed(host, uk, ct_blob, ct_off, trusted=False):
    """the content keys of n records (headers or full ciphertexts) under one user key: key i = SHA3-256(bytes(decrypt_gt(uk, record i))), from
    four Miller loops per item whatever the conjunction's length.  Returns (keys uint8 [n, 32], status int32 [n]); a failed item has status -1
    and 32 zero bytes.  The sealed parts are neither read nor authenticated."""
    from ..hostlib import packed_decaps
    return packed_decaps(host, "rabe_mke08_kem_decaps", (uk.ptr,), ct_blob, ct_off, trusted)


def keygen_packed(host, pk, msk, names, out=None):
    """one user key per name under the master key (rabe_mke08_keygen_packed).  Returns (uk_blob: numpy uint8 view of the Mke08UserKey
    records with an empty sk_a, uk_off: numpy uint64 [n+1])."""
    import numpy as np
    from ..hostlib import _check, _np_ptr, _strs
    n = len(names)
    arr, _ = _strs(list(names))
    off = np.zeros(n + 1, dtype=np.uint64)
    buf = out if out is not None else np.empty(0, dtype=np.uint8)
    for _ in range(2):
        rc = host.lib.rabe_mke08_keygen_packed(host.h, pk.ptr, msk.ptr, arr, ctypes.c_size_t(n), _np_ptr(buf), ctypes.c_size_t(buf.size), _np_ptr(off))
        if rc != 1:
            break
        buf = np.empty(int(off[n]), dtype=np.uint8)
    _check(rc, host.h)
    return buf[:int(off[n])], off


def public_user_key_record(uk_record):
    """the Mke08PublicUserKey record (name | u1 | u2) inside a serialized user key: what a user hands to an authority"""
    rec = bytes(uk_record)
    end = 192 + 4 + int.from_bytes(rec[192:196], "little") + 192
    if len(rec) < 196 or len(rec) < end:
        raise ValueError("not a serialized user key")
    return rec[192:end]


def request_authority_sk_packed(host, ska, attr_sets, item_set, upk_blob, upk_off, trusted=False):
    """the secret attribute keys of attr_sets[item_set[i]] for the public user key record i of upk_blob (rabe_mke08_request_authority_sk_packed).
    Returns (blob view of the records -- u32 count + rows (attribute, au1, au2), the sk_a tail of a user-key record --, off uint64 [n+1],
    status int32 [n]); a failed item has status -1 and an empty slot."""
    import numpy as np
    from ..hostlib import PACKED_TRUSTED, _as_u8, _check, _np_ptr, _strs
    n = len(upk_off) - 1
    arr, _ = _strs([a for s_ in attr_sets for a in s_])
    counts = (ctypes.c_size_t * max(len(attr_sets), 1))(*[len(s_) for s_ in attr_sets])
    it = np.ascontiguousarray(item_set, dtype=np.uint32)
    if len(it) != n:
        raise ValueError("request_authority_sk_packed: one item_set entry per record")
    blob = _as_u8(upk_blob)
    uo = np.ascontiguousarray(upk_off, dtype=np.uint64)
    off = np.zeros(n + 1, dtype=np.uint64)
    status = np.zeros(max(n, 1), dtype=np.int32)
    buf = np.empty(0, dtype=np.uint8)
    for _ in range(2):
        rc = host.lib.rabe_mke08_request_authority_sk_packed(host.h, ska.ptr, arr, counts, ctypes.c_size_t(len(attr_sets)), ctypes.c_size_t(n), _np_ptr(it), _np_ptr(blob),
                            ctypes.c_size_t(blob.size), _np_ptr(uo), ctypes.c_uint32(PACKED_TRUSTED if trusted else 0), _np_ptr(status),
                            _np_ptr(buf), ctypes.c_size_t(buf.size), _np_ptr(off))
        if rc != 1:
            break
        buf = np.empty(int(off[n]), dtype=np.uint8)
    _check(rc, host.h)
    return buf[:int(off[n])], off, status[:n]
