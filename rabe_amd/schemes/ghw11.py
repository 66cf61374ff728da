"""rabe::schemes::ghw11 (src/schemes/ghw11/mod.rs:92-305) over the host layer: CP-ABE with outsourced decryption.
`transform` is the part a server runs (m + 2 pairings per ciphertext), `decrypt_out` the client's one Gt power."""
import ctypes

from ..hostlib import JSON_POLICY, Obj, _strs


def setup(host):
    pk, msk = ctypes.c_void_p(), ctypes.c_void_p()
    host.call("rabe_ghw11_setup", ctypes.byref(pk), ctypes.byref(msk))
    return Obj("ghw11_pk", pk), Obj("ghw11_msk", msk)


def keygen(host, pk, msk, attributes):
    """Option<Ghw11SecretKey>: None for an empty attribute list."""
    arr, n = _strs(attributes)
    sk = ctypes.c_void_p()
    if host.call("rabe_ghw11_keygen", pk.ptr, msk.ptr, arr, n, ctypes.byref(sk)) is None:
        return None
    return Obj("ghw11_sk", sk)


def tkgen(host, sk):
    tk, rk = ctypes.c_void_p(), ctypes.c_void_p()
    host.call("rabe_ghw11_tkgen", sk.ptr, ctypes.byref(tk), ctypes.byref(rk))
    return Obj("ghw11_tk", tk), Obj("ghw11_rk", rk)


def encrypt(host, pk, policy, language, plaintext):
    ct = ctypes.c_void_p()
    host.call("rabe_ghw11_encrypt", pk.ptr, policy.encode("utf-8"), language, bytes(plaintext), ctypes.c_size_t(len(plaintext)), ctypes.byref(ct))
    return Obj("ghw11_ct", ct)


def transform(host, ct, tk):
    out = ctypes.c_void_p()
    host.call("rabe_ghw11_transform", ct.ptr, tk.ptr, ctypes.byref(out))
    return Obj("ghw11_tct", out)


def transform_batch(host, cts, tks):
    """n independent transforms in one launch set; None where the transform key does not satisfy the ciphertext's policy."""
    n = len(cts)
    a = (ctypes.c_void_p * max(1, n))(*[c.ptr for c in cts])
    b = (ctypes.c_void_p * max(1, n))(*[t.ptr for t in tks])
    status = (ctypes.c_int32 * max(1, n))()
    out = (ctypes.c_void_p * max(1, n))()
    host.call("rabe_ghw11_transform_batch", ctypes.c_size_t(n), a, b, status, out)
    return [Obj("ghw11_tct", ctypes.c_void_p(out[i])) if status[i] == 0 else None for i in range(n)]


def decrypt_out(host, tct, rk, ct):
    """`ct` supplies the symmetric data field (the reference passes it as a separate Vec<u8>)."""
    return host.out_bytes("rabe_ghw11_decrypt_out", tct.ptr, rk.ptr, ct.ptr)


def decrypt_out_gt(host, tct, rk):
    return host.out_gt("rabe_ghw11_decrypt_out_gt", tct.ptr, rk.ptr)


def decrypt(host, sk, ct):
    """The key holder's own decrypt, no proxy (rabe_ghw11_decrypt): what decrypt_out(transform(ct, tk), rk, ct) gives for any (tk, rk) =
    tkgen(sk), without z, the G2 multiplications or the Gt power."""
    return host.out_bytes("rabe_ghw11_decrypt", sk.ptr, ct.ptr)


def decrypt_gt(host, sk, ct):
    """c * t_1^-1, t_1 = transform's expression on the secret key's own elements (rabe_ghw11_decrypt_gt)."""
    return host.out_gt("rabe_ghw11_decrypt_gt", sk.ptr, ct.ptr)


def decrypt_packed(host, sk, ct_blob, ct_off, out=None, trusted=False):
    """n ciphertext records under one secret key of the holder's own (rabe_ghw11_decrypt_packed): by definition the result of tkgen ->
    transform_packed -> decrypt_out_packed for any z.  Returns (pt_blob view, pt_off uint64 [n+1], status int32 [n]); a failed item has
    status -1 and an empty plaintext slot."""
    from ..hostlib import packed_decrypt
    return packed_decrypt(host, "rabe_ghw11_decrypt_packed", (sk.ptr,), ct_blob, ct_off, out, trusted)


def transform_packed(host, tk, ct_blob, ct_off, trusted=False):
    """n transforms under one transform key over a blob of serialized ciphertexts (rabe_ghw11_transform_packed).
    Returns (tct: numpy uint8 [n, 768] -- row i = the Ghw11TransformCiphertext record c | t --, status: numpy int32 [n])."""
    import numpy as np
    from ..hostlib import PACKED_TRUSTED, _as_u8, _np_ptr
    n = len(ct_off) - 1
    ct = _as_u8(ct_blob)
    co = np.ascontiguousarray(ct_off, dtype=np.uint64)
    out = np.zeros((max(n, 1), 768), dtype=np.uint8)
    status = np.zeros(max(n, 1), dtype=np.int32)
    host.call("rabe_ghw11_transform_packed", tk.ptr, ctypes.c_size_t(n), _np_ptr(ct), ctypes.c_size_t(ct.size), _np_ptr(co),
              ctypes.c_uint32(PACKED_TRUSTED if trusted else 0), _np_ptr(status), _np_ptr(out), ctypes.c_size_t(out.size))
    return out[:n], status[:n]


class TkStore:
    """A proxy's transform keys, resident on the device (rabe_ghw11_tk_store_create, or tk_store_open for an empty one).  key_status: numpy
    int32 [n_keys] of the creating call, -1 where a key's record was refused.  add / revoke change the store in place; the calls on one store
    run one at a time.  free() -- or closing the host, or the garbage collector -- releases the device memory."""

    def __init__(self, host, ptr, key_status):
        import weakref
        self.host, self.ptr, self.key_status = host, ptr, key_status
        if not hasattr(host, "_stores"):
            host._stores = weakref.WeakSet()
        host._stores.add(self)

    def nbytes(self):
        """device memory held, over all engines that have prepared the store's lines (rabe_ghw11_tk_store_bytes)"""
        self.host.lib.rabe_ghw11_tk_store_bytes.restype = ctypes.c_uint64
        return int(self.host.lib.rabe_ghw11_tk_store_bytes(self.ptr))

    def add(self, tk_blob, tk_off, trusted=False):
        """more keys, in place (rabe_ghw11_tk_store_add): records as tk_store_create takes them.  Returns (ids: numpy uint32 [n] -- what
        item_key names, 0xFFFFFFFF where the key was refused --, status: numpy int32 [n]), or None when the well-formed keys do not all find
        room: nothing was added then."""
        import numpy as np
        from ..hostlib import PACKED_TRUSTED, _as_u8, _np_ptr
        n = len(tk_off) - 1
        tk = _as_u8(tk_blob)
        to = np.ascontiguousarray(tk_off, dtype=np.uint64)
        status = np.zeros(max(n, 1), dtype=np.int32)
        ids = np.zeros(max(n, 1), dtype=np.uint32)
        if self.host.call("rabe_ghw11_tk_store_add", self.ptr, ctypes.c_size_t(n), _np_ptr(tk), ctypes.c_size_t(tk.size), _np_ptr(to),
                          ctypes.c_uint32(PACKED_TRUSTED if trusted else 0), _np_ptr(status), _np_ptr(ids)) is None:
            return None
        return ids[:n], status[:n]

    def revoke(self, ids):
        """keys out, in place (rabe_ghw11_tk_store_revoke): their lines are zeroed on every device before this returns.  Returns status:
        numpy int32 [n], -1 for an id that was never issued, failed or is revoked already."""
        import numpy as np
        from ..hostlib import _np_ptr
        ki = np.ascontiguousarray(ids, dtype=np.uint32)
        status = np.zeros(max(ki.size, 1), dtype=np.int32)
        self.host.call("rabe_ghw11_tk_store_revoke", self.ptr, ctypes.c_size_t(ki.size), _np_ptr(ki), _np_ptr(status))
        return status[:ki.size]

    def stat(self):
        """(live keys, capacity in blocks, blocks in use, largest free contiguous range) (rabe_ghw11_tk_store_stat)"""
        out = (ctypes.c_uint64 * 4)()
        if self.host.lib.rabe_ghw11_tk_store_stat(self.ptr, out) != 0:
            raise ValueError("tk store: freed")
        return tuple(int(v) for v in out)

    def free(self):
        if self.ptr and self.host.h:
            from ..hostlib import KINDS
            self.host.lib.rabe_obj_free(KINDS["ghw11_tk_store"], self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def tk_store_create(host, tk_blob, tk_off, trusted=False):
    """the transform keys of many users -- the Ghw11TransformKey records tkgen_packed / provision_packed write -- uploaded once, with ONE set
    of prepared lines over all their elements (rabe_ghw11_tk_store_create).  Returns a TkStore."""
    import numpy as np
    from ..hostlib import PACKED_TRUSTED, _as_u8, _np_ptr
    n = len(tk_off) - 1
    tk = _as_u8(tk_blob)
    to = np.ascontiguousarray(tk_off, dtype=np.uint64)
    status = np.zeros(max(n, 1), dtype=np.int32)
    store = ctypes.c_void_p()
    host.call("rabe_ghw11_tk_store_create", ctypes.c_size_t(n), _np_ptr(tk), ctypes.c_size_t(tk.size), _np_ptr(to),
              ctypes.c_uint32(PACKED_TRUSTED if trusted else 0), _np_ptr(status), ctypes.byref(store))
    return TkStore(host, store, status[:n])


def tk_store_open(host, capacity_blocks):
    """an empty store with room for capacity_blocks blocks (rabe_ghw11_tk_store_open): a key of a attributes takes a + 2 contiguous blocks.
    Keys come and go with TkStore.add / TkStore.revoke.  Returns a TkStore."""
    import numpy as np
    store = ctypes.c_void_p()
    host.call("rabe_ghw11_tk_store_open", ctypes.c_uint64(capacity_blocks), ctypes.byref(store))
    return TkStore(host, store, np.zeros(0, dtype=np.int32))


def transform_keyed(host, store, item_key, ct_blob, ct_off, trusted=False):
    """a mixed queue in one call (rabe_ghw11_transform_keyed): record i is transformed under key item_key[i] of the store -- by definition what
    transform_packed gives for that record alone under that key.  Returns (tct: numpy uint8 [n, 768], status: numpy int32 [n])."""
    import numpy as np
    from ..hostlib import PACKED_TRUSTED, _as_u8, _np_ptr
    n = len(ct_off) - 1
    if len(item_key) != n:
        raise ValueError("transform_keyed: %d item keys for %d records" % (len(item_key), n))
    ct = _as_u8(ct_blob)
    co = np.ascontiguousarray(ct_off, dtype=np.uint64)
    ik = np.ascontiguousarray(item_key, dtype=np.uint32)
    out = np.zeros((max(n, 1), 768), dtype=np.uint8)
    status = np.zeros(max(n, 1), dtype=np.int32)
    host.call("rabe_ghw11_transform_keyed", store.ptr, ctypes.c_size_t(n), _np_ptr(ik), _np_ptr(ct), ctypes.c_size_t(ct.size), _np_ptr(co),
              ctypes.c_uint32(PACKED_TRUSTED if trusted else 0), _np_ptr(status), _np_ptr(out), ctypes.c_size_t(out.size))
    return out[:n], status[:n]


def encrypt_packed(host, pk, policies, item_policy, pt_blob, pt_off, language=JSON_POLICY, out=None):
    """n encryptions in one call (rabe_ghw11_encrypt_packed): policies are distinct texts, item_policy[i] indexes them, plaintext
    i = pt_blob[pt_off[i]:pt_off[i+1]] -> (ct_blob, ct_off), the serialized Ghw11Ciphertext records"""
    import numpy as np
    from ..hostlib import _as_u8, packed_produce
    return packed_produce(host, "rabe_ghw11_encrypt_packed", (pk.ptr,), policies, item_policy, language,
                          (_as_u8(pt_blob), np.ascontiguousarray(pt_off, dtype=np.uint64)), out)


def decrypt_out_packed(host, rk, tct, ct_blob, ct_off, trusted=False):
    """n decrypt_out calls under one retrieve key (rabe_ghw11_decrypt_out_packed).  `tct`: the [n, 768] array transform_packed returns
    (or its bytes), `ct_blob` / `ct_off`: the ciphertext records, which carry the sealed data.  Returns (pt_blob view, pt_off uint64 [n+1],
    status int32 [n]); a failed item has status -1 and an empty or zeroed plaintext slot."""
    import numpy as np
    from ..hostlib import PACKED_TRUSTED, _as_u8, _np_ptr
    n = len(ct_off) - 1
    t = np.ascontiguousarray(_as_u8(tct) if not isinstance(tct, np.ndarray) else tct, dtype=np.uint8).reshape(-1)
    if t.size < 768 * n:
        raise ValueError("decrypt_out_packed: tct holds %d bytes, %d items need %d" % (t.size, n, 768 * n))
    ct = _as_u8(ct_blob)
    co = np.ascontiguousarray(ct_off, dtype=np.uint64)
    po = np.zeros(n + 1, dtype=np.uint64)
    status = np.zeros(max(n, 1), dtype=np.int32)
    lo, hi = co[:-1], co[1:]
    okm = (lo <= hi) & (hi <= ct.size)
    need = int((hi[okm] - lo[okm]).sum()) if n else 0
    buf = np.empty(max(need, 1), dtype=np.uint8)
    host.call("rabe_ghw11_decrypt_out_packed", rk.ptr, ctypes.c_size_t(n), _np_ptr(t), _np_ptr(ct), ctypes.c_size_t(ct.size), _np_ptr(co),
              ctypes.c_uint32(PACKED_TRUSTED if trusted else 0), _np_ptr(status), _np_ptr(buf), ctypes.c_size_t(buf.size), _np_ptr(po))
    return buf[:int(po[n])], po, status[:n]


# ---- key encapsulation (rabe_ghw11_{encaps,decaps_out,decaps}_packed): the packed service without payloads
def encaps_packed(host, pk, policies, item_policy, language=JSON_POLICY, out=None):
    """n key encapsulations (rabe_ghw11_encaps_packed): header i is the Ghw11Ciphertext record encrypt_packed writes for the same draws
    with an empty sealed part; transform_packed takes the headers as they are.  Returns (hdr_blob, hdr_off uint64 [n+1], keys uint8 [n, 32])."""
    from ..hostlib import packed_encaps
    return packed_encaps(host, "rabe_ghw11_encaps_packed", (pk.ptr,), policies, item_policy, language, out)


def decaps_out_packed(host, rk, tct, trusted=False):
    """the thin client's half (rabe_ghw11_decaps_out_packed): `tct` = the [n, 768] array transform_packed returns (or its bytes) and nothing
    else -- no ciphertext blob.  Row i of the result = SHA3-256(bytes(c_i * t_i^-z)): the KDF of decrypt_out_gt.  Returns (keys uint8
    [n, 32] -- zeros where status is -1 --, status int32 [n]).  With trusted=True a non-member's key is unspecified."""
    import numpy as np
    from ..hostlib import PACKED_TRUSTED, _as_u8, _np_ptr
    t = np.ascontiguousarray(_as_u8(tct) if not isinstance(tct, np.ndarray) else tct, dtype=np.uint8).reshape(-1)
    if t.size % 768:
        raise ValueError("decaps_out_packed: tct holds %d bytes, not a whole number of 768-byte records" % t.size)
    n = t.size // 768
    status = np.zeros(max(n, 1), dtype=np.int32)
    keys = np.full((max(n, 1), 32), 0xEE, dtype=np.uint8)
    host.call("rabe_ghw11_decaps_out_packed", rk.ptr, ctypes.c_size_t(n), _np_ptr(t), ctypes.c_uint32(PACKED_TRUSTED if trusted else 0),
              _np_ptr(status), _np_ptr(keys))
    return keys[:n], status[:n]


def decaps_packed(host, sk, ct_blob, ct_off, trusted=False):
    """the key holder's own decapsulation, no proxy (rabe_ghw11_decaps_packed): headers from encaps_packed or full records from
    encrypt_packed; the sealed part is skipped, never read.  Returns (keys uint8 [n, 32] -- zeros where status is -1 --, status int32 [n])."""
    from ..hostlib import packed_decaps
    return packed_decaps(host, "rabe_ghw11_decaps_packed", (sk.ptr,), ct_blob, ct_off, trusted)


def keygen_packed(host, pk, msk, attr_sets, item_set, out=None):
    """n keys under one master key (rabe_ghw11_keygen_packed): attr_sets = distinct attribute lists, item_set[i] indexes them.
    Returns (sk_blob: numpy uint8 view of the Ghw11SecretKey records, sk_off: numpy uint64 [n+1])."""
    import numpy as np
    from ..hostlib import _check, _np_ptr
    n = len(item_set)
    arr, _ = _strs([a for s_ in attr_sets for a in s_])
    counts = (ctypes.c_size_t * max(len(attr_sets), 1))(*[len(s_) for s_ in attr_sets])
    it = np.ascontiguousarray(item_set, dtype=np.uint32)
    so = np.zeros(n + 1, dtype=np.uint64)
    buf = out if out is not None else np.empty(0, dtype=np.uint8)
    for _ in range(2):
        rc = host.lib.rabe_ghw11_keygen_packed(host.h, pk.ptr, msk.ptr, arr, counts, ctypes.c_size_t(len(attr_sets)), ctypes.c_size_t(n), _np_ptr(it),
                                               _np_ptr(buf), ctypes.c_size_t(buf.size), _np_ptr(so))
        if rc != 1:
            break
        buf = np.empty(int(so[n]), dtype=np.uint8)
    _check(rc, host.h)
    return buf[:int(so[n])], so


def tkgen_packed(host, sk_blob, sk_off, trusted=False):
    """n tkgen calls, one per Ghw11SecretKey record of sk_blob (rabe_ghw11_tkgen_packed).  Returns (tk_blob view of the Ghw11TransformKey
    records, tk_off uint64 [n+1], rk: numpy uint8 [n, 32] -- row i = the Ghw11RetrieveKey record z --, status int32 [n]); a failed item has
    status -1, an empty tk slot and a zero rk row."""
    import numpy as np
    from ..hostlib import PACKED_TRUSTED, _as_u8, _np_ptr
    n = len(sk_off) - 1
    sk = _as_u8(sk_blob)
    so = np.ascontiguousarray(sk_off, dtype=np.uint64)
    to = np.zeros(n + 1, dtype=np.uint64)
    rk = np.zeros((max(n, 1), 32), dtype=np.uint8)
    status = np.zeros(max(n, 1), dtype=np.int32)
    lo, hi = so[:-1], so[1:]
    okm = (lo <= hi) & (hi <= sk.size)
    need = int((hi[okm] - lo[okm]).sum()) if n else 0
    buf = np.empty(max(need, 1), dtype=np.uint8)
    host.call("rabe_ghw11_tkgen_packed", ctypes.c_size_t(n), _np_ptr(sk), ctypes.c_size_t(sk.size), _np_ptr(so),
              ctypes.c_uint32(PACKED_TRUSTED if trusted else 0), _np_ptr(status), _np_ptr(buf), ctypes.c_size_t(buf.size), _np_ptr(to), _np_ptr(rk))
    return buf[:int(to[n])], to, rk[:n], status[:n]


def provision_packed(host, pk, msk, sets, item_set, want_sk=True):
    """n users and their proxies provisioned in one call (rabe_ghw11_provision_packed): by definition keygen_packed followed by tkgen_packed
    on its output -- draws r_0 .. r_{n-1}, then z_0 .. z_{n-1} -- for an authority that issues both, so every element is a fixed-base
    multiple and nothing leaves the device in between.  sets = distinct attribute lists, item_set[i] indexes them.  Returns (sk_blob, sk_off,
    tk_blob, tk_off, rk): the Ghw11SecretKey records (None, None with want_sk=False: not computed, same draws), the Ghw11TransformKey
    records, and rk: numpy uint8 [n, 32], row i = the Ghw11RetrieveKey record z_i.  An empty attribute list or an item_set out of range is
    refused here, before the device is touched."""
    import numpy as np
    from ..hostlib import _check, _np_ptr
    sets = [list(s_) for s_ in sets]
    for s_ in sets:
        if not s_:
            raise ValueError("provision_packed: an empty attribute list (ghw11::keygen returns None for it)")
    n = len(item_set)
    if any(not 0 <= int(s_) < len(sets) for s_ in item_set):
        raise ValueError("provision_packed: item_set out of range")
    arr, _ = _strs([a for s_ in sets for a in s_])
    counts = (ctypes.c_size_t * max(len(sets), 1))(*[len(s_) for s_ in sets])
    it = np.ascontiguousarray(item_set, dtype=np.uint32)
    so = np.zeros(n + 1, dtype=np.uint64) if want_sk else None
    to = np.zeros(n + 1, dtype=np.uint64)
    rk = np.zeros((max(n, 1), 32), dtype=np.uint8)
    sk_buf = tk_buf = np.empty(0, dtype=np.uint8)
    for _ in range(2):
        rc = host.lib.rabe_ghw11_provision_packed(host.h, pk.ptr, msk.ptr, arr, counts, ctypes.c_size_t(len(sets)), ctypes.c_size_t(n), _np_ptr(it),
                                                  _np_ptr(sk_buf), ctypes.c_size_t(sk_buf.size), _np_ptr(so) if want_sk else None,
                                                  _np_ptr(tk_buf), ctypes.c_size_t(tk_buf.size), _np_ptr(to), _np_ptr(rk))
        if rc != 1:
            break
        tk_buf = np.empty(int(to[n]), dtype=np.uint8)
        if want_sk:
            sk_buf = np.empty(int(so[n]), dtype=np.uint8)
    _check(rc, host.h)
    if not want_sk:
        return None, None, tk_buf[:int(to[n])], to, rk[:n]
    return sk_buf[:int(so[n])], so, tk_buf[:int(to[n])], to, rk[:n]
