"""GPU checks of BDABE and MKE08 as a key encapsulation (include/rabe_host.h: rabe_{bdabe,mke08}_kem_{encaps,decaps}), in the form of
tests/test_gpu_aw11_kem.py.  The references are calls that exist: encrypt_packed on the same tape for the headers, decrypt_gt -- the general
pairing-job path, m + 3 Miller loops -- plus hashlib's SHA3-256 for EVERY key, the Python oracle's msg for three of them, decrypt_packed for the
statuses.  70 items (one 64-lane wave and a ragged tail), two authorities, three policies:
  P0  A0                                                       one attribute
  P1  (A1 and A2) or A3                                        the key holds A1, A2 and not A3
  P2  (A9 and A10 and A11) or (A4 and A5 and A6 and A7 and A8) the key lacks A4 of the five and holds the three
The conjunction LISTS of a record are what the reference's json_to_dnf makes of the text -- P1: [A3], [A1, A2]; P2: [A4], [A9, A10, A11],
[A5 .. A8] -- so under this key the chosen conjunction of P1 and of P2 is the record's second, of two and of three attributes, behind a first
one the key cannot satisfy.  A second user key holds A0 only.

What the launch record can show (kernel names and launch counts, nothing else): a decaps launches k_dnf_dec_pairs once and none of
rhip_pairing_jobs' kernels, and no seal / open kernel.  That the Miller stage then sees four pairs per live item -- two of them walked -- is
asserted where the pair lists are visible: tests/test_gpu_dnf_one_uk.py reads the walk counters of the same entry point.

Stated here, not recorded from the code: a null `status` or `key_buf` in decaps with n_items > 0 is REFUSED (-1, "null input"), exactly as
rabe_ac17_cp_decaps_packed refuses it: decaps_shape hands the uncut call to the host's own engine whenever one of (ct_off, status, key_buf) is
missing, and the scheme function throws.  With n_items = 0 nothing is written and the call returns 0."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

from rabe_amd import hostlib as hl
from tests.test_gpu_dnf_packed import Scheme, offsets, policy, records

pytestmark = pytest.mark.gpu
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
N = 70
A = ["aa%d::A%d" % (1 + i % 2, i) for i in range(12)]
TERMS = [[[A[0]]], [[A[1], A[2]], [A[3]]], [[A[9], A[10], A[11]], [A[4], A[5], A[6], A[7], A[8]]]]
POLICIES = [policy(t, hl.JSON_POLICY) for t in TERMS]
LISTS = [[[A[0]]], [[A[3]], [A[1], A[2]]], [[A[4]], [A[9], A[10], A[11]], [A[5], A[6], A[7], A[8]]]]          # json_to_dnf's conjunctions
CHOSEN = [0, 1, 1]
KEY_ATTRS = [A[0], A[1], A[2]] + A[5:12]
DUP_POLICY = policy([[A[1], A[1]]], hl.JSON_POLICY)          # one conjunction that names A1 twice
SEAL_KERNELS = ("k_sym_setup", "k_sym_ctr", "k_sym_ghash_seg", "k_sym_tag")
JOBS_KERNELS = ("k_jobs_pairs", "k_cpair_off", "k_g1_to_mont", "k_naf_masks")
NO_MATCH = "attributes in sk do not match policy in ct"
SCHEMES = ["bdabe", "mke08"]


def kdf(gt):
    """the reference's kdf (src/utils/aes/mod.rs:47-55) on the 384 wire bytes of a Gt: its 12 coefficients as 32 big-endian bytes each"""
    assert len(gt) == 384
    return hashlib.sha3_256(b"".join(gt[32 * i:32 * i + 32][::-1] for i in range(12))).digest()


def neg_fp(b):
    v = int.from_bytes(b, "little")
    return ((P - v) % P).to_bytes(32, "little")


def neg_g1(b):
    return b[:32] + neg_fp(b[32:64])


def neg_g2(b):
    return b[:64] + neg_fp(b[64:96]) + neg_fp(b[96:128])


def conj_offsets(rec, n_gt):
    """per conjunction of a ciphertext record: (names, offset of its first Gt element); then the offset of the sealed part's length field"""
    at = 4 + int.from_bytes(rec[:4], "little") + 1
    n_conj = int.from_bytes(rec[at:at + 4], "little")
    at += 4
    out = []
    for _ in range(n_conj):
        na = int.from_bytes(rec[at:at + 4], "little")
        at += 4
        names = []
        for _ in range(na):
            l = int.from_bytes(rec[at:at + 4], "little")
            names.append((at + 4, rec[at + 4:at + 4 + l].decode()))
            at += 4 + l
        out.append((names, at))
        at += 384 * n_gt + 384
    return out, at


def join(recs):
    return np.frombuffer(b"".join(recs), dtype=np.uint8), offsets(recs)


@pytest.fixture(scope="module")
def host():
    h = hl.Host(0)
    yield h
    h.close()


@pytest.fixture(scope="module", params=SCHEMES)
def kem(request, host):
    """one encaps of 70 items on a tape, the full records for the same draws, and decrypt_gt of every full record: shared, nobody changes them"""
    s = Scheme(request.param)
    pk, msk, ska = s.setup(host, ("aa1", "aa2"))
    pkas = [s.attr_pk(host, pk, ska, a) for a in A]
    uk = s.user_key(host, pk, msk, ska, KEY_ATTRS)
    uk_b = s.user_key(host, pk, msk, ska, [A[0]])          # satisfies the one-attribute policy only
    assert [hl.policy_dnf_terms(p, A, hl.JSON_POLICY) for p in POLICIES] == LISTS
    rnd = random.Random(0x646E666B + s.n_gt)
    item_pol = [i % 3 for i in range(N)]
    draws = [[rnd.randrange(1, R) for _ in range(s.lead + len(LISTS[item_pol[i]]))] for i in range(N)]
    nonces = [rnd.randrange(1, R) for _ in range(N)]
    tape = [v for d in draws for v in d]
    host.set_tape(tape)
    hdr, hdr_off, keys = s.mod.encaps_packed(host, pk, pkas, POLICIES, item_pol)
    pts = [b"sixteen byte pt!"] * N
    host.set_tape([v for d, nonce in zip(draws, nonces) for v in d + [nonce]])
    blob, off = s.mod.encrypt_packed(host, pk, pkas, POLICIES, item_pol, b"".join(pts), offsets(pts))
    host.clear_tape()
    recs = records(blob, off)
    gts = [s.mod.decrypt_gt(host, uk, hl.Obj.deserialize(s.ct_kind(), r)) for r in recs]
    return {"s": s, "pk": pk, "pkas": pkas, "uk": uk, "uk_b": uk_b, "item_pol": item_pol, "draws": draws, "tape": tape, "hdr": hdr.copy(),
            "hdr_off": hdr_off, "hdrs": records(hdr, hdr_off), "keys": keys.copy(), "blob": blob.copy(), "off": off, "recs": recs, "gts": gts}


def test_headers_are_encrypt_packed_records_without_a_sealed_part(kem):
    assert len(kem["recs"]) == len(kem["hdrs"]) == N
    for i in range(N):
        assert kem["hdrs"][i] == kem["recs"][i][:-(4 + 16 + 28)] + bytes(4), i          # the record up to its length field, which is 0; nothing follows
        assert [t[0] for t in kem["s"].tuples(kem["hdrs"][i])] == LISTS[kem["item_pol"][i]]


def test_encaps_keys_are_the_kdf_of_decrypt_gt(kem):
    for i in range(N):
        assert bytes(kem["keys"][i]) == kdf(kem["gts"][i]), i


def test_encaps_keys_are_sha3_of_the_oracles_msg(kem):
    from oracle import bn254 as bn
    from oracle import policy as pol
    from oracle import schemes as sch
    from oracle.tape import ListRng
    s = kem["s"]
    pk = hl.parse_obj(s.name + "_pk", kem["pk"].serialize())
    o_pk = {"p1": bn.g1_from_le(pk["p1"]), "p2": bn.g2_from_le(pk["p2"])}
    k = hl.parse_obj(s.name + "_pka", kem["pkas"][0].serialize())          # P0 names A0 alone
    if s.name == "bdabe":
        o_k = {"attr": k["attr"], "a1": bn.g1_from_le(k["a1"]), "a2": bn.g2_from_le(k["a2"]), "a3": bn.gt_from_le(k["a3"])}
    else:
        o_k = {"attr": k["attr"], "g1": bn.g1_from_le(k["g1"]), "g2": bn.g2_from_le(k["g2"]), "gt1": bn.gt_from_le(k["gt1"]), "gt2": bn.gt_from_le(k["gt2"])}
    enc = sch.bdabe_encrypt if s.name == "bdabe" else sch.mke08_encrypt
    for i in (0, 3, 69):
        assert kem["item_pol"][i] == 0
        _ct, msg = enc(o_pk, [o_k], POLICIES[0], pol.JSON, ListRng(kem["draws"][i]))
        assert bytes(kem["keys"][i]) == kdf(bn.gt_to_le(msg)), i


def test_decaps_keys_from_headers_and_from_full_records(host, kem):
    s = kem["s"]
    for trusted in (False, True):
        k_h, st_h = s.mod.decaps_packed(host, kem["uk"], kem["hdr"], kem["hdr_off"], trusted)
        k_f, st_f = s.mod.decaps_packed(host, kem["uk"], kem["blob"], kem["off"], trusted)
        assert (st_h == 0).all() and (st_f == 0).all()
        assert (k_h == k_f).all() and (k_h == kem["keys"]).all()
        for i in range(N):
            assert bytes(k_f[i]) == kdf(kem["gts"][i]), i          # the general pairing-job path is the reference


def test_a_key_that_lacks_the_attributes_fails_those_items_only(host, kem):
    s = kem["s"]
    keys, status = s.mod.decaps_packed(host, kem["uk_b"], kem["hdr"], kem["hdr_off"])
    msg = host.lib.rabe_host_last_error(host.h).decode()
    assert NO_MATCH in msg, msg
    for i in range(N):
        if kem["item_pol"][i] == 0:
            gt = s.mod.decrypt_gt(host, kem["uk_b"], hl.Obj.deserialize(s.ct_kind(), kem["recs"][i])) if i < 9 else None
            assert status[i] == 0 and bytes(keys[i]) == bytes(kem["keys"][i]) and (gt is None or bytes(keys[i]) == kdf(gt)), i
        else:
            assert status[i] == -1 and bytes(keys[i]) == bytes(32), i


def test_untrusted_input_fails_item_by_item(host, kem):
    from oracle import bn254 as bn
    from tests.test_gpu_ghw11_keys_packed import twist_point_outside_g2
    s = kem["s"]
    outside = bn.g2_to_le(twist_point_outside_g2())
    recs = list(kem["recs"][:12])
    g = 384 * s.n_gt          # a conjunction's elements: Gt element(s) | G1 G2 G1 G2

    def put(i, conj, at, data):
        r = bytearray(recs[i])
        base = conj_offsets(recs[i], s.n_gt)[0][conj][1]
        r[base + at:base + at + len(data)] = data
        recs[i] = bytes(r)
    recs[1] = recs[1][:-7]                                         # cut short
    recs[2] = recs[2] + b"\x00\x01\x02"                            # trailing bytes
    x = int.from_bytes(recs[3][conj_offsets(recs[3], s.n_gt)[0][0][1] + g:][:32], "little")
    put(3, 0, g, ((x + 1) % P).to_bytes(32, "little"))             # e2 off the curve
    put(4, CHOSEN[kem["item_pol"][4]], g + 64, outside)            # e3 of the chosen conjunction: WALKED
    put(5, 0, g + 64, outside)                                     # P2's first conjunction is not the chosen one
    assert kem["item_pol"][5] == 2 and kem["item_pol"][6] == 0
    at, name = conj_offsets(recs[6], s.n_gt)[0][0][0][0]
    r = bytearray(recs[6])
    r[at:at + len(name)] = name.replace("A0", "Z0").encode()       # the lists satisfy nothing although the policy text does
    recs[6] = bytes(r)
    blob, off = join(recs)
    off = off.copy()
    bad_off = off.copy()
    bad_off[9] = blob.size + 40                                    # record 8 ends, and record 9 starts, outside the blob
    bad = {1, 2, 3, 4, 5, 6}
    keys, status = s.mod.decaps_packed(host, kem["uk"], blob, off)
    for i in range(12):
        assert status[i] == (-1 if i in bad else 0), i
        assert bytes(keys[i]) == (bytes(32) if i in bad else bytes(kem["keys"][i])), i
    _pt, _po, st_dec = s.mod.decrypt_packed(host, kem["uk"], blob, off)
    # decrypt_packed fails the same items -- record 6 at its tag -- with ONE exception the KEM's rule names: its decoder stops at the sealed
    # part's end and does not look for trailing bytes, which the KEM refuses as every other record reader of packed.cpp does
    assert [int(x) for x in st_dec] == [(-1 if i in bad - {2} else 0) for i in range(12)]
    keys, status = s.mod.decaps_packed(host, kem["uk"], blob, bad_off)
    for i in range(12):
        assert status[i] == (-1 if i in bad | {8, 9} else 0), i
        assert bytes(keys[i]) == (bytes(32) if i in bad | {8, 9} else bytes(kem["keys"][i])), i
    # the stated difference, alone: its own message, where decrypt_gt hands out Gt::one()
    b6, o6 = join([recs[6]])
    keys, status = s.mod.decaps_packed(host, kem["uk"], b6, o6)
    assert status[0] == -1 and bytes(keys[0]) == bytes(32)
    assert "none of its conjunction lists" in host.lib.rabe_host_last_error(host.h).decode()
    one = s.mod.decrypt_gt(host, kem["uk"], hl.Obj.deserialize(s.ct_kind(), recs[6]))
    assert one == bn.gt_to_le(bn.GT_ONE)


def test_degenerate_sums_and_a_duplicated_name(host, kem):
    s = kem["s"]
    # a user key whose rows for A1 and A2 are negatives of each other: S1 = S2 = O for the class [A1, A2]
    raw = bytearray(kem["uk"].serialize())
    at = 64 + 128                                                            # sk.u1, sk.u2
    at += 4 + int.from_bytes(raw[at:at + 4], "little") + 64 + 128          # the name, pk.u1, pk.u2
    count, rows = int.from_bytes(raw[at:at + 4], "little"), {}
    at += 4
    for _ in range(count):                                                   # name, au1, au2
        l = int.from_bytes(raw[at:at + 4], "little")
        rows[bytes(raw[at + 4:at + 4 + l]).decode()] = at + 4 + l
        at += 4 + l + 192
    assert at == len(raw) and list(rows) == KEY_ATTRS
    a, b = rows[A[1]], rows[A[2]]
    raw[b:b + 64] = neg_g1(bytes(raw[a:a + 64]))
    raw[b + 64:b + 192] = neg_g2(bytes(raw[a + 64:a + 192]))
    uk_deg = hl.Obj.deserialize(s.name + "_uk", bytes(raw))
    idx = [i for i in range(N) if kem["item_pol"][i] == 1][:3] + [0]
    blob, off = join([kem["recs"][i] for i in idx])
    keys, status = s.mod.decaps_packed(host, uk_deg, blob, off)
    assert (status == 0).all()
    for t, i in enumerate(idx):
        gt = s.mod.decrypt_gt(host, uk_deg, hl.Obj.deserialize(s.ct_kind(), kem["recs"][i]))
        assert bytes(keys[t]) == kdf(gt), i
        assert (bytes(keys[t]) == bytes(kem["keys"][i])) == (i == 0)          # the cancelled rows change the element; the one-attribute item is untouched
    # a class with a duplicated name: the row is summed twice, as decrypt_gt's plan does
    hdr, hdr_off, k_enc = s.mod.encaps_packed(host, kem["pk"], kem["pkas"], [DUP_POLICY, POLICIES[0]], [0, 1, 0])
    assert [t[0] for t in s.tuples(records(hdr, hdr_off)[0])] == [[A[1], A[1]]]
    keys, status = s.mod.decaps_packed(host, kem["uk"], hdr, hdr_off)
    assert (status == 0).all() and (keys == k_enc).all()


def test_launch_records(host, kem):
    s = kem["s"]
    host.kernel_timing(True)
    try:
        host.kernel_launches()
        s.mod.encaps_packed(host, kem["pk"], kem["pkas"], POLICIES, kem["item_pol"])
        seen = host.kernel_launches()
        assert not [k for k in SEAL_KERNELS if k in seen], seen
        assert seen.get("k_sym_kdf") == 1 and seen.get("k_assemble_records") == 1 and "k_sym_kdf_rows" not in seen, seen
        assert all(k in seen for k in ("k_dnf_enc_g1", "k_dnf_enc_g2", "k_dnf_enc_gt")), seen
        for b, o in ((kem["hdr"], kem["hdr_off"]), (kem["blob"], kem["off"])):
            s.mod.decaps_packed(host, kem["uk"], b, o)
            seen = host.kernel_launches()
            assert not [k for k in SEAL_KERNELS + JOBS_KERNELS if k in seen], seen
            assert seen.get("k_dnf_dec_pairs") == 1 and seen.get("k_sym_kdf_rows") == 1 and "k_sym_kdf" not in seen, seen
        s.mod.decrypt_packed(host, kem["uk"], kem["blob"], kem["off"])          # the yardstick keeps its kernels
        seen = host.kernel_launches()
        assert "k_jobs_pairs" in seen and "k_dnf_dec_pairs" not in seen and "k_sym_tag" in seen, seen
    finally:
        host.kernel_timing(False)
        host.kernel_launches()


def test_a_group_of_two_engines_gives_the_same_bytes(kem):
    s = kem["s"]
    g = hl.Host(devices=[0, 0])
    try:
        g.set_tape(kem["tape"])
        hdr, hdr_off, keys = s.mod.encaps_packed(g, kem["pk"], kem["pkas"], POLICIES, kem["item_pol"])
        g.clear_tape()
        assert bytes(hdr) == bytes(kem["hdr"]) and (hdr_off == kem["hdr_off"]).all() and (keys == kem["keys"]).all()
        recs = list(kem["recs"])
        recs[40] = recs[40][:-5]          # a failure in the second block
        blob, off = join(recs)
        k_g, st_g = s.mod.decaps_packed(g, kem["uk"], blob, off)
    finally:
        g.close()
    want = [(-1 if i == 40 else 0) for i in range(N)]
    assert [int(x) for x in st_g] == want
    for i in range(N):
        assert bytes(k_g[i]) == (bytes(32) if i == 40 else bytes(kem["keys"][i])), i


def test_contract(host, kem):
    s = kem["s"]
    lib, name = host.lib, s.name
    enc, dec = getattr(lib, "rabe_%s_kem_encaps" % name), getattr(lib, "rabe_%s_kem_decaps" % name)
    n = 6
    arr, npol = hl._strs(POLICIES)
    pkarr = (ctypes.c_void_p * len(kem["pkas"]))(*[p.ptr for p in kem["pkas"]])
    ip = np.array(kem["item_pol"][:n], dtype=np.uint32)
    tape = [v for d in kem["draws"][:n] for v in d]
    want_off = [int(x) for x in kem["hdr_off"][:n + 1]]

    def encaps(n_items, item, buf, cap, off, keys):
        return enc(host.h, kem["pk"].ptr, pkarr, ctypes.c_size_t(len(kem["pkas"])), arr, npol, hl.JSON_POLICY, ctypes.c_size_t(n_items),
                   hl._np_ptr(item) if item is not None else None, hl._np_ptr(buf) if buf is not None else None, ctypes.c_size_t(cap),
                   hl._np_ptr(off) if off is not None else None, hl._np_ptr(keys) if keys is not None else None)
    host.set_tape(tape)
    try:
        ho, keys = np.zeros(n + 1, dtype=np.uint64), np.full((n, 32), 0xA5, dtype=np.uint8)
        assert encaps(n, ip, None, 0, ho, keys) == 1 and [int(x) for x in ho] == want_off          # a sizing call fills hdr_off
        buf = np.full(want_off[n], 0xA5, dtype=np.uint8)
        assert encaps(n, ip, buf, want_off[n] - 1, ho, keys) == 1                                    # one byte short
        assert (buf == 0xA5).all() and (keys == 0xA5).all() and [int(x) for x in ho] == want_off
        assert encaps(n, ip, buf, want_off[n], ho, keys) == 0                                        # ... and nothing was drawn: the tape starts here
        assert bytes(buf) == bytes(kem["hdr"][:want_off[n]]) and (keys == kem["keys"][:n]).all()
        ho[0] = 7
        assert encaps(0, ip, buf, buf.size, ho, keys) == 0 and int(ho[0]) == 0                       # n_items = 0
        for item, off in ((None, ho), (ip, None)):
            assert encaps(n, item, buf, buf.size, off, keys) == -1
            assert "null input" in lib.rabe_host_last_error(host.h).decode()
    finally:
        host.clear_tape()
    blob, off = join(kem["hdrs"][:n])
    status, keys = np.zeros(n, dtype=np.int32), np.zeros((n, 32), dtype=np.uint8)

    def decaps(n_items, o, st, kb):
        return dec(host.h, kem["uk"].ptr, ctypes.c_size_t(n_items), hl._np_ptr(blob), ctypes.c_size_t(blob.size), hl._np_ptr(o) if o is not None else None,
                   ctypes.c_uint32(0), hl._np_ptr(st) if st is not None else None, hl._np_ptr(kb) if kb is not None else None)
    for o, st, kb in ((None, status, keys), (off, None, keys), (off, status, None)):          # refused, as rabe_ac17_cp_decaps_packed refuses them
        assert decaps(n, o, st, kb) == -1
        assert "null input" in lib.rabe_host_last_error(host.h).decode()
    assert decaps(0, off, None, None) == 0          # nothing to write
    assert decaps(n, off, status, keys) == 0 and (status == 0).all() and (keys == kem["keys"][:n]).all()
