"""GPU checks of the key-encapsulation forms of AC17 (CP) and BSW (include/rabe_host.h: rabe_{ac17_cp,bsw}_{encaps,decaps}_packed): the packed
encrypt / decrypt without payloads.  Their definitions are compositions of existing calls, so those calls are the reference: encrypt_packed on
the same tape for the headers, decrypt_gt + hashlib's SHA3-256 for the keys (and the Python oracle's msg for three of them).  70 items per
scheme -- one 64-lane wave and a ragged tail -- over three small policies: the launches take the small-launch pairing kernels, and the suite's
pairing mode (99, tests/conftest.py) runs every one of them again with each kernel family forced and compares on the device."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

from rabe_amd import hostlib as hl
from rabe_amd.schemes import ac17, bsw

pytestmark = pytest.mark.gpu
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
N = 70
SEAL_KERNELS = ("k_sym_setup", "k_sym_ctr", "k_sym_ghash_seg", "k_sym_tag")


def leaf(a):
    return '{"name": "%s"}' % a


def gate(op, *children):
    return '{"name": "%s", "children": [%s]}' % (op, ", ".join(children))


def offsets(items):
    return np.concatenate([[0], np.cumsum([len(p) for p in items])]).astype(np.uint64)


def records(blob, off):
    return [bytes(blob[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


def kdf(gt):
    """the reference's kdf (src/utils/aes/mod.rs:47-55) on the 384 wire bytes of a Gt: its 12 coefficients as 32 big-endian bytes each"""
    assert len(gt) == 384
    return hashlib.sha3_256(b"".join(gt[32 * i:32 * i + 32][::-1] for i in range(12))).digest()


class Ac17:
    name, ct_kind, sealed_field = "ac17", "ac17_cp_ct", "ct"
    key_attrs = ["A", "B", "C", "D"]
    # a single leaf, an AND of two, (A and B) or C: at most 4 attributes
    policies = [leaf("A"), gate("and", leaf("A"), leaf("B")), gate("or", gate("and", leaf("A"), leaf("B")), leaf("C"))]
    draws = [3, 3, 3]          # per item s0, s1, msg -- then the nonce (encrypt only)
    msg_draw = 2

    @staticmethod
    def keys(host):
        pk, msk = ac17.setup(host)
        return pk, ac17.cp_keygen(host, msk, Ac17.key_attrs)

    encrypt = staticmethod(lambda host, pk, pols, ip, pt, po: ac17.cp_encrypt_packed(host, pk, pols, ip, pt, po))
    decrypt = staticmethod(ac17.cp_decrypt_packed)
    encaps = staticmethod(ac17.cp_encaps_packed)
    decaps = staticmethod(ac17.cp_decaps_packed)
    decrypt_gt = staticmethod(ac17.cp_decrypt_gt)
    encaps_fn, decaps_fn = "rabe_ac17_cp_encaps_packed", "rabe_ac17_cp_decaps_packed"

    @staticmethod
    def g1_at(rec):
        """offset of the x coordinate of the first G1 element of a record (row 0, element 0)"""
        g = hl.parse_obj("ac17_cp_ct", rec)
        return rec.index(g["c"][0][1][0])


class Bsw:
    name, ct_kind, sealed_field = "bsw", "bsw_ct", "data"
    key_attrs = ["A", "B", "C", "D"]
    # one leaf, a 3-ary AND (two coefficient draws), an OR (none)
    policies = [leaf("A"), gate("and", leaf("A"), leaf("B"), leaf("C")), gate("or", leaf("A"), leaf("D"))]
    draws = [2, 4, 2]          # per item secret, msg, the gate coefficients -- then the nonce (encrypt only)
    msg_draw = 1

    @staticmethod
    def keys(host):
        pk, msk = bsw.setup(host)
        return pk, bsw.keygen(host, pk, msk, Bsw.key_attrs)

    encrypt = staticmethod(lambda host, pk, pols, ip, pt, po: bsw.encrypt_packed(host, pk, pols, ip, pt, po))
    decrypt = staticmethod(bsw.decrypt_packed)
    encaps = staticmethod(bsw.encaps_packed)
    decaps = staticmethod(bsw.decaps_packed)
    decrypt_gt = staticmethod(bsw.decrypt_gt)
    encaps_fn, decaps_fn = "rabe_bsw_encaps_packed", "rabe_bsw_decaps_packed"

    @staticmethod
    def g1_at(rec):
        g = hl.parse_obj("bsw_ct", rec)
        return rec.index(g["c"])


@pytest.fixture(scope="module")
def host():
    h = hl.Host(0)
    yield h
    h.close()


@pytest.fixture(scope="module", params=[Ac17, Bsw], ids=["ac17", "bsw"])
def kem(request, host):
    """one encaps of 70 items on a tape, shared by the tests (nobody changes it): the scheme, its keys, the draws, headers and keys"""
    S = request.param
    pk, sk = S.keys(host)
    rnd = random.Random(70 + len(S.name))
    item_pol = [i % 3 for i in range(N)]
    draws = [[rnd.randrange(1, R) for _ in range(S.draws[item_pol[i]])] for i in range(N)]
    nonces = [rnd.randrange(1, R) for _ in range(N)]
    tape = [v for d in draws for v in d]
    host.set_tape(tape)
    hdr, hdr_off, keys = S.encaps(host, pk, S.policies, item_pol)
    host.clear_tape()
    return {"S": S, "pk": pk, "sk": sk, "item_pol": item_pol, "draws": draws, "nonces": nonces, "tape": tape,
            "hdr": hdr.copy(), "hdr_off": hdr_off, "keys": keys.copy()}


def test_headers_are_encrypt_packed_records_without_a_sealed_part(host, kem):
    S = kem["S"]
    tape = [v for d, nonce in zip(kem["draws"], kem["nonces"]) for v in d + [nonce]]          # the same draws, the nonce after every item's
    pts = [b"\x5a"] * N
    host.set_tape(tape)
    blob, off = S.encrypt(host, kem["pk"], S.policies, kem["item_pol"], b"".join(pts), offsets(pts))
    host.clear_tape()
    full, hdrs = records(blob, off), records(kem["hdr"], kem["hdr_off"])
    assert len(full) == len(hdrs) == N
    for i in range(N):
        a, b = hl.parse_obj(S.ct_kind, full[i]), hl.parse_obj(S.ct_kind, hdrs[i])
        assert set(a) == set(b)
        for field in a:
            if field != S.sealed_field:
                assert a[field] == b[field], (i, field)          # policy bytes and every group element
        assert len(a[S.sealed_field]) == 1 + 28 and b[S.sealed_field] == b"", i
        assert hdrs[i] == full[i][:-(4 + 1 + 28)] + bytes(4), i          # the record up to its length field, which is 0; nothing follows


def test_keys_are_sha3_of_the_gt_decrypt_gt_returns(host, kem):
    S = kem["S"]
    hdrs = records(kem["hdr"], kem["hdr_off"])
    for i in range(N):
        ct = hl.Obj.deserialize(S.ct_kind, hdrs[i])
        assert bytes(kem["keys"][i]) == kdf(S.decrypt_gt(host, kem["sk"], ct)), i


def test_keys_are_sha3_of_the_oracles_msg(kem):
    from oracle import bn254 as bn
    S = kem["S"]
    e = bn.pairing(bn.G1_GEN, bn.G2_GEN)          # msg = e(G1::one(), G2::one())^rho, rho the item's msg draw
    for i in (0, 1, N - 1):
        msg = bn.gt_to_le(bn.gt_pow(e, kem["draws"][i][S.msg_draw]))
        assert bytes(kem["keys"][i]) == kdf(msg), i


def test_round_trip(host, kem):
    S = kem["S"]
    for trusted in (False, True):
        keys, status = S.decaps(host, kem["sk"], kem["hdr"], kem["hdr_off"], trusted=trusted)
        assert (status == 0).all()
        assert (keys == kem["keys"]).all()


def test_decaps_on_full_records_and_decrypt_packed_untouched(host, kem):
    S = kem["S"]
    rnd = random.Random(4)
    pts = [bytes(rnd.randrange(256) for _ in range(100)) for _ in range(N)]
    blob, off = S.encrypt(host, kem["pk"], S.policies, kem["item_pol"], b"".join(pts), offsets(pts))
    blob = blob.copy()
    keys, status = S.decaps(host, kem["sk"], blob, off)
    assert (status == 0).all()
    recs = records(blob, off)
    for i in range(N):
        ct = hl.Obj.deserialize(S.ct_kind, recs[i])
        assert bytes(keys[i]) == kdf(S.decrypt_gt(host, kem["sk"], ct)), i
    pt, po, st = S.decrypt(host, kem["sk"], blob, off)
    assert (st == 0).all() and bytes(pt) == b"".join(pts) and po.tolist() == offsets(pts).tolist()
    # the sealed part is not authenticated: a flipped tag byte fails decrypt_packed's item and leaves decaps's key alone
    bad = blob.copy()
    bad[int(off[6]) - 1] ^= 1
    keys2, status2 = S.decaps(host, kem["sk"], bad, off)
    assert (status2 == 0).all() and (keys2 == keys).all()
    assert S.decrypt(host, kem["sk"], bad, off)[2].tolist() == [-1 if i == 5 else 0 for i in range(N)]


def test_failures_isolate(host, kem):
    S = kem["S"]
    recs = records(kem["hdr"], kem["hdr_off"])
    unsat, _off, _keys = S.encaps(host, kem["pk"], [leaf("Z")], [0])
    recs[3] = bytes(unsat)                                   # a policy the key does not satisfy
    recs[10] = recs[10][:-9]                                 # a truncated record
    at = S.g1_at(recs[20])
    recs[20] = recs[20][:at] + P.to_bytes(32, "little") + recs[20][at + 32:]          # a G1 coordinate equal to p: not canonical
    blob = np.frombuffer(b"".join(recs), dtype=np.uint8)
    off = offsets(recs)
    off[N] += 5                                              # the last item's bounds run past ct_len
    failed = [3, 10, 20, N - 1]
    keys, status = S.decaps(host, kem["sk"], blob, off)          # checked mode
    for i in range(N):
        if i in failed:
            assert status[i] == -1 and bytes(keys[i]) == bytes(32), i
        else:
            assert status[i] == 0 and bytes(keys[i]) == bytes(kem["keys"][i]), i
    assert (host.lib.rabe_host_last_error(None) or b"") != b""


def test_capacity_and_nothing_drawn(host, kem):
    S = kem["S"]
    arr, npol = hl._strs(S.policies)
    ip = np.ascontiguousarray(kem["item_pol"], dtype=np.uint32)
    need = int(kem["hdr_off"][N])
    ho = np.full(N + 1, 99, dtype=np.uint64)
    buf = np.full(need, 0xAB, dtype=np.uint8)
    keys = np.full((N, 32), 0xCD, dtype=np.uint8)

    def call(cap):
        return getattr(host.lib, S.encaps_fn)(host.h, kem["pk"].ptr, arr, npol, hl.JSON_POLICY, ctypes.c_size_t(N), hl._np_ptr(ip), hl._np_ptr(buf),
                                              ctypes.c_size_t(cap), hl._np_ptr(ho), hl._np_ptr(keys))
    host.set_tape(kem["tape"])          # exactly the draws of one call: a short call that drew anything would exhaust it below
    assert call(need - 1) == 1
    assert int(ho[N]) == need and ho.tolist() == kem["hdr_off"].tolist()
    assert (buf == 0xAB).all() and (keys == 0xCD).all()
    assert call(need) == 0
    host.clear_tape()
    assert bytes(buf) == bytes(kem["hdr"]) and (keys == kem["keys"]).all()          # the bytes of the fresh run on that tape


def test_no_seal_or_open_kernel_is_launched(host, kem):
    S = kem["S"]
    pts = [b"sixteen byte pt!"] * 5
    host.kernel_timing(True)
    try:
        host.kernel_launches()
        blob, off = S.encrypt(host, kem["pk"], S.policies, kem["item_pol"][:5], b"".join(pts), offsets(pts))
        blob = blob.copy()
        seen = host.kernel_launches()
        assert all(k in seen for k in ("k_sym_kdf", "k_sym_setup", "k_sym_ctr", "k_sym_ghash_seg", "k_sym_tag")), seen          # the record sees them
        S.decrypt(host, kem["sk"], blob, off)
        seen = host.kernel_launches()
        assert all(k in seen for k in ("k_sym_setup", "k_sym_tag")), seen
        S.encaps(host, kem["pk"], S.policies, kem["item_pol"])
        seen = host.kernel_launches()
        assert not [k for k in SEAL_KERNELS if k in seen], seen
        assert seen.get("k_sym_kdf") == 1 and seen.get("k_assemble_records") == 1 and "k_sym_kdf_rows" not in seen, seen
        for b, o in ((kem["hdr"], kem["hdr_off"]), (blob, off)):
            S.decaps(host, kem["sk"], b, o)
            seen = host.kernel_launches()
            assert not [k for k in SEAL_KERNELS if k in seen], seen
            assert seen.get("k_sym_kdf_rows") == 1 and "k_sym_kdf" not in seen, seen
    finally:
        host.kernel_timing(False)
        host.kernel_launches()


def test_empty_batches(host, kem):
    S = kem["S"]
    hdr, ho, keys = S.encaps(host, kem["pk"], S.policies, [])
    assert len(hdr) == 0 and ho.tolist() == [0] and len(keys) == 0
    keys, status = S.decaps(host, kem["sk"], b"", [0])
    assert len(keys) == 0 and len(status) == 0


def test_kdf_rows_masks_on_the_device():
    """Level S (include/rabe_hip.h: rhip_gt_kdf_rows) on its own: rows picked by index, zeros for NO_ROW and for an index past the array, more than
    one 256-lane block"""
    from rabe_amd import Engine
    from rabe_amd import symlib as sym
    eng = Engine(0)
    rnd = random.Random(9)
    gts = [bytes(rnd.randrange(256) for _ in range(384)) for _ in range(3)]          # the KDF is byte work: any 384 bytes
    rows = [(i * 7) % 3 for i in range(300)]
    rows[0], rows[17], rows[256], rows[299] = sym.NO_ROW, 3, sym.NO_ROW, 2
    got = sym.gt_kdf_rows(eng, gts, rows)
    want = [kdf(gts[r]) if r < 3 else bytes(32) for r in rows]
    assert got == want
    assert sym.gt_kdf_rows(eng, [], [0, sym.NO_ROW]) == [bytes(32)] * 2
    assert got[1] == sym.gt_kdf(eng, gts, [rows[1]])[0]
    eng.close()
