"""GPU checks of the key-encapsulation forms of the two key-policy schemes, LSW and AC17 KP (include/rabe_host.h:
rabe_{lsw,ac17_kp}_{encaps,decaps}_packed): the packed encrypt / decrypt without payloads, modelled on tests/test_gpu_kem.py.  Their definitions
are compositions of existing calls, so those calls are the reference: encrypt_packed on the same tape for the headers (for LSW that is the
four-launch row path against the fused row kernel, byte for byte), decrypt_gt + hashlib's SHA3-256 for the keys (and the Python oracle's msg for
three of them).  70 items per scheme -- one 64-lane wave and a ragged tail -- over attribute lists of 1, 2 and 5 names; the suite's pairing mode
(99, tests/conftest.py) runs every decaps again with each kernel family forced and compares on the device."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

from rabe_amd import hostlib as hl
from rabe_amd.schemes import ac17, lsw

pytestmark = pytest.mark.gpu
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
N = 70
SEAL_KERNELS = ("k_sym_setup", "k_sym_ctr", "k_sym_ghash_seg", "k_sym_tag")
SETS = [["A"], ["A", "B"], ["A", "B", "C", "D", "E"]]
# satisfied by every one of the three lists (through A), and through B and C by the longest
POLICY = '{"name": "or", "children": [{"name": "A"}, {"name": "and", "children": [{"name": "B"}, {"name": "C"}]}]}'


def offsets(items):
    return np.concatenate([[0], np.cumsum([len(p) for p in items])]).astype(np.uint64)


def records(blob, off):
    return [bytes(blob[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


def kdf(gt):
    """the reference's kdf (src/utils/aes/mod.rs:47-55) on the 384 wire bytes of a Gt: its 12 coefficients as 32 big-endian bytes each"""
    assert len(gt) == 384
    return hashlib.sha3_256(b"".join(gt[32 * i:32 * i + 32][::-1] for i in range(12))).digest()


class Lsw:
    name, ct_kind, sealed_field = "lsw", "lsw_ct", "ct"
    draws = [1 + len(s) + 1 for s in SETS]          # per item secret, one sx per attribute, the msg exponent -- then the nonce (encrypt only)
    msg_draw = -1

    @staticmethod
    def keys(host):
        pk, msk = lsw.setup(host)
        return pk, msk, lsw.keygen(host, pk, msk, POLICY, hl.JSON_POLICY)

    encrypt = staticmethod(lsw.encrypt_packed)
    decrypt = staticmethod(lsw.decrypt_one_sk_packed)
    encaps = staticmethod(lsw.encaps_packed)
    decaps = staticmethod(lsw.decaps_packed)
    decrypt_gt = staticmethod(lsw.decrypt_gt)
    encaps_fn = "rabe_lsw_encaps_packed"
    cut = ("decaps",)          # encaps stays on the group's first device, as rabe_lsw_encrypt_packed does

    @staticmethod
    def g1_at(rec):
        """offset of the x coordinate of the first G1 element of a record (row 0: e3)"""
        return rec.index(hl.parse_obj("lsw_ct", rec)["ej"][0][1])


class Ac17Kp:
    name, ct_kind, sealed_field = "ac17_kp", "ac17_kp_ct", "ct"
    draws = [3, 3, 3]          # per item s0, s1, msg -- then the nonce (encrypt only)
    msg_draw = 2

    @staticmethod
    def keys(host):
        pk, msk = ac17.setup(host)
        return pk, msk, ac17.kp_keygen(host, msk, POLICY, hl.JSON_POLICY)

    encrypt = staticmethod(ac17.kp_encrypt_packed)
    decrypt = staticmethod(ac17.kp_decrypt_packed)
    encaps = staticmethod(ac17.kp_encaps_packed)
    decaps = staticmethod(ac17.kp_decaps_packed)
    decrypt_gt = staticmethod(ac17.kp_decrypt_gt)
    encaps_fn = "rabe_ac17_kp_encaps_packed"
    cut = ("encaps", "decaps")

    @staticmethod
    def g1_at(rec):
        return rec.index(hl.parse_obj("ac17_kp_ct", rec)["c"][0][1][0])


@pytest.fixture(scope="module")
def host():
    h = hl.Host(0)
    yield h
    h.close()


@pytest.fixture(scope="module", params=[Lsw, Ac17Kp], ids=["lsw", "ac17_kp"])
def kem(request, host):
    """one encaps of 70 items on a tape, shared by the tests (nobody changes it): the scheme, its keys, the draws, headers and keys"""
    S = request.param
    pk, msk, sk = S.keys(host)
    rnd = random.Random(170 + len(S.name))
    item_set = [i % 3 for i in range(N)]
    draws = [[rnd.randrange(1, R) for _ in range(S.draws[item_set[i]])] for i in range(N)]
    nonces = [rnd.randrange(1, R) for _ in range(N)]
    tape = [v for d in draws for v in d]
    host.set_tape(tape)
    hdr, hdr_off, keys = S.encaps(host, pk, SETS, item_set)
    host.clear_tape()
    return {"S": S, "pk": pk, "msk": msk, "sk": sk, "item_set": item_set, "draws": draws, "nonces": nonces, "tape": tape,
            "hdr": hdr.copy(), "hdr_off": hdr_off, "keys": keys.copy()}


def test_headers_are_encrypt_packed_records_without_a_sealed_part(host, kem):
    S = kem["S"]
    tape = [v for d, nonce in zip(kem["draws"], kem["nonces"]) for v in d + [nonce]]          # the same draws, the nonce after every item's
    pts = [b"\x5a"] * N
    host.set_tape(tape)
    blob, off = S.encrypt(host, kem["pk"], SETS, kem["item_set"], b"".join(pts), offsets(pts))
    host.clear_tape()
    full, hdrs = records(blob, off), records(kem["hdr"], kem["hdr_off"])
    assert len(full) == len(hdrs) == N
    for i in range(N):
        a, b = hl.parse_obj(S.ct_kind, full[i]), hl.parse_obj(S.ct_kind, hdrs[i])
        assert set(a) == set(b)
        for field in a:
            if field != S.sealed_field:
                assert a[field] == b[field], (i, field)          # attribute names and every group element
        assert len(a[S.sealed_field]) == 1 + 28 and b[S.sealed_field] == b"", i
        assert hdrs[i] == full[i][:-(4 + 1 + 28)] + bytes(4), i          # the record up to its length field, which is 0; nothing follows
    if S is Lsw:          # lsw/mod.rs:197-200: sx[0] loses sx[i], not the new element -- with ONE attribute that is secret minus itself, the identity
        for i in range(N):
            row0 = hl.parse_obj("lsw_ct", hdrs[i])["ej"][0]
            assert row0[1] != bytes(64) and ((row0[2] == bytes(64) and row0[3] == bytes(64)) == (len(SETS[kem["item_set"][i]]) == 1)), i


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
    blob, off = S.encrypt(host, kem["pk"], SETS, kem["item_set"], b"".join(pts), offsets(pts))
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
    unsat, _off, _keys = S.encaps(host, kem["pk"], [["Z"]], [0])
    recs[3] = bytes(unsat)                                   # a list that does not satisfy the key's policy
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
    # trusted: the membership checks are what is skipped -- the three failures that are not about membership still fail alone
    recs[20] = records(kem["hdr"], kem["hdr_off"])[20]
    blob = np.frombuffer(b"".join(recs), dtype=np.uint8)
    off = offsets(recs)
    off[N] += 5
    keys, status = S.decaps(host, kem["sk"], blob, off, trusted=True)
    for i in range(N):
        if i in (3, 10, N - 1):
            assert status[i] == -1 and bytes(keys[i]) == bytes(32), i
        else:
            assert status[i] == 0 and bytes(keys[i]) == bytes(kem["keys"][i]), i


def test_lsw_selected_negative_attribute_fails_the_item(host, kem):
    if kem["S"] is not Lsw:
        return          # the AC17 KP variant has no negative attributes
    pol = '{"name": "or", "children": [{"name": "and", "children": [{"name": "A"}, {"name": "B"}]}, {"name": "!N"}]}'
    sk = lsw.keygen(host, kem["pk"], kem["msk"], pol, hl.JSON_POLICY)
    hdr, off, keys = lsw.encaps_packed(host, kem["pk"], [["A", "B"], ["!N", "A"]], [0, 1, 0])
    got, status = lsw.decaps_packed(host, sk, hdr, off)
    assert status.tolist() == [0, -1, 0]
    assert bytes(got[1]) == bytes(32) and bytes(got[0]) == bytes(keys[0]) and bytes(got[2]) == bytes(keys[2])
    assert b"a negative attribute is selected" in (host.lib.rabe_host_last_error(None) or b"")


def test_capacity_and_nothing_drawn(host, kem):
    S = kem["S"]
    arr, _ = hl._strs([a for s in SETS for a in s])
    counts = (ctypes.c_size_t * len(SETS))(*[len(s) for s in SETS])
    it = np.ascontiguousarray(kem["item_set"], dtype=np.uint32)
    need = int(kem["hdr_off"][N])
    ho = np.full(N + 1, 99, dtype=np.uint64)
    buf = np.full(need, 0xAB, dtype=np.uint8)
    keys = np.full((N, 32), 0xCD, dtype=np.uint8)

    def call(cap):
        return getattr(host.lib, S.encaps_fn)(host.h, kem["pk"].ptr, arr, counts, ctypes.c_size_t(len(SETS)), ctypes.c_size_t(N), hl._np_ptr(it),
                                              hl._np_ptr(buf), ctypes.c_size_t(cap), hl._np_ptr(ho), hl._np_ptr(keys))
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
        blob, off = S.encrypt(host, kem["pk"], SETS, kem["item_set"][:5], b"".join(pts), offsets(pts))
        blob = blob.copy()
        seen = host.kernel_launches()
        assert all(k in seen for k in ("k_sym_kdf", "k_sym_setup", "k_sym_ctr", "k_sym_ghash_seg", "k_sym_tag")), seen          # the record sees them
        S.decrypt(host, kem["sk"], blob, off)
        seen = host.kernel_launches()
        assert all(k in seen for k in ("k_sym_setup", "k_sym_tag")), seen
        S.encaps(host, kem["pk"], SETS, kem["item_set"])
        seen = host.kernel_launches()
        assert not [k for k in SEAL_KERNELS if k in seen], seen
        assert seen.get("k_sym_kdf") == 1 and seen.get("k_assemble_records") == 1 and "k_sym_kdf_rows" not in seen, seen
        if S is Lsw:          # the rows are the fused kernel's: no G1 table launch, no addition
            assert seen.get("k_lsw_enc_rows") == 1 and "k_table_mul_g1" not in seen and "k_g1_add" not in seen, seen
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
    hdr, ho, keys = S.encaps(host, kem["pk"], SETS, [])
    assert len(hdr) == 0 and ho.tolist() == [0] and len(keys) == 0
    keys, status = S.decaps(host, kem["sk"], b"", [0])
    assert len(keys) == 0 and len(status) == 0


def test_device_group_gives_the_same_bytes_and_verdicts(host, kem):
    """two engines on the one GPU: the calls that are cut (S.cut; LSW encaps runs on the group's first device) give the single-device bytes"""
    S = kem["S"]
    recs = records(kem["hdr"], kem["hdr_off"])
    recs[10] = recs[10][:-4] + (1000).to_bytes(4, "little")          # a sealed length that runs past the record, in the first block
    recs[50] = recs[50][:-9]                                          # a truncated record, in the second
    bad_blob, bad_off = np.frombuffer(b"".join(recs), dtype=np.uint8), offsets(recs)
    got = []
    for h in (host, hl.Host(devices=[0, 0])):
        try:
            assert h.group_size() == (1 if h is host else 2)
            h.set_tape(kem["tape"])
            hdr, ho, keys = S.encaps(h, kem["pk"], SETS, kem["item_set"])
            h.clear_tape()
            k_ok, s_ok = S.decaps(h, kem["sk"], kem["hdr"], kem["hdr_off"])
            k_bad, s_bad = S.decaps(h, kem["sk"], bad_blob, bad_off)
            got.append((bytes(hdr), ho.tolist(), keys.tobytes(), k_ok.tobytes(), s_ok.tolist(), k_bad.tobytes(), s_bad.tolist()))
        finally:
            if h is not host:
                h.close()
    assert got[0] == got[1]
    assert got[0][0] == bytes(kem["hdr"]) and got[0][2] == kem["keys"].tobytes() and got[0][3] == kem["keys"].tobytes()
    assert got[0][6] == [-1 if i in (10, 50) else 0 for i in range(N)]
