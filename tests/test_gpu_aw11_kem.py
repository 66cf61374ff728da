"""GPU checks of AW11 as a key encapsulation (include/rabe_host.h: rabe_aw11_{encaps,decaps}_packed), in the form of tests/test_gpu_kem.py.  The
two calls are compositions of existing ones, so those are the reference: encrypt_packed on the same tape for the headers, decrypt_gt + hashlib's
SHA3-256 for the keys (and the Python oracle's msg for three of them).  Two authorities, 70 items -- one 64-lane wave and a ragged tail -- over
policies of 1, 2 and 5 leaves.  The windowed leading factor measured slower than the NAF walk on this scheme's coefficients (docs/tried.md), so
the decaps keeps k_gt_multiexp_partial + k_gt_lead as decrypt_packed does; RABE_AW11_LEAD_W4=1 puts the width-4 window kernels
(rhip_gt_multiexp_rows') in their place, with the same keys: the launch records say which ran."""
import hashlib
import os
import random

import numpy as np
import pytest

from rabe_amd import hostlib as hl
from rabe_amd.schemes import aw11

pytestmark = pytest.mark.gpu
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
N = 70
SEAL_KERNELS = ("k_sym_setup", "k_sym_ctr", "k_sym_ghash_seg", "k_sym_tag")
W4_KERNELS = ("k_gtmexp4_digits", "k_gtmexp4_table", "k_gt_mexp4_partial", "k_gt_mexp4_finish")
NAF_KERNELS = ("k_gt_multiexp_partial", "k_gt_lead")


def leaf(a):
    return '{"name": "%s"}' % a


def gate(op, *children):
    return '{"name": "%s", "children": [%s]}' % (op, ", ".join(children))


# 1, 2 and 5 leaves; D and E belong to the second authority
# (the scheme's MSP conversion takes two children per AND gate)
POLICIES = [leaf("A"), gate("and", leaf("A"), leaf("D")),
            gate("and", gate("and", leaf("A"), leaf("B")), gate("and", leaf("C"), gate("and", leaf("D"), leaf("E"))))]
# per item: s, the gate coefficients of the s-shares then of the 0-shares (one per binary AND gate, twice), msg, one r_x per leaf -- then the
# nonce (encrypt only)
DRAWS = [1 + 0 + 1 + 1, 1 + 2 + 1 + 2, 1 + 8 + 1 + 5]
MSG_DRAW = [1, 3, 9]


def offsets(items):
    return np.concatenate([[0], np.cumsum([len(p) for p in items])]).astype(np.uint64)


def records(blob, off):
    return [bytes(blob[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


def kdf(gt):
    """the reference's kdf (src/utils/aes/mod.rs:47-55) on the 384 wire bytes of a Gt: its 12 coefficients as 32 big-endian bytes each"""
    assert len(gt) == 384
    return hashlib.sha3_256(b"".join(gt[32 * i:32 * i + 32][::-1] for i in range(12))).digest()


@pytest.fixture(scope="module")
def host():
    h = hl.Host(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def kem(host):
    """one encaps of 70 items on a tape, shared by the tests (nobody changes it)"""
    gk = aw11.setup(host)
    pk1, msk1 = aw11.authgen(host, gk, ["A", "B", "C"])
    pk2, msk2 = aw11.authgen(host, gk, ["D", "E"])
    sk = aw11.keygen(host, gk, msk1, "alice", ["A", "B", "C"])
    aw11.add_to_attribute(host, gk, msk2, "D", sk)
    aw11.add_to_attribute(host, gk, msk2, "E", sk)
    sk_a = aw11.keygen(host, gk, msk1, "bob", ["A"])          # satisfies the one-leaf policy only
    rnd = random.Random(0x61773131)
    item_pol = [i % 3 for i in range(N)]
    draws = [[rnd.randrange(1, R) for _ in range(DRAWS[item_pol[i]])] for i in range(N)]
    nonces = [rnd.randrange(1, R) for _ in range(N)]
    tape = [v for d in draws for v in d]
    host.set_tape(tape)
    hdr, hdr_off, keys = aw11.encaps_packed(host, gk, [pk1, pk2], POLICIES, item_pol)
    host.clear_tape()
    return {"gk": gk, "pks": [pk1, pk2], "sk": sk, "sk_a": sk_a, "item_pol": item_pol, "draws": draws, "nonces": nonces, "tape": tape,
            "hdr": hdr.copy(), "hdr_off": hdr_off, "keys": keys.copy()}


@pytest.fixture(scope="module")
def full(host, kem):
    """encrypt_packed on the same draws (the nonce after every item's) with 16-byte payloads"""
    tape = [v for d, nonce in zip(kem["draws"], kem["nonces"]) for v in d + [nonce]]
    pts = [b"sixteen byte pt!"] * N
    host.set_tape(tape)
    blob, off = aw11.encrypt_packed(host, kem["gk"], kem["pks"], POLICIES, kem["item_pol"], b"".join(pts), offsets(pts))
    host.clear_tape()
    return {"blob": blob.copy(), "off": off, "pts": pts}


def test_headers_are_encrypt_packed_records_without_a_sealed_part(kem, full):
    recs, hdrs = records(full["blob"], full["off"]), records(kem["hdr"], kem["hdr_off"])
    assert len(recs) == len(hdrs) == N
    for i in range(N):
        a, b = hl.parse_obj("aw11_ct", recs[i]), hl.parse_obj("aw11_ct", hdrs[i])
        assert set(a) == set(b)
        for field in a:
            if field != "ct":
                assert a[field] == b[field], (i, field)          # policy bytes and every group element
        assert len(a["ct"]) == 16 + 28 and b["ct"] == b"", i
        assert len(a["c"]) == (1, 2, 5)[kem["item_pol"][i]]
        assert hdrs[i] == recs[i][:-(4 + 16 + 28)] + bytes(4), i          # the record up to its length field, which is 0; nothing follows


def test_encaps_keys_are_sha3_of_the_oracles_msg(kem):
    from oracle import bn254 as bn
    e = bn.pairing(bn.G1_GEN, bn.G2_GEN)          # msg = e(G1::one(), G2::one())^rho, rho the item's msg draw
    for i in (0, 1, 2, N - 1):
        msg = bn.gt_to_le(bn.gt_pow(e, kem["draws"][i][MSG_DRAW[kem["item_pol"][i]]]))
        assert bytes(kem["keys"][i]) == kdf(msg), i


def test_decaps_keys_are_sha3_of_decrypt_gt_for_headers_and_full_records(host, kem, full):
    for blob, off in ((kem["hdr"], kem["hdr_off"]), (full["blob"], full["off"])):
        recs = records(blob, off)
        for trusted in (False, True):
            keys, status = aw11.decaps_packed(host, kem["gk"], kem["sk"], blob, off, trusted=trusted)
            assert (status == 0).all()
            assert (keys == kem["keys"]).all()          # the keys the encaps handed out
        for i in (0, 1, 2, 33, N - 1):
            ct = hl.Obj.deserialize("aw11_ct", recs[i])
            assert bytes(keys[i]) == kdf(aw11.decrypt_gt(host, kem["gk"], kem["sk"], ct)), i
    # the sealed part is not authenticated: a flipped tag byte fails decrypt_packed's item and leaves decaps's key alone
    bad = full["blob"].copy()
    bad[int(full["off"][6]) - 1] ^= 1
    keys2, status2 = aw11.decaps_packed(host, kem["gk"], kem["sk"], bad, full["off"])
    assert (status2 == 0).all() and (keys2 == kem["keys"]).all()
    pt, po, st = aw11.decrypt_packed(host, kem["gk"], kem["sk"], bad, full["off"])
    assert st.tolist() == [-1 if i == 5 else 0 for i in range(N)]


def row_elem(rec, row, which):
    """offset of C2 (which = 2) or C3 (3) of a row of an Aw11Ciphertext record"""
    ln = int.from_bytes(rec[:4], "little")
    at = 4 + ln + 1 + 384
    rows = int.from_bytes(rec[at:at + 4], "little")
    assert row < rows
    at += 4
    for y in range(rows):
        nl = int.from_bytes(rec[at:at + 4], "little")
        at += 4 + nl + 384
        if y == row:
            return at + (128 if which == 3 else 0)
        at += 256
    raise AssertionError


def test_failures_isolate(host, kem):
    from oracle import bn254 as bn
    from tests.test_gpu_ghw11_keys_packed import twist_point_outside_g2
    outside = bn.g2_to_le(twist_point_outside_g2())
    recs = records(kem["hdr"], kem["hdr_off"])
    r = bytearray(recs[8])                                   # five rows: C2 of row 3 (walked by its pairing) leaves the subgroup
    at = row_elem(r, 3, 2)
    r[at:at + 128] = outside
    recs[8] = bytes(r)
    r = bytearray(recs[13])                                  # two rows: C3 of row 1 (a term of the G2 sum)
    at = row_elem(r, 1, 3)
    r[at:at + 128] = outside
    recs[13] = bytes(r)
    recs[20] = recs[20][:-9]                                 # a truncated record
    blob = np.frombuffer(b"".join(recs), dtype=np.uint8)
    off = offsets(recs)
    off[N] += 5                                              # the last item's bounds run past ct_len
    failed = [8, 13, 20, N - 1]
    keys, status = aw11.decaps_packed(host, kem["gk"], kem["sk"], blob, off)          # checked mode
    for i in range(N):
        if i in failed:
            assert status[i] == -1 and bytes(keys[i]) == bytes(32), i
        else:
            assert status[i] == 0 and bytes(keys[i]) == bytes(kem["keys"][i]), i
    assert (host.lib.rabe_host_last_error(None) or b"") != b""


def test_a_key_without_the_attributes_fails_its_items_alone(host, kem):
    keys, status = aw11.decaps_packed(host, kem["gk"], kem["sk_a"], kem["hdr"], kem["hdr_off"])
    for i in range(N):
        if kem["item_pol"][i] == 0:
            assert status[i] == 0 and bytes(keys[i]) == bytes(kem["keys"][i]), i
        else:
            assert status[i] == -1 and bytes(keys[i]) == bytes(32), i


def test_launch_records(host, kem, full):
    host.kernel_timing(True)
    try:
        host.kernel_launches()
        aw11.encaps_packed(host, kem["gk"], kem["pks"], POLICIES, kem["item_pol"])
        seen = host.kernel_launches()
        assert not [k for k in SEAL_KERNELS if k in seen], seen
        assert seen.get("k_sym_kdf") == 1 and seen.get("k_assemble_records") == 1 and "k_sym_kdf_rows" not in seen, seen
        for b, o in ((kem["hdr"], kem["hdr_off"]), (full["blob"], full["off"])):
            aw11.decaps_packed(host, kem["gk"], kem["sk"], b, o)
            seen = host.kernel_launches()
            assert not [k for k in SEAL_KERNELS if k in seen], seen
            assert seen.get("k_sym_kdf_rows") == 1 and "k_sym_kdf" not in seen, seen
            assert all(k in seen for k in NAF_KERNELS), seen          # the measured choice: the decrypt's own lead kernels
            assert not [k for k in W4_KERNELS if k in seen], seen
            assert "k_aw11_dec_pairs" in seen and "k_msm_partial_g2" in seen and "k_naf_masks" in seen, seen          # the rest of the launch set
        # the windowed leading factor behind its switch: the new partial kernel runs, the NAF pair does not, the keys are the same
        assert "RABE_AW11_LEAD_W4" not in os.environ
        os.environ["RABE_AW11_LEAD_W4"] = "1"
        try:
            for b, o in ((kem["hdr"], kem["hdr_off"]), (full["blob"], full["off"])):
                keys, status = aw11.decaps_packed(host, kem["gk"], kem["sk"], b, o)
                seen = host.kernel_launches()
                assert (status == 0).all() and (keys == kem["keys"]).all()
                assert all(k in seen for k in W4_KERNELS), seen
                assert not [k for k in NAF_KERNELS + SEAL_KERNELS if k in seen], seen
                assert "k_aw11_dec_pairs" in seen and "k_msm_partial_g2" in seen and seen.get("k_sym_kdf_rows") == 1, seen
            aw11.decrypt_packed(host, kem["gk"], kem["sk"], full["blob"], full["off"])          # the switch does not reach the yardstick
        finally:
            del os.environ["RABE_AW11_LEAD_W4"]
        seen = host.kernel_launches()
        assert all(k in seen for k in NAF_KERNELS), seen          # the yardstick keeps its kernels
        assert not [k for k in W4_KERNELS if k in seen], seen
        assert all(k in seen for k in ("k_sym_setup", "k_sym_tag")), seen
    finally:
        host.kernel_timing(False)
        host.kernel_launches()


def test_a_group_of_two_engines_gives_the_same_bytes(host, kem):
    h2 = hl.Host(devices=[0, 0])
    try:
        assert h2.group_size() == 2
        h2.set_tape(kem["tape"])
        hdr, hdr_off, keys = aw11.encaps_packed(h2, kem["gk"], kem["pks"], POLICIES, kem["item_pol"])
        h2.clear_tape()
        assert bytes(hdr) == bytes(kem["hdr"]) and hdr_off.tolist() == kem["hdr_off"].tolist() and (keys == kem["keys"]).all()
        keys2, status = aw11.decaps_packed(h2, kem["gk"], kem["sk"], kem["hdr"], kem["hdr_off"])
        assert (status == 0).all() and (keys2 == kem["keys"]).all()
    finally:
        h2.close()


def test_empty_batches(host, kem):
    hdr, ho, keys = aw11.encaps_packed(host, kem["gk"], kem["pks"], POLICIES, [])
    assert len(hdr) == 0 and ho.tolist() == [0] and len(keys) == 0
    keys, status = aw11.decaps_packed(host, kem["gk"], kem["sk"], b"", [0])
    assert len(keys) == 0 and len(status) == 0
