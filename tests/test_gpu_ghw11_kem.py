"""GPU checks of GHW11 as a key encapsulation (include/rabe_host.h: rabe_ghw11_{encaps,decaps_out,decaps}_packed).  The definitions are
compositions of existing calls, so those calls are the reference: encrypt_packed on the same tape for the headers, hashlib's SHA3-256 of the
oracle's msg and of decrypt_out_gt for the keys.  70 items -- one 64-lane wave and a ragged tail -- over three small policies, in the
suite's cross-check pairing mode."""
import hashlib
import random

import numpy as np
import pytest

from rabe_amd import hostlib as hl
from rabe_amd.schemes import ghw11
from tests.test_gpu_kem import SEAL_KERNELS

pytestmark = pytest.mark.gpu
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
N = 70
ATTRS = ["A", "B", "C", "D"]


def leaf(a):
    return '{"name": "%s"}' % a


def gate(op, *children):
    return '{"name": "%s", "children": [%s]}' % (op, ", ".join(children))


# a leaf, an AND of two, (A and B) or C
POLICIES = [leaf("A"), gate("and", leaf("A"), leaf("B")), gate("or", gate("and", leaf("A"), leaf("B")), leaf("C"))]
DRAWS = [3, 5, 6]          # per item: secret, msg, the gate coefficients, one t per share -- then the nonce (encrypt only)


def offsets(items):
    return np.concatenate([[0], np.cumsum([len(p) for p in items])]).astype(np.uint64)


def records(blob, off):
    return [bytes(blob[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


def kdf(gt):
    """the reference's kdf on the 384 wire bytes of a Gt: its 12 coefficients as 32 big-endian bytes each"""
    assert len(gt) == 384
    return hashlib.sha3_256(b"".join(gt[32 * i:32 * i + 32][::-1] for i in range(12))).digest()


@pytest.fixture(scope="module")
def host():
    h = hl.Host(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def kem(host):
    """one encaps of 70 items on a tape, the full records of encrypt_packed on the same draws, both transformed: shared, nobody changes it"""
    pk, msk = ghw11.setup(host)
    sk = ghw11.keygen(host, pk, msk, ATTRS)
    tk, rk = ghw11.tkgen(host, sk)
    rnd = random.Random(0x6b656d)
    item_pol = [i % 3 for i in range(N)]
    draws = [[rnd.randrange(1, R) for _ in range(DRAWS[item_pol[i]])] for i in range(N)]
    nonces = [rnd.randrange(1, R) for _ in range(N)]
    tape = [v for d in draws for v in d]
    host.set_tape(tape)
    hdr, hdr_off, keys = ghw11.encaps_packed(host, pk, POLICIES, item_pol)
    pts = [b"sixteen byte pt!"] * N
    host.set_tape([v for d, nonce in zip(draws, nonces) for v in d + [nonce]])          # the same draws, the nonce after every item's
    blob, off = ghw11.encrypt_packed(host, pk, POLICIES, item_pol, b"".join(pts), offsets(pts))
    host.clear_tape()
    hdr, blob = hdr.copy(), blob.copy()
    tct, st = ghw11.transform_packed(host, tk, hdr, hdr_off)
    tct_full, st_full = ghw11.transform_packed(host, tk, blob, off)
    return {"pk": pk, "msk": msk, "sk": sk, "tk": tk, "rk": rk, "item_pol": item_pol, "draws": draws, "tape": tape, "hdr": hdr, "hdr_off": hdr_off,
            "keys": keys.copy(), "blob": blob, "off": off, "pts": pts, "tct": tct.copy(), "st": st.copy(), "tct_full": tct_full.copy(),
            "st_full": st_full.copy()}


def test_headers_are_encrypt_packed_records_without_a_sealed_part(kem):
    full, hdrs = records(kem["blob"], kem["off"]), records(kem["hdr"], kem["hdr_off"])
    assert len(full) == len(hdrs) == N
    for i in range(N):
        a, b = hl.parse_obj("ghw11_ct", full[i]), hl.parse_obj("ghw11_ct", hdrs[i])
        assert len(a["data"]) == 16 + 28 and b["data"] == b"", i
        assert hdrs[i] == full[i][:-(4 + 16 + 28)] + bytes(4), i          # the record up to its length field, which is 0; nothing follows


def test_keys_are_sha3_of_the_oracles_msg(kem):
    from oracle import bn254 as bn
    e = bn.pairing(bn.G1_GEN, bn.G2_GEN)          # msg = e(G1::one(), G2::one())^rho, rho the item's second draw
    for i in (0, 1, 2, N - 1):
        assert bytes(kem["keys"][i]) == kdf(bn.gt_to_le(bn.gt_pow(e, kem["draws"][i][1]))), i


def test_transform_gives_the_same_records_on_headers_and_on_full_records(kem):
    assert (kem["st"] == 0).all() and (kem["st_full"] == 0).all()
    assert (kem["tct"] == kem["tct_full"]).all()
    assert kem["tct"].shape == (N, 768) and kem["tct"].any(axis=1).all()


def test_decaps_out_keys_are_the_kdf_of_decrypt_out_gt_and_the_encaps_keys(host, kem):
    for trusted in (False, True):
        keys, status = ghw11.decaps_out_packed(host, kem["rk"], kem["tct"], trusted=trusted)
        assert (status == 0).all()
        assert (keys == kem["keys"]).all()
    for i in range(N):
        tobj = hl.Obj.deserialize("ghw11_tct", kem["tct"][i].tobytes())
        assert bytes(keys[i]) == kdf(ghw11.decrypt_out_gt(host, tobj, kem["rk"])), i


def test_decaps_gives_the_same_keys_from_headers_and_full_records_and_for_any_z(host, kem):
    for trusted in (False, True):
        keys, status = ghw11.decaps_packed(host, kem["sk"], kem["hdr"], kem["hdr_off"], trusted=trusted)
        assert (status == 0).all() and (keys == kem["keys"]).all()
    keys, status = ghw11.decaps_packed(host, kem["sk"], kem["blob"], kem["off"])
    assert (status == 0).all() and (keys == kem["keys"]).all()
    # the blinding cancels: a second tkgen draws another z, and the chain through it ends on the same keys
    tk2, rk2 = ghw11.tkgen(host, kem["sk"])
    assert rk2.serialize() != kem["rk"].serialize()
    tct2, st2 = ghw11.transform_packed(host, tk2, kem["hdr"], kem["hdr_off"])
    assert (st2 == 0).all() and not (tct2[:, 384:] == kem["tct"][:, 384:]).all(axis=1).any()
    keys2, status2 = ghw11.decaps_out_packed(host, rk2, tct2)
    assert (status2 == 0).all() and (keys2 == kem["keys"]).all()
    # decrypt_packed itself is untouched: the full records still open
    pt, po, st = ghw11.decrypt_packed(host, kem["sk"], kem["blob"], kem["off"])
    assert (st == 0).all() and bytes(pt) == b"".join(kem["pts"])


def test_decaps_out_failures_isolate(host, kem):
    tct = kem["tct"].copy()
    tct[4, :] = 0                      # the transform's failure mark
    tct[9, 5] ^= 0x20                  # c with one coefficient bumped: not in Gt
    tct[66, 384 + 40] ^= 1             # t not in Gt, in the ragged tail
    failed = [4, 9, 66]
    keys, status = ghw11.decaps_out_packed(host, kem["rk"], tct)          # checked mode
    for i in range(N):
        if i in failed:
            assert status[i] == -1 and bytes(keys[i]) == bytes(32), i
        else:
            assert status[i] == 0 and bytes(keys[i]) == bytes(kem["keys"][i]), i
    assert (host.lib.rabe_host_last_error(None) or b"") != b""
    # trusted mode: the zero record still fails, a non-member's key is unspecified, the neighbours are untouched
    keys, status = ghw11.decaps_out_packed(host, kem["rk"], tct, trusted=True)
    assert status.tolist() == [-1 if i == 4 else 0 for i in range(N)] and bytes(keys[4]) == bytes(32)
    for i in range(N):
        if i not in failed:
            assert bytes(keys[i]) == bytes(kem["keys"][i]), i
    # a wrong rk: a KEM has no tag -- another key, status 0
    _tk2, rk2 = ghw11.tkgen(host, kem["sk"])
    keys, status = ghw11.decaps_out_packed(host, rk2, kem["tct"])
    assert (status == 0).all()
    assert not (keys == kem["keys"]).all(axis=1).any()


def test_decaps_failures_isolate(host, kem):
    recs = records(kem["hdr"], kem["hdr_off"])
    unsat, _off, _keys = ghw11.encaps_packed(host, kem["pk"], [leaf("Z")], [0])
    recs[3] = bytes(unsat)                                              # a policy the key does not satisfy
    recs[10] = recs[10][:-4] + (1000).to_bytes(4, "little")             # a length field that points outside the record
    g = hl.parse_obj("ghw11_ct", recs[20])
    at = recs[20].index(g["c"])
    bumped = bytearray(recs[20])
    bumped[at + 5] ^= 0x20                                              # c with one coefficient bumped: not in Gt
    recs[20] = bytes(bumped)
    blob = np.frombuffer(b"".join(recs), dtype=np.uint8)
    off = offsets(recs)
    failed = [3, 10, 20]
    keys, status = ghw11.decaps_packed(host, kem["sk"], blob, off)          # checked mode
    for i in range(N):
        if i in failed:
            assert status[i] == -1 and bytes(keys[i]) == bytes(32), i
        else:
            assert status[i] == 0 and bytes(keys[i]) == bytes(kem["keys"][i]), i
    # a key that satisfies none of the AND policies: those items fail alone
    sk_c = ghw11.keygen(host, kem["pk"], kem["msk"], ["C"])
    keys, status = ghw11.decaps_packed(host, sk_c, kem["hdr"], kem["hdr_off"])
    for i in range(N):
        if kem["item_pol"][i] == 2:
            assert status[i] == 0 and bytes(keys[i]) == bytes(kem["keys"][i]), i
        else:
            assert status[i] == -1 and bytes(keys[i]) == bytes(32), i


def test_no_seal_kernel_and_no_window_power(host, kem):
    host.kernel_timing(True)
    try:
        host.kernel_launches()
        ghw11.encaps_packed(host, kem["pk"], POLICIES, kem["item_pol"])
        seen = host.kernel_launches()
        assert not [k for k in SEAL_KERNELS if k in seen], seen
        assert seen.get("k_sym_kdf") == 1, seen
        ghw11.decaps_out_packed(host, kem["rk"], kem["tct"])
        seen = host.kernel_launches()
        assert not [k for k in SEAL_KERNELS if k in seen], seen
        assert "k_gt_pow" not in seen and "k_gt_mul" not in seen, seen
        assert seen.get("k_gt_pow_rows") == 1 and seen.get("k_gtpow4_masks") == 1 and seen.get("k_sym_kdf_rows") == 1, seen
        for b, o in ((kem["hdr"], kem["hdr_off"]), (kem["blob"], kem["off"])):
            ghw11.decaps_packed(host, kem["sk"], b, o)
            seen = host.kernel_launches()
            assert not [k for k in SEAL_KERNELS if k in seen], seen
            assert "k_gt_pow" not in seen and "k_gt_pow_rows" not in seen and seen.get("k_sym_kdf_rows") == 1, seen
    finally:
        host.kernel_timing(False)
        host.kernel_launches()


def test_device_group_gives_the_same_bytes_and_verdicts(kem):
    tct = kem["tct"].copy()
    tct[4, :] = 0
    tct[40, 5] ^= 0x20
    recs = records(kem["hdr"], kem["hdr_off"])
    recs[10] = recs[10][:-4] + (1000).to_bytes(4, "little")
    bad_blob, bad_off = np.frombuffer(b"".join(recs), dtype=np.uint8), offsets(recs)
    got = []
    for devices in (None, [0, 0, 0]):
        h = hl.Host(0) if devices is None else hl.Host(devices=devices)
        try:
            h.set_tape(kem["tape"])
            hdr, ho, keys = ghw11.encaps_packed(h, kem["pk"], POLICIES, kem["item_pol"])
            h.clear_tape()
            k_out, s_out = ghw11.decaps_out_packed(h, kem["rk"], tct)
            k_dec, s_dec = ghw11.decaps_packed(h, kem["sk"], bad_blob, bad_off)
            got.append((bytes(hdr), ho.tolist(), keys.tobytes(), k_out.tobytes(), s_out.tolist(), k_dec.tobytes(), s_dec.tolist()))
        finally:
            h.close()
    assert got[0] == got[1]
    assert got[0][0] == bytes(kem["hdr"]) and got[0][2] == kem["keys"].tobytes()
    assert got[0][4] == [-1 if i in (4, 40) else 0 for i in range(N)] and got[0][6] == [-1 if i == 10 else 0 for i in range(N)]


def test_empty_batches(host, kem):
    hdr, ho, keys = ghw11.encaps_packed(host, kem["pk"], POLICIES, [])
    assert len(hdr) == 0 and ho.tolist() == [0] and len(keys) == 0
    keys, status = ghw11.decaps_packed(host, kem["sk"], b"", [0])
    assert len(keys) == 0 and len(status) == 0
    keys, status = ghw11.decaps_out_packed(host, kem["rk"], b"")
    assert len(keys) == 0 and len(status) == 0
