#!/usr/bin/env python3
"""The two key-policy schemes as a key encapsulation against the packed calls they spare a caller, one GPU, one process, --items items
(16 384) under a list of --attrs attributes (50), the key's policy an AND over them:
  Level B   rhip_lsw_encrypt_rows (one lane per row, the products formed on the device, one inversion per block) against the row stage of
            rabe_lsw_encrypt_packed on the same scalars: four rhip_g1_table_mul launches fed host-formed products plus rhip_g1_add.  Timed
            around the launches and one sync, on device-resident scalars, and again with the upload of the per-row scalars in front (32 against
            96 bytes per row)
  (a) lsw.encaps_packed                     against (b) lsw.encrypt_packed with 16-byte plaintexts
  (c) lsw.decaps_packed on the headers of (a) against (d) lsw.decrypt_one_sk_packed on the records of (b)
  (e) .. (h) the same four for the AC17 KP pair
Every host leg is timed around its whole call, in the default, checked mode.  One warm-up round, then --rounds rounds in which the legs
ALTERNATE, so drift on a shared machine falls on all of them; best and median per leg (docs/measurement.md).  Before the timing the keys of
the decaps legs are compared with those of the encaps legs, the fused rows with the four launches byte for byte.  One JSON line, to stdout
and appended to --out.
usage: python tools/bench_kp_kem.py [--items 16384] [--attrs 50] [--rounds 5] [--out profiles/kp_kem_packed.jsonl]"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rabe_amd import Engine  # noqa: E402
from rabe_amd import engine as E  # noqa: E402
from rabe_amd import hostlib as hl  # noqa: E402
from rabe_amd.schemes import ac17, lsw  # noqa: E402

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
ap = argparse.ArgumentParser()
ap.add_argument("--items", type=int, default=16384)
ap.add_argument("--attrs", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default="")
args = ap.parse_args()
n, m = args.items, args.attrs
host = hl.Host(0)
attrs = ["g%03d" % i for i in range(m)]


def and_tree(names):
    """a balanced tree of binary ANDs (the AC17 KP variant's MSP conversion takes two children per gate)"""
    if len(names) == 1:
        return '{"name": "%s"}' % names[0]
    half = len(names) // 2
    return '{"name": "and", "children": [%s, %s]}' % (and_tree(names[:half]), and_tree(names[half:]))


policy = and_tree(attrs)
pt_blob = np.frombuffer(b"".join(b"%016d" % i for i in range(n)), dtype=np.uint8)
pt_off = (16 * np.arange(n + 1)).astype(np.uint64)
item_set = [0] * n

legs, sizes = [], {}
for name, S in (("lsw", lsw), ("ac17_kp", ac17)):
    kp = name == "ac17_kp"
    pk, msk = S.setup(host)
    sk = S.kp_keygen(host, msk, policy, hl.JSON_POLICY) if kp else S.keygen(host, pk, msk, policy, hl.JSON_POLICY)
    encaps, decaps = (S.kp_encaps_packed, S.kp_decaps_packed) if kp else (S.encaps_packed, S.decaps_packed)
    encrypt, decrypt = (S.kp_encrypt_packed, S.kp_decrypt_packed) if kp else (S.encrypt_packed, S.decrypt_one_sk_packed)
    hdr, hdr_off, keys = encaps(host, pk, [attrs], item_set)          # the warm-up round, and the comparisons
    hdr, keys = hdr.copy(), keys.copy()
    ct, ct_off = encrypt(host, pk, [attrs], item_set, pt_blob, pt_off)
    ct = ct.copy()
    back, st = decaps(host, sk, hdr, hdr_off)
    assert (st == 0).all() and (back == keys).all()
    pt, po, st = decrypt(host, sk, ct, ct_off)
    assert (st == 0).all() and bytes(pt) == bytes(pt_blob)
    del back, pt, po, st
    sizes[name] = (int(hdr_off[n]), int(ct_off[n]))
    legs += [(name + "_encaps_packed", lambda encaps=encaps, pk=pk: encaps(host, pk, [attrs], item_set)),
             (name + "_encrypt_packed_16B", lambda encrypt=encrypt, pk=pk: encrypt(host, pk, [attrs], item_set, pt_blob, pt_off)),
             (name + "_decaps_packed", lambda decaps=decaps, sk=sk, hdr=hdr, hdr_off=hdr_off: decaps(host, sk, hdr, hdr_off)),
             (name + "_decrypt_packed_16B", lambda decrypt=decrypt, sk=sk, ct=ct, ct_off=ct_off: decrypt(host, sk, ct, ct_off))]
    if not kp:
        lsw_pk = hl.parse_obj("lsw_pk", pk.serialize())

# Level B: the row stage alone, on random scalars (sx of an item's first row as the reference's loop leaves it)
eng = Engine(0)
tbls = []
for field in ("g1", "g1_b", "g1_b2", "h_b"):
    t = eng.g1_table(lsw_pk[field])
    t.add_w16()
    tbls.append(t)
rnd = random.Random(50)
total = n * m
h = [rnd.randrange(1, R) for _ in range(m)]
secret = [rnd.randrange(1, R) for _ in range(n)]
sx = [rnd.randrange(1, R) for _ in range(total)]


def le(v):
    return b"".join(int(x).to_bytes(32, "little") for x in v)


b_sx = le(sx)
b_four = le(h[t % m] * secret[t // m] % R for t in range(total)) + b_sx + le(sx[t] * h[t % m] % R for t in range(total))          # host-formed products
d_row_off, d_hash_off = eng.upload_u32([m * i for i in range(n + 1)]), eng.upload_u32([0] * n)
d_hash, d_secret = eng.upload(le(h)), eng.upload(le(secret))
d_sx, d_four = eng.upload(b_sx), eng.upload(b_four)
d_rows, d_e3, d_e4, d_t1, d_t2, d_e5 = (eng.alloc(192 * total),) + tuple(eng.alloc(64 * total) for _ in range(5))
ct_ = ctypes.c_size_t(total)


def up(dev, data):
    eng._check(eng.lib.rhip_upload(eng.ctx, dev.ptr, data, ctypes.c_size_t(len(data))))


def rows_fused(upload=False):
    if upload:
        up(d_sx, b_sx)
    E.lsw_encrypt_rows_dev(eng, tbls[0], tbls[1], tbls[2], tbls[3], n, total, d_row_off, d_hash_off, d_hash, d_secret, d_sx, d_rows)
    eng.sync()


def rows_four(upload=False):
    if upload:
        up(d_four, b_four)
    base = d_four.ptr.value
    ka, kb, kc = (ctypes.c_void_p(base + 32 * total * j) for j in range(3))
    for tbl, k, out in ((tbls[0], ka, d_e3), (tbls[1], kb, d_e4), (tbls[2], kc, d_t1), (tbls[3], kb, d_t2)):
        eng._check(eng.lib.rhip_g1_table_mul(eng.ctx, tbl.h, ct_, k, out.ptr))
    eng._check(eng.lib.rhip_g1_add(eng.ctx, ct_, d_t1.ptr, d_t2.ptr, d_e5.ptr))
    eng.sync()


rows_fused()
rows_four()
fused = np.frombuffer(eng.download(d_rows, 192 * total), dtype=np.uint8).reshape(total, 3, 64)
for j, d in enumerate((d_e3, d_e4, d_e5)):
    assert fused[:, j, :].tobytes() == eng.download(d, 64 * total), "fused rows differ from the four launches in element %d" % j
del fused
legs = [("lsw_rows_fused", rows_fused), ("lsw_rows_four_launches_plus_add", rows_four),
        ("lsw_rows_fused_with_upload", lambda: rows_fused(True)), ("lsw_rows_four_launches_plus_add_with_upload", lambda: rows_four(True))] + legs

times = {leg: [] for leg, _ in legs}
for _ in range(args.rounds):
    for leg, fn in legs:
        t0 = time.perf_counter()
        fn()
        times[leg].append(time.perf_counter() - t0)
line = {"config": "LSW and AC17 KP key encapsulation, %d items under a list of %d attributes, the key's policy an AND over them: the fused LSW row "
                  "kernel against four table launches + the addition on the same scalars (rows per second), encaps / decaps against encrypt / decrypt "
                  "with 16-byte plaintexts (items per second), checked mode, legs alternating, %d rounds after one warm-up" % (n, m, args.rounds),
        "schemes": ["LSW", "AC17 KP"], "batch": n, "attributes": m, "rows": total, "rounds": args.rounds, "keys_equal": True, "rows_equal": True,
        "lsw_header_bytes": sizes["lsw"][0], "lsw_record_bytes": sizes["lsw"][1], "ac17_kp_header_bytes": sizes["ac17_kp"][0],
        "ac17_kp_record_bytes": sizes["ac17_kp"][1]}
for leg, _ in legs:
    unit, count = ("_rows_per_s", total) if leg.startswith("lsw_rows") else ("_items_per_s", n)
    line[leg + unit] = round(count / min(times[leg]), 1)
    line[leg + unit + "_median"] = round(count / statistics.median(times[leg]), 1)
    line[leg + "_s"] = [round(t, 5) for t in times[leg]]
text = json.dumps(line)
print(text, flush=True)
if args.out:
    with open(args.out, "a") as f:
        f.write(text + "\n")
for t in tbls:
    t.destroy()
eng.close()
host.close()
