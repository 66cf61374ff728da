#!/usr/bin/env python3
"""Key encapsulation against the packed calls it spares a caller, one GPU, one process: --items items (16 384) of AC17 CP and of BSW under an
AND (a chain of two-child gates) over --attrs attributes (20: every row is selected), one secret key, four legs per scheme:
  (a) encaps_packed                                 -- headers + 32-byte content keys
  (b) encrypt_packed with 16-byte plaintexts        -- the yardstick: what a caller who wanted only keys had to run (dummy payloads)
  (c) decaps_packed on the headers of (a)           -- content keys back
  (d) decrypt_packed on the records of (b)          -- the yardstick on the other side
Every leg is timed around its whole call (each ends in a copy out, which waits for the device), in the default, checked mode.  One warm-up
round (window tables, prepared key lines, arenas, pinned staging), then --rounds rounds in which the four legs ALTERNATE, so drift on a
shared machine falls on all of them; best and median per leg.  Before the timing the keys of (c) are compared with those of (a) and the
plaintexts of (d) with what was encrypted.  The headers of (a) are shorter than the records of (b) by 16 + 28 bytes per item: what (c) and (d)
upload differs by that much.  One JSON line per scheme, to stdout and appended to --out.
usage: python tools/bench_kem.py [--items 16384] [--attrs 20] [--rounds 5] [--out profiles/kem_packed.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rabe_amd import hostlib as hl  # noqa: E402
from rabe_amd.schemes import ac17, bsw  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--items", type=int, default=16384)
ap.add_argument("--attrs", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default="")
args = ap.parse_args()
n = args.items
host = hl.Host(0)
attrs = ["g%03d" % i for i in range(args.attrs)]
policy = '{"name": "%s"}' % attrs[0]          # a chain of two-child ANDs: AC17's MSP takes binary gates only
for a in attrs[1:]:
    policy = '{"name": "and", "children": [%s, {"name": "%s"}]}' % (policy, a)
pts = [b"%016d" % i for i in range(n)]
pt_blob = np.frombuffer(b"".join(pts), dtype=np.uint8)
pt_off = (16 * np.arange(n + 1)).astype(np.uint64)
item_pol = [0] * n


def scheme_ac17():
    pk, msk = ac17.setup(host)
    sk = ac17.cp_keygen(host, msk, attrs)
    return ("AC17 CP", lambda: ac17.cp_encaps_packed(host, pk, [policy], item_pol),
            lambda: ac17.cp_encrypt_packed(host, pk, [policy], item_pol, pt_blob, pt_off),
            lambda blob, off: ac17.cp_decaps_packed(host, sk, blob, off), lambda blob, off: ac17.cp_decrypt_packed(host, sk, blob, off))


def scheme_bsw():
    pk, msk = bsw.setup(host)
    sk = bsw.keygen(host, pk, msk, attrs)
    return ("BSW", lambda: bsw.encaps_packed(host, pk, [policy], item_pol), lambda: bsw.encrypt_packed(host, pk, [policy], item_pol, pt_blob, pt_off),
            lambda blob, off: bsw.decaps_packed(host, sk, blob, off), lambda blob, off: bsw.decrypt_packed(host, sk, blob, off))


for make in (scheme_ac17, scheme_bsw):
    name, encaps, encrypt, decaps, decrypt = make()
    hdr, hdr_off, keys = encaps()                        # the warm-up round, and the comparison
    hdr, keys = hdr.copy(), keys.copy()
    ct, ct_off = encrypt()
    ct = ct.copy()
    back, st = decaps(hdr, hdr_off)
    assert (st == 0).all() and (back == keys).all(), name
    pt, po, st = decrypt(ct, ct_off)
    assert (st == 0).all() and bytes(pt) == bytes(pt_blob) and po.tolist() == pt_off.tolist(), name
    del back, pt, po, st
    legs = [("encaps_packed", encaps), ("encrypt_packed_16B", encrypt), ("decaps_packed", lambda: decaps(hdr, hdr_off)),
            ("decrypt_packed_16B", lambda: decrypt(ct, ct_off))]
    times = {leg: [] for leg, _ in legs}
    for _ in range(args.rounds):
        for leg, fn in legs:
            t0 = time.perf_counter()
            fn()
            times[leg].append(time.perf_counter() - t0)
    line = {"config": "%s key encapsulation, %d items under an AND of %d attributes, one secret key: encaps_packed against encrypt_packed with 16-byte "
                      "plaintexts, decaps_packed against decrypt_packed, checked mode, legs alternating, %d rounds after one warm-up"
                      % (name, n, args.attrs, args.rounds),
            "scheme": name, "batch": n, "attributes": args.attrs, "rounds": args.rounds, "keys_equal": True, "header_bytes": int(hdr_off[n]),
            "record_bytes": int(ct_off[n])}
    for leg, _ in legs:
        line[leg + "_items_per_s"] = round(n / min(times[leg]), 1)
        line[leg + "_items_per_s_median"] = round(n / statistics.median(times[leg]), 1)
        line[leg + "_s"] = [round(t, 4) for t in times[leg]]
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")
host.close()
