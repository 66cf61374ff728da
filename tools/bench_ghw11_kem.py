#!/usr/bin/env python3
"""GHW11 as a key encapsulation against the packed calls it spares a caller, one GPU, one process, --items items (16 384):
  Level E   rhip_gt_pow_rows (one item, every row under one scalar, mul given, inverted) against rhip_gt_pow + rhip_gt_mul on the same
            device-resident elements: the power of the thin client, timed around the launches and one sync
  (a) encaps_packed                       against (b) encrypt_packed with 16-byte plaintexts
  (c) decaps_out_packed on c | t records  against (d) decrypt_out_packed on the same records + the ciphertext blob of (b)
  (e) decaps_packed on the headers of (a) against (f) decrypt_packed on the records of (b)
under an AND over --attrs attributes (20).  Every host leg is timed around its whole call, in the default, checked mode.  One warm-up round,
then --rounds rounds in which the legs ALTERNATE, so drift on a shared machine falls on all of them; best and median per leg (docs/measurement.md).
Before the timing the keys of (c) and (e) are compared with those of (a), the row power with the window power byte for byte.  One JSON
line, to stdout and appended to --out.
usage: python tools/bench_ghw11_kem.py [--items 16384] [--attrs 20] [--rounds 5] [--out profiles/ghw11_kem_packed.jsonl]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rabe_amd import Engine  # noqa: E402
from rabe_amd import hostlib as hl  # noqa: E402
from rabe_amd.schemes import ghw11  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--items", type=int, default=16384)
ap.add_argument("--attrs", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default="")
args = ap.parse_args()
n = args.items
host = hl.Host(0)
attrs = ["g%03d" % i for i in range(args.attrs)]
policy = '{"name": "and", "children": [%s]}' % ", ".join('{"name": "%s"}' % a for a in attrs)
pts = [b"%016d" % i for i in range(n)]
pt_blob = np.frombuffer(b"".join(pts), dtype=np.uint8)
pt_off = (16 * np.arange(n + 1)).astype(np.uint64)
item_pol = [0] * n
pk, msk = ghw11.setup(host)
sk = ghw11.keygen(host, pk, msk, attrs)
tk, rk = ghw11.tkgen(host, sk)

hdr, hdr_off, keys = ghw11.encaps_packed(host, pk, [policy], item_pol)          # the warm-up round, and the comparisons
hdr, keys = hdr.copy(), keys.copy()
ct, ct_off = ghw11.encrypt_packed(host, pk, [policy], item_pol, pt_blob, pt_off)
ct = ct.copy()
tct, st = ghw11.transform_packed(host, tk, hdr, hdr_off)
assert (st == 0).all()
tct_ct, st = ghw11.transform_packed(host, tk, ct, ct_off)
assert (st == 0).all()
back, st = ghw11.decaps_out_packed(host, rk, tct)
assert (st == 0).all() and (back == keys).all()
back, st = ghw11.decaps_packed(host, sk, hdr, hdr_off)
assert (st == 0).all() and (back == keys).all()
pt, po, st = ghw11.decrypt_out_packed(host, rk, tct_ct, ct, ct_off)
assert (st == 0).all() and bytes(pt) == bytes(pt_blob)
pt, po, st = ghw11.decrypt_packed(host, sk, ct, ct_off)
assert (st == 0).all() and bytes(pt) == bytes(pt_blob)
del back, pt, po, st

# Level E on the c | t records themselves: c * t^-z
eng = Engine(0)
d_c = eng.upload(np.ascontiguousarray(tct[:, :384]).tobytes())
d_t = eng.upload(np.ascontiguousarray(tct[:, 384:]).tobytes())
z = rk.serialize()
nz = ((-int.from_bytes(z, "little")) % 21888242871839275222246405745257275088548364400416034343698204186575808495617).to_bytes(32, "little")
d_z, d_nz, d_off = eng.upload(z), eng.upload(nz * n), eng.upload_u32([0, n])
d_p, d_out_w, d_out_r = eng.alloc(384 * n), eng.alloc(384 * n), eng.alloc(384 * n)
cn = ctypes.c_size_t(n)


def power_window():
    eng._check(eng.lib.rhip_gt_pow(eng.ctx, cn, d_t.ptr, d_nz.ptr, d_p.ptr))
    eng._check(eng.lib.rhip_gt_mul(eng.ctx, cn, d_c.ptr, d_p.ptr, d_out_w.ptr))
    eng.sync()


def power_rows():
    eng._check(eng.lib.rhip_gt_pow_rows(eng.ctx, cn, d_off.ptr, d_t.ptr, ctypes.c_size_t(1), d_z.ptr, d_c.ptr, ctypes.c_uint32(1), d_out_r.ptr))
    eng.sync()


power_window()
power_rows()
assert eng.download(d_out_w, 384 * n) == eng.download(d_out_r, 384 * n)

legs = [("gt_pow_plus_gt_mul", power_window), ("gt_pow_rows", power_rows),
        ("encaps_packed", lambda: ghw11.encaps_packed(host, pk, [policy], item_pol)),
        ("encrypt_packed_16B", lambda: ghw11.encrypt_packed(host, pk, [policy], item_pol, pt_blob, pt_off)),
        ("decaps_out_packed", lambda: ghw11.decaps_out_packed(host, rk, tct)),
        ("decrypt_out_packed_16B", lambda: ghw11.decrypt_out_packed(host, rk, tct_ct, ct, ct_off)),
        ("decaps_packed", lambda: ghw11.decaps_packed(host, sk, hdr, hdr_off)),
        ("decrypt_packed_16B", lambda: ghw11.decrypt_packed(host, sk, ct, ct_off))]
times = {leg: [] for leg, _ in legs}
for _ in range(args.rounds):
    for leg, fn in legs:
        t0 = time.perf_counter()
        fn()
        times[leg].append(time.perf_counter() - t0)
line = {"config": "GHW11 key encapsulation, %d items under an AND of %d attributes, one key of each kind: the row power against gt_pow + gt_mul on the "
                  "device, encaps / decaps_out / decaps against encrypt / decrypt_out / decrypt with 16-byte plaintexts, checked mode, legs alternating, "
                  "%d rounds after one warm-up" % (n, args.attrs, args.rounds),
        "scheme": "GHW11", "batch": n, "attributes": args.attrs, "rounds": args.rounds, "keys_equal": True, "powers_equal": True,
        "header_bytes": int(hdr_off[n]), "record_bytes": int(ct_off[n])}
for leg, _ in legs:
    line[leg + "_items_per_s"] = round(n / min(times[leg]), 1)
    line[leg + "_items_per_s_median"] = round(n / statistics.median(times[leg]), 1)
    line[leg + "_s"] = [round(t, 5) for t in times[leg]]
text = json.dumps(line)
print(text, flush=True)
if args.out:
    with open(args.out, "a") as f:
        f.write(text + "\n")
eng.close()
host.close()
