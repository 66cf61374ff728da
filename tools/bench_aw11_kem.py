#!/usr/bin/env python3
"""AW11 as a key encapsulation against the packed calls it spares a caller, one GPU, one process, --items items (16 384) under one policy, a
tree of binary ANDs over --rows attributes (20, 200) of one authority, the key holding all of them:
  lead      the leading factor c_0 * prod C1^-c alone, on the same device-resident terms (the gathered C1 rows of the records of (b)): the
            width-4 window kernels (k_gtmexp4_digits + k_gtmexp4_table + k_gt_mexp4_partial + k_gt_mexp4_finish: decaps_packed under
            RABE_AW11_LEAD_W4=1) against k_gt_multiexp_partial + k_gt_lead (decaps_packed as it ships); HIP-event times of those kernels,
            taken from the host's launch record in rounds of their own
  (a) aw11.encaps_packed                     against (b) aw11.encrypt_packed with 16-byte plaintexts
  (c) aw11.decaps_packed on the records of (b) against (d) aw11.decrypt_packed on the same records
  (e) aw11.decaps_packed under RABE_AW11_LEAD_W4=1 on the same records, against (c)
Every host leg is timed around its whole call, in the default, checked mode, with the launch record off.  One warm-up round, then --rounds
rounds in which the legs ALTERNATE, so drift on a shared machine falls on all of them; best and median per leg and each leg's spread
(max / min - 1) (docs/measurement.md).  Before the timing the headers of an encaps are decapsulated and the keys compared, and decrypt_packed
has to return the plaintexts.  One JSON line, to stdout and appended to --out.
usage: python tools/bench_aw11_kem.py [--items 16384] [--rows 20] [--rounds 5] [--out profiles/aw11_kem_packed.jsonl]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rabe_amd import hostlib as hl  # noqa: E402
from rabe_amd.schemes import aw11  # noqa: E402

W4 = ("k_gtmexp4_digits", "k_gtmexp4_table", "k_gt_mexp4_partial", "k_gt_mexp4_finish")
NAF = ("k_gt_multiexp_partial", "k_gt_lead")
ap = argparse.ArgumentParser()
ap.add_argument("--items", type=int, default=16384)
ap.add_argument("--rows", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default="")
args = ap.parse_args()
n, m = args.items, args.rows
host = hl.Host(0)
attrs = ["G%03d" % i for i in range(m)]


def and_tree(names):
    """a balanced tree of binary ANDs (the scheme's MSP conversion takes two children per gate)"""
    if len(names) == 1:
        return '{"name": "%s"}' % names[0]
    half = len(names) // 2
    return '{"name": "and", "children": [%s, %s]}' % (and_tree(names[:half]), and_tree(names[half:]))


policy = and_tree(attrs)
gk = aw11.setup(host)
pk, msk = aw11.authgen(host, gk, attrs)
sk = aw11.keygen(host, gk, msk, "alice", attrs)
pt_blob = np.frombuffer(b"".join(b"%016d" % i for i in range(n)), dtype=np.uint8)
pt_off = (16 * np.arange(n + 1)).astype(np.uint64)
item_pol = [0] * n


def kernel_ms():
    """drains the host's launch record -> {kernel name: total ms}"""
    buf = ctypes.create_string_buffer(1 << 16)
    hl._check(host.lib.rabe_host_kernel_timing_read(host.h, buf, ctypes.c_size_t(len(buf))), host.h)
    return {f[0]: float(f[1]) for f in (line.split() for line in buf.value.decode().splitlines()) if len(f) == 3}


# the warm-up round, and the comparisons
hdr, hdr_off, keys = aw11.encaps_packed(host, gk, [pk], [policy], item_pol)
back, st = aw11.decaps_packed(host, gk, sk, hdr, hdr_off)
assert (st == 0).all() and (back == keys).all()
hdr_bytes = int(hdr_off[n])
del hdr, hdr_off, keys, back
ct, ct_off = aw11.encrypt_packed(host, gk, [pk], [policy], item_pol, pt_blob, pt_off)
ct = ct.copy()


def decaps_w4():
    os.environ["RABE_AW11_LEAD_W4"] = "1"
    try:
        return aw11.decaps_packed(host, gk, sk, ct, ct_off)
    finally:
        del os.environ["RABE_AW11_LEAD_W4"]


k_naf, st = aw11.decaps_packed(host, gk, sk, ct, ct_off)
assert (st == 0).all()
k_naf = k_naf.copy()
k_w4, st = decaps_w4()
assert (st == 0).all() and (k_w4 == k_naf).all()
pt, po, st = aw11.decrypt_packed(host, gk, sk, ct, ct_off)
assert (st == 0).all() and bytes(pt) == bytes(pt_blob)
del pt, po, st

legs = [("aw11_encaps_packed", lambda: aw11.encaps_packed(host, gk, [pk], [policy], item_pol)),
        ("aw11_encrypt_packed_16B", lambda: aw11.encrypt_packed(host, gk, [pk], [policy], item_pol, pt_blob, pt_off)),
        ("aw11_decaps_packed", lambda: aw11.decaps_packed(host, gk, sk, ct, ct_off)),
        ("aw11_decrypt_packed_16B", lambda: aw11.decrypt_packed(host, gk, sk, ct, ct_off)),
        ("aw11_decaps_packed_lead_w4", decaps_w4)]
times = {leg: [] for leg, _ in legs}
for _ in range(args.rounds):
    for leg, fn in legs:
        t0 = time.perf_counter()
        fn()
        times[leg].append(time.perf_counter() - t0)

# the lead stage: event times of the two kernel sets on the same gathered terms, alternating, the launch record on
lead = {"lead_w4": [], "lead_naf": []}
parts = {}
host.kernel_timing(True)
kernel_ms()
for _ in range(args.rounds):
    got, st = decaps_w4()
    assert (got == k_naf).all()
    ms = kernel_ms()
    assert all(k in ms for k in W4) and not [k for k in NAF if k in ms], sorted(ms)
    lead["lead_w4"].append(sum(ms[k] for k in W4) / 1e3)
    parts.setdefault("w4", []).append({k: round(ms[k], 3) for k in W4})
    aw11.decaps_packed(host, gk, sk, ct, ct_off)
    ms = kernel_ms()
    assert all(k in ms for k in NAF) and not [k for k in W4 if k in ms], sorted(ms)
    lead["lead_naf"].append(sum(ms[k] for k in NAF) / 1e3)
    parts.setdefault("naf", []).append({k: round(ms[k], 3) for k in NAF})
host.kernel_timing(False)
kernel_ms()
times.update(lead)

line = {"config": "AW11 key encapsulation, %d items under a tree of binary ANDs over %d attributes of one authority: the leading factor over width-4 windows "
                  "against k_gt_multiexp_partial + k_gt_lead on the same gathered terms (HIP-event kernel times, terms per second), encaps / decaps "
                  "against encrypt / decrypt with 16-byte plaintexts (items per second), checked mode, legs alternating, %d rounds after one "
                  "warm-up" % (n, m, args.rounds),
        "schemes": ["AW11"], "batch": n, "rows": m, "terms": n * m, "rounds": args.rounds, "keys_equal": True, "header_bytes": hdr_bytes,
        "record_bytes": int(ct_off[n]), "lead_w4_kernels_ms_best_round": min(parts["w4"], key=lambda p: sum(p.values())),
        "lead_naf_kernels_ms_best_round": min(parts["naf"], key=lambda p: sum(p.values()))}
for leg in times:
    unit, count = ("_terms_per_s", n * m) if leg.startswith("lead") else ("_items_per_s", n)
    line[leg + unit] = round(count / min(times[leg]), 1)
    line[leg + unit + "_median"] = round(count / statistics.median(times[leg]), 1)
    line[leg + "_spread"] = round(max(times[leg]) / min(times[leg]) - 1, 4)
    line[leg + "_s"] = [round(t, 5) for t in times[leg]]
for a, b in (("lead_w4", "lead_naf"), ("aw11_encaps_packed", "aw11_encrypt_packed_16B"), ("aw11_decaps_packed", "aw11_decrypt_packed_16B"),
             ("aw11_decaps_packed_lead_w4", "aw11_decaps_packed")):
    line[a + "_over_" + b + "_best"] = round(min(times[b]) / min(times[a]), 4)
    line[a + "_over_" + b + "_median"] = round(statistics.median(times[b]) / statistics.median(times[a]), 4)
text = json.dumps(line)
print(text, flush=True)
if args.out:
    with open(args.out, "a") as f:
        f.write(text + "\n")
host.close()
