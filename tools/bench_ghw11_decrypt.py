#!/usr/bin/env python3
"""GHW11 decrypt for a key holder without a proxy against the three calls it replaces, one GPU, one process: --items ciphertexts (16 384)
under a policy of 50 and of 100 attributes (an AND over all of them: every row is selected), one secret key, through
  (a) decrypt_packed                                                   -- the new call
  (b) tkgen, transform_packed, decrypt_out_packed on the same blob     -- the yardstick: what a key holder had to run before
Both legs are timed around the whole call sequence (every call ends in a copy out, which waits for the device) and run in the default,
checked mode.  One warm-up round (prepared lines of both keys, arenas, pinned staging; (b) draws a new z per round, as a holder without a
stored transform key would, so its lines are prepared in every round -- that is part of what it costs), then --rounds rounds in which the
two legs ALTERNATE, so drift on a shared machine falls on both; best and median per leg.  Before the timing the plaintexts of both legs are
compared with each other and with what was encrypted: faster and different would not be faster.  With --stored-tk a third leg keeps ONE
transform / retrieve key pair across rounds (a holder who ran tkgen once and stored the pair): transform_packed + decrypt_out_packed only.
One JSON line per attribute count, to stdout and appended to --out.
usage: python tools/bench_ghw11_decrypt.py [--items 16384] [--rounds 5] [--stored-tk] [--out profiles/ghw11_decrypt_packed.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rabe_amd import hostlib as hl  # noqa: E402
from rabe_amd.schemes import ghw11  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--items", type=int, default=16384)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--stored-tk", action="store_true")
ap.add_argument("--out", default="")
args = ap.parse_args()
n = args.items
host = hl.Host(0)
pk, msk = ghw11.setup(host)
for n_attr in (50, 100):
    attrs = ["g%03d" % i for i in range(n_attr)]
    policy = '{"name": "and", "children": [%s]}' % ", ".join('{"name": "%s"}' % a for a in attrs)
    sk = ghw11.keygen(host, pk, msk, attrs)
    pts = [b"item %06d of the holder's mail" % i for i in range(n)]
    pt_off = np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.uint64)
    blob, off = ghw11.encrypt_packed(host, pk, [policy], [0] * n, b"".join(pts), pt_off)
    stored = ghw11.tkgen(host, sk)

    def direct():
        return ghw11.decrypt_packed(host, sk, blob, off)

    def three_calls():
        tk, rk = ghw11.tkgen(host, sk)
        tct, _st = ghw11.transform_packed(host, tk, blob, off)
        return ghw11.decrypt_out_packed(host, rk, tct, blob, off)

    def two_calls_stored_tk():
        tct, _st = ghw11.transform_packed(host, stored[0], blob, off)
        return ghw11.decrypt_out_packed(host, stored[1], tct, blob, off)

    legs = [("decrypt_packed", direct), ("tkgen_transform_decrypt_out", three_calls)]
    if args.stored_tk:
        legs.append(("transform_decrypt_out_stored_tk", two_calls_stored_tk))
    for _name, fn in legs:                               # the warm-up round, and the comparison
        pt, po, status = fn()
        assert (status == 0).all() and bytes(pt) == b"".join(pts) and po.tolist() == pt_off.tolist(), _name
    del pt, po, status
    times = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    line = {"config": "GHW11 decrypt without a proxy, %d ciphertexts of %d attributes under one secret key: decrypt_packed against tkgen + "
                      "transform_packed + decrypt_out_packed, checked mode, legs alternating, %d rounds after one warm-up" % (n, n_attr, args.rounds),
            "batch": n, "attributes": n_attr, "rounds": args.rounds, "plaintexts_equal": True}
    for name, _ in legs:
        line[name + "_items_per_s"] = round(n / min(times[name]), 1)
        line[name + "_items_per_s_median"] = round(n / statistics.median(times[name]), 1)
        line[name + "_s"] = [round(t, 4) for t in times[name]]
    line["ratio"] = round(min(times["tkgen_transform_decrypt_out"]) / min(times["decrypt_packed"]), 2)
    line["ratio_median"] = round(statistics.median(times["tkgen_transform_decrypt_out"]) / statistics.median(times["decrypt_packed"]), 2)
    if args.stored_tk:
        line["ratio_stored_tk"] = round(min(times["transform_decrypt_out_stored_tk"]) / min(times["decrypt_packed"]), 2)
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")
host.close()
