#!/usr/bin/env python3
"""GHW11: a proxy's mixed queue in one call against the best a caller could do before, one GPU, one process: --items headers (16 384) under an
AND over 20 attributes, spread evenly over U = 1, 64 and 1024 users' transform keys (provision_packed's blob, loaded once into a store), through
  (a) transform_keyed on the queue as it is                                            -- the new call
  (b) one transform_packed per key over that key's items, the queue sorted by key      -- the yardstick
Both legs run in the default, checked mode and are timed around the whole call sequence (every call ends in a copy out, which waits for the
device).  (b) is handed its per-key blobs, offsets and key objects ready made: the sort is not timed, the scatter of the 768-byte records
back into queue order is (a caller needs them there); at U = 1 (b) is the one-key call on the queue itself.  The one-key call keeps the prepared
lines of FOUR keys across calls, so with more users than that (b) prepares a key's lines in every call -- that is what the one-key call costs
a proxy with many users, and part of what is measured.  One warm-up round per leg, in which the records of the two legs are compared byte for
byte (faster and different would not be faster), then --rounds rounds in which the legs ALTERNATE, so drift on a shared machine falls on
both; best and median per leg.  At U = 1 the two legs are the same launch set but for the gather kernel: the line's `spread` is the larger
relative spread (max / min - 1) of the two legs' times, and `slower_beyond_spread` says whether the new call's best time exceeds the
yardstick's by more than that -- at U = 1 that fails the run (exit status 1), at the other U it is written down.  One JSON line per U, to
stdout and appended to --out.
usage: python tools/bench_ghw11_keyed.py [--items 16384] [--rounds 5] [--users 1,64,1024] [--out profiles/ghw11_transform_keyed.jsonl]"""
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
ap.add_argument("--users", default="1,64,1024")
ap.add_argument("--out", default="")
args = ap.parse_args()
n = args.items
N_ATTR = 20


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


host = hl.Host(0)
pk, msk = ghw11.setup(host)
attrs = ["g%02d" % i for i in range(N_ATTR)]
policy = '{"name": "and", "children": [%s]}' % ", ".join('{"name": "%s"}' % a for a in attrs)
hdr, hoff, _keys = ghw11.encaps_packed(host, pk, [policy], [0] * n)
hdr = np.ascontiguousarray(hdr).copy()
failed = False
for users in [int(u) for u in args.users.split(",")]:
    _sk, _so, tk_blob, tk_off, _rk = ghw11.provision_packed(host, pk, msk, [attrs], [0] * users, want_sk=False)
    store = ghw11.tk_store_create(host, tk_blob, tk_off)
    assert not store.key_status.any()
    item_key = np.arange(n, dtype=np.uint32) % users          # user u owns items u, u + U, ...: a queue in arrival order
    per_key = []                                               # the sorted queue, cut per key (untimed)
    for u in range(users):
        mine = np.arange(u, n, users)
        recs = [hdr[int(hoff[i]):int(hoff[i + 1])] for i in mine]
        tk = hl.Obj.deserialize("ghw11_tk", bytes(tk_blob[int(tk_off[u]):int(tk_off[u + 1])]))
        per_key.append((mine, tk, np.concatenate(recs), offsets([r.size for r in recs])))

    def keyed():
        return ghw11.transform_keyed(host, store, item_key, hdr, hoff)

    def per_key_calls():
        if users == 1:                                         # nothing to sort back: the one-key call on the queue as it is
            return ghw11.transform_packed(host, per_key[0][1], hdr, hoff)
        out = np.zeros((n, 768), dtype=np.uint8)
        status = np.zeros(n, dtype=np.int32)
        for mine, tk, blob, off in per_key:
            o, s = ghw11.transform_packed(host, tk, blob, off)
            out[mine], status[mine] = o, s
        return out, status

    legs = [("transform_keyed", keyed), ("transform_packed_per_key", per_key_calls)]
    first = [fn() for _name, fn in legs]                       # the warm-up round, and the comparison
    assert not first[0][1].any() and not first[1][1].any()
    assert (first[0][0] == first[1][0]).all()
    del first
    times = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    line = {"config": "GHW11 transform of a mixed queue: %d headers under an AND over %d attributes, spread evenly over %d transform keys; "
                      "transform_keyed against one transform_packed per key on the sorted queue, checked mode, legs alternating, %d rounds "
                      "after one warm-up" % (n, N_ATTR, users, args.rounds),
            "batch": n, "attributes": N_ATTR, "users": users, "rounds": args.rounds, "records_equal": True, "store_bytes": store.nbytes()}
    for name, _ in legs:
        line[name + "_items_per_s"] = round(n / min(times[name]), 1)
        line[name + "_items_per_s_median"] = round(n / statistics.median(times[name]), 1)
        line[name + "_s"] = [round(t, 4) for t in times[name]]
    line["ratio"] = round(min(times["transform_packed_per_key"]) / min(times["transform_keyed"]), 2)
    line["ratio_median"] = round(statistics.median(times["transform_packed_per_key"]) / statistics.median(times["transform_keyed"]), 2)
    line["spread"] = round(max(max(t) / min(t) - 1 for t in times.values()), 3)
    # the bar at U = 1: the new call's best time is not above the one-key call's by more than the legs' own spread
    line["slower_beyond_spread"] = bool(min(times["transform_keyed"]) > min(times["transform_packed_per_key"]) * (1 + line["spread"]))
    failed = failed or (users == 1 and line["slower_beyond_spread"])
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")
    store.free()
host.close()
sys.exit(1 if failed else 0)
