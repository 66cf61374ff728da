#!/usr/bin/env python3
"""GHW11: what a change to a proxy's key store costs, one GPU, one process.  A store of N = --keys (1024) transform keys of 20 attributes (22
blocks each), and per k in --k (1, 16, 256):
  (a) add     TkStore.add of k more keys into the store that stays                          -- the new call
  (b) revoke  TkStore.revoke of those k keys (their lines zeroed on the device)             -- the new call
  (c) create_plus / create_minus: all there was before -- tk_store_create over the N + k (N - k) keys, then the free of the old store
and once
  (d) transform_keyed on --items (16 384) headers spread over the N keys, against the store that was opened and filled by add and against a
      tk_store_create store of the same keys: the same launch set, so no difference beyond the legs' spread is expected; the records of
      the two are compared byte for byte first.
All in the default, checked mode (the membership pass runs).  Every leg is timed around the whole call; add, revoke, create and free return
after their device work.  One warm-up round, then --rounds rounds in which the legs ALTERNATE, so drift on a shared machine falls on all of
them; best and median per leg.  The store is back at its N keys after every round.  One JSON line per k and one for (d), to stdout and
appended to --out.
usage: python tools/bench_ghw11_store.py [--keys 1024] [--k 1,16,256] [--items 16384] [--rounds 5] [--out profiles/ghw11_store_mutable.jsonl]"""
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
ap.add_argument("--keys", type=int, default=1024)
ap.add_argument("--k", default="1,16,256")
ap.add_argument("--items", type=int, default=16384)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default="")
args = ap.parse_args()
N, n = args.keys, args.items
KS = [int(k) for k in args.k.split(",")]
N_ATTR = 20
BLOCKS = N_ATTR + 2


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


def emit(line):
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


def summary(line, times, count):
    for name, t in times.items():
        line[name + "_ms"] = round(1e3 * min(t), 3)
        line[name + "_ms_median"] = round(1e3 * statistics.median(t), 3)
        line[name + "_s"] = [round(x, 5) for x in t]
    line["spread"] = round(max(max(t) / min(t) - 1 for t in times.values()), 3)


host = hl.Host(0)
pk, msk = ghw11.setup(host)
attrs = ["g%02d" % i for i in range(N_ATTR)]
extra = max(KS)
_sk, _so, tk_blob, tk_off, _rk = ghw11.provision_packed(host, pk, msk, [attrs], [0] * (N + extra), want_sk=False)
tk_blob = np.ascontiguousarray(tk_blob).copy()
tk_off = np.ascontiguousarray(tk_off, dtype=np.uint64).copy()


def keys(lo, hi):
    """records lo .. hi - 1 as a blob of their own"""
    a, b = int(tk_off[lo]), int(tk_off[hi])
    return tk_blob[a:b], tk_off[lo:hi + 1] - tk_off[lo]


store = ghw11.tk_store_open(host, (N + extra) * BLOCKS)
ids, st = store.add(*keys(0, N))
assert not st.any() and ids.tolist() == list(range(N)) and store.stat() == (N, (N + extra) * BLOCKS, N * BLOCKS, extra * BLOCKS)

for k in KS:
    old = [ghw11.tk_store_create(host, *keys(0, N))]          # what the yardstick replaces

    def add():
        got, status = store.add(*keys(N, N + k))
        assert not status.any()
        add.ids = got

    def revoke():
        assert not store.revoke(add.ids).any()

    def create(count):
        fresh = ghw11.tk_store_create(host, *keys(0, count))
        old[0].free()
        old[0] = fresh

    legs = [("add", add), ("revoke", revoke), ("create_plus", lambda: create(N + k)), ("create_minus", lambda: create(N - k))]
    for _name, fn in legs:                                     # the warm-up round
        fn()
    assert store.stat()[0] == N
    times = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    assert store.stat() == (N, (N + extra) * BLOCKS, N * BLOCKS, extra * BLOCKS)
    line = {"config": "GHW11 key store of %d transform keys of %d attributes (%d blocks): add and revoke of k keys in place against "
                      "tk_store_create over the N + k / N - k keys plus the free of the old store, checked mode, legs alternating, %d rounds "
                      "after one warm-up" % (N, N_ATTR, N * BLOCKS, args.rounds),
            "keys": N, "attributes": N_ATTR, "k": k, "rounds": args.rounds, "store_bytes": store.nbytes()}
    summary(line, times, k)
    line["add_ms_per_key"] = round(1e3 * min(times["add"]) / k, 4)
    line["revoke_ms_per_key"] = round(1e3 * min(times["revoke"]) / k, 4)
    line["create_plus_over_add"] = round(min(times["create_plus"]) / min(times["add"]), 1)
    line["create_minus_over_revoke"] = round(min(times["create_minus"]) / min(times["revoke"]), 1)
    emit(line)
    old[0].free()

# (d) the transform does not care how the store came to be
policy = '{"name": "and", "children": [%s]}' % ", ".join('{"name": "%s"}' % a for a in attrs)
hdr, hoff, _keys = ghw11.encaps_packed(host, pk, [policy], [0] * n)
hdr = np.ascontiguousarray(hdr).copy()
item_key = np.arange(n, dtype=np.uint32) % N
made = ghw11.tk_store_create(host, *keys(0, N))
legs = [("keyed_mutable", lambda: ghw11.transform_keyed(host, store, item_key, hdr, hoff)),
        ("keyed_created", lambda: ghw11.transform_keyed(host, made, item_key, hdr, hoff))]
first = [fn() for _name, fn in legs]
assert not first[0][1].any() and not first[1][1].any() and (first[0][0] == first[1][0]).all()
del first
times = {name: [] for name, _ in legs}
for _ in range(args.rounds):
    for name, fn in legs:
        t0 = time.perf_counter()
        fn()
        times[name].append(time.perf_counter() - t0)
line = {"config": "GHW11 transform_keyed: %d headers under an AND over %d attributes over %d keys, on the store filled by add against a "
                  "tk_store_create store of the same keys, checked mode, legs alternating, %d rounds after one warm-up" % (n, N_ATTR, N, args.rounds),
        "batch": n, "keys": N, "rounds": args.rounds, "records_equal": True}
summary(line, times, n)
for name in times:
    line[name + "_items_per_s"] = round(n / min(times[name]), 1)
line["ratio"] = round(min(times["keyed_created"]) / min(times["keyed_mutable"]), 3)
line["differs_beyond_spread"] = bool(abs(line["ratio"] - 1) > line["spread"])
emit(line)
made.free()
store.free()
host.close()
