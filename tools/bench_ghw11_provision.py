#!/usr/bin/env python3
"""GHW11 bulk provisioning against the two calls it fuses, one GPU, one process: --keys keys (16 384) of 50 and of 100 attributes through
  (a) provision_packed, secret + transform + retrieve keys
  (b) provision_packed, transform + retrieve keys only
  (c) keygen_packed, then tkgen_packed(trusted) on its output          -- the yardstick: both are what they were before (a) existed
Every leg is timed around the whole call (the calls end in a copy out, which waits for the device); OS randomness, as a service draws.
One warm-up round (window tables, arenas, pinned staging), then --rounds rounds in which the three legs ALTERNATE, so drift on a shared
machine falls on all of them; best and median per leg.  Before the timing, one tape drives (a), (b) and (c) at the timed size and the
bytes are compared: faster and different would not be faster.  One JSON line per attribute count, to stdout and appended to --out.
usage: python tools/bench_ghw11_provision.py [--keys 16384] [--rounds 5] [--out profiles/ghw11_provision_packed.jsonl]"""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rabe_amd import hostlib as hl  # noqa: E402
from rabe_amd.schemes import ghw11  # noqa: E402

R_ORDER = 21888242871839275222246405745257275088548364400416034343698204186575808495617
ap = argparse.ArgumentParser()
ap.add_argument("--keys", type=int, default=16384)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default="")
args = ap.parse_args()
n = args.keys
host = hl.Host(0)
pk, msk = ghw11.setup(host)


def both(attrs):
    return ghw11.provision_packed(host, pk, msk, [attrs], [0] * n)


def tk_only(attrs):
    return ghw11.provision_packed(host, pk, msk, [attrs], [0] * n, want_sk=False)


def two_calls(attrs):
    blob, off = ghw11.keygen_packed(host, pk, msk, [attrs], [0] * n)
    tkb, to, rk, st = ghw11.tkgen_packed(host, blob, off, trusted=True)
    return blob, off, tkb, to, rk


LEGS = (("provision_both", both), ("provision_tk_only", tk_only), ("keygen_then_tkgen_trusted", two_calls))
for n_attr in (50, 100):
    attrs = ["g%03d" % i for i in range(n_attr)]
    rnd = random.Random(n_attr)
    tape = [rnd.randrange(1, R_ORDER) for _ in range(2 * n)]
    got = []
    for _name, fn in LEGS:                               # also the warm-up round
        host.set_tape(tape)
        got.append(fn(attrs))
        host.clear_tape()
    a, b, c = got
    assert bytes(a[0]) == bytes(c[0]) and a[1].tolist() == c[1].tolist(), "secret keys differ from keygen_packed's"
    assert bytes(a[2]) == bytes(c[2]) == bytes(b[2]) and a[3].tolist() == c[3].tolist() == b[3].tolist(), "transform keys differ from tkgen_packed's"
    assert a[4].tobytes() == c[4].tobytes() == b[4].tobytes(), "retrieve keys differ"
    del got, a, b, c
    times = {name: [] for name, _ in LEGS}
    for _ in range(args.rounds):
        for name, fn in LEGS:
            t0 = time.perf_counter()
            fn(attrs)
            times[name].append(time.perf_counter() - t0)
    line = {"config": "GHW11 provisioning, %d keys of %d attributes: provision_packed (both outputs; transform keys only) against keygen_packed + "
                      "tkgen_packed(trusted), legs alternating, %d rounds after one warm-up" % (n, n_attr, args.rounds),
            "batch": n, "attributes": n_attr, "rounds": args.rounds, "bytes_equal_on_one_tape": True}
    for name, _ in LEGS:
        line[name + "_keys_per_s"] = round(n / min(times[name]), 1)
        line[name + "_keys_per_s_median"] = round(n / statistics.median(times[name]), 1)
        line[name + "_s"] = [round(t, 4) for t in times[name]]
    base = min(times["keygen_then_tkgen_trusted"])
    line["ratio_both"] = round(base / min(times["provision_both"]), 2)
    line["ratio_tk_only"] = round(base / min(times["provision_tk_only"]), 2)
    line["ratio_both_median"] = round(statistics.median(times["keygen_then_tkgen_trusted"]) / statistics.median(times["provision_both"]), 2)
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")
host.close()
