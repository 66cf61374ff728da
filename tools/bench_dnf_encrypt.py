#!/usr/bin/env python3
"""BDABE / MKE08 packed encrypt (rabe_{bdabe,mke08}_encrypt_packed): one policy of --terms terms over one authority's attribute keys,
--items items per call.  The first call of a policy folds its terms and builds their window tables (k_dnf_tables_g1, k_attr_tables_g2,
k_attr_tables_gt); the timed calls after it find them cached.  Wall times are printed as JSON; per-kernel times come from running this
under `rocprofv3 --kernel-trace --stats -- python tools/bench_dnf_encrypt.py`.
usage: python tools/bench_dnf_encrypt.py [--items 65536] [--terms 8] [--reps 3] [--only bdabe|mke08]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from rabe_amd import hostlib as hl  # noqa: E402
from rabe_amd.schemes import bdabe, mke08  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--items", type=int, default=65536)
ap.add_argument("--terms", type=int, default=8)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--only", default="")
args = ap.parse_args()
PT = b"dance like no one's watching, encrypt like everyone is!"
host = hl.Host(0)
for scheme in ("bdabe", "mke08"):
    if args.only and args.only != scheme:
        continue
    names = ["aa1::T%d" % i for i in range(args.terms)]
    if scheme == "bdabe":
        mod = bdabe
        pk, msk = bdabe.setup(host)
        au = bdabe.authgen(host, pk, msk, "aa1")
        keys = [bdabe.request_attribute_pk(host, pk, au, n) for n in names]
    else:
        mod = mke08
        pk, msk = mke08.setup(host)
        au = mke08.authgen(host, "aa1")
        keys = [mke08.request_authority_pk(host, pk, n, au) for n in names]
    pol = '{"name": "or", "children": [%s]}' % ", ".join('{"name": "%s"}' % n for n in names) if args.terms > 1 else '{"name": "%s"}' % names[0]
    n = args.items
    pt_off = np.arange(n + 1, dtype=np.uint64) * len(PT)
    t0 = time.perf_counter()
    mod.encrypt_packed(host, pk, keys, [pol], [0] * n, PT * n, pt_off)
    first = time.perf_counter() - t0
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        blob, off = mod.encrypt_packed(host, pk, keys, [pol], [0] * n, PT * n, pt_off)
        times.append(time.perf_counter() - t0)
    print(json.dumps({"scheme": scheme, "items": n, "terms": args.terms, "rows": n * args.terms, "first_call_s": round(first, 4),
                      "seconds": [round(t, 4) for t in times], "encrypts_per_s": round(n / min(times), 1), "record_bytes": int(blob.size)}), flush=True)
host.close()
