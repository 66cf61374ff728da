#!/usr/bin/env python3
"""GHW11 encrypt rows: the fused row kernel (k_ghw11_enc_rows, one lane per row: share, C = g1_a*lambda + g1*(-H t) on one accumulator,
D = g1*t) against the unfused composition lsw::encrypt_packed uses for its rows -- three rhip_g1_table_mul launches over the same
16-bit tables and one rhip_g1_add -- on the same number of rows, in one process.  Wall times are printed as JSON; per-kernel times come
from running this under `rocprofv3 --kernel-trace --stats -- python tools/bench_ghw11_rows.py`.
usage: python tools/bench_ghw11_rows.py [--items 1024] [--attrs 50] [--reps 3]"""
import argparse
import ctypes
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from rabe_amd import engine as E  # noqa: E402
from rabe_amd import hostlib as hl  # noqa: E402
from rabe_amd.schemes import ghw11  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--items", type=int, default=1024)
ap.add_argument("--attrs", type=int, default=50)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()
PT = b"dance like no one's watching, encrypt like everyone is!"
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def nest(ns):
    if len(ns) == 1:
        return '{"name": "%s"}' % ns[0]
    h = len(ns) // 2
    return '{"name": "and", "children": [%s, %s]}' % (nest(ns[:h]), nest(ns[h:]))


host = hl.Host(0)
pk, _msk = ghw11.setup(host)
n = args.items
rows = n * args.attrs
policy = nest(["g%d" % i for i in range(args.attrs)])
pt_off = np.arange(n + 1, dtype=np.uint64) * len(PT)
fused = []
for _ in range(args.reps + 1):
    t0 = time.perf_counter()
    ghw11.encrypt_packed(host, pk, [policy], [0] * n, PT * n, pt_off)
    fused.append(time.perf_counter() - t0)

# the composition on a device context of its own: C = g1_a*k0 + g1*k1, D = g1*k2
eng = E.Engine(0)
g = hl.parse_obj("ghw11_pk", pk.serialize())
t_g1, t_g1a = eng.g1_table(g["g1"]), eng.g1_table(g["g1_a"])
t_g1.add_w16()
t_g1a.add_w16()
rnd = random.Random(1)
ks = [eng.upload(b"".join(rnd.randrange(R).to_bytes(32, "little") for _ in range(rows))) for _ in range(3)]
outs = [eng.alloc(rows * 64) for _ in range(4)]
lib = eng.lib


def composition():
    eng._check(lib.rhip_g1_table_mul(eng.ctx, t_g1a.h, ctypes.c_size_t(rows), ks[0].ptr, outs[0].ptr))
    eng._check(lib.rhip_g1_table_mul(eng.ctx, t_g1.h, ctypes.c_size_t(rows), ks[1].ptr, outs[1].ptr))
    eng._check(lib.rhip_g1_table_mul(eng.ctx, t_g1.h, ctypes.c_size_t(rows), ks[2].ptr, outs[2].ptr))
    eng._check(lib.rhip_g1_add(eng.ctx, ctypes.c_size_t(rows), outs[0].ptr, outs[1].ptr, outs[3].ptr))
    eng.sync()


comp = []
for _ in range(args.reps + 1):
    t0 = time.perf_counter()
    composition()
    comp.append(time.perf_counter() - t0)
print(json.dumps({"items": n, "attrs": args.attrs, "rows": rows, "encrypt_packed_s_best": round(min(fused[1:]), 4),
                  "encrypts_per_s": round(n / min(fused[1:]), 1), "composition_rows_s_best": round(min(comp[1:]), 4),
                  "note": "per-kernel times: rocprofv3 --kernel-trace --stats (k_ghw11_enc_rows vs 3 x k_table_mul_g1 + k_g1_add)"}), flush=True)
for t in (t_g1, t_g1a):
    t.destroy()
eng.close()
host.close()
