#!/usr/bin/env python3
"""LSW decrypt of many ciphertexts under ONE key: a flat AND of m leaves against --items ciphertexts of m attributes, m = 50 and 200.
Per shape, one JSON line per path:
  packed   rabe_lsw_decrypt_one_sk_packed on the records rabe_lsw_encrypt_packed wrote, checked and trusted decode
  one_sk   rhip_lsw_decrypt_batch_one_sk on the elements of those records (key-side Miller loops on prepared lines, one shared sum)
  general  rhip_lsw_decrypt_batch with sk_idx = all zero on the same device arrays
Not the judged metric (bench.py is config 2).  Warm-up call, then the best of --reps, timed around call + sync; the two device paths
must return the same bytes.
usage: python tools/bench_lsw_one_sk.py [--items 16384] [--out profiles/lsw_one_sk_packed.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rabe_amd import Engine  # noqa: E402
from rabe_amd import engine as E  # noqa: E402
from rabe_amd import hostlib as hl  # noqa: E402
from rabe_amd import hostprep as hp  # noqa: E402
from rabe_amd.schemes import lsw  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--items", type=int, default=16384)
ap.add_argument("--shapes", default="50,200")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default="")
args = ap.parse_args()
N = args.items
PT = b"dance like no one's watching, encrypt like everyone is!"


def best_of(fn):
    fn()
    best, r = None, None
    for _ in range(args.reps):
        t0 = time.perf_counter()
        r = fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, r


def emit(line):
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


host = hl.Host(0)
eng = Engine(0)
pk, msk = lsw.setup(host)
for m in [int(x) for x in args.shapes.split(",")]:
    attrs = ["c%03d" % i for i in range(m)]          # names of one length: the records' elements sit at a fixed stride
    policy = '{"name": "and", "children": [%s]}' % ", ".join('{"name": "%s"}' % a for a in attrs)
    sk = lsw.keygen(host, pk, msk, policy, hl.JSON_POLICY)
    blob, off = lsw.encrypt_packed(host, pk, [attrs], [0] * N, PT * N, np.arange(N + 1, dtype=np.uint64) * len(PT))
    blob = np.ascontiguousarray(blob)
    buf = np.zeros(blob.size, dtype=np.uint8)
    t = {}
    for trusted in (False, True):
        t[trusted], (out, oo, st) = best_of(lambda: lsw.decrypt_one_sk_packed(host, sk, blob, off, out=buf, trusted=trusted))
        assert not st.any() and out.tobytes() == PT * N
    shape = "flat AND of %d leaves, %d ciphertexts of %d attributes" % (m, N, m)
    emit({"config": "LSW one key, packed (rabe_lsw_decrypt_one_sk_packed): " + shape, "path": "packed", "m": m, "batch": N,
          "decrypts_per_s": round(N / t[False], 1), "decrypts_per_s_trusted": round(N / t[True], 1), "seconds": round(t[False], 4),
          "seconds_trusted": round(t[True], 4), "record_bytes": int(blob.size)})
    # ---- the two device-level paths on the elements of these records
    rec = int(off[1])
    view = blob.reshape(N, rec)
    row = 4 + len(attrs[0]) + 192
    e1j = np.ascontiguousarray(view[:, 516:516 + m * row].reshape(N, m, row)[:, :, 4 + len(attrs[0]):4 + len(attrs[0]) + 64])
    key = hl.parse_obj("lsw_sk", sk.serialize())["dj"]
    assert [r[0] for r in key] == attrs
    z = hp.leaf_coefficients(("and", [("leaf", a) for a in attrs]))
    d = dict(pair_off=eng.upload_u32([i * (m + 1) for i in range(N + 1)]), sel_start=eng.upload_u32([0] * N), sel_sk=eng.upload_u32(list(range(m))),
             sel_ct=eng.upload_u32(list(range(m))), sel_z=eng.upload(b"".join(hp.fr_le(c) for c in z)),
             e1=eng.upload(np.ascontiguousarray(view[:, :384]).tobytes()), e2=eng.upload(np.ascontiguousarray(view[:, 384:512]).tobytes()),
             e1j=eng.upload(e1j.tobytes()), attr_off=eng.upload_u32([i * m for i in range(N + 1)]), d1=eng.upload(b"".join(r[1] for r in key)),
             d2=eng.upload(b"".join(r[2] for r in key)), leaf_off=eng.upload_u32([0, m]), zeros=eng.upload_u32([0] * N),
             group_off=eng.upload_u32([0, m]))
    del e1j
    lines = E.G2Lines(eng, m, d["d2"])
    out_a, out_b = eng.alloc(N * 384), eng.alloc(N * 384)

    def run_one_sk():
        E.lsw_decrypt_one_sk_dev(eng, N, m + 1, N * (m + 1), m, d["pair_off"], d["sel_start"], d["sel_sk"], d["sel_ct"], d["sel_z"], 1, d["group_off"],
                                 d["zeros"], d["e1"], d["e2"], d["e1j"], d["attr_off"], d["d1"], lines, out_a)
        eng.sync()

    def run_general():
        E.lsw_decrypt_dev(eng, N, m + 1, N * (m + 1), m, d["pair_off"], d["sel_start"], d["sel_sk"], d["sel_ct"], d["sel_z"], d["e1"], d["e2"], d["e1j"],
                          d["attr_off"], None, d["d1"], d["d2"], d["leaf_off"], d["zeros"], None, out_b)
        eng.sync()
    t_one, _ = best_of(run_one_sk)
    t_gen, _ = best_of(run_general)
    assert eng.download(out_a) == eng.download(out_b)
    emit({"config": "LSW one key, device level (rhip_lsw_decrypt_batch_one_sk): " + shape, "path": "one_sk", "m": m, "batch": N,
          "items_per_s": round(N / t_one, 1), "seconds": round(t_one, 4), "ratio_to_general": round(t_gen / t_one, 3)})
    emit({"config": "LSW one key, device level (rhip_lsw_decrypt_batch, sk_idx = 0, the same arrays): " + shape, "path": "general", "m": m, "batch": N,
          "items_per_s": round(N / t_gen, 1), "seconds": round(t_gen, 4)})
    lines.destroy()
    for b in list(d.values()) + [out_a, out_b]:
        if hasattr(b, "free"):
            b.free()
eng.close()
host.close()
