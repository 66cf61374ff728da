#!/usr/bin/env python3
"""BDABE / MKE08 as a key encapsulation against the packed calls it spares a caller, one GPU, one process, --items items (16 384) under one
policy, a conjunction of --attrs attributes (1, 3, 8) of one authority, the user key holding all of them:
  (a) encaps_packed                              against (b) encrypt_packed with 16-byte plaintexts
  (c) decaps_packed on the records of (b)        against (d) decrypt_packed on the same records
  stage  rhip_dnf_decrypt_batch_one_uk (four Miller loops per item, two on prepared lines) against rhip_pairing_jobs as decrypt_packed's
         plan fills it (m + 3 Miller loops per item), on the same device-resident elements of the records of (b); timed around the call and a
         4-byte download that waits for it
Every leg is timed around its whole call, with the launch record off.  One warm-up round, then --rounds rounds in which the legs ALTERNATE, so
drift on a shared machine falls on all of them; best and median per leg and each leg's spread (max / min - 1) (docs/measurement.md).  Before
the timing the headers of an encaps are decapsulated and the keys compared, every full record has to decapsulate, decrypt_packed has to return
the plaintexts, and the two stage legs have to agree byte for byte (MKE08: both take j1 as the leading factor; the product j1 j2 is one
rhip_gt_mul in front of either).  One JSON line per scheme, to stdout and appended to --out.
usage: python tools/bench_dnf_kem.py [--scheme both] [--items 16384] [--attrs 3] [--rounds 5] [--out profiles/dnf_kem_packed.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rabe_amd import Engine  # noqa: E402
from rabe_amd import engine as E  # noqa: E402
from rabe_amd import hostlib as hl  # noqa: E402
from rabe_amd.schemes import bdabe, mke08  # noqa: E402

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
ap = argparse.ArgumentParser()
ap.add_argument("--scheme", default="both", choices=["bdabe", "mke08", "both"])
ap.add_argument("--items", type=int, default=16384)
ap.add_argument("--attrs", type=int, default=3)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default="")
args = ap.parse_args()
n, m = args.items, args.attrs
attrs = ["aa1::B%d" % i for i in range(m)]
leaves = ", ".join('{"name": "%s"}' % a for a in attrs)
policy = leaves if m == 1 else '{"name": "and", "children": [%s]}' % leaves
pt_blob = np.frombuffer(b"".join(b"%016d" % i for i in range(n)), dtype=np.uint8)
pt_off = (16 * np.arange(n + 1)).astype(np.uint64)
item_pol = [0] * n


def run(name):
    mod, n_gt = (bdabe, 1) if name == "bdabe" else (mke08, 2)
    host = hl.Host(0)
    pk, msk = mod.setup(host)
    if name == "bdabe":
        ska = bdabe.authgen(host, pk, msk, "aa1")
        pkas = [bdabe.request_attribute_pk(host, pk, ska, a) for a in attrs]
        uk = bdabe.keygen(host, pk, ska, "u1")
        for a in attrs:
            bdabe.request_attribute_sk(host, uk, ska, a)
    else:
        ska = mke08.authgen(host, "aa1")
        pkas = [mke08.request_authority_pk(host, pk, a, ska) for a in attrs]
        uk = mke08.keygen(host, pk, msk, "user1")
        for a in attrs:
            mke08.request_authority_sk(host, uk, a, ska)
    # the warm-up round, and the comparisons
    hdr, hdr_off, keys = mod.encaps_packed(host, pk, pkas, [policy], item_pol)
    back, st = mod.decaps_packed(host, uk, hdr, hdr_off)
    assert (st == 0).all() and (back == keys).all()
    hdr_bytes = int(hdr_off[n])
    del hdr, hdr_off, keys, back
    ct, ct_off = mod.encrypt_packed(host, pk, pkas, [policy], item_pol, pt_blob, pt_off)
    ct = ct.copy()
    k_full, st = mod.decaps_packed(host, uk, ct, ct_off)
    assert (st == 0).all()
    pt, _po, st = mod.decrypt_packed(host, uk, ct, ct_off)
    assert (st == 0).all() and bytes(pt) == bytes(pt_blob)
    del pt, _po

    # the decrypt stage alone: every record has one skeleton, so its elements sit at fixed offsets of equally long records
    rec_len = int(ct_off[1])
    assert (np.diff(ct_off.astype(np.int64)) == rec_len).all()
    recs = ct.reshape(n, rec_len)
    at = 4 + len(policy) + 1 + 4 + 4 + sum(4 + len(a) for a in attrs)          # policy, language, conjunction count, the one list of names
    g = at + 384 * n_gt
    lead, e2, e3, e4, e5 = recs[:, at:at + 384], recs[:, g:g + 64], recs[:, g + 64:g + 192], recs[:, g + 192:g + 256], recs[:, g + 256:g + 384]
    key = hl.parse_obj(name + "_uk", uk.serialize())
    u1, u2 = (key["sk"]["u1"], key["sk"]["u2"]) if name == "bdabe" else (key["sk"]["g1"], key["sk"]["g2"])
    rows = key["sk_a"]
    eng = Engine(0)
    s1, s2 = rows[0][1], rows[0][2]
    for r in rows[1:]:
        s1, s2 = eng.g1_add([s1], [r[1]])[0], eng.g2_add([s2], [r[2]])[0]
    lines = E.G2Lines(eng, 2, eng.upload(u2 + s2))
    d_class, d_s1, d_skip, d_nu1 = eng.upload_u32([0] * n), eng.upload(s1), eng.upload(bytes(1)), eng.upload(eng.g1_neg([u1])[0])
    d_g1 = eng.upload(np.ascontiguousarray(np.concatenate([e2, e4], axis=1)).tobytes())
    d_g2 = eng.upload(np.ascontiguousarray(np.concatenate([e3, e5], axis=1)).tobytes())
    d_lead, d_out4, d_outj = eng.upload(np.ascontiguousarray(lead).tobytes()), eng.alloc(n * 384), eng.alloc(n * 384)
    # rhip_pairing_jobs: per item m pairs (e2, au2_k), (e4, u2) and (u1, e5) with the scalar -1, and the summed pair (sum au1_k, e3)
    one, minus_one = (1).to_bytes(32, "little"), (R - 1).to_bytes(32, "little")
    base = np.concatenate([np.repeat(e2, m, axis=0).reshape(n, m * 64), e4, np.broadcast_to(np.frombuffer(u1, dtype=np.uint8), (n, 64))], axis=1)
    qq = np.concatenate([np.broadcast_to(np.frombuffer(b"".join(r[2] for r in rows), dtype=np.uint8), (n, m * 128)),
                         np.broadcast_to(np.frombuffer(u2, dtype=np.uint8), (n, 128)), e5], axis=1)
    jobs = (eng.upload_u32([(m + 2) * i for i in range(n + 1)]), eng.upload(np.ascontiguousarray(base).tobytes()),
            eng.upload((one * m + minus_one * 2) * n), eng.upload(np.ascontiguousarray(qq).tobytes()))
    sums = (eng.upload_u32([m * i for i in range(n + 1)]), eng.upload(b"".join(r[1] for r in rows) * n), eng.upload(one * m * n),
            eng.upload(np.ascontiguousarray(e3).tobytes()))

    def stage_four():
        E.dnf_decrypt_one_uk_dev(eng, n, 1, d_class, d_s1, d_skip, d_nu1, lines, d_g1, d_g2, d_lead, d_out4)
        eng.download(d_out4, 4)

    def stage_jobs():
        eng._check(eng.lib.rhip_pairing_jobs(eng.ctx, E._sz(n), E._sz(m + 2), E._sz(n * (m + 2)), *(E._p(x) for x in jobs), E._sz(m), E._sz(n * m),
                                             *(E._p(x) for x in sums), E._p(d_lead), E._p(d_outj)))
        eng.download(d_outj, 4)
    stage_four()
    stage_jobs()
    assert eng.download(d_out4) == eng.download(d_outj)

    legs = [(name + "_encaps_packed", lambda: mod.encaps_packed(host, pk, pkas, [policy], item_pol)),
            (name + "_encrypt_packed_16B", lambda: mod.encrypt_packed(host, pk, pkas, [policy], item_pol, pt_blob, pt_off)),
            (name + "_decaps_packed", lambda: mod.decaps_packed(host, uk, ct, ct_off)),
            (name + "_decrypt_packed_16B", lambda: mod.decrypt_packed(host, uk, ct, ct_off)),
            ("stage_one_uk", stage_four), ("stage_pairing_jobs", stage_jobs)]
    times = {leg: [] for leg, _ in legs}
    for _ in range(args.rounds):
        for leg, fn in legs:
            t0 = time.perf_counter()
            fn()
            times[leg].append(time.perf_counter() - t0)
    line = {"config": "%s key encapsulation, %d items under one conjunction of %d attributes: encaps / decaps against encrypt / decrypt with 16-byte "
                      "plaintexts, and the decrypt stage alone (rhip_dnf_decrypt_batch_one_uk, 4 Miller loops per item, against rhip_pairing_jobs, "
                      "%d) on the same device-resident elements; items per second, legs alternating, %d rounds after one warm-up"
                      % (name.upper(), n, m, m + 3, args.rounds),
            "schemes": [name.upper()], "batch": n, "attrs": m, "rounds": args.rounds, "keys_equal": True, "stages_equal": True, "header_bytes": hdr_bytes,
            "record_bytes": int(ct_off[n])}
    for leg in times:
        line[leg + "_items_per_s"] = round(n / min(times[leg]), 1)
        line[leg + "_items_per_s_median"] = round(n / statistics.median(times[leg]), 1)
        line[leg + "_spread"] = round(max(times[leg]) / min(times[leg]) - 1, 4)
        line[leg + "_s"] = [round(t, 5) for t in times[leg]]
    for a, b in ((name + "_encaps_packed", name + "_encrypt_packed_16B"), (name + "_decaps_packed", name + "_decrypt_packed_16B"),
                 ("stage_one_uk", "stage_pairing_jobs")):
        line[a + "_over_" + b + "_best"] = round(min(times[b]) / min(times[a]), 4)
        line[a + "_over_" + b + "_median"] = round(statistics.median(times[b]) / statistics.median(times[a]), 4)
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")
    del k_full
    lines.destroy()
    eng.close()
    host.close()


for scheme in (("bdabe", "mke08") if args.scheme == "both" else (args.scheme,)):
    run(scheme)
