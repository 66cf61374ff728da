#!/usr/bin/env python3
"""Throughput of the bsw / lsw / aw11 batch entry points (BASELINE configs 3-5 at a reduced batch) through the host
layer, one GPU.  Not the judged metric (bench.py is config 2); prints one JSON line per config.
usage: python tools/bench_schemes.py [--batch 256]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rabe_amd import hostlib as hl  # noqa: E402
from rabe_amd.schemes import aw11, bdabe, bsw, ghw11, lsw, mke08  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--only", default="")
ap.add_argument("--key-items", type=int, default=65536, help="keys per call of the key-issuing legs (--only ghw11keys, --only dnfkeys)")
ap.add_argument("--rounds", type=int, default=2, help="timed repetitions per config: the first meets cold fixed-base tables of the key elements, later ones warm ones")
args = ap.parse_args()
B = args.batch
PT = b"dance like no one's watching, encrypt like everyone is!"
host = hl.Host(0)
if os.environ.get("RABE_FIXED_BASE_MIN"):
    host.set_fixed_base_min(int(os.environ["RABE_FIXED_BASE_MIN"]))


def leaf(a):
    return '{"name": "%s"}' % a


def nest(ns):
    if len(ns) == 1:
        return leaf(ns[0])
    h = len(ns) // 2
    return '{"name": "and", "children": [%s, %s]}' % (nest(ns[:h]), nest(ns[h:]))


def report(name, n_ops, secs, extra):
    print(json.dumps({"config": name, "batch": B, "ops_per_s": round(n_ops / secs, 1), "seconds": round(secs, 3), **extra}), flush=True)


if args.only in ("", "bsw"):
    attrs = ["b%d" % i for i in range(100)]
    flat = '{"name": "and", "children": [%s]}' % ", ".join(leaf(a) for a in attrs)
    pk, msk = bsw.setup(host)
    sk = bsw.keygen(host, pk, msk, attrs)
    bsw.decrypt_batch(host, [sk] * 2, bsw.encrypt_batch(host, pk, [flat] * 2, hl.JSON_POLICY, [PT] * 2))   # warm-up (tables)
    for rd in range(args.rounds):
        t0 = time.perf_counter()
        cts = bsw.encrypt_batch(host, pk, [flat] * B, hl.JSON_POLICY, [PT] * B)
        t1 = time.perf_counter()
        pts = bsw.decrypt_batch(host, [sk] * B, cts)
        t2 = time.perf_counter()
        assert pts == [PT] * B
        report("3: BSW CP-ABE, 100-leaf AND tree (201 pairings/item)", B, t2 - t0, {"round": rd, "encrypt_s": round(t1 - t0, 3), "decrypt_s": round(t2 - t1, 3)})

if args.only in ("", "lsw"):
    attrs = ["c%d" % i for i in range(200)]
    policy = '{"name": "and", "children": [%s]}' % ", ".join(leaf(a) for a in attrs)
    pk, msk = lsw.setup(host)
    ct = lsw.encrypt(host, pk, attrs, PT)
    lsw.decrypt_batch(host, lsw.keygen_batch(host, pk, msk, [policy] * 2, hl.JSON_POLICY), [ct] * 2)
    for rd in range(args.rounds):
        t0 = time.perf_counter()
        sks = lsw.keygen_batch(host, pk, msk, [policy] * B, hl.JSON_POLICY)
        t1 = time.perf_counter()
        pts = lsw.decrypt_batch(host, sks, [ct] * B)
        t2 = time.perf_counter()
        assert pts == [PT] * B
        report("4: LSW KP-ABE keygen+decrypt, 200 attributes (400 pairings/item)", B, t2 - t0, {"round": rd, "keygen_s": round(t1 - t0, 3), "decrypt_s": round(t2 - t1, 3)})

if args.only in ("", "aw11"):
    gk = aw11.setup(host)
    auth, names = [], []
    for a in range(10):
        n = ["AUTH%dX%d" % (a, k) for k in range(20)]
        names += n
        auth.append(aw11.authgen(host, gk, n))
    policy = nest(names)
    sk = aw11.keygen(host, gk, auth[0][1], "alice", names[:20])
    for a in range(1, 10):
        for n in names[20 * a:20 * a + 20]:
            aw11.add_to_attribute(host, gk, auth[a][1], n, sk)
    pks = [p for p, _ in auth]
    aw11.decrypt_batch(host, gk, [sk] * 2, aw11.encrypt_batch(host, gk, pks, [policy] * 2, hl.JSON_POLICY, [PT] * 2))
    for rd in range(args.rounds):
        t0 = time.perf_counter()
        cts = aw11.encrypt_batch(host, gk, pks, [policy] * B, hl.JSON_POLICY, [PT] * B)
        t1 = time.perf_counter()
        pts = aw11.decrypt_batch(host, gk, [sk] * B, cts)
        t2 = time.perf_counter()
        assert pts == [PT] * B
        report("5: AW11, 10 authorities x 20 attributes (400 pairings/item)", B, t2 - t0, {"round": rd, "encrypt_s": round(t1 - t0, 3), "decrypt_s": round(t2 - t1, 3)})
if args.only in ("", "ghw11"):
    import numpy as np

    def ghw11_records(pk, policy, n):
        """n ciphertexts of PT under `policy` from ONE packed encrypt (device-resident rows, records sealed on the device)"""
        return ghw11.encrypt_packed(host, pk, [policy], [0] * n, PT * n, np.arange(n + 1, dtype=np.uint64) * len(PT))

    attrs = ["g%d" % i for i in range(50)]
    policy = nest(attrs)
    pk, msk = ghw11.setup(host)
    tk, rk = ghw11.tkgen(host, ghw11.keygen(host, pk, msk, attrs))
    blob, off = ghw11_records(pk, policy, B)
    items = [hl.Obj.deserialize("ghw11_ct", bytes(blob[int(off[i]):int(off[i + 1])])) for i in range(B)]
    ghw11.transform_batch(host, items[:2], [tk] * 2)
    t0 = time.perf_counter()
    tcts = ghw11.transform_batch(host, items, [tk] * B)
    t1 = time.perf_counter()
    assert ghw11.decrypt_out(host, tcts[-1], rk, items[-1]) == PT
    report("8f-1: GHW11 transform (outsourced decryption), 50-attribute AND policy (52 pairings/item)", B, t1 - t0, {"transform_s": round(t1 - t0, 3)})
    # the whole service through the packed, device-resident entry points: encrypt_packed (one lane per ciphertext row), transform_packed
    # (prepared lines of the transform key, no G2 arithmetic), decrypt_out_packed (c * t^-z, KDF and AES-GCM open on the device); checked
    # and trusted decode; best of two after a warm-up call
    def best_of(fn, reps=2):
        fn()
        best = None
        for _ in range(reps):
            t0 = time.perf_counter()
            r = fn()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return best, r

    for n_attr, n_items in ((50, 16384), (100, 8192)):
        attrs = ["g%d" % i for i in range(n_attr)]
        policy = nest(attrs)
        tk, rk = ghw11.tkgen(host, ghw11.keygen(host, pk, msk, attrs))
        t_enc, (blob, off) = best_of(lambda: ghw11_records(pk, policy, n_items))
        t_tr = {}
        t_do = {}
        for trusted in (False, True):
            t_tr[trusted], (out, status) = best_of(lambda: ghw11.transform_packed(host, tk, blob, off, trusted=trusted))
            assert not status.any()
            t_do[trusted], (pt, po, st) = best_of(lambda: ghw11.decrypt_out_packed(host, rk, out, blob, off, trusted=trusted))
            assert not st.any() and pt.tobytes() == PT * n_items

        def chain():
            b, o = ghw11_records(pk, policy, n_items)
            tct, s1 = ghw11.transform_packed(host, tk, b, o)
            return ghw11.decrypt_out_packed(host, rk, tct, b, o), s1
        t_chain, ((pt, po, st), s1) = best_of(chain)
        assert not s1.any() and not st.any() and pt.tobytes() == PT * n_items
        assert ghw11.decrypt_out(host, hl.Obj.deserialize("ghw11_tct", out[n_items - 1].tobytes()), rk,
                                 hl.Obj.deserialize("ghw11_ct", bytes(blob[int(off[n_items - 1]):]))) == PT
        print(json.dumps({"config": "8f-1: GHW11 packed service, %d-attribute AND policy (encrypt: %d rows/item; transform: %d Miller loops/item, "
                                    "all on prepared lines; decrypt_out: one Gt power/item)" % (n_attr, n_attr, n_attr + 2), "batch": n_items,
                          "encrypts_per_s": round(n_items / t_enc, 1),
                          "transforms_per_s": round(n_items / t_tr[False], 1), "transforms_per_s_trusted": round(n_items / t_tr[True], 1),
                          "decrypt_outs_per_s": round(n_items / t_do[False], 1), "decrypt_outs_per_s_trusted": round(n_items / t_do[True], 1),
                          "chain_per_s": round(n_items / t_chain, 1), "seconds": round(t_tr[False], 4), "record_bytes": int(blob.size)}), flush=True)

if args.only in ("", "ghw11keys"):
    # GHW11 bulk key issuing: keygen_packed (fixed-base rows) and tkgen_packed (variable-base G2 rows, four-way split), and beside the
    # latter the A/B of its kernel against rhip_g2_mul (the binary chain) on the same elements and scalars -- device-level calls on one
    # Engine of this process, warm-up then best of three, timed around call + sync
    import ctypes
    import random
    import numpy as np
    from rabe_amd import Engine
    R_ORDER = 21888242871839275222246405745257275088548364400416034343698204186575808495617

    def best3(fn):
        fn()
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            r = fn()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return best, r

    pk, msk = ghw11.setup(host)
    eng = Engine(0)
    n_keys = args.key_items
    for n_attr in (50, 100):
        attrs = ["g%03d" % i for i in range(n_attr)]          # names of one length: the records' elements sit at a fixed stride
        t_kg, (sk_blob, sk_off) = best3(lambda: ghw11.keygen_packed(host, pk, msk, [attrs], [0] * n_keys))
        t_tk, t_tk_tr = [best3(lambda: ghw11.tkgen_packed(host, sk_blob, sk_off, trusted=tr)) for tr in (False, True)]
        tkb, to, rkz, st = t_tk[1]
        assert not st.any()
        # the first key through the object API's transform path: the records are usable
        tk0 = hl.Obj.deserialize("ghw11_tk", bytes(tkb[:int(to[1])]), host=host)
        ctb, cto = ghw11.encrypt_packed(host, pk, [nest(attrs)], [0], PT, [0, len(PT)])
        tct, s1 = ghw11.transform_packed(host, tk0, ctb, cto)
        pt, po, s2 = ghw11.decrypt_out_packed(host, hl.Obj.deserialize("ghw11_rk", rkz[0].tobytes()), tct, ctb, cto)
        assert not s1.any() and not s2.any() and pt.tobytes() == PT
        # kernel A/B on the elements of these keys: rows = every G2 element, item scalar = a random Fr (as z^-1 is)
        rows = 2 + n_attr
        rec = int(sk_off[1])
        view = np.ascontiguousarray(sk_blob).reshape(n_keys, rec)
        name = (rec - 260) // n_attr - 128
        cols = [np.arange(0, 256)] + [260 + y * (name + 128) + name + np.arange(128) for y in range(n_attr)]
        pts = np.ascontiguousarray(view[:, np.concatenate(cols)]).reshape(-1)
        n_rows = n_keys * rows
        ks = np.frombuffer(b"".join(random.randrange(1, R_ORDER).to_bytes(32, "little") for _ in range(n_keys)), dtype=np.uint8).reshape(n_keys, 32)
        d_p, d_k = eng.upload(pts.tobytes()), eng.upload(ks.tobytes())
        d_kk = eng.upload(np.repeat(ks, rows, axis=0).tobytes())
        d_off = eng.upload((np.arange(n_keys + 1, dtype=np.uint32) * rows).tobytes())
        d_a, d_b = eng.alloc(n_rows * 128), eng.alloc(n_rows * 128)

        def run_rows():
            eng._check(eng.lib.rhip_g2_mul_rows(eng.ctx, ctypes.c_size_t(n_rows), d_off.ptr, d_p.ptr, ctypes.c_size_t(n_keys), d_k.ptr, d_a.ptr))
            eng.sync()

        def run_binary():
            eng._check(eng.lib.rhip_g2_mul(eng.ctx, ctypes.c_size_t(n_rows), d_p.ptr, d_kk.ptr, d_b.ptr))
            eng.sync()
        t_rows, _ = best3(run_rows)
        t_bin, _ = best3(run_binary)
        assert eng.download(d_a) == eng.download(d_b)
        print(json.dumps({"config": "GHW11 key issuing, %d attributes: keygen_packed, tkgen_packed; k_g2_mul_rows against k_g2_mul on the same %d elements "
                                    "and scalars" % (n_attr, n_rows), "batch": n_keys, "keygen_keys_per_s": round(n_keys / t_kg, 1),
                          "tkgen_keys_per_s": round(n_keys / t_tk[0], 1), "tkgen_keys_per_s_trusted": round(n_keys / t_tk_tr[0], 1),
                          "g2_mul_rows_elements_per_s": round(n_rows / t_rows, 1), "g2_mul_elements_per_s": round(n_rows / t_bin, 1),
                          "g2_mul_rows_s": round(t_rows, 4), "g2_mul_s": round(t_bin, 4), "kernel_ratio": round(t_bin / t_rows, 3),
                          "seconds": round(t_tk[0], 4), "record_bytes": int(sk_blob.size)}), flush=True)
    eng.close()

if args.only in ("", "dnfkeys"):
    # BDABE / MKE08 bulk key issuing: keygen_packed (fixed-base rows) and request_*_sk_packed (variable-base G1 and G2 rows, 8 attributes per
    # user) at --key-items users, the object API on 256 users of the same inputs, and the A/B of k_g1_mul_rows against k_g1_mul on the same
    # elements and scalars -- one process, warm-up then best of three, timed around call (+ sync for the device-level calls)
    import ctypes
    import random
    import numpy as np
    from rabe_amd import Engine
    R_ORDER = 21888242871839275222246405745257275088548364400416034343698204186575808495617

    def best3(fn):
        fn()
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            r = fn()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return best, r

    eng = Engine(0)
    n_users, n_obj = args.key_items, 256
    attrs = ["aa1::b%d" % i for i in range(8)]
    names = ["user%05d" % (i % 100000) for i in range(n_users)]          # names of one length: the records sit at a fixed stride
    for scheme, mod in (("bdabe", bdabe), ("mke08", mke08)):
        pk, msk = mod.setup(host)
        if scheme == "bdabe":
            au = bdabe.authgen(host, pk, msk, "aa1")
            issuer, req_obj, req_packed = au, (lambda uk, a: bdabe.request_attribute_sk(host, uk, au, a)), bdabe.request_attribute_sk_packed
        else:
            au = mke08.authgen(host, "aa1")
            issuer, req_obj, req_packed = msk, (lambda uk, a: mke08.request_authority_sk(host, uk, a, au)), mke08.request_authority_sk_packed
        t_kg, (uk_blob, uk_off) = best3(lambda: mod.keygen_packed(host, pk, issuer, names))
        rec = int(uk_off[1])
        view = np.ascontiguousarray(uk_blob).reshape(n_users, rec)
        upk = np.ascontiguousarray(view[:, 192:rec - 4])
        upk_off = np.arange(n_users + 1, dtype=np.uint64) * (rec - 196)
        assert bytes(upk[0]) == mod.public_user_key_record(bytes(view[0]))
        t_rq, t_rq_tr = [best3(lambda: req_packed(host, au, [attrs], [0] * n_users, upk.reshape(-1), upk_off, trusted=tr)) for tr in (False, True)]
        ob, oo, st = t_rq[1]
        assert not st.any()
        # the object API on the first 256 users: one keygen call and eight request calls per user
        mod.keygen(host, pk, issuer, "warm")
        t0 = time.perf_counter()
        uks = [mod.keygen(host, pk, issuer, names[i]) for i in range(n_obj)]
        t_kg_obj = time.perf_counter() - t0
        uks = [hl.Obj.deserialize(scheme + "_uk", bytes(view[i]), host=host) for i in range(n_obj)]          # the packed call's users
        t0 = time.perf_counter()
        for uk in uks:
            for a in attrs:
                req_obj(uk, a)
        t_rq_obj = time.perf_counter() - t0
        for i in (0, n_obj - 1):
            assert uks[i].serialize() == bytes(view[i, :rec - 4]) + bytes(ob[int(oo[i]):int(oo[i + 1])])
        # kernel A/B on these users' u1: one scalar per attribute, its rows = every user
        n_rows = n_users * len(attrs)
        u1 = np.ascontiguousarray(upk[:, -192:-128])
        ks = np.frombuffer(b"".join(random.randrange(1, R_ORDER).to_bytes(32, "little") for _ in attrs), dtype=np.uint8).reshape(len(attrs), 32)
        d_p = eng.upload(np.tile(u1, (len(attrs), 1)).tobytes())
        d_k, d_kk = eng.upload(ks.tobytes()), eng.upload(np.repeat(ks, n_users, axis=0).tobytes())
        d_off = eng.upload((np.arange(len(attrs) + 1, dtype=np.uint32) * n_users).tobytes())
        d_a, d_b = eng.alloc(n_rows * 64), eng.alloc(n_rows * 64)

        def run_rows():
            eng._check(eng.lib.rhip_g1_mul_rows(eng.ctx, ctypes.c_size_t(n_rows), d_off.ptr, d_p.ptr, ctypes.c_size_t(len(attrs)), d_k.ptr, d_a.ptr))
            eng.sync()

        def run_glv():
            eng._check(eng.lib.rhip_g1_mul(eng.ctx, ctypes.c_size_t(n_rows), d_p.ptr, d_kk.ptr, d_b.ptr))
            eng.sync()
        t_rows, _ = best3(run_rows)
        t_glv, _ = best3(run_glv)
        assert eng.download(d_a) == eng.download(d_b)
        print(json.dumps({"config": "%s key issuing, %d attributes per user: keygen_packed, request_sk_packed; the object API on %d users; k_g1_mul_rows "
                                    "against k_g1_mul on the same %d elements and scalars" % (scheme.upper(), len(attrs), n_obj, n_rows), "batch": n_users,
                          "keygen_keys_per_s": round(n_users / t_kg, 1), "keygen_keys_per_s_object": round(n_obj / t_kg_obj, 1),
                          "request_sk_users_per_s": round(n_users / t_rq[0], 1), "request_sk_users_per_s_trusted": round(n_users / t_rq_tr[0], 1),
                          "request_sk_users_per_s_object": round(n_obj / t_rq_obj, 1),
                          "g1_mul_rows_elements_per_s": round(n_rows / t_rows, 1), "g1_mul_elements_per_s": round(n_rows / t_glv, 1),
                          "g1_mul_rows_s": round(t_rows, 4), "g1_mul_s": round(t_glv, 4), "kernel_ratio": round(t_glv / t_rows, 3),
                          "seconds": round(t_rq[0], 4), "record_bytes": int(uk_blob.size) + int(ob.size)}), flush=True)
    eng.close()

if args.only in ("", "dnf"):
    # 8f-4: the DNF schemes' decrypt (m + 3 pairings per item on one accumulator): a 3-conjunction policy, the key satisfies the last one
    pol_dnf = ('{"name": "or", "children": [{"name": "and", "children": [{"name": "%s::A"}, {"name": "%s::Z"}]}, '
               '{"name": "and", "children": [{"name": "%s::B"}, {"name": "%s::C"}, {"name": "%s::D"}]}]}')
    pk, msk = bdabe.setup(host)
    au = bdabe.authgen(host, pk, msk, "aa1")
    uk = bdabe.keygen(host, pk, au, "u1")
    names = ["aa1::" + x for x in "ABCDZ"]
    pkas = [bdabe.request_attribute_pk(host, pk, au, n) for n in names]
    for n in names[1:4]:
        bdabe.request_attribute_sk(host, uk, au, n)
    n_ct = min(B, 32)
    cts = [bdabe.encrypt(host, pk, pkas, pol_dnf % (("aa1",) * 5), hl.JSON_POLICY, PT) for _ in range(n_ct)]
    items = [cts[i % n_ct] for i in range(B)]
    bdabe.decrypt_batch(host, [uk] * 2, items[:2])
    t0 = time.perf_counter()
    pts = bdabe.decrypt_batch(host, [uk] * B, items)
    t1 = time.perf_counter()
    assert pts == [PT] * B
    report("8f-4: BDABE decrypt, 3-attribute conjunction (6 pairings/item)", B, t1 - t0, {"decrypt_s": round(t1 - t0, 3)})

    def packed_dnf(mod, key, records, label):
        import numpy as np
        for n_items in (B, 16 * B):
            recs = [records[i % len(records)] for i in range(n_items)]
            blob = np.frombuffer(b"".join(recs), dtype=np.uint8)
            off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)
            buf = np.zeros(blob.size, dtype=np.uint8)
            best = {}
            for tr in (False, True):
                for rep in range(3):
                    t0_ = time.perf_counter()
                    out, oo, st = mod.decrypt_packed(host, key, blob, off, out=buf, trusted=tr)
                    dt = time.perf_counter() - t0_
                    assert not st.any() and bytes(out[:len(PT)]) == PT
                    if rep:
                        best[tr] = min(best.get(tr, 9e9), dt)
            print(json.dumps({"config": label, "batch": n_items, "decrypts_per_s": round(n_items / best[False], 1),
                              "decrypts_per_s_trusted": round(n_items / best[True], 1), "seconds": round(best[False], 4)}), flush=True)
    packed_dnf(bdabe, uk, [c.serialize() for c in cts], "8f-4: BDABE decrypt, packed records (rabe_bdabe_decrypt_packed)")

    def encrypt_dnf(mod, pk, attr_pk, scheme, auth):
        """per-call encrypt (a few hundred calls) against the packed encrypt at 4096 and 65 536 items, policies of 1, 3 and 8 terms"""
        import numpy as np
        names8 = ["%s::T%d" % (auth, i) for i in range(8)]
        keys = [attr_pk(n) for n in names8]
        pol = {t: leaf(names8[0]) if t == 1 else '{"name": "or", "children": [%s]}' % ", ".join(leaf(x) for x in names8[:t]) for t in (1, 3, 8)}
        calls = 256
        mod.encrypt(host, pk, keys, pol[3], hl.JSON_POLICY, PT)
        t0_ = time.perf_counter()
        for _ in range(calls):
            mod.encrypt(host, pk, keys, pol[3], hl.JSON_POLICY, PT)
        dt = time.perf_counter() - t0_
        print(json.dumps({"config": "8f-4: %s encrypt, per call (rabe_%s_encrypt), 3 terms" % (scheme.upper(), scheme), "batch": calls,
                          "encrypts_per_s": round(calls / dt, 1), "seconds": round(dt, 4)}), flush=True)
        for terms in (1, 3, 8):
            for n_items in (4096, 65536):
                pt_off = np.arange(n_items + 1, dtype=np.uint64) * len(PT)
                t0_ = time.perf_counter()
                blob, off = mod.encrypt_packed(host, pk, keys, [pol[terms]], [0] * n_items, PT * n_items, pt_off)
                first = time.perf_counter() - t0_
                best = 9e9
                for _ in range(2):
                    t0_ = time.perf_counter()
                    blob, off = mod.encrypt_packed(host, pk, keys, [pol[terms]], [0] * n_items, PT * n_items, pt_off)
                    best = min(best, time.perf_counter() - t0_)
                last = hl.Obj.deserialize(scheme + "_ct", bytes(blob[int(off[n_items - 1]):]))
                assert len(hl.parse_obj(scheme + "_ct", last.serialize())["j" if scheme == "bdabe" else "e"]) == terms
                line = {"config": "8f-4: %s encrypt, packed (rabe_%s_encrypt_packed), %d terms" % (scheme.upper(), scheme, terms), "batch": n_items,
                        "encrypts_per_s": round(n_items / best, 1), "seconds": round(best, 4), "first_call_s": round(first, 4),
                        "record_bytes": int(blob.size)}
                if n_items == 4096:          # the first call of a policy also folds its terms and builds their tables
                    line["table_build_s_per_term"] = round((first - best) / terms, 4)
                print(json.dumps(line), flush=True)
    encrypt_dnf(bdabe, pk, lambda n: bdabe.request_attribute_pk(host, pk, au, n), "bdabe", "aa1")
    pk, msk = mke08.setup(host)
    uk = mke08.keygen(host, pk, msk, "user1")
    au = mke08.authgen(host, "auth1")
    names = ["auth1::" + x for x in "ABCDZ"]
    pkas = [mke08.request_authority_pk(host, pk, n, au) for n in names]
    for n in names[1:4]:
        mke08.request_authority_sk(host, uk, n, au)
    cts = [mke08.encrypt(host, pk, pkas, pol_dnf % (("auth1",) * 5), hl.JSON_POLICY, PT) for _ in range(n_ct)]
    items = [cts[i % n_ct] for i in range(B)]
    mke08.decrypt_batch(host, [uk] * 2, items[:2])
    t0 = time.perf_counter()
    pts = mke08.decrypt_batch(host, [uk] * B, items)
    t1 = time.perf_counter()
    assert pts == [PT] * B
    report("8f-4: MKE08 decrypt, 3-attribute conjunction (6 pairings/item)", B, t1 - t0, {"decrypt_s": round(t1 - t0, 3)})
    packed_dnf(mke08, uk, [c.serialize() for c in cts], "8f-4: MKE08 decrypt, packed records (rabe_mke08_decrypt_packed)")
    encrypt_dnf(mke08, pk, lambda n: mke08.request_authority_pk(host, pk, n, au), "mke08", "auth1")
host.close()
