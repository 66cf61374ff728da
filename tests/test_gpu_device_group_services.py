"""A device GROUP under the calls added for services that run at node scale (include/rabe_host.h, device-group paragraph): the GHW11 service
(keygen / provision / encrypt / transform / decrypt_out / the holder's decrypt), the AC17 KP pair, the KEM pairs of ac17 and bsw.  The group
lists device 0 two and three times, as tests/test_gpu_device_group.py does.  Per call: the group's bytes on a fixed tape are the plain
host's (itself pinned to the oracle elsewhere); an item that must fail -- placed in the SECOND block -- fails alone, with the plain host's
status, slot and error text; rabe_host_group_items shows that the call was cut ([3, 2], [2, 2, 1], [1, 1, 0]); a short buffer returns 1 with
the size to come back with and nothing drawn.  Shapes: AND / OR over three attributes, plaintexts of 1 .. 40 bytes, 5 items on 2 and 3
engines (uneven blocks), 2 items on 3 engines (fewer items than engines)."""
import ctypes

import numpy as np
import pytest

from rabe_amd import hostlib as hl

pytestmark = pytest.mark.gpu

CASES = [(2, 5, [3, 2]), (3, 5, [2, 2, 1]), (3, 2, [1, 1, 0])]          # engines, items, the cut
IDS = ["2x5", "3x5", "3x2"]
POLS = ['"A" and "B"', '"A" or "C"', '"C" and ("A" or "B")']             # a key over {A, B} satisfies the first two only
SETS = [["A", "B", "C"], ["A", "B"], ["C"]]
KP_POLICY = '("A" and "B") or "C"'
LENS = [1, 40, 7, 13, 22]


def shape(n):
    """item -> policy (the one a key over {A, B} does not satisfy at `fail`), plaintexts, the item of the second block that is made to fail"""
    fail = 3 if n == 5 else 1
    item_pol = [(2 if i == fail else i % 2) for i in range(n)]
    pts = [bytes((37 * i + j) % 251 for j in range(LENS[i])) for i in range(n)]
    return fail, item_pol, pts


def offsets(items):
    return np.concatenate([[0], np.cumsum([len(p) for p in items])]).astype(np.uint64)


def tape_of(seed, count):
    return [1000003 * (i + seed) + 7 * seed + 1 for i in range(count)]


def same(a, b):
    return len(a) == len(b) and all((x is None and y is None) or np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def last_error(h):
    return (h.lib.rabe_host_last_error(h.h) or b"").decode()


def on_tape(h, tape, fn):
    h.set_tape(tape)
    try:
        return fn(h)
    finally:
        h.clear_tape()


def both(hosts, g, cut, fn, tape=None, errors=False):
    """fn(host) on the plain host and on the group of g engines (each on `tape`, if given): the same outputs, the same error text, the group's
    item counts moved by `cut`.  Returns the outputs."""
    run = (lambda h: on_tape(h, tape, fn)) if tape is not None else fn
    ref = tuple(run(hosts[1]))
    ref_err = last_error(hosts[1])
    before = hosts[g].group_items()
    got = tuple(run(hosts[g]))
    delta = [b - a for a, b in zip(before, hosts[g].group_items())]
    assert same(ref, got), "group of %d engines differs from the single engine" % g
    if errors:
        assert ref_err and last_error(hosts[g]) == ref_err
    assert delta == cut, "the call was not cut as announced: %r" % (delta,)
    return ref


def spoil(blob, off, fail, how):
    """records with item `fail` made to fail: "tag" flips the record's last byte (the AES-GCM tag), "length" sets the sealed part's length
    field of a header to 1 (outside the record), "bounds" gives the item decreasing offsets -- every other item keeps well-formed bounds,
    which needs the records behind it moved to the front of the blob: offsets are shared boundaries."""
    blob, off = np.array(blob, dtype=np.uint8), np.array(off, dtype=np.uint64)
    n = len(off) - 1
    if how == "tag":
        blob[int(off[fail + 1]) - 1] ^= 1
        return blob, off
    if how == "length":
        blob[int(off[fail + 1]) - 4] = 1
        return blob, off
    recs = [blob[int(off[i]):int(off[i + 1])] for i in range(n)]
    tail, head = recs[fail + 1:], recs[:fail]
    new = np.concatenate(tail + head) if tail or head else np.zeros(0, np.uint8)
    o = np.zeros(n + 1, dtype=np.uint64)
    at = sum(len(r) for r in tail)
    for i in range(fail):
        o[i] = at
        at += len(recs[i])
    o[fail] = at                                   # = len(new): item `fail` runs from the end of the blob backwards
    at = 0
    for i in range(fail + 1, n):
        o[i] = at
        at += len(recs[i])
    o[n] = at
    assert o[fail] > o[fail + 1]
    return new, o


@pytest.fixture(scope="module")
def hosts():
    hs = {1: hl.Host(0), 2: hl.Host(devices=[0, 0]), 3: hl.Host(devices=[0, 0, 0])}
    assert [h.group_size() for h in hs.values()] == [1, 2, 3]
    assert hs[1].group_items() == [0]
    yield hs
    for h in hs.values():
        h.close()


@pytest.fixture(scope="module")
def ghw(hosts):
    """one GHW11 key pair for the whole module (its window tables are built once per engine), a full key and one over {A, B} with their proxies"""
    from rabe_amd.schemes import ghw11
    h = hosts[1]
    pk, msk = ghw11.setup(h)
    sk = ghw11.keygen(h, pk, msk, ["A", "B", "C"])
    sk_ab = ghw11.keygen(h, pk, msk, ["A", "B"])
    tk, rk = ghw11.tkgen(h, sk)
    tk_ab, rk_ab = ghw11.tkgen(h, sk_ab)
    return dict(pk=pk, msk=msk, sk=sk, sk_ab=sk_ab, tk=tk, rk=rk, tk_ab=tk_ab, rk_ab=rk_ab)


@pytest.fixture(scope="module")
def ghw_cts(hosts, ghw):
    """the ciphertext records of both shapes, made once on the plain host"""
    from rabe_amd.schemes import ghw11
    out = {}
    for n in (5, 2):
        _fail, item_pol, pts = shape(n)
        out[n] = on_tape(hosts[1], tape_of(11, 40 * n),
                         lambda h: ghw11.encrypt_packed(h, ghw["pk"], POLS, item_pol, b"".join(pts), offsets(pts), hl.HUMAN_POLICY))
    return out


def test_plain_host_counts_in_its_one_entry(hosts, ghw):
    from rabe_amd.schemes import ghw11
    h = hosts[1]
    before = h.group_items()
    ghw11.keygen_packed(h, ghw["pk"], ghw["msk"], SETS, [0, 1, 2, 0])
    assert [b - a for a, b in zip(before, h.group_items())] == [4]
    out = (ctypes.c_uint64 * 1)()
    assert h.lib.rabe_host_group_items(hosts[3].h, out, ctypes.c_size_t(1)) == -1          # cap below the group size
    assert h.lib.rabe_host_group_items(hosts[3].h, (ctypes.c_uint64 * 4)(), ctypes.c_size_t(4)) == 3


@pytest.mark.parametrize("g,n,cut", CASES, ids=IDS)
def test_ghw11_keygen_and_provision(hosts, ghw, g, n, cut):
    from rabe_amd.schemes import ghw11
    pk, msk = ghw["pk"], ghw["msk"]
    item_set = [i % 3 for i in range(n)]
    tape = tape_of(3, 2 * n)
    keys = both(hosts, g, cut, lambda h: ghw11.keygen_packed(h, pk, msk, SETS, item_set), tape)
    prov = both(hosts, g, cut, lambda h: ghw11.provision_packed(h, pk, msk, SETS, item_set), tape)
    tks = both(hosts, g, cut, lambda h: ghw11.provision_packed(h, pk, msk, SETS, item_set, want_sk=False), tape)
    assert same(prov[2:], tks[2:]), "sk_off = NULL: other transform / retrieve keys"
    assert same(keys, prov[:2])

    # BY DEFINITION keygen_packed, then tkgen_packed on its output, on one tape and one engine
    def two_calls(h):
        sk_blob, sk_off = ghw11.keygen_packed(h, pk, msk, SETS, item_set)
        tk_blob, tk_off, rk, status = ghw11.tkgen_packed(h, sk_blob, sk_off)
        assert not status.any()
        return sk_blob, sk_off, tk_blob, tk_off, rk
    assert same(on_tape(hosts[1], tape, two_calls), on_tape(hosts[g], tape, lambda h: ghw11.provision_packed(h, pk, msk, SETS, item_set)))


@pytest.mark.parametrize("g,n,cut", CASES, ids=IDS)
def test_ghw11_provision_z_zero_fails_the_call_and_writes_nothing(hosts, ghw, g, n, cut):
    """z of an item of the SECOND block is zero: the whole call fails as tkgen's inverse().unwrap() does, and no block has written a record"""
    fail, _pol, _pts = shape(n)
    item_set = [i % 3 for i in range(n)]
    tape = tape_of(5, 2 * n)
    tape[n + fail] = 0
    for h in (hosts[1], hosts[g]):
        rc, bufs = on_tape(h, tape, lambda hh: raw_provision(hh, ghw, item_set, short_tk=0, fill=0xEE))
        assert rc == -2 and "inverse of zero" in last_error(h)
        assert all((b == 0xEE).all() for b in bufs), "a record was written although z = 0 fails the call"


def raw_provision(h, ghw, item_set, short_tk=0, short_sk=0, fill=0):
    """rabe_ghw11_provision_packed with buffers `short_*` bytes below what the records need -> (rc, (sk_buf, tk_buf, rk_buf)) or (rc, offsets)"""
    n = len(item_set)
    need = [128 + 128 + 4 + sum(4 + len(a) + 128 for a in SETS[s]) for s in item_set]
    arr, _ = hl._strs([a for s_ in SETS for a in s_])
    counts = (ctypes.c_size_t * len(SETS))(*[len(s_) for s_ in SETS])
    it = np.ascontiguousarray(item_set, dtype=np.uint32)
    so, to = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64)
    sk_buf = np.full(sum(need) - short_sk, fill, dtype=np.uint8)
    tk_buf = np.full(sum(need) - short_tk, fill, dtype=np.uint8)
    rk = np.full((n, 32), fill, dtype=np.uint8)
    p = hl._np_ptr
    rc = h.lib.rabe_ghw11_provision_packed(h.h, ghw["pk"].ptr, ghw["msk"].ptr, arr, counts, ctypes.c_size_t(len(SETS)), ctypes.c_size_t(n), p(it), p(sk_buf),
                                           ctypes.c_size_t(sk_buf.size), p(so), p(tk_buf), ctypes.c_size_t(tk_buf.size), p(to), p(rk))
    if short_tk or short_sk:
        return rc, (so, to, sum(need))
    return rc, (sk_buf, tk_buf, rk)


@pytest.mark.parametrize("g,n,cut", CASES, ids=IDS)
def test_ghw11_encrypt_transform_decrypt_out(hosts, ghw, ghw_cts, g, n, cut):
    from rabe_amd.schemes import ghw11
    fail, item_pol, pts = shape(n)
    enc = both(hosts, g, cut, lambda h: ghw11.encrypt_packed(h, ghw["pk"], POLS, item_pol, b"".join(pts), offsets(pts), hl.HUMAN_POLICY), tape_of(11, 40 * n))
    assert same(enc, ghw_cts[n])
    blob, off = enc
    tct, status = both(hosts, g, cut, lambda h: ghw11.transform_packed(h, ghw["tk"], blob, off))
    assert not status.any() and tct.any(axis=1).all()
    pt, pt_off, status = both(hosts, g, cut, lambda h: ghw11.decrypt_out_packed(h, ghw["rk"], tct, blob, off))
    assert not status.any() and pt.tobytes() == b"".join(pts) and np.array_equal(pt_off, offsets(pts))
    # a key that does not satisfy ONE item's policy: a zeroed slot in the second block, its neighbours untouched
    tct_ab, status = both(hosts, g, cut, lambda h: ghw11.transform_packed(h, ghw["tk_ab"], blob, off), errors=True)
    assert [int(s) for s in status] == [-1 if i == fail else 0 for i in range(n)]
    assert not tct_ab[fail].any() and all(tct_ab[i].any() for i in range(n) if i != fail)
    # ... which decrypt_out then refuses alone, the items behind it at the right offsets
    survivors = [p for i, p in enumerate(pts) if i != fail]
    pt, pt_off, status = both(hosts, g, cut, lambda h: ghw11.decrypt_out_packed(h, ghw["rk_ab"], tct_ab, blob, off), errors=True)
    assert [int(s) for s in status] == [-1 if i == fail else 0 for i in range(n)] and pt.tobytes() == b"".join(survivors)
    assert pt_off[fail] == pt_off[fail + 1] and int(pt_off[n]) == sum(len(p) for p in survivors)
    # bad bounds of one item: transform zeroes its slot, decrypt_out leaves its plaintext slot empty
    bblob, boff = spoil(blob, off, fail, "bounds")
    tct_b, status = both(hosts, g, cut, lambda h: ghw11.transform_packed(h, ghw["tk"], bblob, boff), errors=True)
    assert [int(s) for s in status] == [-1 if i == fail else 0 for i in range(n)] and not tct_b[fail].any()
    assert np.array_equal(np.delete(tct_b, fail, axis=0), np.delete(tct, fail, axis=0))
    for how, b, o in (("bounds", bblob, boff),) + ((("tag",) + spoil(blob, off, fail, "tag")),):
        pt, pt_off, status = both(hosts, g, cut, lambda h: ghw11.decrypt_out_packed(h, ghw["rk"], tct, b, o), errors=True)
        assert [int(s) for s in status] == [-1 if i == fail else 0 for i in range(n)], how
        good = np.concatenate([pt[int(pt_off[i]):int(pt_off[i + 1])] for i in range(n) if i != fail]).tobytes()
        assert good == b"".join(survivors), how


@pytest.mark.parametrize("g,n,cut", CASES, ids=IDS)
def test_ghw11_holder_decrypt(hosts, ghw, ghw_cts, g, n, cut):
    from rabe_amd.schemes import ghw11
    fail, _item_pol, pts = shape(n)
    blob, off = ghw_cts[n]
    survivors = [p for i, p in enumerate(pts) if i != fail]
    pt, pt_off, status = both(hosts, g, cut, lambda h: ghw11.decrypt_packed(h, ghw["sk"], blob, off))
    assert not status.any() and pt.tobytes() == b"".join(pts) and np.array_equal(pt_off, offsets(pts))
    cases = [("policy", ghw["sk_ab"], blob, off)] + [(how, ghw["sk"]) + spoil(blob, off, fail, how) for how in ("tag", "bounds")]
    for how, key, b, o in cases:
        pt, pt_off, status = both(hosts, g, cut, lambda h: ghw11.decrypt_packed(h, key, b, o), errors=True)
        assert [int(s) for s in status] == [-1 if i == fail else 0 for i in range(n)], how
        assert pt.tobytes() == b"".join(survivors) and pt_off[fail] == pt_off[fail + 1], how          # an EMPTY slot, the rest closed up


@pytest.mark.parametrize("g,n,cut", CASES, ids=IDS)
def test_ac17_kp_pair(hosts, g, n, cut):
    from rabe_amd.schemes import ac17
    h1 = hosts[1]
    fail, _item_pol, pts = shape(n)
    pk, msk = ac17.setup(h1)
    sk = ac17.kp_keygen(h1, msk, KP_POLICY, hl.HUMAN_POLICY)
    item_set = [(1 if i == fail else 2 * (i % 2)) for i in range(n)]          # {A, B, C} / {C}; {A, B} at `fail`: every list satisfies the key
    blob, off = both(hosts, g, cut, lambda h: ac17.kp_encrypt_packed(h, pk, SETS, item_set, b"".join(pts), offsets(pts)), tape_of(13, 4 * n))
    pt, pt_off, status = both(hosts, g, cut, lambda h: ac17.kp_decrypt_packed(h, sk, blob, off))
    assert not status.any() and pt.tobytes() == b"".join(pts) and np.array_equal(pt_off, offsets(pts))
    sk_c = ac17.kp_keygen(h1, msk, '"C" and ("A" or "B")', hl.HUMAN_POLICY)     # {A, B} does not satisfy it: item `fail` alone... and {C}
    unsat = [i for i in range(n) if item_set[i] != 0]
    _pt, _po, status = both(hosts, g, cut, lambda h: ac17.kp_decrypt_packed(h, sk_c, blob, off, trusted=True), errors=True)
    assert [int(s) for s in status] == [-1 if i in unsat else 0 for i in range(n)]
    survivors = [p for i, p in enumerate(pts) if i != fail]
    for how in ("tag", "bounds"):
        b, o = spoil(blob, off, fail, how)
        pt, pt_off, status = both(hosts, g, cut, lambda h: ac17.kp_decrypt_packed(h, sk, b, o), errors=True)
        assert [int(s) for s in status] == [-1 if i == fail else 0 for i in range(n)], how
        good = np.concatenate([pt[int(pt_off[i]):int(pt_off[i + 1])] for i in range(n) if i != fail]).tobytes()
        assert good == b"".join(survivors), how


@pytest.mark.parametrize("scheme", ["ac17", "bsw"])
@pytest.mark.parametrize("g,n,cut", CASES, ids=IDS)
def test_kem_pair(hosts, scheme, g, n, cut):
    h1 = hosts[1]
    fail, item_pol, _pts = shape(n)
    if scheme == "ac17":
        from rabe_amd.schemes import ac17
        pk, msk = ac17.setup(h1)
        sk, sk_ab = ac17.cp_keygen(h1, msk, ["A", "B", "C"]), ac17.cp_keygen(h1, msk, ["A", "B"])
        encaps, decaps = ac17.cp_encaps_packed, ac17.cp_decaps_packed
    else:
        from rabe_amd.schemes import bsw
        pk, msk = bsw.setup(h1)
        sk, sk_ab = bsw.keygen(h1, pk, msk, ["A", "B", "C"]), bsw.keygen(h1, pk, msk, ["A", "B"])
        encaps, decaps = bsw.encaps_packed, bsw.decaps_packed
    hdr, hdr_off, keys = both(hosts, g, cut, lambda h: encaps(h, pk, POLS, item_pol, hl.HUMAN_POLICY), tape_of(17, 40 * n))
    assert keys.any(axis=1).all()
    # the keys a group decapsulates are the keys the plain host encapsulated for the same headers
    got, status = both(hosts, g, cut, lambda h: decaps(h, sk, hdr, hdr_off))
    assert not status.any() and np.array_equal(got, keys)
    cases = [("policy", sk_ab, hdr, hdr_off)] + [(how, sk) + spoil(hdr, hdr_off, fail, how) for how in ("length", "bounds")]
    for how, key, b, o in cases:
        got, status = both(hosts, g, cut, lambda h: decaps(h, key, b, o), errors=True)
        assert [int(s) for s in status] == [-1 if i == fail else 0 for i in range(n)], how
        assert not got[fail].any() and np.array_equal(np.delete(got, fail, axis=0), np.delete(keys, fail, axis=0)), how


def spy(monkeypatch, lib, name):
    """the return codes of every call of lib.<name> from here on"""
    rcs, real = [], getattr(lib, name)

    def call(*args):
        rcs.append(real(*args))
        return rcs[-1]
    monkeypatch.setattr(lib, name, call, raising=False)
    return rcs


def test_a_short_record_buffer_returns_1_and_draws_nothing(hosts, ghw, monkeypatch):
    """records out: a buffer one byte short -> 1, the size in the last offset entry, no draw: the wrapper's second call, on the SAME tape, gives
    the bytes of a fresh one"""
    from rabe_amd.schemes import ac17, bsw, ghw11
    h1, h = hosts[1], hosts[3]
    n = 5
    _fail, item_pol, pts = shape(n)
    item_set = [i % 3 for i in range(n)]
    apk, _amsk = ac17.setup(h1)
    bpk, _bmsk = bsw.setup(h1)
    calls = [("rabe_ghw11_keygen_packed", lambda hh, out: ghw11.keygen_packed(hh, ghw["pk"], ghw["msk"], SETS, item_set, out)),
             ("rabe_ghw11_encrypt_packed", lambda hh, out: ghw11.encrypt_packed(hh, ghw["pk"], POLS, item_pol, b"".join(pts), offsets(pts), hl.HUMAN_POLICY, out)),
             ("rabe_ac17_kp_encrypt_packed", lambda hh, out: ac17.kp_encrypt_packed(hh, apk, SETS, item_set, b"".join(pts), offsets(pts), out)),
             ("rabe_ac17_cp_encaps_packed", lambda hh, out: ac17.cp_encaps_packed(hh, apk, POLS, item_pol, hl.HUMAN_POLICY, out)),
             ("rabe_bsw_encaps_packed", lambda hh, out: bsw.encaps_packed(hh, bpk, POLS, item_pol, hl.HUMAN_POLICY, out))]
    tape = tape_of(19, 40 * n)
    for name, fn in calls:
        ref = on_tape(h1, tape, lambda hh: fn(hh, None))
        rcs = spy(monkeypatch, h.lib, name)
        before = h.group_items()
        got = on_tape(h, tape, lambda hh: fn(hh, np.empty(ref[0].size - 1, dtype=np.uint8)))
        assert rcs == [1, 0], (name, rcs)
        assert same(ref, got), name
        assert [b - a for a, b in zip(before, h.group_items())] == [2, 2, 1], name          # the refused call counts nothing
        monkeypatch.undo()
    # provision: either buffer short; then, the tape untouched, the real call
    ref = on_tape(h1, tape, lambda hh: ghw11.provision_packed(hh, ghw["pk"], ghw["msk"], SETS, item_set))

    def short_then_real(hh):
        for short in (dict(short_tk=1), dict(short_sk=1)):
            rc, (so, to, need) = raw_provision(hh, ghw, item_set, **short)
            assert rc == 1 and int(so[n]) == need and int(to[n]) == need
        return ghw11.provision_packed(hh, ghw["pk"], ghw["msk"], SETS, item_set)
    assert same(ref, on_tape(h, tape, short_then_real))


def test_a_short_plaintext_buffer_returns_1_with_the_size_of_the_records(hosts, ghw, ghw_cts):
    """records in: a group that cuts the batch needs the total size of the well-formed records; one byte less -> 1, pt_off[n] = that size"""
    from rabe_amd.schemes import ac17, ghw11
    h1, h = hosts[1], hosts[3]
    n = 5
    _fail, _item_pol, pts = shape(n)
    blob, off = ghw_cts[n]
    tct, _status = ghw11.transform_packed(h1, ghw["tk"], blob, off)
    apk, amsk = ac17.setup(h1)
    ksk = ac17.kp_keygen(h1, amsk, KP_POLICY, hl.HUMAN_POLICY)
    kblob, koff = ac17.kp_encrypt_packed(h1, apk, SETS, [0] * n, b"".join(pts), offsets(pts))
    p, size = hl._np_ptr, ctypes.c_size_t

    def decrypt_shaped(name, head, b, o):
        b, o = hl._as_u8(b), np.ascontiguousarray(o, dtype=np.uint64)
        span = int(o[n] - o[0])
        status, po, buf = np.zeros(n, dtype=np.int32), np.zeros(n + 1, dtype=np.uint64), np.full(span - 1, 0xEE, dtype=np.uint8)
        before = h.group_items()
        rc = getattr(h.lib, name)(h.h, *head, size(n), p(b), size(b.size), p(o), ctypes.c_uint32(0), p(status), p(buf), size(buf.size), p(po))
        assert rc == 1 and int(po[n]) == span, (name, rc, int(po[n]), span)
        assert (buf == 0xEE).all() and h.group_items() == before, name
    decrypt_shaped("rabe_ghw11_decrypt_packed", (ghw["sk"].ptr,), blob, off)
    decrypt_shaped("rabe_ac17_kp_decrypt_packed", (ksk.ptr,), kblob, koff)
    # decrypt_out: the tct slots in front of the blob
    b, o = hl._as_u8(blob), np.ascontiguousarray(off, dtype=np.uint64)
    span = int(o[n])
    status, po, buf = np.zeros(n, dtype=np.int32), np.zeros(n + 1, dtype=np.uint64), np.empty(span - 1, dtype=np.uint8)
    t = np.ascontiguousarray(tct).reshape(-1)
    rc = h.lib.rabe_ghw11_decrypt_out_packed(h.h, ghw["rk"].ptr, size(n), p(t), p(b), size(b.size), p(o), ctypes.c_uint32(0), p(status), p(buf), size(buf.size), p(po))
    assert rc == 1 and int(po[n]) == span
    # transform: 768 n - 1 bytes of slots
    out = np.full(768 * n - 1, 0xEE, dtype=np.uint8)
    rc = h.lib.rabe_ghw11_transform_packed(h.h, ghw["tk"].ptr, size(n), p(b), size(b.size), p(o), ctypes.c_uint32(0), p(status), p(out), size(out.size))
    assert rc == 1 and (out == 0xEE).all()


def test_round_trip_across_engine_counts(hosts, ghw):
    """provision under 3 engines, encrypt under 2, transform under 3, decrypt_out on the plain host: the plaintexts -- no replica cache is
    keyed on anything engine-local"""
    from rabe_amd.schemes import ghw11
    n = 5
    _fail, _item_pol, pts = shape(n)
    _sk, _so, tk_blob, tk_off, rk = ghw11.provision_packed(hosts[3], ghw["pk"], ghw["msk"], SETS, [0] * n)
    item_pol = [i % 3 for i in range(n)]
    blob, off = ghw11.encrypt_packed(hosts[2], ghw["pk"], POLS, item_pol, b"".join(pts), offsets(pts), hl.HUMAN_POLICY)
    for user in (0, n - 1):          # a user of the first block and one of the last
        tk = hl.Obj.deserialize("ghw11_tk", tk_blob[int(tk_off[user]):int(tk_off[user + 1])].tobytes())
        rko = hl.Obj.deserialize("ghw11_rk", rk[user].tobytes())
        tct, status = ghw11.transform_packed(hosts[3], tk, blob, off)
        assert not status.any()
        pt, pt_off, status = ghw11.decrypt_out_packed(hosts[1], rko, tct, blob, off)
        assert not status.any() and pt.tobytes() == b"".join(pts) and np.array_equal(pt_off, offsets(pts))
