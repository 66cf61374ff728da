"""GPU checks of the proxy's call for a mixed queue (include/rabe_host.h: rabe_ghw11_tk_store_create, rabe_ghw11_transform_keyed): item i is
transformed under key item_key[i] of a device-resident store.  The definition is rabe_ghw11_transform_packed for that record under that key,
byte for byte, so every expectation here is that call's output: per item and alone for the small queue, per key over the key's own records
for the 132-item one (that transform_packed gives an item the same bytes alone and in a batch is tests/test_gpu_ghw11.py's ground).  Keys come
from provision_packed on a tape; three users with 1, 3 and 2 attributes, so their lines start at blocks 0, 3 and 8 of the store's handle."""
import ctypes

import numpy as np
import pytest

from rabe_amd import hostlib as hl
from rabe_amd.schemes import ghw11

pytestmark = pytest.mark.gpu

SETS = [["A"], ["A", "B", "C"], ["B", "C"]]
LEAF = '{"name": "%s"}'
POLS = [LEAF % "A",
        '{"name": "and", "children": [%s, %s]}' % (LEAF % "A", LEAF % "B"),
        '{"name": "or", "children": [%s, %s]}' % (LEAF % "B", LEAF % "C"),
        '{"name": "and", "children": [%s, %s, %s]}' % (LEAF % "A", LEAF % "B", LEAF % "C"),
        '{"name": "and", "children": [%s, %s]}' % (LEAF % "B", LEAF % "C")]
# which key satisfies which policy: key 0 = {A}: 0; key 1 = {A, B, C}: all; key 2 = {B, C}: 2 and 4
SATISFIES = {(0, 0), (1, 0), (1, 1), (1, 2), (1, 3), (1, 4), (2, 2), (2, 4)}
# the small queue: keys interleaved 2,0,1,1,2,0,...; items 6, 7 and 10 name a key that does not satisfy their policy
Q_KEY = [2, 0, 1, 1, 2, 0, 2, 0, 1, 1, 2, 0]
Q_POL = [2, 0, 0, 1, 2, 0, 0, 1, 2, 2, 1, 0]
TWIN = (0, 9)          # ONE record (policy 2) queued twice: under key 2 and under key 1
# the ragged queue: selections of 3, 1, 2, 1, 2, 1 entries side by side in every 64-item tile, three tiles, the last one not full
R_COMBO = [(1, 3), (0, 0), (1, 1), (2, 2), (2, 4), (1, 0)]
R_N = 132


def offsets(items):
    return np.concatenate([[0], np.cumsum([len(p) for p in items])]).astype(np.uint64)


def records(blob, off):
    return [bytes(blob[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


class World:
    pass


@pytest.fixture(scope="module")
def world():
    w = World()
    w.host = host = hl.Host(0)
    w.pk, w.msk = ghw11.setup(host)
    host.set_tape([11, 12, 13, 101, 102, 103])          # r_0 .. r_2, then z_0 .. z_2
    _sk, _so, tk_blob, tk_off, rk = ghw11.provision_packed(host, w.pk, w.msk, SETS, [0, 1, 2], want_sk=False)
    host.clear_tape()
    w.tk_recs = records(tk_blob, tk_off)
    w.tk = [hl.Obj.deserialize("ghw11_tk", r) for r in w.tk_recs]
    w.rk = [hl.Obj.deserialize("ghw11_rk", rk[u].tobytes()) for u in range(3)]
    w.store = ghw11.tk_store_create(host, b"".join(w.tk_recs), offsets(w.tk_recs))
    assert w.store.key_status.tolist() == [0, 0, 0]
    # the small queue: full records, item i's plaintext names it
    w.q_pts = [b"queue item %d" % i for i in range(len(Q_KEY))]
    blob, off = ghw11.encrypt_packed(host, w.pk, POLS, Q_POL, b"".join(w.q_pts), offsets(w.q_pts))
    recs = records(blob, off)
    recs[TWIN[1]] = recs[TWIN[0]]
    w.q_pts[TWIN[1]] = w.q_pts[TWIN[0]]
    w.q_recs = recs
    w.q_ref = []
    for i, rec in enumerate(recs):          # the definition: the record alone under its key
        out, st = ghw11.transform_packed(host, w.tk[Q_KEY[i]], rec, [0, len(rec)])
        w.q_ref.append((out[0].tobytes(), int(st[0])))
    # the ragged queue: headers (encaps), references per key over the key's own records
    w.r_key = [R_COMBO[i % len(R_COMBO)][0] for i in range(R_N)]
    r_pol = [R_COMBO[i % len(R_COMBO)][1] for i in range(R_N)]
    hdr, hoff, w.r_keys = ghw11.encaps_packed(host, w.pk, POLS, r_pol)
    w.r_recs = records(hdr, hoff)
    w.r_keys = w.r_keys.copy()
    w.r_ref = [None] * R_N
    for u in range(3):
        mine = [i for i in range(R_N) if w.r_key[i] == u]
        out, st = ghw11.transform_packed(host, w.tk[u], b"".join(w.r_recs[i] for i in mine), offsets([w.r_recs[i] for i in mine]))
        for j, i in enumerate(mine):
            w.r_ref[i] = (out[j].tobytes(), int(st[j]))
    yield w
    host.close()


def keyed(host, store, item_key, recs, trusted=False):
    out, st = ghw11.transform_keyed(host, store, item_key, b"".join(recs), offsets(recs), trusted=trusted)
    return [(out[i].tobytes(), int(st[i])) for i in range(len(recs))]


def test_mixed_keys_equal_the_definition(world):
    """every record and verdict of the 12-item queue is transform_packed's for that record alone under the item's key, in checked and in
    trusted mode; the items whose key does not satisfy their policy have status -1 and 768 zero bytes"""
    for trusted in (False, True):
        got = keyed(world.host, world.store, Q_KEY, world.q_recs, trusted)
        for i, (g, want) in enumerate(zip(got, world.q_ref)):
            assert g == want, i
    for i in range(len(Q_KEY)):
        ok = (Q_KEY[i], Q_POL[i]) in SATISFIES
        assert world.q_ref[i][1] == (0 if ok else -1), i
        assert any(world.q_ref[i][0]) == ok, i
    assert sum(st for _b, st in world.q_ref) == -3


def test_one_record_under_two_keys(world):
    """a wrong line base cannot hide: the same (policy, record) under key 2 (lines from block 8) and under key 1 (from block 3) gives two
    different records, each its own key's"""
    a, b = TWIN
    assert world.q_recs[a] == world.q_recs[b] and Q_KEY[a] != Q_KEY[b]
    got = keyed(world.host, world.store, Q_KEY, world.q_recs)
    assert got[a][1] == got[b][1] == 0
    assert got[a][0] != got[b][0]
    assert got[a][0][:384] == got[b][0][:384]          # c is the record's; t is the key's
    assert got[a] == world.q_ref[a] and got[b] == world.q_ref[b]


def test_ragged_queue_over_three_tiles(world):
    """132 items whose selections have 3, 1, 2, 1, 2, 1 entries side by side: the tiled gather map, every key's base in every tile"""
    world.host.kernel_timing(True)
    world.host.kernel_launches()
    got = keyed(world.host, world.store, world.r_key, world.r_recs)
    launches = world.host.kernel_launches()
    world.host.kernel_timing(False)
    assert launches.get("k_ghw11_pairs_keyed") == 1 and launches.get("k_tile_offsets") == 1 and "k_ghw11_pairs" not in launches, launches
    assert all(st == 0 for _b, st in world.r_ref)
    for i in range(R_N):
        assert got[i] == world.r_ref[i], i


def test_failures_stay_with_their_item(world):
    host, recs, ref = world.host, world.q_recs, world.q_ref
    zero = (bytes(768), -1)
    # an item_key out of range
    ik = list(Q_KEY)
    ik[2] = 3
    ik[8] = 0xFFFFFFFF
    got = keyed(host, world.store, ik, recs)
    assert got == [zero if i in (2, 8) else ref[i] for i in range(len(recs))]
    assert b"item_key" in host.lib.rabe_host_last_error(host.h)
    # a store with a truncated key record (key 0 loses its last 5 bytes by its offsets): that key fails alone, and its items with it
    cut = [world.tk_recs[0][:-5]] + world.tk_recs[1:]
    store = ghw11.tk_store_create(host, b"".join(cut), offsets(cut))
    assert store.key_status.tolist() == [-1, 0, 0]
    got = keyed(host, store, Q_KEY, recs)
    assert got == [zero if Q_KEY[i] == 0 else ref[i] for i in range(len(recs))]
    store.free()
    # a key with a G2 element off its curve (the last k_x of key 2): refused in checked mode only
    bad = bytearray(world.tk_recs[2])
    bad[-128] ^= 1
    dented = [world.tk_recs[0], world.tk_recs[1], bytes(bad)]
    store = ghw11.tk_store_create(host, b"".join(dented), offsets(dented))
    assert store.key_status.tolist() == [0, 0, -1]
    assert b"not a member of G2" in host.lib.rabe_host_last_error(host.h)
    got = keyed(host, store, Q_KEY, recs)
    assert got == [zero if Q_KEY[i] == 2 else ref[i] for i in range(len(recs))]
    store.free()
    store = ghw11.tk_store_create(host, b"".join(dented), offsets(dented), trusted=True)
    assert store.key_status.tolist() == [0, 0, 0]
    store.free()
    # a malformed ciphertext record (item 3 loses 30 bytes by its offsets) and offsets that run backwards (item 5)
    blob, off = b"".join(recs), offsets(recs)
    short = blob[:int(off[4]) - 30] + blob[int(off[4]):]
    o = off.copy()
    o[4:] -= 30
    o[6] = np.uint64(int(o[5]) - 4)
    out, st = ghw11.transform_keyed(host, world.store, Q_KEY, short, o)
    got = [(out[i].tobytes(), int(st[i])) for i in range(len(recs))]
    assert got == [zero if i in (3, 5, 6) else ref[i] for i in range(len(recs))]          # item 6's slice starts before item 5's end


def test_edges(world):
    host, recs, ref = world.host, world.q_recs, world.q_ref
    lib = host.lib
    blob, off = np.frombuffer(b"".join(recs), dtype=np.uint8), offsets(recs)
    ik = np.array(Q_KEY, dtype=np.uint32)
    n = len(recs)
    # no items: nothing is touched
    assert lib.rabe_ghw11_transform_keyed(host.h, world.store.ptr, ctypes.c_size_t(0), None, None, ctypes.c_size_t(0), hl._np_ptr(off[:1].copy()),
                                          ctypes.c_uint32(0), hl._np_ptr(np.zeros(1, dtype=np.int32)), hl._np_ptr(np.zeros(1, dtype=np.uint8)), ctypes.c_size_t(0)) == 0
    # a buffer one byte short: 1, nothing written
    out = np.full(768 * n - 1, 0xEE, dtype=np.uint8)
    status = np.full(n, 7, dtype=np.int32)
    assert lib.rabe_ghw11_transform_keyed(host.h, world.store.ptr, ctypes.c_size_t(n), hl._np_ptr(ik), hl._np_ptr(blob), ctypes.c_size_t(blob.size), hl._np_ptr(off),
                                          ctypes.c_uint32(0), hl._np_ptr(status), hl._np_ptr(out), ctypes.c_size_t(out.size)) == 1
    assert (out == 0xEE).all() and (status == 7).all()
    # a key no item uses (key 1 stays idle)
    idle = [i for i in range(n) if Q_KEY[i] != 1]
    assert keyed(host, world.store, [Q_KEY[i] for i in idle], [recs[i] for i in idle]) == [ref[i] for i in idle]
    # one key registered twice: the same bytes under either index
    four = world.tk_recs + [world.tk_recs[1]]
    store = ghw11.tk_store_create(host, b"".join(four), offsets(four))
    assert store.key_status.tolist() == [0, 0, 0, 0]
    assert keyed(host, store, [3 if u == 1 else u for u in Q_KEY], recs) == keyed(host, store, Q_KEY, recs) == ref
    # what a store holds, to the byte: per element the 88 line triples of 192 bytes and one flag, and -- where the reduced-radix kernels are
    # in use -- their copy of the triples, 88 records of nine 16-byte words
    elements = sum(2 + len(s) for s in SETS) + 2 + len(SETS[1])
    assert store.nbytes() in (elements * (88 * 192 + 1), elements * (88 * 192 + 1 + 88 * 144)), store.nbytes()
    store.free()
    # a one-key store is transform_packed on the whole blob
    mine = [recs[i] for i in range(n) if Q_KEY[i] == 1] + [recs[6]]
    store = ghw11.tk_store_create(host, world.tk_recs[1], [0, len(world.tk_recs[1])])
    out, st = ghw11.transform_packed(host, world.tk[1], b"".join(mine), offsets(mine))
    assert keyed(host, store, [0] * len(mine), mine) == [(out[i].tobytes(), int(st[i])) for i in range(len(mine))]
    store.free()


def test_the_chain_gives_every_user_their_keys(world):
    """encaps_packed -> transform_keyed -> decaps_out_packed per user with that user's rk: the encapsulated keys; and a full record through
    decrypt_out_packed: its plaintext"""
    host = world.host
    out, st = ghw11.transform_keyed(host, world.store, world.r_key, b"".join(world.r_recs), offsets(world.r_recs))
    assert not st.any()
    for u in range(3):
        mine = [i for i in range(R_N) if world.r_key[i] == u]
        keys, ds = ghw11.decaps_out_packed(host, world.rk[u], out[mine])
        assert not ds.any() and (keys == world.r_keys[mine]).all(), u
    keys, _ds = ghw11.decaps_out_packed(host, world.rk[0], out[[i for i in range(R_N) if world.r_key[i] == 1][:4]])
    assert not (keys == world.r_keys[[i for i in range(R_N) if world.r_key[i] == 1][:4]]).all(axis=1).any()          # another user's z opens nothing
    out, st = ghw11.transform_keyed(host, world.store, Q_KEY, b"".join(world.q_recs), offsets(world.q_recs))
    i = 3                                                                   # key 1, "A and B"
    pt, po, ps = ghw11.decrypt_out_packed(host, world.rk[Q_KEY[i]], out[i:i + 1], world.q_recs[i], [0, len(world.q_recs[i])])
    assert ps.tolist() == [0] and bytes(pt[:int(po[1])]) == world.q_pts[i]


def test_device_group_gives_the_same_bytes(world):
    """two engines on GPU 0: the queue is cut in two, each engine prepares its replica of the store's lines on first use"""
    group = hl.Host(devices=[0, 0])
    try:
        store = ghw11.tk_store_create(group, b"".join(world.tk_recs), offsets(world.tk_recs))
        one = store.nbytes()
        before = group.group_items()
        assert keyed(group, store, world.r_key, world.r_recs) == world.r_ref
        after = group.group_items()
        assert [a - b for a, b in zip(after, before)] == [R_N // 2, R_N // 2]
        assert store.nbytes() == 2 * one
        store.free()
    finally:
        group.close()
