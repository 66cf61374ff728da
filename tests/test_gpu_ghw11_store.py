"""GPU checks of the GHW11 key store that adds and revokes keys in place (include/rabe_host.h: rabe_ghw11_tk_store_open, _add, _revoke, _stat).
The world is that of tests/test_gpu_ghw11_keyed.py: users A, B, C with 1, 3 and 2 attributes -- 3, 5 and 4 blocks -- plus D (2 attributes) and
E (3) for the holes; keys from provision_packed on a tape; one ciphertext per user that is the AND over the user's attributes, and one under an
attribute no user holds.  The yardstick everywhere is rabe_ghw11_transform_packed for one record alone under one key: every expectation is
that call's 768 bytes and verdict."""
import numpy as np
import pytest

from rabe_amd import hostlib as hl
from rabe_amd.schemes import ghw11

pytestmark = pytest.mark.gpu

SETS = [["A"], ["A", "B", "C"], ["B", "C"], ["A", "C"], ["A", "B", "D"]]          # users A, B, C, D, E
A, B, C, D, E = range(5)
BLOCKS = [2 + len(s) for s in SETS]
LEAF = '{"name": "%s"}'
AND = lambda names: LEAF % names[0] if len(names) == 1 else '{"name": "and", "children": [%s]}' % ", ".join(LEAF % x for x in names)
POLS = [AND(s) for s in SETS] + [LEAF % "Z"]          # policy u: the AND over user u's attributes; the last one: nobody's
# the mixed queue: (user, policy).  Items 4 and 5 name a policy their user cannot satisfy; B also satisfies A's, C's and D's policies
QUEUE = [(A, 0), (B, 1), (C, 2), (B, 2), (A, 5), (C, 0), (B, 0), (C, 2)]
ZERO = (bytes(768), -1)
NONE = 0xFFFFFFFF


def offsets(items):
    return np.concatenate([[0], np.cumsum([len(p) for p in items])]).astype(np.uint64)


def records(blob, off):
    return [bytes(blob[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


class World:
    def want(self, user, pol):
        """the definition: the policy's record alone under the user's key (made once per pair)"""
        if (user, pol) not in self._ref:
            rec = self.recs[pol]
            out, st = ghw11.transform_packed(self.host, self.tk[user], rec, [0, len(rec)])
            self._ref[(user, pol)] = (out[0].tobytes(), int(st[0]))
        return self._ref[(user, pol)]

    def blob(self, users):
        recs = [self.tk_recs[u] for u in users]
        return b"".join(recs), offsets(recs)


@pytest.fixture(scope="module")
def world():
    w = World()
    w.host = host = hl.Host(0)
    w.pk, w.msk = ghw11.setup(host)
    host.set_tape([11, 12, 13, 14, 15, 101, 102, 103, 104, 105])          # r_0 .. r_4, then z_0 .. z_4
    _sk, _so, tk_blob, tk_off, _rk = ghw11.provision_packed(host, w.pk, w.msk, SETS, list(range(5)), want_sk=False)
    host.clear_tape()
    w.tk_recs = records(tk_blob, tk_off)
    w.tk = [hl.Obj.deserialize("ghw11_tk", r) for r in w.tk_recs]
    pts = [b"under policy %d" % p for p in range(len(POLS))]
    blob, off = ghw11.encrypt_packed(host, w.pk, POLS, list(range(len(POLS))), b"".join(pts), offsets(pts))
    w.recs = records(blob, off)
    w._ref = {}
    for user, pol in QUEUE:
        w.want(user, pol)
    assert [w.want(u, p)[1] for u, p in QUEUE] == [0, 0, 0, 0, -1, -1, 0, 0]
    assert w.want(B, 2)[0] != w.want(C, 2)[0]          # one record under two keys: two different answers
    yield w
    host.close()


def served(w, store, ids, queue=QUEUE, trusted=False, host=None):
    """the queue against the store: item j under store id ids[user of item j]"""
    recs = [w.recs[p] for _u, p in queue]
    out, st = ghw11.transform_keyed(host or w.host, store, [ids[u] for u, _p in queue], b"".join(recs), offsets(recs), trusted=trusted)
    return [(out[j].tobytes(), int(st[j])) for j in range(len(queue))]


def wanted(w, queue=QUEUE, gone=()):
    return [ZERO if u in gone else w.want(u, p) for u, p in queue]


def last_error(host):
    return host.lib.rabe_host_last_error(host.h)


def test_open_add_revoke_and_reuse(world):
    w, host = world, world.host
    # 1. an empty store of 16 blocks, three keys: blocks 0-2, 3-7, 8-11
    store = ghw11.tk_store_open(host, 16)
    assert store.stat() == (0, 16, 0, 16)
    ids, st = store.add(*w.blob([A, B, C]))
    assert ids.tolist() == [0, 1, 2] and st.tolist() == [0, 0, 0]
    assert store.stat() == (3, 16, 12, 4)
    of = {A: 0, B: 1, C: 2}
    for trusted in (False, True):
        assert served(w, store, of, trusted=trusted) == wanted(w), trusted
    made = ghw11.tk_store_create(host, *w.blob([A, B, C]))
    assert served(w, made, of) == wanted(w)
    made.free()
    # 2. B is revoked: its items fail alone, the others keep their bytes
    assert store.revoke([1]).tolist() == [0]
    assert store.stat() == (2, 16, 7, 5)
    assert served(w, store, of) == wanted(w, gone=(B,))
    assert b"transform key revoked" in last_error(host)
    assert store.revoke([1]).tolist() == [-1]
    assert b"revoked" in last_error(host)
    assert store.revoke([99]).tolist() == [-1]
    assert b"never issued" in last_error(host)
    assert store.revoke([99, 1, NONE]).tolist() == [-1, -1, -1]
    assert store.stat() == (2, 16, 7, 5)
    # 3. D (4 blocks) lands in B's hole at the lowest address: blocks 3-6, block 7 and blocks 12-15 stay free
    ids, st = store.add(*w.blob([D]))
    assert ids.tolist() == [3] and st.tolist() == [0]
    assert store.stat() == (3, 16, 11, 4)
    of[D] = 3
    queue = QUEUE + [(D, 3), (D, 0), (D, 2)]          # D holds A and C: its own policy and A's, not C's
    assert [w.want(u, p)[1] for u, p in queue[-3:]] == [0, 0, -1]
    assert served(w, store, of, queue) == wanted(w, queue, gone=(B,))
    # 4. E needs 5 blocks; 1 + 4 are free, not contiguous: refused, nothing changed
    assert store.add(*w.blob([E])) is None
    assert store.stat() == (3, 16, 11, 4)
    assert served(w, store, of, queue) == wanted(w, queue, gone=(B,))
    assert store.revoke([3]).tolist() == [0]
    assert store.stat() == (2, 16, 7, 5)
    ids, st = store.add(*w.blob([E]))
    assert ids.tolist() == [4] and st.tolist() == [0]          # the refused call took no id
    assert store.stat() == (3, 16, 12, 4)
    of[E] = 4
    queue = queue + [(E, 4), (E, 0), (E, 2)]
    assert [w.want(u, p)[1] for u, p in queue[-3:]] == [0, 0, -1]
    assert served(w, store, of, queue) == wanted(w, queue, gone=(B, D))
    assert b"transform key revoked" in last_error(host)
    store.free()


def test_a_bad_key_fails_alone_in_an_add(world):
    from tests.ac17_packed_cases import non_members
    w, host = world, world.host
    outside = bytearray(w.tk_recs[C])
    outside[-128:] = non_members()["twist"]          # C's last k_x: on the twist, outside the subgroup
    good = [w.tk_recs[A], w.tk_recs[B]]
    cut = w.tk_recs[D][:-5]
    batch = [good[0], cut, bytes(outside), good[1]]
    store = ghw11.tk_store_open(host, 16)
    ids, st = store.add(b"".join(batch), offsets(batch))
    assert st.tolist() == [0, -1, -1, 0] and ids.tolist() == [0, NONE, NONE, 1]
    assert b"deserialize" in last_error(host)          # the first error: the truncated record
    assert store.stat() == (2, 16, 8, 4)               # A at 0-2, B at 7-11; the non-member's blocks 3-6 are free again
    queue = [q for q in QUEUE if q[0] != C]
    assert served(w, store, {A: 0, B: 1}, queue) == wanted(w, queue)
    # alone, so that its message is the call's first
    ids, st = store.add(bytes(outside), [0, len(outside)])
    assert st.tolist() == [-1] and ids.tolist() == [NONE] and b"not a member of G2" in last_error(host)
    assert store.stat() == (2, 16, 8, 4)
    # in trusted mode the membership pass is the caller's word: the key is taken, and the next id is 2
    ids, st = store.add(bytes(outside), [0, len(outside)], trusted=True)
    assert st.tolist() == [0] and ids.tolist() == [2]
    assert store.stat() == (3, 16, 12, 4)
    assert served(w, store, {A: 0, B: 1}, queue) == wanted(w, queue)
    store.free()


def test_a_created_store_is_full_until_a_key_is_revoked(world):
    w, host = world, world.host
    store = ghw11.tk_store_create(host, *w.blob([A, B, C]))
    assert store.key_status.tolist() == [0, 0, 0]
    assert store.stat() == (3, 12, 12, 0)
    held = store.nbytes()
    assert store.add(*w.blob([A])) is None
    assert store.stat() == (3, 12, 12, 0)
    assert store.revoke([1]).tolist() == [0]          # B, the 5-block key
    assert store.stat() == (2, 12, 7, 5)
    ids, st = store.add(*w.blob([E]))                  # 5 blocks: exactly B's hole
    assert ids.tolist() == [3] and st.tolist() == [0]
    assert store.stat() == (3, 12, 12, 0)
    assert store.nbytes() == held
    of = {A: 0, B: 1, C: 2, E: 3}
    queue = QUEUE + [(E, 4), (E, 0)]
    assert served(w, store, of, queue) == wanted(w, queue, gone=(B,))
    store.free()


def test_a_device_group_follows_every_change(world):
    """two engines on GPU 0.  First store: both replicas exist before the changes, which reach both.  Second store: the second engine meets
    the store after the changes and prepares its replica from the store as it is then."""
    w = world
    group = hl.Host(devices=[0, 0])
    try:
        queue = QUEUE + [(D, 3), (D, 0)]
        of = {A: 0, B: 1, C: 2, D: 3}
        want = wanted(w, queue, gone=(B,))
        for early in (True, False):
            store = ghw11.tk_store_open(group, 16)
            one = store.nbytes()
            assert one > 0
            ids, _st = store.add(*w.blob([A, B, C]))
            assert ids.tolist() == [0, 1, 2]
            if early:
                assert served(w, store, of, QUEUE, host=group) == wanted(w)          # cut in two: the replicas get made
                assert store.nbytes() == 2 * one
            else:
                assert served(w, store, of, QUEUE[:1], host=group) == wanted(w, QUEUE[:1])          # one item: the first engine alone
                assert store.nbytes() == one
            assert store.revoke([1]).tolist() == [0]
            ids, _st = store.add(*w.blob([D]))
            assert ids.tolist() == [3] and store.stat() == (3, 16, 11, 4)
            before = group.group_items()
            assert served(w, store, of, queue, host=group) == want, early
            assert [a - b for a, b in zip(group.group_items(), before)] == [len(queue) // 2, len(queue) // 2]
            assert store.nbytes() == 2 * one
            store.free()
    finally:
        group.close()
