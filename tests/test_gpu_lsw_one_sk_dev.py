"""Device-level LSW decrypt of many ciphertexts under ONE key (rhip_lsw_decrypt_batch_one_sk): the key-side Miller loops replay the key's
prepared lines, sum -c_e D1_e is computed once per selection group.  Against rhip_lsw_decrypt_batch with sk_idx = 0 on the same arrays,
byte for byte, and against the oracle's decrypt for the items whose selection is the real one.

Shapes: one key of 6 leaves (one negative), 130 ciphertexts = two 64-item gather tiles and a remainder, 1 .. 8 attribute rows, selections
of 1 .. 5 entries (ragged pair counts inside every tile); half the items share one of three groups, the others own theirs."""
import random

import pytest

from oracle import bn254 as bn
from oracle import policy as pol
from oracle import schemes as sch
from oracle.tape import SeededRng
from rabe_amd import Engine
from rabe_amd import engine as E
from rabe_amd import hostprep as hp

pytestmark = pytest.mark.gpu

N_ITEMS = 130
KEY = ("or", [("and", [("leaf", "A"), ("leaf", "B"), ("leaf", "C")]), ("and", [("leaf", "D"), ("leaf", "E")]), ("leaf", "!N")])
NEG_ROW = 5
POOL_ATTRS = [["D"], ["E", "D"], ["C", "A", "B"], ["A", "B", "C", "X"], ["D", "A", "E", "B", "Y"], ["B", "X", "A", "Y", "C", "Z"],
              ["E", "A", "X", "D", "Y", "Z", "W"], ["X", "C", "Y", "B", "Z", "A", "W", "V"]]
REAL_ITEMS = [1, 3, 5, 7]                   # odd items of the first round: their own group is the pruned selection of their ciphertext
ORACLE_DECRYPTS = [1, 3]                    # ... of which the oracle decrypts these (a Python pairing per entry); the others against the sealed Gt


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def le(x):
    return hp.fr_le(x)


def offsets(counts):
    out = [0]
    for c in counts:
        out.append(out[-1] + c)
    return out


@pytest.fixture(scope="module")
def world():
    """key, the pool of 8 real ciphertexts (1 .. 8 rows) and the oracle's decrypt of the real items: computed once"""
    rng = SeededRng(61)
    pk, msk = sch.lsw_setup(rng)
    sk = sch.lsw_keygen(pk, msk, hp.to_json(KEY), pol.JSON, rng)
    assert [r[0] for r in sk["dj"]] == ["A", "B", "C", "D", "E", "!N"] and sk["dj"][NEG_ROW][1] is None
    msgs = [bn.gt_pow(pk["e_gg_alpha"], 1000003 + 17 * p) for p in range(len(POOL_ATTRS))]
    cts = [sch.lsw_encrypt(pk, a, rng, m) for a, m in zip(POOL_ATTRS, msgs)]
    want = {}
    for i in REAL_ITEMS:
        want[i] = bn.gt_to_le(msgs[i % 8])
        if i in ORACLE_DECRYPTS:
            assert bn.gt_to_le(sch.lsw_decrypt(sk, cts[i % 8])) == want[i]
    return sk, cts, want


def selections():
    """(groups, item_group): group = list of (key leaf row, ciphertext row, coefficient)"""
    rnd = random.Random(23)
    z = hp.leaf_coefficients(KEY)
    shared = [[(2, 0, rnd.randrange(1, bn.R))],
              [(0, 2, rnd.randrange(1, bn.R)), (4, 0, rnd.randrange(1, bn.R)), (1, 1, bn.R - 5)],
              [(4, 4, rnd.randrange(1, bn.R)), (3, 0, 1), (2, 3, rnd.randrange(1, bn.R)), (1, 1, rnd.randrange(1, bn.R)), (0, 2, 2)]]
    groups, item_group = list(shared), []
    for i in range(N_ITEMS):
        rows = i % 8 + 1
        if i % 2 == 0:
            item_group.append(2 if rows >= 5 and i % 4 == 0 else 1 if rows >= 3 else 0)
            continue
        attrs = POOL_ATTRS[i % 8]
        if (i // 8) % 2 == 0:                                            # the real selection of this ciphertext under the key
            ok, idx = hp.pruned_leaf_indices(attrs, KEY)
            assert ok
            g = [(y, attrs.index(hp.leaves(KEY)[y]), z[y]) for y in idx]
        else:                                                            # any rows, any coefficients: the two entry points compute one formula
            m = min((i // 16) % 5 + 1, rows)
            g = [(rnd.randrange(5), rnd.randrange(rows), rnd.randrange(1, bn.R)) for _ in range(m)]
            if i % 16 == 9:
                g[0] = (NEG_ROW, g[0][1], g[0][2])                       # the key's negative leaf: D1 and D2 are the identity -> a skipped pair
        item_group.append(len(groups))
        groups.append(g)
    return groups, item_group


def run_both(eng, world, one_group_per_item=False, identity_e2_item=None):
    sk, cts, _ = world
    groups, item_group = selections()
    if one_group_per_item:
        groups, item_group = [groups[g] for g in item_group], list(range(N_ITEMS))
    group_off = offsets([len(g) for g in groups])
    entries = [e for g in groups for e in g]
    sel_start = [group_off[g] for g in item_group]
    pair_off = offsets([len(groups[g]) + 1 for g in item_group])
    assert len(set(item_group[i] for i in range(0, N_ITEMS, 2))) == (3 if not one_group_per_item else N_ITEMS // 2)
    assert set(len(g) for g in groups) == {1, 2, 3, 4, 5}
    pool = [i % 8 for i in range(N_ITEMS)]
    e2 = [bn.g2_to_le(cts[p]["e2"]) for p in pool]
    if identity_e2_item is not None:
        e2[identity_e2_item] = bytes(128)
    d = dict(
        pair_off=eng.upload_u32(pair_off), sel_start=eng.upload_u32(sel_start), sel_sk=eng.upload_u32([e[0] for e in entries]),
        sel_ct=eng.upload_u32([e[1] for e in entries]), sel_z=eng.upload(b"".join(le(e[2]) for e in entries)),
        e1=eng.upload(b"".join(bn.gt_to_le(cts[p]["e1"]) for p in pool)), e2=eng.upload(b"".join(e2)),
        e1j=eng.upload(b"".join(bn.g1_to_le(row[1]) for p in pool for row in cts[p]["ej"])),
        attr_off=eng.upload_u32(offsets([p + 1 for p in pool])),
        d1=eng.upload(b"".join(bn.g1_to_le(r[1]) for r in sk["dj"])), d2=eng.upload(b"".join(bn.g2_to_le(r[2]) for r in sk["dj"])))
    max_pairs = max(b - a for a, b in zip(pair_off, pair_off[1:]))
    general, one_sk = eng.alloc(N_ITEMS * 384), eng.alloc(N_ITEMS * 384)
    E.lsw_decrypt_dev(eng, N_ITEMS, max_pairs, pair_off[-1], len(entries), d["pair_off"], d["sel_start"], d["sel_sk"], d["sel_ct"], d["sel_z"], d["e1"],
                      d["e2"], d["e1j"], d["attr_off"], None, d["d1"], d["d2"], eng.upload_u32([0, len(sk["dj"])]), eng.upload_u32([0] * N_ITEMS), None,
                      general)
    lines = E.G2Lines(eng, len(sk["dj"]), d["d2"])
    E.lsw_decrypt_one_sk_dev(eng, N_ITEMS, max_pairs, pair_off[-1], len(entries), d["pair_off"], d["sel_start"], d["sel_sk"], d["sel_ct"], d["sel_z"],
                             len(groups), eng.upload_u32(group_off), eng.upload_u32(item_group), d["e1"], d["e2"], d["e1j"], d["attr_off"], d["d1"], lines,
                             one_sk)
    a, b = eng.download(general), eng.download(one_sk)
    lines.destroy()
    return [a[384 * i:384 * i + 384] for i in range(N_ITEMS)], [b[384 * i:384 * i + 384] for i in range(N_ITEMS)]


def differing(a, b):
    return [i for i in range(len(a)) if a[i] != b[i]]


def test_one_sk_equals_the_general_entry_point_and_the_oracle(eng, world):
    general, one_sk = run_both(eng, world)
    assert differing(general, one_sk) == []
    assert len(set(one_sk)) > 8                                          # not one constant
    for i, want in world[2].items():
        assert one_sk[i] == want, i


def test_one_group_per_item(eng, world):
    general, one_sk = run_both(eng, world, one_group_per_item=True)
    assert differing(general, one_sk) == []
    for i, want in world[2].items():
        assert one_sk[i] == want, i


def test_identity_e2_takes_the_skipped_pair(eng, world):
    plain = run_both(eng, world)[1]
    general, one_sk = run_both(eng, world, identity_e2_item=67)
    assert differing(general, one_sk) == []
    assert differing(plain, one_sk) == [67]
