"""GPU checks of the shared-doubling sums at the inputs where an addition chain goes wrong: k_naf_masks, k_msm_partial<G1|G2>,
k_msm_finish_g1 / _g2 / _groups_g1, k_gt_multiexp_partial and k_gt_lead, through rhip_pairing_jobs (the summed pair), rhip_aw11_decrypt_batch
and rhip_lsw_decrypt_batch_one_sk.

tests/msm_cases.py builds the items -- duplicated, opposite and infinite bases, scalars at the edges of ld_scalar and fr_shorten, ragged
term counts -- and proves in integers which branch each reaches (tests/test_msm_precheck.py runs the proofs without a GPU).  Here the same
items run in two regimes computed from the device's own compute-unit count with the function the engine uses (rb_msm_chunks): `small`,
where every lane holds one term and all adding is the finish kernels', and `chunked`, the smallest launch at which lanes hold two terms
or more.  Items are tiles of at most 24 kinds (msm_cases.layout puts them on the wave and block edges).

Reference: oracle.bn254 alone.  Every element is a known power, so an expected output is e(g1, g2)^x with x computed in Python integers:
exact, byte for byte, and the same for every tile of a kind."""
import time

import pytest

from oracle import bn254 as bn
from rabe_amd import engine as E
from rabe_amd.engine import Engine
from tests import msm_cases as mc
from tests.hostsim import build as hsb

pytestmark = pytest.mark.gpu
R = bn.R
INF1, INF2 = bytes(64), bytes(128)


class World:
    """g1 * log, g2 * log and e(g1, g2)^log as the engine's records, each computed once"""

    def __init__(self):
        self.egg = bn.pairing(bn.G1_GEN, bn.G2_GEN)
        self.c1, self.c2, self.ct = {0: INF1}, {0: INF2}, {0: bn.gt_to_le(bn.GT_ONE)}

    def g1(self, log):
        log %= R
        if log not in self.c1:
            self.c1[log] = bn.g1_to_le(bn.g1_mul(bn.G1_GEN, log))
        return self.c1[log]

    def g2(self, log):
        log %= R
        if log not in self.c2:
            self.c2[log] = bn.g2_to_le(bn.g2_mul(bn.G2_GEN, log))
        return self.c2[log]

    def gt(self, log):
        log %= R
        if log not in self.ct:
            self.ct[log] = bn.gt_to_le(bn.gt_pow(self.egg, log))
        return self.ct[log]


@pytest.fixture(scope="module")
def world():
    return World()


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def regimes(eng):
    """{name: (n_items, max_terms, L, C)} for this device, from the engine's own chunk choice"""
    hs = hsb.load()
    n_cu = eng.device_info()[0]
    simds = 4 * n_cu
    small = (mc.SMALL_ITEMS, mc.SMALL_TERMS) + mc.chunks(hs, simds, mc.SMALL_ITEMS, mc.SMALL_TERMS)
    assert small[3] == 1 and small[2] == mc.SMALL_TERMS, small           # one term per lane
    n = mc.chunked_items(hs, simds)
    if n_cu == 256:
        assert n is not None and n <= 4200, n
    out = {"small": small, "chunked": None if n is None else (n, mc.CHUNKED_TERMS) + mc.chunks(hs, simds, n, mc.CHUNKED_TERMS)}
    print("msm regimes on %d CUs (n_items, max_terms, L, C):" % n_cu, out)
    return out


def regime_of(regimes, name):
    if regimes[name] is None:
        pytest.skip("no n_items up to 8192 gives chunks of two terms at %d terms on this device" % mc.CHUNKED_TERMS)
    n, max_terms, L, C = regimes[name]
    assert (C >= 2 and L >= 2) if name == "chunked" else C == 1
    return n, max_terms, mc.cases(max_terms, L, C), mc.layout(n)


def kind_index(kind):
    return mc.KINDS.index(kind)


def offsets(counts):
    out = [0]
    for c in counts:
        out.append(out[-1] + c)
    return out


def assert_tiles(got, kinds, want):
    """every item's 384 bytes against its kind's expected Gt"""
    assert len(got) == len(kinds)
    wrong = sorted({k for g, k in zip(got, kinds) if g != want[k]})
    assert wrong == [], "kinds with a wrong output: %s (first items %s)" % (wrong, [kinds.index(k) for k in wrong])
    assert len(set(want.values())) == len(want)                          # no two kinds share an expected value: an item cannot pass as its neighbour


# ---------------------------------------------------------------------------------------------------- rhip_pairing_jobs: the summed pair
@pytest.mark.parametrize("shape", ["sum only", "two pairs and the sum"])
@pytest.mark.parametrize("regime", ["small", "chunked"])
def test_pairing_jobs_summed_pair(eng, world, regimes, regime, shape):
    """k_msm_partial<G1> with flip = 0 and k_msm_finish_g1 writing into the combined pair list.  An infinite sum is a skipped pair:
    out = lead * FE(the other pairs), and out = lead where the sum is the item's only pair."""
    n, _max_terms, cases, kinds = regime_of(regimes, regime)
    per, want = {}, {}
    for kind, case in cases.items():
        pairs, q_s, lead, x = mc.jobs_item(case, kind_index(kind), shape != "sum only")
        per[kind] = dict(p=[world.g1(p) for p, _k, _q in pairs], k=[mc.word_bytes(k) for _p, k, _q in pairs], q=[world.g2(q) for _p, _k, q in pairs],
                         sb=[world.g1(d) for d, _w in case.terms], sk=[mc.word_bytes(w) for _d, w in case.terms], sq=world.g2(q_s),
                         lead=world.gt(lead))
        want[kind] = world.gt(x)
        if kind in mc.INFINITE and shape == "sum only":
            assert want[kind] == per[kind]["lead"]
    p, k, q, sb, sk = ([x for kind in kinds for x in per[kind][f]] for f in ("p", "k", "q", "sb", "sk"))
    t0 = time.time()
    got = eng.pairing_jobs(offsets([len(per[kind]["p"]) for kind in kinds]), p, q, scal=k or None, lead=[per[kind]["lead"] for kind in kinds],
                           sum_offsets=offsets([len(per[kind]["sb"]) for kind in kinds]), s_base=sb, s_scal=sk, s_q=[per[kind]["sq"] for kind in kinds])
    print("rhip_pairing_jobs %s / %s: %d items, %.2f s" % (regime, shape, n, time.time() - t0))
    assert_tiles(got, kinds, want)


# ---------------------------------------------------------------------------------------------------- rhip_aw11_decrypt_batch
@pytest.mark.parametrize("regime", ["small", "chunked"])
def test_aw11_decrypt_sum_and_leading_factor(eng, world, regimes, regime):
    """k_msm_partial<G2> (flip = 0) with k_msm_finish_g2, and k_gt_multiexp_partial (flip = 1) with k_gt_lead, on one set of coefficient
    words.  The items of a kind share their selection entries, ciphertext rows and key, so sel_start (per kind) differs from the term
    offsets (per item): the masks are indexed by the one, the gathered bases by the other."""
    n, _max_terms, cases, kinds = regime_of(regimes, regime)
    sel_start, row_off, attr_off, want, a0 = {}, {}, {}, {}, {}
    sel_row, sel_attr, coeff, c1, c2, c3, sk_k, sk_h = [], [], [], [], [], [], [], []
    key_of = {kind: i for i, kind in enumerate(cases)}
    for kind, case in cases.items():
        rows, h, a0[kind], x = mc.aw11_item(case, kind_index(kind))
        sel_start[kind], row_off[kind], attr_off[kind] = len(sel_row), len(c1), len(sk_k)
        # the entries walk the rows backwards and the key's attributes forwards: row, attribute and entry index all differ
        m = len(rows)
        sel_row += [m - 1 - j for j in range(m)]
        sel_attr += list(range(m))
        coeff += [mc.word_bytes(w) for _t, w in case.terms]
        stored = rows[::-1]
        c1 += [world.gt(a) for a, _u, _t, _k in stored]
        c2 += [world.g2(u) for _a, u, _t, _k in stored]
        c3 += [world.g2(t) for _a, _u, t, _k in stored]
        sk_k += [world.g1(kp) for _a, _u, _t, kp in rows]
        sk_h.append(world.g1(h))
        want[kind] = world.gt(x)
    assert any(sel_start[k] != o for k, o in zip(kinds, offsets([len(cases[k].terms) for k in kinds])))
    pair_off = offsets([len(cases[kind].terms) + 1 for kind in kinds])
    d_out = eng.alloc(n * 384)
    up = lambda rec, pad: eng.upload(b"".join(rec) or pad)
    t0 = time.time()
    E.aw11_decrypt_dev(eng, n, max(b - a for a, b in zip(pair_off, pair_off[1:])), pair_off[-1], len(sel_row), eng.upload_u32(pair_off),
                       eng.upload_u32([sel_start[kind] for kind in kinds]), eng.upload_u32(sel_row), eng.upload_u32(sel_attr), up(coeff, bytes(32)),
                       eng.upload(b"".join(world.gt(a0[kind]) for kind in kinds)), up(c1, bytes(384)), up(c2, INF2), up(c3, INF2),
                       eng.upload_u32([row_off[kind] for kind in kinds]), up(sk_h, INF1), up(sk_k, INF1),
                       eng.upload_u32([attr_off[kind] for kind in cases] + [len(sk_k)]), eng.upload_u32([key_of[kind] for kind in kinds]), d_out)
    raw = eng.download(d_out)
    print("rhip_aw11_decrypt_batch %s: %d items, %d pairs, %.2f s" % (regime, n, pair_off[-1], time.time() - t0))
    assert_tiles([raw[384 * i:384 * i + 384] for i in range(n)], kinds, want)


# ---------------------------------------------------------------------------------------------------- rhip_lsw_decrypt_batch_one_sk
LSW_ITEMS = 130


@pytest.mark.parametrize("regime", ["small", "chunked"])
def test_lsw_one_sk_group_sums(eng, world, regimes, regime):
    """k_msm_partial<G1> with flip = 1 and k_msm_finish_groups_g1: the groups are the sums' items (their count chooses the chunks), 130
    decrypt items point at the groups on the wave and block edges, at the ordinary block's infinite sums (gsum_inf) and at the last block."""
    n_groups, _max_terms, cases, group_kind = regime_of(regimes, regime)
    d1_logs = sorted({d for case in cases.values() for d, _w in case.terms})
    row_of = {d: i for i, d in enumerate(d1_logs)}
    attrs = sorted({e for kind, case in cases.items() for e in mc.lsw_item(case, kind_index(kind), 0)[0]})
    attr_of = {e: i for i, e in enumerate(attrs)}
    group_off = offsets([len(cases[kind].terms) for kind in group_kind])
    sel_sk, sel_ct, coeff = [], [], []
    per = {}
    for kind, case in cases.items():
        eps = mc.lsw_item(case, kind_index(kind), 0)[0]
        per[kind] = ([row_of[d] for d, _w in case.terms], [attr_of[e] for e in eps], [mc.word_bytes(w) for _d, w in case.terms])
    for kind in group_kind:
        sel_sk += per[kind][0]
        sel_ct += per[kind][1]
        coeff += per[kind][2]
    picked = [g for g in list(range(70)) + [127, 128, 255, 256, 2 * mc.G1_FINISH_BLOCK + 87, 2 * mc.G1_FINISH_BLOCK + 88,
                                            2 * mc.G1_FINISH_BLOCK + mc.G2_FINISH_BLOCK + 41] if g < n_groups - 8]
    picked += list(range(n_groups - 8, n_groups))
    item_group = [picked[i % len(picked)] for i in range(LSW_ITEMS)]
    assert {group_kind[g] for g in item_group} == set(cases)
    want, e1, e2 = [], [], []
    for i, g in enumerate(item_group):
        _eps, x, y, expo = mc.lsw_item(cases[group_kind[g]], kind_index(group_kind[g]), i)
        e1.append(world.gt(x)), e2.append(world.g2(y)), want.append(world.gt(expo))
    pair_off = offsets([len(cases[group_kind[g]].terms) + 1 for g in item_group])
    d_d2 = eng.upload(b"".join(world.g2(mc.lsw_d2(d)) for d in d1_logs))
    lines = E.G2Lines(eng, len(d1_logs), d_d2)
    d_out = eng.alloc(LSW_ITEMS * 384)
    t0 = time.time()
    E.lsw_decrypt_one_sk_dev(eng, LSW_ITEMS, max(b - a for a, b in zip(pair_off, pair_off[1:])), pair_off[-1], len(sel_sk), eng.upload_u32(pair_off),
                             eng.upload_u32([group_off[g] for g in item_group]), eng.upload_u32(sel_sk), eng.upload_u32(sel_ct), eng.upload(b"".join(coeff)),
                             n_groups, eng.upload_u32(group_off), eng.upload_u32(item_group), eng.upload(b"".join(e1)), eng.upload(b"".join(e2)),
                             eng.upload(b"".join(world.g1(e) for e in attrs)), eng.upload_u32([0] * (LSW_ITEMS + 1)),
                             eng.upload(b"".join(world.g1(d) for d in d1_logs)), lines, d_out)
    raw = eng.download(d_out)
    print("rhip_lsw_decrypt_batch_one_sk %s: %d groups, %d items, %.2f s" % (regime, n_groups, LSW_ITEMS, time.time() - t0))
    lines.destroy()
    got = [raw[384 * i:384 * i + 384] for i in range(LSW_ITEMS)]
    wrong = [(i, item_group[i], group_kind[item_group[i]]) for i in range(LSW_ITEMS) if got[i] != want[i]]
    assert wrong == []
    for a in range(LSW_ITEMS):                                            # items of one group and one (e1, e2) are equal; others are not
        for b in range(a + len(picked), LSW_ITEMS, len(picked)):
            assert item_group[a] == item_group[b] and (got[a] == got[b]) == (want[a] == want[b])
