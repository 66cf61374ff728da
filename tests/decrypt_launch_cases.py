"""The table behind tests/test_gpu_decrypt_launch_contract.py and tools/record_decrypt_launch_contract.py: every device entry point whose host
side is the decrypt launch code of rabe_amd/csrc/engine_jobs.hip, and the shapes each one is run through.

What is recorded is how a call is LAUNCHED -- the return code, which kernels ran how often, the bytes that came out -- not whether a scheme
decrypts (the scheme tests do that), so the inputs are synthetic: every group element is a fixed multiple of a generator, computed on the device
by kernels the launch code under test does not touch (rhip_g1_mul, rhip_g2_mul, rhip_pairing), every index table is arithmetic on the shape.
A record is a pure function of the library and of the device's compute-unit count (the kernel families are chosen by it).

Shapes -- selected leaves per item, at most four; the smallest that reach each branch of the launch code:
  one            1 item
  uniform3       3 items, equal pair counts: the uniform gather map (ppi != 0), the (L, C) Miller geometry
  ragged5        5 items, differing pair counts: lane = pair (fewer than 64 items), the device-planned Miller geometry
  tiled65        65 items, differing pair counts: the tiled gather map, two tiles, one item in the last -- the one with the most pairs
  shared64       64 items on ONE selection (n_sel far below the pair count): BSW one-key scales once per entry and compacts the gather
                 (ppi >= 3), LSW one-ciphertext scales once per entry
  ragged5_shared 5 items on prefixes of one selection: the per-entry scaling without the compact gather
  empty          3 items, the middle one with an empty selection
  all_empty      2 items with empty selections: no term at all, the (n ? n : 1) sizes of the sum's arenas
  two_groups     LSW under one key: two selection groups of unequal size, three items
Every selection holds a coefficient above r / 2 (fr_shorten folds its sign) beside small and full-size ones."""
import hashlib
import random
import re

from oracle import bn254 as bn
from rabe_amd import engine as E

R = bn.R
ROWS = 4                       # rows of a ciphertext, attributes of a key
N_KEYS = 2
MODES = (0, 99)
G1, G2, GT = 64, 128, 384

SHAPES = {
    "one": [2],
    "uniform3": [2, 2, 2],
    "ragged5": [1, 3, 2, 4, 1],
    "tiled65": [1 + i % 3 for i in range(64)] + [4],
    "shared64": [3] * 64,
    "ragged5_shared": [1, 3, 2, 4, 1],
    "empty": [2, 0, 1],
    "all_empty": [0, 0],
    "two_groups": [3, 1, 3],
}
SHARED = ("shared64", "ragged5_shared")
BASIC = ("one", "uniform3", "ragged5", "tiled65", "shared64", "empty")

_rnd = random.Random("decrypt launch contract")
COEFFS = [_rnd.randrange(1 << 200, (R - 1) // 2), R - 3, 1, _rnd.randrange(1 << 100, 1 << 128), _rnd.randrange((R + 1) // 2, R), 2, _rnd.randrange(1 << 250, R)]
assert all(0 < c < R for c in COEFFS) and sum(c > R // 2 for c in COEFFS) >= 2


class World:
    """pools of group elements (device-computed multiples of the generators, pairings of them) and the arrays cut from them"""

    def __init__(self, eng):
        self.eng = eng
        rnd = random.Random("decrypt launch pools")
        k = lambda n: [int(rnd.randrange(1, R)).to_bytes(32, "little") for _ in range(n)]
        self.p1 = eng.g1_mul([bn.g1_to_le(bn.G1_GEN)] * 17, k(17))
        self.p2 = eng.g2_mul([bn.g2_to_le(bn.G2_GEN)] * 13, k(13))
        self.pt = eng.pairing(self.p1[:7], self.p2[:7])

    def g1(self, n, salt):
        return self.eng.upload(b"".join(self.p1[(i + salt) % 17] for i in range(max(n, 1))))

    def g2(self, n, salt):
        return self.eng.upload(b"".join(self.g2_list(n, salt)))

    def g2_list(self, n, salt):
        return [self.p2[(i + salt) % 13] for i in range(max(n, 1))]

    def gt(self, n, salt):
        return self.eng.upload(b"".join(self.pt[(i + salt) % 7] for i in range(max(n, 1))))

    def u32(self, values):
        return self.eng.upload_u32(list(values) or [0])


def offsets(counts):
    out = [0]
    for c in counts:
        out.append(out[-1] + c)
    return out


class Selection:
    """the selection tables of a shape: item i selects m[i] entries from sel_start[i]; entry e names row e % 4 of the item's ciphertext and
    attribute (e + 1) % 4 of its key -- distinct within an item -- and owns coefficient COEFFS[e % 7]"""

    def __init__(self, w, shape):
        self.m = m = SHAPES[shape]
        self.n = len(m)
        shared = shape in SHARED
        self.start = [0] * self.n if shared else offsets(m)[:-1]
        self.n_sel = max(m) if shared else sum(m)
        room = max(self.n_sel, 1)                      # the tables are never empty buffers
        self.d_start = w.u32(self.start)
        self.d_a = w.u32([e % ROWS for e in range(room)])
        self.d_b = w.u32([(e + 1) % ROWS for e in range(room)])
        self.d_coeff = w.eng.upload(b"".join(int(COEFFS[e % len(COEFFS)]).to_bytes(32, "little") for e in range(room)))
        self.d_row_off = w.u32(offsets([ROWS] * self.n))           # every item owns four rows
        self.d_key_off = w.u32(offsets([ROWS] * N_KEYS))
        self.d_key_idx = w.u32([i % N_KEYS for i in range(self.n)])

    def pairs(self, w, per_leaf, other):
        """(max_pairs, total_pairs, device pair_off): per_leaf pairs per selected leaf and `other` more per item"""
        counts = [per_leaf * x + other for x in self.m]
        off = offsets(counts)
        return max(counts), off[-1], w.u32(off)


# ---- the entry points: each builder returns a function of the output buffer that makes the call
def bsw(w, shape, one_sk):
    s = Selection(w, shape)
    mx, total, d_off = s.pairs(w, 2, 1)
    d_d, d_dj2 = w.g2(N_KEYS, 1), w.g2(ROWS * N_KEYS, 3)
    lines = E.BswSkLines(w.eng, N_KEYS, ROWS * N_KEYS, d_d, d_dj2)
    ct = (w.g1(s.n, 2), w.gt(s.n, 1), w.g1(ROWS * s.n, 5), w.g2(ROWS * s.n, 7), s.d_row_off)
    sk = (d_d, w.g1(ROWS * N_KEYS, 11), d_dj2, s.d_key_off)
    if one_sk:
        return s.n, lines, lambda out: E.bsw_decrypt_one_sk_dev(w.eng, s.n, mx, total, s.n_sel, d_off, s.d_start, s.d_a, s.d_b, s.d_coeff, *ct, *sk, lines, out)
    return s.n, lines, lambda out: E.bsw_decrypt_dev(w.eng, s.n, mx, total, d_off, s.d_start, s.d_a, s.d_b, s.d_coeff, *ct, *sk, s.d_key_idx, lines, out)


def lsw(w, shape, one_ct):
    s = Selection(w, shape)
    n_sel = max(s.n_sel, 1)                      # the call refuses n_sel = 0; an all-empty batch leaves its one entry unused
    mx, total, d_off = s.pairs(w, 1, 1)
    n_ct = 1 if one_ct else s.n
    e2 = w.g2_list(n_ct, 2)
    d_e2 = w.eng.upload(b"".join(e2))
    lines = E.G2Lines(w.eng, n_ct, d_e2)
    d_e1, d_e1j = w.gt(s.n, 2), w.g1(ROWS * n_ct, 4)           # e1: one leading factor per item in both forms
    sk = (w.g1(ROWS * N_KEYS, 6), w.g2(ROWS * N_KEYS, 8), s.d_key_off, s.d_key_idx)
    if one_ct:
        return s.n, lines, lambda out: E.lsw_decrypt_one_ct_dev(w.eng, s.n, mx, total, n_sel, d_off, s.d_start, s.d_a, s.d_b, s.d_coeff, d_e1, d_e2, d_e1j, *sk, lines, out)
    d_ct_idx = w.u32(range(s.n))
    return s.n, lines, lambda out: E.lsw_decrypt_dev(w.eng, s.n, mx, total, n_sel, d_off, s.d_start, s.d_a, s.d_b, s.d_coeff, d_e1, d_e2, d_e1j, s.d_row_off, d_ct_idx,
                                                     *sk, lines, out)


def lsw_one_sk(w, shape):
    """one selection group per distinct leaf count of the shape (groups of unequal size wherever the counts differ); an item's entries are
    its group's"""
    m = SHAPES[shape]
    sizes = sorted(set(m), reverse=True)
    group_off = offsets(sizes)
    item_group = [sizes.index(x) for x in m]
    n, n_sel = len(m), max(group_off[-1], 1)
    counts = [x + 1 for x in m]
    pair_off = offsets(counts)
    d_d2 = w.g2(ROWS, 8)
    lines = E.G2Lines(w.eng, ROWS, d_d2)
    d = (w.u32(pair_off), w.u32([group_off[g] for g in item_group]), w.u32([e % ROWS for e in range(n_sel)]), w.u32([(e + 1) % ROWS for e in range(n_sel)]),
         w.eng.upload(b"".join(int(COEFFS[e % len(COEFFS)]).to_bytes(32, "little") for e in range(n_sel))))
    groups = (w.u32(group_off), w.u32(item_group))
    ct = (w.gt(n, 2), w.g2(n, 2), w.g1(ROWS * n, 4), w.u32(offsets([ROWS] * n)))
    d_d1 = w.g1(ROWS, 6)
    return n, lines, lambda out: E.lsw_decrypt_one_sk_dev(w.eng, n, max(counts), pair_off[-1], n_sel, *d, len(sizes), *groups, *ct, d_d1, lines, out)


def ghw11(w, shape, decrypt):
    s = Selection(w, shape)
    mx, total, d_off = s.pairs(w, 1, 2)
    d_key = w.g2(2 + ROWS, 9)                      # k, l, k_x[0 .. 3]
    lines = E.G2Lines(w.eng, 2 + ROWS, d_key)
    ct = (w.g1(s.n, 3), w.g1(ROWS * s.n, 5), w.g1(ROWS * s.n, 10), s.d_row_off)
    d_c = w.gt(s.n, 3)
    lib, eng = w.eng.lib, w.eng
    head = lambda: (eng.ctx, E._sz(s.n), E._sz(mx), E._sz(total), E._sz(s.n_sel), E._p(d_off), E._p(s.d_start), E._p(s.d_a), E._p(s.d_b), E._p(s.d_coeff)) + \
        tuple(E._p(x) for x in ct) + (lines.h,)
    if decrypt:
        return s.n, lines, lambda out: eng._check(lib.rhip_ghw11_decrypt_batch(*head(), E._p(d_c), E._p(out)))
    return s.n, lines, lambda out: eng._check(lib.rhip_ghw11_transform_batch(*head(), E._p(out)))


def aw11(w, shape, w4):
    s = Selection(w, shape)
    n_sel = max(s.n_sel, 1)
    mx, total, d_off = s.pairs(w, 1, 1)
    ct = (w.gt(s.n, 4), w.gt(ROWS * s.n, 5), w.g2(ROWS * s.n, 6), w.g2(ROWS * s.n, 10), s.d_row_off)
    sk = (w.g1(N_KEYS, 12), w.g1(ROWS * N_KEYS, 13), s.d_key_off, s.d_key_idx)
    return s.n, None, lambda out: E.aw11_decrypt_dev(w.eng, s.n, mx, total, n_sel, d_off, s.d_start, s.d_a, s.d_b, s.d_coeff, *ct, *sk, out, w4=w4)


def jobs(w, shape, with_sum):
    """item i: m[i] + 1 plain pairs (scaled), and with the sum m[i] terms under one more G2 point"""
    m = SHAPES[shape]
    n = len(m)
    pair_off, sum_off = offsets([x + 1 for x in m]), offsets(m)
    n_pairs, n_terms = pair_off[-1], sum_off[-1]
    k = lambda cnt, salt: w.eng.upload(b"".join(int(COEFFS[(e + salt) % len(COEFFS)]).to_bytes(32, "little") for e in range(max(cnt, 1))))
    d = (w.u32(pair_off), w.g1(n_pairs, 1), k(n_pairs, 0), w.g2(n_pairs, 2))
    d_sum = (w.u32(sum_off), w.g1(n_terms, 7), k(n_terms, 3), w.g2(n, 5)) if with_sum else (None, None, None, None)
    d_lead = w.gt(n, 6)
    lib, eng = w.eng.lib, w.eng
    return n, None, lambda out: eng._check(lib.rhip_pairing_jobs(eng.ctx, E._sz(n), E._sz(max(m) + 1), E._sz(n_pairs), *(E._p(x) for x in d),
                                                                E._sz(max(m) if with_sum else 0), E._sz(n_terms if with_sum else 0),
                                                                *(E._p(x) for x in d_sum), E._p(d_lead), E._p(out)))


def ac17(w, shape, prepared):
    """six pairs per item whatever the selection; item i sums m[i] ciphertext rows and m[i] key rows"""
    m = SHAPES[shape]
    n = len(m)
    sel_off = offsets(m)
    sel = [j for x in m for j in range(x)]
    k0 = w.g2_list(3 * N_KEYS, 4)
    d_k0 = w.eng.upload(b"".join(k0))
    lines = E.Ac17SkLines(w.eng, N_KEYS, d_k0) if prepared else None
    ct = (w.g2(3 * n, 1), w.g1(3 * ROWS * n, 2), w.u32(offsets([ROWS] * n)), w.gt(n, 5))
    sk = (w.g1(3 * ROWS * N_KEYS, 9), w.u32(offsets([ROWS] * N_KEYS)), w.g1(3 * N_KEYS, 14), w.u32([i % N_KEYS for i in range(n)]))
    sels = (w.u32(sel), w.u32(sel_off), w.u32(sel), w.u32(sel_off))
    if prepared:
        return n, lines, lambda out: E.ac17_decrypt_prepared_dev(w.eng, n, *ct, lines, *sk, *sels, out)
    return n, None, lambda out: E.ac17_decrypt_dev(w.eng, n, *ct, d_k0, *sk, *sels, out)


ENTRIES = {
    "rhip_bsw_decrypt_batch": (lambda w, s: bsw(w, s, False), BASIC),
    "rhip_bsw_decrypt_batch_one_sk": (lambda w, s: bsw(w, s, True), BASIC + ("ragged5_shared",)),
    "rhip_lsw_decrypt_batch": (lambda w, s: lsw(w, s, False), BASIC + ("all_empty",)),
    "rhip_lsw_decrypt_batch_one_ct": (lambda w, s: lsw(w, s, True), BASIC + ("ragged5_shared", "all_empty")),
    "rhip_lsw_decrypt_batch_one_sk": (lsw_one_sk, ("one", "uniform3", "ragged5", "tiled65", "shared64", "two_groups", "empty")),
    "rhip_ghw11_transform_batch": (lambda w, s: ghw11(w, s, False), BASIC + ("all_empty",)),
    "rhip_ghw11_decrypt_batch": (lambda w, s: ghw11(w, s, True), BASIC + ("all_empty",)),
    "rhip_aw11_decrypt_batch": (lambda w, s: aw11(w, s, False), BASIC + ("all_empty",)),
    "rhip_aw11_decrypt_batch_w4": (lambda w, s: aw11(w, s, True), BASIC + ("all_empty",)),
    "rhip_pairing_jobs:sum": (lambda w, s: jobs(w, s, True), ("one", "uniform3", "ragged5", "tiled65", "empty", "all_empty")),
    "rhip_pairing_jobs:plain": (lambda w, s: jobs(w, s, False), ("one", "uniform3", "ragged5", "tiled65")),
    "rhip_ac17_cp_decrypt_batch": (lambda w, s: ac17(w, s, False), ("one", "uniform3", "ragged5", "tiled65", "shared64", "empty")),
    "rhip_ac17_cp_decrypt_batch_prepared": (lambda w, s: ac17(w, s, True), ("one", "uniform3", "ragged5", "tiled65", "shared64", "empty")),
}
CASES = [(entry, shape) for entry, (_build, shapes) in ENTRIES.items() for shape in shapes]


def run_case(w, entry, shape):
    """{mode: record} of one case: the return code, {kernel: launches} and the SHA-256 of the n_items Gt outputs (over a buffer of zeroes)"""
    eng = w.eng
    n, handle, call = ENTRIES[entry][0](w, shape)
    out = {}
    for mode in MODES:
        eng.set_pairing_mode(mode)
        d_out = eng.upload(bytes(n * GT))
        eng.timing(True)
        eng.timing_read()
        rc = 0
        try:
            call(d_out)
        except E.EngineError as err:
            rc = int(re.search(r"\((-?\d+)\)", str(err)).group(1))
        launches = {name: cnt for name, (_ms, cnt) in sorted(eng.timing_read().items())}
        eng.timing(False)
        out[str(mode)] = {"rc": rc, "launches": launches, "sha256": hashlib.sha256(eng.download(d_out, n * GT)).hexdigest()}
    eng.set_pairing_mode(0)
    if handle is not None:
        handle.destroy()
    return out
