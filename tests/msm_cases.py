"""Inputs that drive the shared-doubling sums (k_naf_masks, k_msm_partial<G1|G2>, k_msm_finish_g1 / _g2 / _groups_g1, and AW11's
k_gt_multiexp_partial / k_gt_lead) into the special cases of their additions, and the proof -- in integers, without a GPU -- that each of
them gets there.

Every base is a known multiple of a generator (a power of e(g1, g2) in Gt), so an item of a sum is a list of terms (log, scalar word): log 0
is the point at infinity (the all-zero record), the word is the 256-bit value the kernel reads, canonical or not.  `replay` restates what
the kernels do to an item cut into L chunks of C terms: the word reduced mod R (ld_scalar), the shorter of c and R - c with the sign folded
into the masks (fr_shorten), its NAF (unique: any correct NAF is the kernel's), chunk c = terms [c C, (c + 1) C), a walk over bits 255 .. 0
that doubles once started and then visits the chunk's terms in index order, skipping bases at infinity (jac_msm_naf), and the left-to-right
fold of the L partial sums (the finish kernels).  On the logs an addition is exceptional when the running log equals the addend's ("dbl":
the doubling branch of g1_madd_inl / jac_add_aff in a lane, of jac_add in the fold) or is its negative ("cancel": infinity in mid-walk, an
infinite partial or an infinite sum).  A case states the events it intends as (chunk or "finish", bit or partial index, kind); `check`
asserts that the replay meets exactly those and no other, so a test cannot silently miss its branch.

(L, C) is never restated here: the callers take it from rb_msm_chunks (rabe_amd/csrc/msm_chunks.h) through the host build's hs_msm_chunks.
tests/test_msm_precheck.py runs these proofs on the CPU; tests/test_gpu_msm_degenerate.py launches the same items."""
import ctypes
import random

from oracle import bn254 as bn

R = bn.R
HALF = (R - 1) // 2                 # fr_above_half: k > HALF takes R - k and the opposite sign
TWO256 = 1 << 256
FINISH = "finish"
G1_FINISH_BLOCK = 256               # RB_PAIRS_BLOCK: k_msm_finish_g1, k_msm_finish_groups_g1
G2_FINISH_BLOCK = 128               # the __launch_bounds__ of k_msm_finish_g2
SMALL_TERMS, CHUNKED_TERMS = 9, 17  # max_terms of the two regimes
SMALL_ITEMS = 130                   # two waves and two lanes; one G1 finish block partly inactive, one G2 finish block and two lanes


def chunks(hs, n_simds, n_items, max_terms):
    """(L, C) of rb_msm_chunks; hs: the loaded host build (tests/hostsim)"""
    L, C = ctypes.c_uint32(), ctypes.c_uint32()
    hs.hs_msm_chunks(ctypes.c_size_t(n_simds), ctypes.c_size_t(n_items), ctypes.c_size_t(max_terms), ctypes.byref(L), ctypes.byref(C))
    return L.value, C.value


def chunked_items(hs, n_simds, limit=8192):
    """the smallest n_items, off every multiple of 64 (hence of 128 and 256), at which CHUNKED_TERMS terms are cut into chunks of at least
    two terms and at least two chunks; None when there is none up to `limit`"""
    for n in range(65, limit + 1):
        if n % 64:
            L, C = chunks(hs, n_simds, n, CHUNKED_TERMS)
            if C >= 2 and L >= 2:
                return n
    return None


# ---------------------------------------------------------------------------------------------------- the replay
def naf(k):
    """{bit: +1 | -1} of the non-adjacent form of k >= 0"""
    out, b = {}, 0
    while k:
        if k & 1:
            d = 2 - (k & 3)
            out[b] = d
            k -= d
        k >>= 1
        b += 1
    return out


def signed_digits(word, flip):
    """the masks k_naf_masks writes for a scalar word, read with `flip`: {bit: +1 | -1}"""
    assert 0 <= word < TWO256
    k, sign = word % R, 1
    if k > HALF:
        k, sign = R - k, -1
    if flip:
        sign = -sign
    d = naf(k)
    assert all(b < 255 for b in d) and all(not (b + 1 in d) for b in d)
    return {b: sign * v for b, v in d.items()}


def top_bit(word):
    return max(signed_digits(word, False))


def replay(item, L, C, flip=False):
    """item: [(log of the base, scalar word)].  Returns (events, log of the sum), log 0 standing for infinity."""
    assert len(item) <= L * C
    events, parts = [], []
    for c in range(L):
        terms = [(log % R, signed_digits(word, flip)) for log, word in item[c * C:(c + 1) * C]]
        acc, started = None, False
        for bit in range(255, -1, -1):
            if started and acc is not None:
                acc = 2 * acc % R
            for log, dig in terms:
                if bit not in dig or log == 0:
                    continue
                e = dig[bit] * log % R
                if acc is None:
                    acc = e
                elif acc == e:
                    events.append((c, bit, "dbl"))
                    acc = 2 * e % R
                elif (acc + e) % R == 0:
                    events.append((c, bit, "cancel"))
                    acc = None
                else:
                    acc = (acc + e) % R
                started = True
        parts.append(acc)
    acc = parts[0]
    for c in range(1, L):
        e = parts[c]
        if e is None:
            continue
        if acc is None:
            acc = e
        elif acc == e:
            events.append((FINISH, c, "dbl"))
            acc = 2 * e % R
        elif (acc + e) % R == 0:
            events.append((FINISH, c, "cancel"))
            acc = None
        else:
            acc = (acc + e) % R
    return events, (0 if acc is None else acc)


def sum_log(item, flip=False):
    s = sum(log * (word % R) for log, word in item) % R
    return (R - s) % R if flip else s


def check(item, L, C, intended, flip=False):
    events, log = replay(item, L, C, flip)
    assert events == intended, (events, intended)
    assert log == sum_log(item, flip)
    return log


# ---------------------------------------------------------------------------------------------------- the kinds
ORDINARY = ("ordinary", "ordinary five")
INFINITE = ("twin-opposite alone", "opposite across chunks", "zero terms", "zero scalars")        # the whole sum is the point at infinity
KINDS = ("short", "ordinary", "twin", "ordinary five", "twin-opposite", "twin-opposite bases", "ordinary", "twin across chunks",
         "opposite across chunks", "ordinary five", "dbl mid-walk", "cancel mid-walk", "ordinary", "scalar edges a", "scalar edges b",
         "ordinary five", "twin-opposite alone", "zero terms", "ordinary", "zero scalars")         # the tiling order: ordinary neighbours
MID_S, MID_U = 100, 50
# the logs every ordinary base is drawn from (an item takes each at most once): the oracle computes a few dozen points for the whole module
POOL = [random.Random("msm pool %d" % i).randrange(1 << 200, R) for i in range(24)]
assert len({min(d, R - d) for d in POOL}) == len(POOL)


class Case:
    def __init__(self, kind, terms, events):
        self.kind, self.terms, self.events = kind, terms, events


def build(kind, max_terms, L, C, seed=""):
    """the one item of `kind` for a launch whose sums are cut into L chunks of C terms; the same for every tile of the kind"""
    rnd = random.Random("msm %s %d %d %d %s" % (kind, max_terms, L, C, seed))
    pool = rnd.sample(POOL, len(POOL))

    def base():                           # distinct within the item
        return pool.pop()

    def scalar():
        return rnd.randrange(1 << 200, R)

    def nothing(i):                       # a term that adds nothing: a zero scalar, or the point at infinity under a full-size scalar
        return (base(), 0) if i % 2 == 0 else (0, scalar())

    def padded(terms):                    # the special terms own their chunks; the rest of the item is ordinary
        terms = list(terms)
        while len(terms) % C:
            terms.append(nothing(len(terms)))
        return terms

    def filled(terms, upto=max_terms):
        terms = padded(terms)
        while len(terms) < upto:
            terms.append((base(), scalar()))
        assert len(terms) <= max_terms
        return terms

    in_lane = C >= 2
    d, k = base(), scalar()
    nz = sorted(signed_digits(k, False), reverse=True)
    if kind == "ordinary":
        return Case(kind, filled([]), [])
    if kind == "ordinary five":
        return Case(kind, [(base(), scalar()) for _ in range(5)], [])
    if kind == "short":                   # not a multiple of C (C >= 2), fewer than L chunks: a short last chunk and empty chunks behind it
        return Case(kind, [(base(), scalar()) for _ in range(3)], [])
    if kind == "twin":
        return Case(kind, filled([(d, k), (d, k)]), [(0, nz[0], "dbl")] if in_lane else [(FINISH, 1, "dbl")])
    if kind in ("twin-opposite", "twin-opposite bases", "twin-opposite alone"):
        pair = [(d, k), (R - d, k)] if kind == "twin-opposite bases" else [(d, k), (d, R - k)]
        events = [(0, b, "cancel") for b in nz] if in_lane else [(FINISH, 1, "cancel")]
        return Case(kind, pair if kind == "twin-opposite alone" else filled(pair), events)
    if kind in ("twin across chunks", "opposite across chunks"):
        first = padded([(d, k)])
        if kind == "twin across chunks":
            return Case(kind, filled(first + padded([(d, k)])), [(FINISH, 1, "dbl")])
        return Case(kind, first + [(d, R - k)], [(FINISH, 1, "cancel")])
    if kind == "dbl mid-walk":            # d 2^s after s doublings meets the base d 2^s at bit 0
        terms = [(d, 1 << MID_S), (d * (1 << MID_S) % R, 1)]
        return Case(kind, filled(terms), [(0, 0, "dbl")] if in_lane else [(FINISH, 1, "dbl")])
    if kind == "cancel mid-walk":         # ... meets its opposite at bit u: infinity, u doublings there, and the same term leaves it at bit 0
        terms = [(d, 1 << (MID_S + MID_U)), (R - d * (1 << MID_S) % R, (1 << MID_U) + 1), (base(), 1)]
        return Case(kind, filled(terms), [(0, MID_U, "cancel")] if in_lane else [])
    if kind == "scalar edges a":
        return Case(kind, [(0, scalar()), (base(), 0), (base(), 1), (base(), 2), (base(), R - 1), (base(), HALF)], [])
    if kind == "scalar edges b":
        big = rnd.randrange(1, TWO256 - 5 * R)
        return Case(kind, [(base(), HALF + 1), (base(), R), (base(), scalar() % (TWO256 - R) + R), (base(), big + 5 * R), (base(), TWO256 - 1)], [])
    if kind == "zero terms":
        return Case(kind, [], [])
    assert kind == "zero scalars"
    return Case(kind, [(base(), 0), (base(), R), (0, scalar()), (base(), 0)], [])


def cases(max_terms, L, C, seed=""):
    """{kind: Case}, every one checked against the replay for both orientations of the masks"""
    out = {}
    for kind in dict.fromkeys(KINDS):
        case = build(kind, max_terms, L, C, seed)
        assert len(case.terms) <= max_terms <= L * C
        for flip in (False, True):
            log = check(case.terms, L, C, case.events, flip)
            assert (log == 0) == (kind in INFINITE), kind
        out[kind] = case
    assert len(out["ordinary"].terms) == max_terms and len(out) <= 24
    return out


def layout(n_items):
    """the kind of every item: KINDS tiled, so that a degenerate item has ordinary neighbours in its wave; degenerate items on both sides
    of the first 64-lane edge and of the first edge of a G2 and of a G1 finish block; where there are three G1 finish blocks, the third
    (items 512 .. 767, two G2 blocks) is ordinary but for one infinite sum in each of its G2 halves; an infinite sum in the last, partly
    inactive block; item 0 is not the one with max_terms"""
    kinds = [KINDS[i % len(KINDS)] for i in range(n_items)]
    edges = {63: "twin-opposite", 64: "zero terms", 127: "twin", 128: "opposite across chunks", 255: "twin-opposite alone", 256: "dbl mid-walk"}
    for i, kind in edges.items():
        if i < n_items:
            kinds[i] = kind
    if n_items >= 3 * G1_FINISH_BLOCK:
        for i in range(2 * G1_FINISH_BLOCK, 3 * G1_FINISH_BLOCK):
            kinds[i] = ORDINARY[i % 2]
        kinds[2 * G1_FINISH_BLOCK + 88] = "opposite across chunks"
        kinds[2 * G1_FINISH_BLOCK + G2_FINISH_BLOCK + 41] = "zero scalars"
    kinds[n_items - 2] = "twin-opposite alone"
    assert n_items % 64 and kinds[0] == "short" and set(kinds) == set(KINDS)
    return kinds


def word_bytes(w):
    return int(w).to_bytes(32, "little")


# ---------------------------------------------------------------------------------------------------- the calls, on the logs
# Whatever a call adds around its sum is drawn from POOL too: pool(i) is a log, e(g1, g2)^pool(i) a member of Gt.
MU = POOL[7]                          # the Gt base of a term is e(g1, g2)^(log MU): equal G2 bases have equal Gt bases, infinity has the identity


def pool(i):
    return POOL[i % len(POOL)]


def jobs_item(case, index, with_pairs):
    """rhip_pairing_jobs: (pairs [(log p, scalar, log q)], log of s_q, log of lead, the exponent of e(g1, g2) in out)
    out = lead * FE( prod ML(k p, q) * ML(sum s d, s_q) )"""
    pairs = [(pool(index + 1), pool(index + 2), pool(index + 3)), (pool(index + 4), R - 3 - index, pool(index + 5))] if with_pairs else []
    q_s, lead = pool(index + 6), pool(index + 8)
    return pairs, q_s, lead, (lead + sum(p * k * q for p, k, q in pairs) + q_s * sum_log(case.terms)) % R


def aw11_item(case, index):
    """rhip_aw11_decrypt_batch (engine_jobs.hip, "decrypt (aw11/mod.rs ...)"): term j has the coefficient word c_j, the ciphertext row
    C1 = e(g1, g2)^a_j, C2 = g2 u_j, C3 = g2 t_j (t_j: the case's log) and the key attribute K_j = g1 kappa_j; H(gid) = g1 h, c_0 = e(g1, g2)^a0:
      out = c_0 prod C1_j^(-c_j)  *  FE( prod ML(c_j K_j, C2_j) * ML(-H, sum c_j C3_j) )
    Returns (rows [(a, u, t, kappa)], h, a0, exponent)."""
    rows = [(t * MU % R, pool(index + 2 * j + 1), t, pool(index + 2 * j + 2)) for j, (t, _w) in enumerate(case.terms)]
    h, a0 = pool(index + 9), pool(index + 11)
    c = [w % R for _t, w in case.terms]
    exponent = (a0 - sum(cj * a for cj, (a, _u, _t, _k) in zip(c, rows)) + sum(cj * k * u for cj, (_a, u, _t, k) in zip(c, rows))
                - h * sum_log(case.terms)) % R
    return rows, h, a0, exponent


def lsw_item(case, group_index, item_index):
    """rhip_lsw_decrypt_batch_one_sk: entry j of the group selects the key row with D1 = g1 d_j (the case's log), D2 = g2 delta(d_j), and the
    ciphertext attribute E_j = g1 eps_j; e1 = e(g1, g2)^x, e2 = g2 y:
      out = e1 * FE( prod ML(c_j E_j, D2_j) * ML(sum -c_j D1_j, e2) )
    Returns (eps per entry, x, y, exponent)."""
    eps = [pool(group_index + 3 * j + 1) for j in range(len(case.terms))]
    x, y = pool(item_index + 5), pool(item_index + 10)
    exponent = (x + sum((w % R) * e * lsw_d2(d) for (d, w), e in zip(case.terms, eps)) + y * sum_log(case.terms, flip=True)) % R
    return eps, x, y, exponent


def lsw_d2(d1_log):
    return (d1_log * POOL[3] + POOL[4]) % R          # the D2 of a key row as a function of its D1: never infinity for the logs in use
