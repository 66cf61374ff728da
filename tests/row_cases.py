"""Inputs that drive the fused row kernels (k_ghw11_enc_rows, k_ghw11_keygen_rows, k_ghw11_provision_rows, k_dnf_keygen_g1 / _g2) into the
exceptional cases of the mixed addition, and the proof -- in integers, without a GPU -- that each of them gets there.

Every base of a test world is a known multiple of one point, so a row is described by discrete logs alone.  `replay` restates what a row
kernel does to its Jacobian accumulator: 16-bit windows, low to high, one table entry added per non-zero digit, first scalar then second,
then (keygen) the key's own point.  On the logs an addition is exceptional when the running log is +entry (the doubling branch) or -entry
(the sum is infinity) mod R.  A case states the events it intends, as (walk, window, kind); `check_row` asserts that the replay meets exactly
those and no other, so a test cannot silently miss its branch.

tests/test_row_kernels_precheck.py runs these proofs on the CPU; tests/test_gpu_row_kernels_degenerate.py launches the same calls."""
import random

from oracle import bn254 as bn

R = bn.R
WINDOWS = 16                      # TBL16_WINDOWS (engine_internal.h)
ROWS_BLOCK = 256                  # RB_ROWS_BLOCK: k_ghw11_enc_rows, k_dnf_keygen_g1
G2_BLOCK = 128                    # the __launch_bounds__ of k_ghw11_keygen_rows, k_ghw11_provision_rows, k_dnf_keygen_g2
RELATIONS = (1, 5, 5 << 16)       # the base of the first walk is the base of the second times one of these


def digits(k):
    assert 0 <= k < R
    return [(k >> (16 * w)) & 0xffff for w in range(WINDOWS)]


def top_window(k):
    return max(w for w, d in enumerate(digits(k)) if d)


def low_window(k):
    return min(w for w, d in enumerate(digits(k)) if d)


def inv(x):
    return bn.fr_inv(x % R)


def replay(walks, tail=None):
    """walks: [(log of the table's base, canonical scalar)]; tail: the log of a point added after the last walk, None for none (or for the
    point at infinity, which the addition skips).  Returns (events, log of the result), the log 0 standing for infinity; an event is
    (walk index -- len(walks) for the tail --, window, "dbl" | "cancel")."""
    steps = [(i, w, base * (d << (16 * w)) % R) for i, (base, k) in enumerate(walks) for w, d in enumerate(digits(k)) if d]
    if tail is not None:
        steps.append((len(walks), 0, tail % R))
    acc, events = None, []
    for i, w, e in steps:
        assert e != 0
        if acc is None:
            acc = e
        elif acc == e:
            events.append((i, w, "dbl"))
            acc = 2 * e % R
        elif (acc + e) % R == 0:
            events.append((i, w, "cancel"))
            acc = None
        else:
            acc = (acc + e) % R
    return events, (0 if acc is None else acc)


def check_row(walks, tail, intended, want_log):
    events, log = replay(walks, tail)
    assert events == intended, (events, intended)
    assert log == want_log % R
    return log


# ---------------------------------------------------------------------------------------------------- k_ghw11_enc_rows
# C = g1_a * lam + g1 * k2 with g1_a = g1 * c and k2 = -H t mod R: walks [(c, lam), (1, k2)].  D = g1 * t.
ENC_KINDS = ("ordinary", "dbl w0", "dbl w1", "dbl top", "cancel last", "cancel mid", "t zero", "both zero")


def enc_case(kind, c, rnd, lam=None):
    """(lam, k2, intended events); a `lam` handed in is kept (rows of a flat OR share it) where the kind leaves it free"""
    assert lam is None or kind in ("ordinary", "cancel last", "t zero") or (kind, lam) == ("both zero", 0)
    if lam is None:
        lam = rnd.randrange(1, R)
    if kind == "ordinary":
        return lam, rnd.randrange(1, R), []
    if kind.startswith("dbl"):
        w = {"dbl w0": 0, "dbl w1": 1, "dbl top": WINDOWS - 1}[kind]
        k2 = rnd.randrange(1, 0x3000) << (16 * w)          # one digit; 0x3000 2^240 < R
        return k2 * inv(c) % R, k2, [(1, w, "dbl")]         # c lam = k2: the accumulator is the entry
    if kind == "cancel last":
        k2 = (R - c * lam) % R
        return lam, k2, [(1, top_window(k2), "cancel")]
    if kind == "cancel mid":
        w = 3
        m = rnd.randrange(1 << (16 * w), 1 << (16 * (w + 1)))                 # digits 0..w, the one at w not zero
        hi = rnd.randrange(1, R >> (16 * (w + 1)))
        return (R - m) * inv(c) % R, m + (hi << (16 * (w + 1))), [(1, w, "cancel")]      # infinity after window w, back at the next digit
    if kind == "t zero":
        return lam, 0, []
    assert kind == "both zero"
    return 0, 0, []


LEAF, OR3, AND2 = 0, 1, 2
ENC_TREES = [("leaf", "A"), ("or", [("leaf", "B"), ("leaf", "C"), ("leaf", "D")]), ("and", [("leaf", "E"), ("leaf", "F")])]
ENC_LEAF_NAMES = "ABCDEF"


class EncCall:
    """one call of rhip_ghw11_encrypt_batch under the relation g1_a = g1 * c; items are added policy by policy, rows in leaf order"""

    def __init__(self, c, seed):
        self.c, self.rnd = c, random.Random("enc %d %s" % (c, seed))
        hrnd = random.Random("leaf hashes")
        self.H = {n: hrnd.randrange(1, R) for n in ENC_LEAF_NAMES}
        self.first_leaf = {LEAF: 0, OR3: 1, AND2: 4}
        self.items = []               # (policy, secret, [coefficient draws])
        self.rows = []                # dict(kind, lam, k2, t, events, c_log, d_log)

    def _row(self, kind, leaf_name, lam=None):
        lam, k2, events = enc_case(kind, self.c, self.rnd, lam)
        t = (R - k2) * inv(self.H[leaf_name]) % R
        assert (R - self.H[leaf_name] * t) % R == k2
        self.rows.append(dict(kind=kind, lam=lam, k2=k2, t=t, events=events, c_log=(self.c * lam + k2) % R, d_log=t))
        return lam

    def leaf(self, kind="ordinary"):
        self.items.append((LEAF, self._row(kind, "A"), []))
        return self

    def or3(self, kinds):
        """three rows with one lam = secret: at most one kind may fix it, and that one comes first in `kinds`"""
        lam = self._row(kinds[0], "B")
        for kind, name in zip(kinds[1:], "CD"):
            self._row(kind, name, lam)
        self.items.append((OR3, lam, []))
        return self

    def and2(self, kind, x):
        """the kind's row is child x (1 or 2) of the AND; its lam = secret + a x through the Horner step, the other child's row is whatever
        that secret and a give"""
        a = self.rnd.randrange(1, R)
        if x == 2:
            self.rows.append(None)
        lam = self._row(kind, "EF"[x - 1])
        secret = (lam - a * x) % R
        ox = 3 - x
        other = dict(kind="ordinary", lam=(secret + a * ox) % R, k2=self.rnd.randrange(1, R), events=[])
        other["t"] = (R - other["k2"]) * inv(self.H["EF"[ox - 1]]) % R
        other["c_log"], other["d_log"] = (self.c * other["lam"] + other["k2"]) % R, other["t"]
        if x == 2:
            self.rows[-2] = other
        else:
            self.rows.append(other)
        self.items.append((AND2, secret, [a]))
        return self

    def shares(self):
        """lam of every row from the items' secrets and draws, the way gen_shares_policy hands them down"""
        out = []
        for pol, secret, coef in self.items:
            out += [secret] if pol == LEAF else [secret] * 3 if pol == OR3 else [(secret + coef[0] * x) % R for x in (1, 2)]
        return out

    def precheck(self):
        assert self.shares() == [r["lam"] for r in self.rows]
        for r in self.rows:
            check_row([(self.c, r["lam"]), (1, r["k2"])], None, r["events"], r["c_log"])
            assert (r["c_log"] == 0) == (r["kind"] in ("cancel last", "both zero"))
            assert (r["d_log"] == 0) == (r["kind"] in ("t zero", "both zero"))
        return self

    def lanes(self, *kinds):
        return [i for i, r in enumerate(self.rows) if r["kind"] in kinds]


def enc_every_case(c):
    """a small call with every kind on a one-leaf policy, in a flat OR and under a two-leaf AND (both children)"""
    call = EncCall(c, "every case")
    for kind in ENC_KINDS:
        call.leaf(kind)
    call.or3(["dbl w1", "ordinary", "t zero"]).or3(["cancel mid", "cancel last", "ordinary"]).or3(["both zero"] * 3)
    call.and2("dbl w0", 1).and2("dbl top", 2).and2("cancel last", 1).and2("cancel mid", 2).and2("both zero", 2)
    return call.precheck()


ENC_257_LANES = {0: "dbl w0", 63: "cancel last", 64: "both zero", 128: "cancel mid", 200: "t zero", 256: "cancel last"}


def enc_257(c=1):
    """one whole block and one row: degenerate rows at lanes 0, 63, 64, 255 (second child of an AND) and 256, and some between; a flat OR
    lies across lanes 60..62"""
    call = EncCall(c, "257")
    while len(call.rows) < ROWS_BLOCK + 1:
        at = len(call.rows)
        if at == 60:
            call.or3(["dbl w1", "ordinary", "ordinary"])
        elif at == 254:
            call.and2("dbl top", 2)
        else:
            call.leaf(ENC_257_LANES.get(at, "ordinary"))
    assert len(call.rows) == ROWS_BLOCK + 1
    assert call.lanes(*ENC_KINDS[1:]) == [0, 60, 63, 64, 128, 200, 255, 256]
    return call.precheck()


def enc_one_row(c, kind):
    return EncCall(c, "one row").leaf(kind).precheck()


# ---------------------------------------------------------------------------------------------------- GHW11 keygen / provision
# g2_a = g2, g2_alpha = g2 * c.  keygen row 1: K = g2_a * r + g2_alpha -- walks [(1, r)], tail c.  provision row 1, with u = 1 / z and
# v = r / z: K_z = g2_alpha * u + g2_a * v -- walks [(c, u), (1, v)].
KEY_KINDS = ("ordinary", "dbl", "cancel", "r zero", "dbl z one")


def key_case(kind, c, rnd):
    """(r, z, events of keygen's row 1, events of provision's row 1)"""
    z = rnd.randrange(2, R)
    if kind == "ordinary":
        return rnd.randrange(1, R), z, [], []
    if kind == "dbl":                        # keygen doubles; provision's second walk starts from g2 (c u) and is ordinary
        return c, z, [(1, 0, "dbl")], []
    if kind == "dbl z one":                  # u = 1, v = c: the second walk's first digit meets its own entry
        return c, 1, [(1, 0, "dbl")], [(1, low_window(c), "dbl")]
    if kind == "cancel":                     # c + r = 0 and c u + v = 0
        r = R - c
        return r, z, [(1, 0, "cancel")], [(1, top_window(r * inv(z) % R), "cancel")]
    assert kind == "r zero"
    return 0, z, [], []


class KeyCall:
    """one call of rhip_ghw11_keygen_batch / rhip_ghw11_provision_batch: items of counts[i] attributes, item i of kind kinds.get(i)"""

    def __init__(self, c, counts, kinds, seed):
        rnd = random.Random("keys %d %s" % (c, seed))
        self.c, self.counts = c, counts
        self.hashes, self.hash_off, self.row_off = [], [], [0]
        for n in counts:
            self.hash_off.append(len(self.hashes))
            self.hashes += [rnd.randrange(1, R) for _ in range(n)]
            self.row_off.append(self.row_off[-1] + 2 + n)
        self.kind = [kinds.get(i, "ordinary") for i in range(len(counts))]
        self.r, self.z, self.ev_sk, self.ev_tk = [], [], [], []
        for kind in self.kind:
            r, z, a, b = key_case(kind, c, rnd)
            self.r.append(r), self.z.append(z), self.ev_sk.append(a), self.ev_tk.append(b)

    def sk_logs(self):
        out = []
        for i, n in enumerate(self.counts):
            r = self.r[i]
            out += [r, (r + self.c) % R] + [self.hashes[self.hash_off[i] + y] * r % R for y in range(n)]
        return out

    def tk_logs(self):
        out = []
        for i, n in enumerate(self.counts):
            u = inv(self.z[i])
            v = self.r[i] * u % R
            out += [v, (self.c * u + v) % R] + [self.hashes[self.hash_off[i] + y] * v % R for y in range(n)]
        return out

    def degenerate_rows(self):
        """rows whose expected value is taken from one exact oracle product"""
        return [self.row_off[i] + 1 for i, k in enumerate(self.kind) if k != "ordinary"]

    def precheck(self):
        sk, tk = self.sk_logs(), self.tk_logs()
        for i, kind in enumerate(self.kind):
            k_row = self.row_off[i] + 1
            check_row([(1, self.r[i])], self.c, self.ev_sk[i], sk[k_row])
            u = inv(self.z[i])
            check_row([(self.c, u), (1, self.r[i] * u % R)], None, self.ev_tk[i], tk[k_row])
            assert (sk[k_row] == 0) == (tk[k_row] == 0) == (kind == "cancel")
            rows = [t for t in range(self.row_off[i], self.row_off[i + 1]) if t != k_row]
            assert all((sk[t] == 0) == (tk[t] == 0) == (kind == "r zero") for t in rows)
        return self


def key_small(c):
    counts = [1, 3, 2, 1, 4, 1, 2, 1, 3, 1, 2, 1]
    return KeyCall(c, counts, {1: "dbl", 3: "cancel", 4: "dbl z one", 6: "r zero", 8: "cancel", 11: "dbl z one"}, "small").precheck()


def key_135(c=1):
    """45 one-attribute items, 135 rows: K of item 21 on lane 64, of item 42 on lane 127 (the last of the whole block), of item 43 on lane 130"""
    call = KeyCall(c, [1] * 45, {0: "dbl z one", 21: "cancel", 42: "dbl", 43: "cancel", 44: "dbl z one"}, "135").precheck()
    assert [t % G2_BLOCK for t in call.degenerate_rows()] == [1, 64, 127, 2, 5] and call.row_off[-1] == G2_BLOCK + 7
    return call


def key_r_zero_130(c=1):
    """one item of 130 attributes with r = 0: of the 128 lanes of the first block only K is finite"""
    call = KeyCall(c, [130], {0: "r zero"}, "r zero").precheck()
    assert call.row_off[-1] > G2_BLOCK
    return call


# ---------------------------------------------------------------------------------------------------- BDABE / MKE08 user keys
# a1 = p1 * c1, a2 = p2 * c2.  Even rows: sk = p * r + a -- walks [(1, r)], tail c.  Odd rows: pk = g * r.
DNF_RELATIONS = ((1, 1), (5, 7), (5 << 16, 3 << 16))
DNF_KINDS = ("ordinary", "dbl g1", "cancel g1", "dbl g2", "cancel g2", "r zero")


class DnfCall:
    """one call of rhip_dnf_keygen_batch; c1 / c2 None: a1 / a2 is the point at infinity"""

    def __init__(self, c1, c2, n_items, kinds, seed):
        rnd = random.Random("dnf %s %s %s" % (c1, c2, seed))
        self.c1, self.c2 = c1, c2
        self.kind = [kinds.get(i, "ordinary") for i in range(n_items)]
        of = {"dbl g1": lambda: c1, "cancel g1": lambda: R - c1, "dbl g2": lambda: c2, "cancel g2": lambda: R - c2, "r zero": lambda: 0,
              "ordinary": lambda: rnd.randrange(1, R)}
        self.r = [of[k]() % R for k in self.kind]

    def sk_logs(self, c):
        return [(r + (c or 0)) % R for r in self.r]

    def events(self, kind, c, mine, r):
        """the events of one group's sk row: those of its own kinds, and of the other group's where the two relations coincide"""
        if c is None or r == 0:
            return []
        if kind in ("dbl " + mine, "cancel " + mine):
            return [(1, 0, kind.split()[0])]
        if kind != "ordinary":
            return [(1, 0, "dbl")] if r == c else [(1, 0, "cancel")] if r == R - c else []
        return []

    def precheck(self):
        for c, mine in ((self.c1, "g1"), (self.c2, "g2")):
            logs = self.sk_logs(c)
            for i, kind in enumerate(self.kind):
                ev = self.events(kind, c, mine, self.r[i])
                check_row([(1, self.r[i])], c, ev, logs[i])
                assert (logs[i] == 0) == bool(ev == [(1, 0, "cancel")] or (c is None and self.r[i] == 0))
                if kind in ("dbl " + mine, "cancel " + mine):
                    assert ev
        return self

    def degenerate_items(self):
        return [i for i, k in enumerate(self.kind) if k != "ordinary"]


def dnf_small(c1, c2):
    return DnfCall(c1, c2, 9, {0: "dbl g1", 2: "cancel g1", 3: "dbl g2", 5: "cancel g2", 6: "r zero", 8: "dbl g2"}, "small").precheck()


def dnf_129(c1, c2):
    """258 rows per group: G1 one block of 256 and two rows, G2 two blocks of 128 and two rows; degenerate items on both sides of every edge"""
    kinds = {0: "dbl g1", 1: "dbl g2", 31: "cancel g1", 32: "cancel g2", 63: "dbl g2", 64: "cancel g1", 100: "r zero", 127: "cancel g2",
             128: "dbl g1"}
    call = DnfCall(c1, c2, 129, kinds, "129").precheck()
    assert 2 * 129 == ROWS_BLOCK + 2 == 2 * G2_BLOCK + 2
    return call


def dnf_one_item(c1, c2, kind):
    return DnfCall(c1, c2, 1, {0: kind}, "one").precheck()


def dnf_a_infinity():
    return DnfCall(None, None, 5, {1: "r zero"}, "a infinity").precheck()


# ---------------------------------------------------------------------------------------------------- raw scalar words
TWO256 = 1 << 256


def raw_words(rnd, n):
    """n pairs (256-bit word, the same scalar below R): k + R, k + 5 R, R itself and 2^256 - 1 in turn"""
    out = []
    for i in range(n):
        if i % 4 == 0:
            k = rnd.randrange(1, R)
            out.append((k + R, k))
        elif i % 4 == 1:
            k = rnd.randrange(1, TWO256 - 5 * R)
            out.append((k + 5 * R, k))
        elif i % 4 == 2:
            out.append((R, 0))
        else:
            out.append((TWO256 - 1, (TWO256 - 1) % R))
    assert all(R <= w < TWO256 and w % R == k for w, k in out)
    return out


def word_bytes(w):
    return int(w).to_bytes(32, "little")
