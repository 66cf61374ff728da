"""TEST INFRASTRUCTURE: the rows that drive rhip_aw11_encrypt_batch (k_aw11_enc_scalars, k_aw11_enc_c1, k_aw11_enc_c3 and the c2 table call) to the
edges of its window walks in every form the per-attribute tables take, the expected bytes of every row, and the integer models that
tests/test_aw11_rows_precheck.py uses to prove -- without a GPU -- that each row is what it claims.

The world is known by its discrete logs: g1 = G1_GEN * a, g2 = G2_GEN * b, E = e(g1, g2), egg_alpha_x = E^alpha_x, g2_y_x = g2 * y_x.  A row is
then four logs:   c0 = msg * E^s    c1 = E^(lambda + alpha_x r)    c2 = g2 * r    c3 = g2 * (y_x r + omega)
and the expected bytes are sums over two 8-bit window tables of E and g2 that the oracle's own multiplication and addition built (class C's
degenerate rows: an exact oracle product).  lambda and omega are this module's own Shamir shares in Python integers.

Row classes (`cls` of a row):
  A  r on the walk edges (tests/walk_scalars.py) under single-leaf policies (lambda = s, omega = 0)
  B  the start of the Gt product: lambda = 0 with a first signed digit of r that is negative / exactly half, lambda and r at 0, 1, R - 1
  C  two bases on one Jacobian accumulator (two-leaf ANDs: lambda = s + a1 x, omega = b1 x): the sum finished at infinity, the doubling branch,
     the accumulator at infinity in mid-walk
  D  raw, non-canonical `rand` words
  E  placement: the rows of a flat OR, an item across a 128-row block boundary
tests/test_gpu_aw11_enc_rows.py launches the list."""
import functools
import random

from oracle import bn254 as bn
from rabe_amd import hostprep as hp
from tests import walk_scalars as ws

R = bn.R
N_ATTRS = 3
C1_BLOCK, C3_BLOCK = 64, 128                      # the __launch_bounds__ of k_aw11_enc_c1, k_aw11_enc_c3
SIGNED_WIDTHS = tuple(range(9, 15))               # RABE_AW11_ATTR_BITS that build signed tables
FORMS = (0, 1) + SIGNED_WIDTHS                    # rhip_aw11_pk_table_form: plain 8-bit, 16-bit per attribute, signed w
HEADS = (1, 63, 64, 65, 127, 128, 129, 257)       # row counts of the leading sub-lists the GPU test also calls with
INF = bytes(128)
GT_ONE = bn.gt_to_le(bn.FP12_ONE)
DBL_LOG = 5 << 32                                 # class C: the log the attribute walk leaves on the accumulator (one digit in both cuts of g2)


# ------------------------------------------------------------------------------------------------ integer models of bn254/table_walk.h
def scalar_bits(k, b, w):
    """bits b .. b + w - 1 of the 256-bit word k; bits past 255 read as zero"""
    assert 0 <= k < 1 << 256 and w <= 32
    return (k >> b) & ((1 << w) - 1)


def digits8(k):
    return [scalar_bits(k, 8 * i, 8) for i in range(32)]


def digits16(k):
    return [scalar_bits(k, 16 * i, 16) for i in range(16)]


def sgn_windows(w):
    return (255 + w - 1) // w


def signed_digits(k, w):
    """SignedRecoder over sgn_windows(w) windows: a window's bits plus the carry of the window below give raw in 0 .. 2^w; above half it stands
    for raw - 2^w and carries one into the next window.  Returns the digits d_i, -2^(w-1) < d_i <= 2^(w-1), and the carry left at the end."""
    half, carry, out = 1 << (w - 1), 0, []
    for i in range(sgn_windows(w)):
        raw = scalar_bits(k, w * i, w) + carry
        carry = 1 if raw > half else 0
        out.append(raw - (carry << w))
    return out, carry


def signed_table_scalar(w, i, d):
    """the multiplier k_attr_tables_{gt,g2}_signed hands to the 8-bit walk for entry (i, d - 1): d << (w i mod 32) as a 64-bit value whose low
    word lands in word (w i) / 32 and whose high word in the next one while there is a next one -- d 2^(w i) cut at 256 bits"""
    b = w * i
    word, sh = b >> 5, b & 31
    lo = (d << sh) & ((1 << 64) - 1)
    m = (lo & 0xffffffff) << (32 * word)
    if word + 1 <= 7:
        m |= (lo >> 32) << (32 * (word + 1))
    return m


def top_window_bound(w):
    """the largest magnitude the top window of a scalar below r can take, the carry of the window below included"""
    return (R >> (w * (sgn_windows(w) - 1))) + 1


def attr_steps(form, k):
    """(window, signed digit, weight of the window) of every table entry the attribute walk of a form takes for the canonical scalar k"""
    if form == 0:
        return [(i, d, 8 * i) for i, d in enumerate(digits8(k)) if d]
    if form == 1:
        return [(i, d, 16 * i) for i, d in enumerate(digits16(k)) if d]
    ds, carry = signed_digits(k, form)
    assert carry == 0
    return [(i, d, form * i) for i, d in enumerate(ds) if d]


def g2_cut(form):
    """the window width of the g2 table k_aw11_enc_c3 walks omega over: the 8-bit table under the plain form, the 16-bit one otherwise"""
    return 8 if form == 0 else 16


def g2_steps(form, k):
    return [(i, d, 8 * i) for i, d in enumerate(digits8(k)) if d] if form == 0 else [(i, d, 16 * i) for i, d in enumerate(digits16(k)) if d]


def replay_c3(form, y, r, omega):
    """what k_aw11_enc_c3 does to its accumulator, on logs mod R: the attribute walk over r (base log y), then the g2 walk over omega (base log 1),
    windows low to high.  Returns (events, final log): an event is (walk, window, kind) with kind "dbl" (accumulator = addend), "cancel"
    (accumulator = -addend, the sum is infinity); the log 0 stands for infinity."""
    steps = [(0, i, y * d * (1 << sh) % R) for i, d, sh in attr_steps(form, r % R)] + [(1, i, d << sh) for i, d, sh in g2_steps(form, omega % R)]
    acc, events = None, []
    for walk, i, e in steps:
        assert e % R
        e %= R
        if acc is None:
            acc = e
        elif acc == e:
            events.append((walk, i, "dbl"))
            acc = 2 * e % R
        elif (acc + e) % R == 0:
            events.append((walk, i, "cancel"))
            acc = None
        else:
            acc = (acc + e) % R
    return events, (0 if acc is None else acc)


def first_take_gt(form, lam, r):
    """the first entry k_aw11_enc_c1 takes (facc_set, the product not started): ("E", +1) when lambda has a digit, else ("attr", sign of the first
    non-zero digit of r), None when both are zero"""
    if lam % R:
        return ("E", 1)
    steps = attr_steps(form, r % R)
    return ("attr", 1 if steps[0][1] > 0 else -1) if steps else None


# ------------------------------------------------------------------------------------------------ shares
def shamir(tree, secret, draws):
    """the share of every leaf, DFS order: a gate with threshold k draws a_1 .. a_(k-1) when it is entered (before its children) and hands child x
    (1-based) secret + a_1 x + ... + a_(k-1) x^(k-1); an OR hands every child the secret and draws nothing"""
    if tree[0] == "leaf":
        return [secret % R]
    ch, out = tree[1], []
    if tree[0] == "or":
        for c in ch:
            out += shamir(c, secret, draws)
        return out
    a = [next(draws) for _ in range(len(ch) - 1)]
    for x, c in enumerate(ch, 1):
        out += shamir(c, (secret + sum(aj * pow(x, j, R) for j, aj in enumerate(a, 1))) % R, draws)
    return out


def n_draws(tree):
    if tree[0] == "leaf":
        return 0
    return (len(tree[1]) - 1 if tree[0] == "and" else 0) + sum(n_draws(c) for c in tree[1])


# ------------------------------------------------------------------------------------------------ reference arithmetic
class Windows:
    """k * base (group written additively) as a sum of 8-bit table entries (d 256^i) * base, every entry and every sum by the oracle's own
    operation: bn.g2_add for G2, bn.gt_mul for Gt.  None is the neutral element."""

    def __init__(self, base, op):
        self.rows = []
        add = lambda p, q: q if p is None else op(p, q)
        for _ in range(32):
            row, acc = [None], None
            for _d in range(1, 256):
                acc = add(acc, base)
                row.append(acc)
            self.rows.append(row)
            base = add(row[-1], base)
        self.add = add

    def mul(self, k):
        k %= R
        acc = None
        for i, row in enumerate(self.rows):
            d = (k >> (8 * i)) & 255
            if d:
                acc = self.add(acc, row[d])
        return acc


def g2_le(pt):
    return INF if pt is None else bn.g2_to_le(pt)


def gt_le(x):
    return GT_ONE if x is None else bn.gt_to_le(x)


# ------------------------------------------------------------------------------------------------ the world and its case list
LEAF = [("leaf", "x%d" % a) for a in range(N_ATTRS)]
AND_PAIRS = [(0, 0), (1, 1), (2, 2), (0, 2), (2, 1)]
TREES = LEAF + [("and", [LEAF[a], LEAF[b]]) for a, b in AND_PAIRS] + [("or", list(LEAF))]
OR3 = len(TREES) - 1


def and_tree(a, b):
    return N_ATTRS + AND_PAIRS.index((a, b))


class Cases:
    def __init__(self):
        rnd = random.Random("aw11 rows world")
        big = lambda: rnd.randrange(1 << 200, R)
        self.a, self.b = big(), big()
        self.alpha = [big() for _ in range(N_ATTRS)]
        self.y = [big() for _ in range(N_ATTRS)]
        self.g1 = bn.g1_mul(bn.G1_GEN, self.a)
        self.g2 = bn.g2_mul(bn.G2_GEN, self.b)
        self.E = bn.pairing(self.g1, self.g2)
        self.t_g2 = Windows(self.g2, bn.g2_add)
        self.t_E = Windows(self.E, bn.gt_mul)
        self.egg_alpha = [self.t_E.mul(x) for x in self.alpha]
        self.g2_y = [self.t_g2.mul(x) for x in self.y]
        self.tt = hp.TreeTables(TREES)
        self.leaf_attr = [int(nm[1:]) for f in self.tt.flat for nm in f["names"]]
        self.rnd = random.Random("aw11 rows")
        self.items = []            # dict(tree, s, m, coefs, row0)
        self.rows = []             # dict(cls, name, item, attr, rand (the raw word), lam, omg, exact)
        self._want, self._msg = {}, {}
        self._build()

    # ---- items
    def _item(self, tree, s, coefs, rows):
        """rows: (cls, name, raw rand word) per leaf, or (cls, name, word, True) for a row whose c3 is taken from an exact oracle product"""
        assert len(coefs) == 2 * n_draws(TREES[tree]) and len(rows) == self.tt.n_leaves(tree)
        half = len(coefs) // 2
        lam = shamir(TREES[tree], s, iter(coefs[:half]))
        omg = shamir(TREES[tree], 0, iter(coefs[half:]))
        first = self.tt.first_leaf[tree]
        self.items.append(dict(tree=tree, s=s, m=self.rnd.randrange(1, R), coefs=list(coefs), row0=len(self.rows)))
        for x, row in enumerate(rows):
            self.rows.append(dict(cls=row[0], name=row[1], item=len(self.items) - 1, attr=self.leaf_attr[first + x], rand=row[2], lam=lam[x],
                                  omg=omg[x], exact=len(row) > 3))

    def _single(self, cls, name, attr, lam, word):
        self._item(attr, lam, [], [(cls, name, word)])

    def _class_a(self):
        out, k = [], 0
        lists = [("common", ws.common())] + [("edge(%d)" % w, ws.edge(w)) for w in (8, 9, 10, 11, 12, 13, 14, 16)]
        lists += [("dense(%d)" % w, ws.dense(w)) for w in (9, 10, 14)]
        for name, scalars in lists:
            for j, r in enumerate(scalars):
                out.append(("A", "%s[%d]" % (name, j), k % N_ATTRS, self.rnd.randrange(1, R), r))
                k += 1
        return out

    def _class_b(self):
        pairs = [("lam 0, r 0", 0, 0), ("lam 0, r 1", 0, 1)]
        pairs += [("lam 0, r half+1 of %d" % w, 0, (1 << (w - 1)) + 1) for w in SIGNED_WIDTHS]
        pairs += [("lam 0, r half of %d" % w, 0, 1 << (w - 1)) for w in SIGNED_WIDTHS]
        pairs += [("lam 1, r 0", 1, 0), ("lam R-1, r 0", R - 1, 0), ("lam R-1, r R-1", R - 1, R - 1)]
        pairs += [("lam edge(16)[%d]" % j, lam, self.rnd.randrange(1, R)) for j, lam in enumerate(ws.edge(16))]
        return [("B", name, k % N_ATTRS, lam, r) for k, (name, lam, r) in enumerate(pairs)]

    def _class_d(self):
        out = []
        for a in range(N_ATTRS):
            k = self.rnd.randrange(1, (1 << 256) - R)
            for name, word in (("k + R", k + R), ("7 + 5 R", 7 + 5 * R), ("2^256 - 1", (1 << 256) - 1), ("R", R)):
                assert R <= word < 1 << 256
                out.append(("D", name, a, self.rnd.randrange(1, R), word))
        return out

    def _class_c(self, kind, a):
        """one two-leaf AND over attribute a twice: omega = b1, 2 b1"""
        y, yinv, rnd = self.y[a], bn.fr_inv(self.y[a]), self.rnd
        s, a1 = rnd.randrange(1, R), rnd.randrange(1, R)
        if kind in ("inf row 1", "inf row 2"):
            r = rnd.randrange(1, R)
            x = 1 if kind == "inf row 1" else 2
            b1 = (R - y * r) * bn.fr_inv(x) % R
            rows = [("C", "%s: %s" % (kind, "infinity" if i == x else "ordinary"), r, True) for i in (1, 2)]
        else:
            sign = 1 if kind == "doubling" else R - 1
            b1 = DBL_LOG + (rnd.randrange(1, 1 << 200) << 48)
            rows = [("C", "%s x%d" % (kind, i), sign * yinv * (i * DBL_LOG) % R, True) for i in (1, 2)]
        self._item(and_tree(a, a), s, [a1, b1], rows)

    def _build(self):
        rnd = self.rnd
        A, B, D = self._class_a(), self._class_b(), self._class_d()
        for row in B + D + A[:16]:
            self._single(*row)
        assert len(self.rows) == 66
        for a in range(N_ATTRS):
            for kind in ("inf row 1", "doubling", "opposite"):
                self._class_c(kind, a)
        word = lambda: rnd.randrange(1, R)
        self._item(OR3, word(), [], [("E", "OR row %d" % x, word()) for x in range(3)])
        fill = 2 * C3_BLOCK - 1 - len(self.rows)
        for row in A[16:16 + fill]:
            self._single(*row)
        assert len(self.rows) == 2 * C3_BLOCK - 1
        self._item(and_tree(0, 2), word(), [word(), word()], [("E", "AND across rows 255 | 256, x%d" % x, word()) for x in (1, 2)])
        for row in A[16 + fill:]:
            self._single(*row)
        self._item(and_tree(2, 1), word(), [word(), word()], [("E", "ordinary AND x%d" % x, word()) for x in (1, 2)])
        self._class_c("inf row 2", N_ATTRS - 1)                       # the last row of the call finishes at infinity
        self.row_off = [it["row0"] for it in self.items] + [len(self.rows)]
        assert all(h in self.row_off for h in HEADS)

    # ---- the call's arrays
    def call_arrays(self, n_items=None):
        """the host-side arrays of rhip_aw11_encrypt_batch over the first n_items items (all of them by default)"""
        items = self.items[:len(self.items) if n_items is None else n_items]
        rows = self.rows[:self.row_off[len(items)]]
        coef_off = [0]
        for it in items:
            coef_off.append(coef_off[-1] + len(it["coefs"]))
        return dict(n_items=len(items), total_rows=len(rows), row_off=self.row_off[:len(items) + 1],
                    tree_leaf=[self.tt.first_leaf[it["tree"]] for it in items], tree_gate=[self.tt.first_gate[it["tree"]] for it in items],
                    n_coef=[len(it["coefs"]) // 2 for it in items], s=[it["s"] for it in items], coefs=[c for it in items for c in it["coefs"]],
                    coef_off=coef_off[:-1], rand=[r["rand"] for r in rows], msg=[self.msg(i) for i in range(len(items))])

    def msg(self, i):
        if i not in self._msg:
            self._msg[i] = gt_le(self.t_E.mul(self.items[i]["m"]))
        return self._msg[i]

    def items_for_rows(self, n_rows):
        return self.row_off.index(n_rows)

    # ---- expected bytes
    def want_c0(self, i):
        it = self.items[i]
        return gt_le(self.t_E.mul(it["m"] + it["s"]))

    def row_logs(self, t):
        """(log of c1 over E, log of c2 over g2, log of c3 over g2) of row t"""
        row = self.rows[t]
        r = row["rand"] % R
        return (row["lam"] + self.alpha[row["attr"]] * r) % R, r, (self.y[row["attr"]] * r + row["omg"]) % R

    def want_row(self, t):
        """(c1, c2, c3) of row t"""
        if t not in self._want:
            l1, l2, l3 = self.row_logs(t)
            if self.rows[t]["exact"]:
                c3 = g2_le(bn.g2_mul(self.g2, l3) if l3 else None)
            else:
                c3 = g2_le(self.t_g2.mul(l3))
            self._want[t] = (gt_le(self.t_E.mul(l1)), g2_le(self.t_g2.mul(l2)), c3)
        return self._want[t]

    def label(self, t):
        row = self.rows[t]
        return "row %d [%s] %s (attribute %d)" % (t, row["cls"], row["name"], row["attr"])


@functools.lru_cache(maxsize=None)
def cases():
    return Cases()
