"""The integer proofs of tests/aw11_row_cases.py, on the CPU: the rows that tests/test_gpu_aw11_enc_rows.py launches are built here and shown to be
what their class claims -- the signed digits at half and past it, the carry through every window, the first take of the Gt product with a
negative digit, the doubling / cancellation of the two-base sum at the stated window in EVERY table form -- and the argument that makes the
256-bit cut of the signed tables sound is checked: a scalar below r never selects an entry of the top window that the cut changed."""
import random

import pytest

from oracle import bn254 as bn
from tests import aw11_row_cases as ac
from tests import walk_scalars as ws

R = ac.R


@pytest.fixture(scope="module")
def cs():
    return ac.cases()


def rows_of(cs, cls):
    return [(t, r) for t, r in enumerate(cs.rows) if r["cls"] == cls]


# ------------------------------------------------------------------------------------------------ the models
@pytest.mark.parametrize("w", ac.SIGNED_WIDTHS)
def test_signed_digits_model(w):
    assert ws.windows(w) == ac.sgn_windows(w) and ac.sgn_windows(w) * w >= 255
    half, n = 1 << (w - 1), ac.sgn_windows(w)
    rnd = random.Random(w)
    for k in [0, 1, R - 1, R - 2, half, half + 1, (1 << 254) - 1 - ((1 << 254) - 1) // R * R] + [rnd.randrange(R) for _ in range(300)]:
        ds, carry = ac.signed_digits(k, w)
        assert carry == 0 and len(ds) == n                                       # the last carry lands in a window
        assert all(-half < d <= half for d in ds)
        assert sum(d << (w * i) for i, d in enumerate(ds)) == k
    assert ac.signed_digits(half, w)[0][:2] == [half, 0]                         # exactly half stays positive
    assert ac.signed_digits(half + 1, w)[0][:2] == [-(half - 1), 1]              # one more turns negative with a carry


@pytest.mark.parametrize("w", ac.SIGNED_WIDTHS)
def test_a_scalar_below_r_never_selects_a_truncated_entry_of_the_top_window(w):
    """k_attr_tables_{gt,g2}_signed shift d into two 32-bit words and drop what passes bit 255: entry (top, d - 1) is (d 2^(w (n-1))) * base only
    while d 2^(w (n-1)) < 2^256.  The top window of a scalar below r holds at most r >> w (n-1), the carry adds one, and that stays at or below
    half (no carry leaves the window): the bound (r >> w (n-1)) + 1 times 2^(w (n-1)) is below 2^256."""
    n, half = ac.sgn_windows(w), 1 << (w - 1)
    b = w * (n - 1)
    bound = ac.top_window_bound(w)
    assert bound <= half and bound << b < 1 << 256
    for d in range(1, bound + 1):
        assert ac.signed_table_scalar(w, n - 1, d) == d << b
    assert any(ac.signed_table_scalar(w, n - 1, d) != d << b for d in range(bound + 1, half + 1))        # the cut is real: entries past the bound differ
    for i in range(n - 1):                                                      # no entry below the top window is cut
        for d in (1, half - 1, half):
            assert ac.signed_table_scalar(w, i, d) == d << (w * i)
    # the bound is met and never passed: the largest top bits with a carry coming in, r - 1, and random scalars
    top = (R >> b) << b
    low_all_carry = sum((half + 1) << (w * i) for i in range(n - 1))
    worst = top + low_all_carry % (1 << b)
    rnd = random.Random(w)
    ks = [R - 1, top] + ([worst] if worst < R else []) + [((R >> b) - 1 << b) + low_all_carry, *(rnd.randrange(R) for _ in range(500))]
    seen = 0
    for k in ks:
        assert k < R
        d = ac.signed_digits(k, w)[0][-1]
        assert 0 <= d <= bound
        seen = max(seen, d)
    assert seen >= bound - 1


def test_replay_follows_the_group_law():
    g = bn.G2_GEN
    y = 3
    for form, r, omega in ((0, 5, 15), (9, 257, 3 * 257), (9, 257, R - 3 * 257), (1, (7 << 16) + 2, 6), (10, 513, (5 << 32) + 1)):
        events, log = ac.replay_c3(form, y, r, omega)
        steps = [y * d * (1 << sh) % R for _i, d, sh in ac.attr_steps(form, r)] + [(d << sh) % R for _i, d, sh in ac.g2_steps(form, omega)]
        acc, seen = None, 0
        for e in steps:
            entry = bn.g2_mul(g, e)
            seen += acc is not None and (acc == entry or acc == bn.g2_neg(entry))
            acc = bn.g2_add(acc, entry)
        assert seen == len(events)
        assert acc == (bn.g2_mul(g, log) if log else None) and log == (y * r + omega) % R
    assert ac.replay_c3(0, y, 5, 15)[0] == [(1, 0, "dbl")]
    assert ac.replay_c3(9, y, 257, R - 3 * 257)[1] == 0


# ------------------------------------------------------------------------------------------------ class A
@pytest.mark.parametrize("w", ac.SIGNED_WIDTHS)
def test_class_a_reaches_the_edges_of_every_signed_width(cs, w):
    n, half = ac.sgn_windows(w), 1 << (w - 1)
    digs = [ac.signed_digits(r["rand"], w)[0] for _t, r in rows_of(cs, "A")]
    assert any(d[:n - 1] == [half] * (n - 1) and d[n - 1] == 0 for d in digs), "every digit at half"
    assert any(all(x < 0 for x in d[:n - 1]) and d[n - 1] == 1 for d in digs), "a carry through every window into the last"
    raw = [[ac.scalar_bits(r["rand"], w * i, w) for i in range(n)] for _t, r in rows_of(cs, "A")]
    for pos in range(n):                                                        # pos = n - 1: the top window is the only non-zero one
        assert any(v[pos] and not any(v[:pos] + v[pos + 1:]) for v in raw), "one non-zero window at %d" % pos
    for j in (1, 2, 3):
        assert any(not any(v[:j]) and all(v[j:n - 1]) for v in raw), "the low %d windows zero" % j
    for dgt in (1, half, half + 1, (1 << w) - 1):
        if w in (9, 10, 14):
            for pos in range(n - 1):
                assert any(v[pos] == dgt and not any(v[:pos] + v[pos + 1:]) for v in raw)


def test_class_a_reaches_the_edges_of_the_plain_cuts_and_every_attribute(cs):
    A = rows_of(cs, "A")
    for cut, n in ((ac.digits8, 32), (ac.digits16, 16)):
        ds = [cut(r["rand"]) for _t, r in A]
        for pos in range(n):
            assert any(v[pos] and not any(v[:pos] + v[pos + 1:]) for v in ds)
    for k in ws.common():
        assert any(r["rand"] == k for _t, r in A)
    assert {r["attr"] for _t, r in A} == set(range(ac.N_ATTRS))
    assert all(r["omg"] == 0 and r["lam"] == cs.items[r["item"]]["s"] != 0 and r["rand"] < R for _t, r in A)


# ------------------------------------------------------------------------------------------------ class B
def test_class_b_starts_the_gt_product_where_it_says(cs):
    B = {r["name"]: r for _t, r in rows_of(cs, "B")}
    assert all(r["omg"] == 0 for r in B.values())
    for w in ac.SIGNED_WIDTHS:
        r = B["lam 0, r half+1 of %d" % w]
        assert r["lam"] == 0 and ac.first_take_gt(w, 0, r["rand"]) == ("attr", -1)               # facc_set of a conjugated entry
        assert ac.attr_steps(w, r["rand"]) == [(0, -((1 << (w - 1)) - 1), 0), (1, 1, w)]
        r = B["lam 0, r half of %d" % w]
        assert r["lam"] == 0 and ac.attr_steps(w, r["rand"]) == [(0, 1 << (w - 1), 0)]            # the last entry of window 0, positive
        for form in (0, 1):
            assert ac.first_take_gt(form, 0, r["rand"]) == ("attr", 1)
    assert (B["lam 0, r 0"]["lam"], B["lam 0, r 0"]["rand"]) == (0, 0)
    assert all(ac.first_take_gt(f, 0, 0) is None for f in ac.FORMS)
    t0 = [t for t, r in enumerate(cs.rows) if r["name"] == "lam 0, r 0"][0]
    assert cs.row_logs(t0) == (0, 0, 0)
    assert (B["lam 0, r 1"]["lam"], B["lam 0, r 1"]["rand"]) == (0, 1)
    assert (B["lam 1, r 0"]["lam"], B["lam 1, r 0"]["rand"]) == (1, 0)
    assert (B["lam R-1, r 0"]["lam"], B["lam R-1, r 0"]["rand"]) == (R - 1, 0)
    assert (B["lam R-1, r R-1"]["lam"], B["lam R-1, r R-1"]["rand"]) == (R - 1, R - 1)
    assert [B["lam edge(16)[%d]" % j]["lam"] for j in range(len(ws.edge(16)))] == ws.edge(16)
    assert all(0 < B["lam edge(16)[%d]" % j]["rand"] < R for j in range(len(ws.edge(16))))


# ------------------------------------------------------------------------------------------------ class C
def top_step(form, k):
    return ac.g2_steps(form, k)[-1][0]


@pytest.mark.parametrize("form", ac.FORMS)
def test_class_c_meets_its_event_in_every_form_and_no_other_row_meets_one(cs, form):
    win = 4 if ac.g2_cut(form) == 8 else 2                      # the window of 5 2^32 in the cut of the g2 table
    kinds = set()
    for t, r in enumerate(cs.rows):
        y = cs.y[r["attr"]]
        events, log = ac.replay_c3(form, y, r["rand"], r["omg"])
        assert log == cs.row_logs(t)[2]
        if r["cls"] != "C":
            assert events == [], cs.label(t)
            continue
        kind = r["name"].split(":")[0].split(" x")[0]
        kinds.add(kind)
        if kind == "doubling":
            assert events == [(1, win, "dbl")] and log, cs.label(t)
            assert ac.g2_steps(form, r["omg"])[0][0] == win and top_step(form, r["omg"]) > win          # the first entry of the g2 walk; more follow
        elif kind == "opposite":
            assert events == [(1, win, "cancel")] and log, cs.label(t)                                     # infinity in mid-walk, then on
            assert ac.g2_steps(form, r["omg"])[0][0] == win and top_step(form, r["omg"]) > win
        elif r["name"].endswith("infinity"):
            assert events == [(1, top_step(form, r["omg"]), "cancel")] and log == 0, cs.label(t)           # the last addition of the lane
        else:
            assert events == [] and log, cs.label(t)
    assert kinds == {"doubling", "opposite", "inf row 1", "inf row 2"}


def test_class_c_rows_are_the_logs_the_issue_names(cs):
    for t, r in rows_of(cs, "C"):
        it = cs.items[r["item"]]
        x = t - it["row0"] + 1
        y, (a1, b1) = cs.y[r["attr"]], it["coefs"]
        assert r["lam"] == (it["s"] + a1 * x) % R and r["omg"] == b1 * x % R
        if r["name"].startswith("doubling"):
            assert y * r["rand"] % R == x * ac.DBL_LOG and b1 & ((1 << 48) - 1) == ac.DBL_LOG and b1 >> 48 and 2 * b1 < R
        if r["name"].startswith("opposite"):
            assert (y * r["rand"] + x * ac.DBL_LOG) % R == 0 and b1 & ((1 << 48) - 1) == ac.DBL_LOG
        if r["name"] == "inf row 1: ordinary":
            assert cs.row_logs(t)[2] == (R - y * r["rand"]) % R                  # -g2 * (y r)
    assert {r["attr"] for _t, r in rows_of(cs, "C")} == set(range(ac.N_ATTRS))


# ------------------------------------------------------------------------------------------------ class D, E and the placement
def test_class_d_words_are_not_canonical(cs):
    D = rows_of(cs, "D")
    assert {r["name"] for _t, r in D} == {"k + R", "7 + 5 R", "2^256 - 1", "R"}
    for t, r in D:
        assert R <= r["rand"] < 1 << 256 and r["rand"] // R <= 5                # what ld_scalar's five subtractions bring below r
        assert cs.row_logs(t)[1] == r["rand"] % R
    assert any(r["rand"] == R and cs.row_logs(t)[1] == 0 for t, r in D) and any(r["rand"] == 7 + 5 * R for _t, r in D)
    assert {r["attr"] for _t, r in D} == set(range(ac.N_ATTRS))


def test_placement(cs):
    n = len(cs.rows)
    assert 300 <= n <= 800 and n % ac.C3_BLOCK and n % ac.C1_BLOCK                                   # a partial last block: shadow lanes in c3
    assert all(h in cs.row_off for h in ac.HEADS)
    # a degenerate row between ordinary neighbours inside the first 128-row block, and one as the last row of the call
    inf = [t for t in range(n) if cs.row_logs(t)[2] == 0 and cs.rows[t]["cls"] == "C"]
    assert any(0 < t < ac.C3_BLOCK - 1 and cs.row_logs(t - 1)[2] and cs.row_logs(t + 1)[2] for t in inf)
    assert n - 1 in inf and cs.rows[n - 1]["attr"] == ac.N_ATTRS - 1
    assert cs.items_for_rows(129) and [cs.rows[t]["cls"] for t in (66, 83)] == ["C", "C"]
    # class E: the OR's three rows take lambda = s and omega = 0 under three attributes; an AND lies across rows 255 | 256
    E = rows_of(cs, "E")
    orr = [(t, r) for t, r in E if r["name"].startswith("OR")]
    assert len(orr) == 3 and [r["attr"] for _t, r in orr] == [0, 1, 2]
    assert all(r["lam"] == cs.items[r["item"]]["s"] and r["omg"] == 0 for _t, r in orr)
    across = [t for t, r in E if r["name"].startswith("AND across")]
    assert across == [2 * ac.C3_BLOCK - 1, 2 * ac.C3_BLOCK] and cs.rows[across[0]]["item"] == cs.rows[across[1]]["item"]
    assert {r["cls"] for r in cs.rows} == set("ABCDE")


def test_shares_equal_a_walk_of_the_flattened_tables(cs):
    """the builder's Shamir shares against a second restatement: Horner along the leaf's path of hostprep.TreeTables (what the device walks)"""
    tt = cs.tt

    def share(leaf, gate0, coefs, secret):
        s = secret
        for e in range(tt.path_off[leaf], tt.path_off[leaf + 1]):
            g = gate0 + tt.path_gate[e]
            k = tt.gate_k[g]
            if k <= 1:
                continue
            a = coefs[tt.gate_coef_off[g]:tt.gate_coef_off[g] + k - 1]
            acc = 0
            for aj in reversed(a):
                acc = (acc + aj) * tt.path_x[e] % R
            s = (s + acc) % R
        return s
    for t, r in enumerate(cs.rows):
        it = cs.items[r["item"]]
        leaf = tt.first_leaf[it["tree"]] + t - it["row0"]
        half = len(it["coefs"]) // 2
        assert r["lam"] == share(leaf, tt.first_gate[it["tree"]], it["coefs"][:half], it["s"])
        assert r["omg"] == share(leaf, tt.first_gate[it["tree"]], it["coefs"][half:], 0)
        assert r["attr"] == cs.leaf_attr[leaf]
    arr = cs.call_arrays(cs.items_for_rows(65))
    assert arr["total_rows"] == 65 and arr["row_off"][-1] == 65 and len(arr["rand"]) == 65 and len(arr["s"]) == arr["n_items"]


# ------------------------------------------------------------------------------------------------ the builder itself
def test_expected_values_equal_direct_oracle_products(cs):
    assert cs.egg_alpha[1] == bn.gt_pow(cs.E, cs.alpha[1]) and cs.g2_y[2] == bn.g2_mul(cs.g2, cs.y[2])
    assert all(x >= 1 << 200 for x in [cs.a, cs.b] + cs.alpha + cs.y)
    rnd = random.Random("self-check")
    n = len(cs.rows)
    picks = rnd.sample(range(n), 3) + [2 * ac.C3_BLOCK, rnd.choice([t for t, r in rows_of(cs, "D")])]
    for t in picks:
        r = cs.rows[t]
        a, k = r["attr"], r["rand"] % R
        c1, c2, c3 = cs.want_row(t)
        assert c1 == bn.gt_to_le(bn.gt_mul(bn.gt_pow(cs.E, r["lam"]), bn.gt_pow(cs.egg_alpha[a], k))), cs.label(t)
        assert c2 == ac.g2_le(bn.g2_mul(cs.g2, k)), cs.label(t)
        assert c3 == ac.g2_le(bn.g2_add(bn.g2_mul(cs.g2_y[a], k), bn.g2_mul(cs.g2, r["omg"]))), cs.label(t)
    i = cs.rows[picks[0]]["item"]
    assert cs.want_c0(i) == bn.gt_to_le(bn.gt_mul(bn.gt_from_le(cs.msg(i)), bn.gt_pow(cs.E, cs.items[i]["s"])))
    assert ac.g2_le(None) == bytes(128) and ac.gt_le(None) == bn.gt_to_le(bn.FP12_ONE)
