"""The integer proofs of tests/row_cases.py, on the CPU: every call that tests/test_gpu_row_kernels_degenerate.py launches is built here and
each of its rows replayed on the discrete logs -- the intended doubling or cancellation happens at the intended window and nowhere else.
The replay itself is checked against the oracle's group law on small cases."""
import pytest

from oracle import bn254 as bn
from tests import row_cases as rc

R = rc.R


def test_replay_follows_the_group_law():
    g = bn.G1_GEN
    for walks, tail in (([(1, 7), (1, 7)], None), ([(5, 3), (1, 15 + (2 << 16))], None), ([(1, 9)], 9), ([(1, R - 9)], 9),
                        ([(3, 0x10000), (1, (5 << 32) + 0x30000)], None), ([(1, R - 5), (1, 5 + (7 << 16))], None)):
        events, log = rc.replay(walks, tail)
        acc, seen = None, []
        steps = [(i, w, base * (d << (16 * w)) % R) for i, (base, k) in enumerate(walks) for w, d in enumerate(rc.digits(k)) if d]
        steps += [(len(walks), 0, tail)] if tail is not None else []
        for i, w, e in steps:
            entry = bn.g1_mul(g, e)
            if acc is not None and acc == entry:
                seen.append((i, w, "dbl"))
            elif acc is not None and acc == bn.g1_neg(entry):
                seen.append((i, w, "cancel"))
            acc = bn.g1_add(acc, entry)
        assert seen == events and seen
        assert acc == (bn.g1_mul(g, log) if log else None)


def test_replay_sees_what_a_case_does_not_intend():
    with pytest.raises(AssertionError):
        rc.check_row([(1, 7), (1, 7)], None, [], 14)
    with pytest.raises(AssertionError):
        rc.check_row([(1, 7), (1, 8)], None, [(1, 0, "dbl")], 15)
    rc.check_row([(1, 7), (1, 7)], None, [(1, 0, "dbl")], 14)


@pytest.mark.parametrize("c", rc.RELATIONS)
def test_ghw11_encrypt_rows_reach_their_branches(c):
    call = rc.enc_every_case(c)
    kinds = {r["kind"] for r in call.rows}
    assert kinds == set(rc.ENC_KINDS)
    for r in call.rows:
        if r["kind"].startswith("dbl"):
            w = {"dbl w0": 0, "dbl w1": 1, "dbl top": 15}[r["kind"]]
            assert r["events"] == [(1, w, "dbl")] and rc.low_window(r["k2"]) == w          # every window below is skipped
            if c == 1:
                assert r["lam"] == r["k2"] and r["lam"] >> (16 * w) < 0x3000
        if r["kind"] == "cancel mid":
            assert r["events"][0][1] < rc.top_window(r["k2"]) and r["c_log"]               # later windows bring the accumulator back
    for kind in rc.ENC_KINDS[1:]:
        rc.enc_one_row(c, kind)


def test_ghw11_encrypt_257_rows_put_the_cases_on_the_block_edges():
    call = rc.enc_257()
    assert {t: call.rows[t]["kind"] for t in (0, 63, 64, 255, 256)} == {0: "dbl w0", 63: "cancel last", 64: "both zero", 255: "dbl top",
                                                                         256: "cancel last"}
    assert len(call.items) == 257 - 2 - 1


@pytest.mark.parametrize("c", rc.RELATIONS)
def test_ghw11_key_rows_reach_their_branches(c):
    call = rc.key_small(c)
    assert set(call.kind) == set(rc.KEY_KINDS)
    for i, kind in enumerate(call.kind):
        if kind == "dbl z one":
            assert call.ev_tk[i] == [(1, 1 if c == 5 << 16 else 0, "dbl")]
    rc.key_135(c)
    rc.key_r_zero_130(c)


@pytest.mark.parametrize("c1,c2", rc.DNF_RELATIONS)
def test_dnf_key_rows_reach_their_branches(c1, c2):
    call = rc.dnf_small(c1, c2)
    assert set(call.kind) == set(rc.DNF_KINDS)
    rc.dnf_129(c1, c2)
    for kind in rc.DNF_KINDS[1:]:
        rc.dnf_one_item(c1, c2, kind)
    rc.dnf_a_infinity()


def test_raw_words_are_not_canonical_and_name_the_same_scalar():
    import random
    words = rc.raw_words(random.Random(1), 8)
    assert [w for w, _k in words[2:4]] == [R, (1 << 256) - 1]
    assert all(w >= R and w % R == k for w, k in words)
    assert words[1][0] - words[1][1] == 5 * R
