"""The integer proofs of tests/msm_cases.py, on the CPU: every item that tests/test_gpu_msm_degenerate.py hands to the shared-doubling sums
is built here for both regimes and replayed on the discrete logs -- the intended doubling or cancellation happens at the intended chunk and
bit (or partial of the fold) and nowhere else.  (L, C) comes from rb_msm_chunks (rabe_amd/csrc/msm_chunks.h: what choose_msm_chunks runs)
through the host build, for a device of 256 compute units; the function is pinned on hand-derived values.  The replay itself is checked
against the oracle's group law and against the host build of jac_msm_naf."""
import ctypes

import pytest

from oracle import bn254 as bn
from tests import msm_cases as mc
from tests.hostsim import build as hsb

R = mc.R
SIMDS = 256 * 4


@pytest.fixture(scope="module")
def hs():
    return hsb.load()


@pytest.fixture(scope="module")
def regimes(hs):
    n = mc.chunked_items(hs, SIMDS)
    assert n is not None and n <= 4200
    return {"small": (mc.SMALL_ITEMS, mc.SMALL_TERMS) + mc.chunks(hs, SIMDS, mc.SMALL_ITEMS, mc.SMALL_TERMS),
            "chunked": (n, mc.CHUNKED_TERMS) + mc.chunks(hs, SIMDS, n, mc.CHUNKED_TERMS)}


def test_msm_chunks_hand_derived(hs):
    """cost(c) = rounds x (2 + c_eff), l = ceil(T / c), c_eff = ceil(T / l), rounds = ceil(ceil(n l / 64) / simds), the first minimum wins.
    (1024, 70, 9):    c = 1: l = 9, 10 waves, 1 round, cost 3; every larger c costs 1 x (2 + c_eff) >= 4           -> L 9, C 1
    (1024, 4096, 17): c = 1: l = 17, 1088 waves, 2 rounds, cost 6; c = 2: l = 9, c_eff = 2, 576 waves, 1 round, cost 4;
                      c >= 3: one round, cost 2 + c_eff >= 5                                                          -> L 9, C 2"""
    assert mc.chunks(hs, 1024, 70, 9) == (9, 1)
    assert mc.chunks(hs, 1024, 4096, 17) == (9, 2)
    # one round holds 64 x 1024 = 65 536 lanes: 3855 x 17 = 65 535 still fits with a lane per term, 3856 x 17 does not
    assert mc.chunks(hs, 1024, 3855, 17) == (17, 1) and mc.chunks(hs, 1024, 3856, 17) == (9, 2)
    assert mc.chunks(hs, 1024, 1, 1) == (1, 1) and mc.chunks(hs, 1024, 5, 0) == (1, 1)
    assert mc.chunks(hs, 4, 100000, 40) == (1, 40)          # a chip that small: one lane per item


def test_regimes_at_256_cus(regimes):
    n, t, L, C = regimes["small"]
    assert 70 <= n <= 130 and n % 64 and t == 9 and (L, C) == (9, 1)
    n, t, L, C = regimes["chunked"]
    assert n == 3856 and n % 64 and t == 17 and C >= 2 and L >= 2
    assert n > 3 * mc.G1_FINISH_BLOCK and n % mc.G1_FINISH_BLOCK and n % mc.G2_FINISH_BLOCK


def test_replay_follows_the_group_law():
    g = bn.G1_GEN
    items = [([(3, 5), (3, 5)], 1, 2), ([(3, 5), (3, R - 5), (7, 9)], 2, 2), ([(3, 5), (3, 5)], 2, 1), ([(3, 5), (R - 3, 5)], 2, 1),
             ([(3, 1 << 4), (48, 1), (5, 3)], 2, 2), ([(3, 1 << 6), (R - 12, 17), (5, 1)], 1, 3), ([(0, 5), (3, 0), (3, R + 2)], 2, 2)]
    total = []
    for item, L, C in items:
        for flip in (False, True):
            events, log = mc.replay(item, L, C, flip)
            seen, parts = [], []
            for c in range(L):
                terms = [(bn.g1_mul(g, d) if d else None, mc.signed_digits(w, flip)) for d, w in item[c * C:(c + 1) * C]]
                acc, started = None, False
                for bit in range(255, -1, -1):
                    if started:
                        acc = bn.g1_add(acc, acc)
                    for pt, dig in terms:
                        if bit in dig and pt is not None:
                            e = pt if dig[bit] > 0 else bn.g1_neg(pt)
                            if acc is not None and acc == e:
                                seen.append((c, bit, "dbl"))
                            elif acc is not None and acc == bn.g1_neg(e):
                                seen.append((c, bit, "cancel"))
                            acc, started = bn.g1_add(acc, e), True
                parts.append(acc)
            acc = parts[0]
            for c in range(1, L):
                if acc is not None and parts[c] is not None and acc == parts[c]:
                    seen.append((mc.FINISH, c, "dbl"))
                elif acc is not None and parts[c] is not None and acc == bn.g1_neg(parts[c]):
                    seen.append((mc.FINISH, c, "cancel"))
                acc = bn.g1_add(acc, parts[c])
            assert seen == events
            assert acc == (bn.g1_mul(g, log) if log else None)
            total += events
    assert {(e[0] == mc.FINISH, e[2]) for e in total} == {(False, "dbl"), (False, "cancel"), (True, "dbl"), (True, "cancel")}


def test_check_sees_what_a_case_does_not_intend():
    with pytest.raises(AssertionError):
        mc.check([(3, 5), (3, 5)], 1, 2, [])
    with pytest.raises(AssertionError):
        mc.check([(3, 5), (4, 5)], 1, 2, [(0, 2, "dbl")])
    mc.check([(3, 5), (3, 5)], 1, 2, [(0, 2, "dbl")])


@pytest.mark.parametrize("regime", ["small", "chunked"])
def test_every_kind_reaches_its_branch(regimes, regime):
    n, max_terms, L, C = regimes[regime]
    cases = mc.cases(max_terms, L, C)
    in_lane = C >= 2
    nonzero = lambda k: len(mc.signed_digits(k, False))
    # what each kind is for, beyond `check` (which mc.cases has run on both mask orientations)
    assert cases["twin"].events == ([(0, mc.top_bit(cases["twin"].terms[0][1]), "dbl")] if in_lane else [(mc.FINISH, 1, "dbl")])
    for kind in ("twin-opposite", "twin-opposite bases", "twin-opposite alone"):
        ev = cases[kind].events
        assert ev == [(mc.FINISH, 1, "cancel")] if not in_lane else (len(ev) == nonzero(cases[kind].terms[0][1]) > 60 and all(e[2] == "cancel" for e in ev))
    assert cases["twin across chunks"].events == [(mc.FINISH, 1, "dbl")] and cases["opposite across chunks"].events == [(mc.FINISH, 1, "cancel")]
    assert cases["dbl mid-walk"].events == ([(0, 0, "dbl")] if in_lane else [(mc.FINISH, 1, "dbl")])
    assert cases["cancel mid-walk"].events == ([(0, mc.MID_U, "cancel")] if in_lane else [])
    for kind in ("ordinary", "ordinary five", "short", "scalar edges a", "scalar edges b", "zero terms", "zero scalars"):
        assert cases[kind].events == []
    words = [w for kind in ("scalar edges a", "scalar edges b") for _d, w in cases[kind].terms]
    assert {0, 1, 2, R - 1, mc.HALF, mc.HALF + 1, R, mc.TWO256 - 1} <= set(words)
    assert any(R < w < 2 * R for w in words) and any(5 * R < w < mc.TWO256 - 1 for w in words)
    assert cases["scalar edges a"].terms[0][0] == 0 and cases["scalar edges a"].terms[0][1] != 0             # the zero record under a scalar
    assert len(cases["short"].terms) < (L - 1) * C and (len(cases["short"].terms) % C != 0 or C == 1)
    assert len(cases["opposite across chunks"].terms) == C + 1                                                 # a last chunk of one term
    kinds = mc.layout(n)
    assert len(kinds) == n and kinds.index("ordinary") > 0
    for edge in (64, mc.G2_FINISH_BLOCK, mc.G1_FINISH_BLOCK):
        if edge < n:
            assert kinds[edge - 1] not in mc.ORDINARY and kinds[edge] not in mc.ORDINARY
    last = n - n % mc.G1_FINISH_BLOCK
    assert any(k in mc.INFINITE for k in kinds[last:]) and n % mc.G1_FINISH_BLOCK
    if regime == "chunked":
        quiet = kinds[2 * mc.G1_FINISH_BLOCK:3 * mc.G1_FINISH_BLOCK]
        for half in (quiet[:mc.G2_FINISH_BLOCK], quiet[mc.G2_FINISH_BLOCK:]):
            assert sorted(k for k in half if k not in mc.ORDINARY) in (["opposite across chunks"], ["zero scalars"])


@pytest.mark.parametrize("regime", ["small", "chunked"])
def test_host_build_of_the_walk_agrees_with_the_replay(hs, regimes, regime):
    """jac_msm_naf compiled for the host on every chunk of every kind (canonical, shortened scalars as k_naf_masks hands them on): the
    partial sum the replay predicts, as a point"""
    _n, max_terms, L, C = regimes[regime]
    g, pts = bn.G1_GEN, {}
    for kind, case in mc.cases(max_terms, L, C).items():
        for c in range(L):
            chunk = case.terms[c * C:(c + 1) * C]
            if not chunk:
                continue
            p, k = b"", b""
            for d, w in chunk:
                kk = w % R
                if d not in pts:
                    pts[d] = bn.g1_mul(g, d) if d else None
                pt = pts[d]
                if kk > mc.HALF:                      # the sign the masks would carry goes onto the base
                    kk, pt = R - kk, (bn.g1_neg(pt) if pt is not None else None)
                p += bn.g1_to_le(pt)
                k += mc.word_bytes(kk)
            out = ctypes.create_string_buffer(64)
            hs.hs_g1_msm(len(chunk), p, k, out)
            _ev, log = mc.replay(chunk, 1, len(chunk))
            assert out.raw == bn.g1_to_le(bn.g1_mul(g, log) if log else None), (kind, c)


def test_aw11_exponent_is_the_scheme_decrypt(regimes):
    """mc.aw11_item's exponent (derived from the kernels' comments) against the arithmetic of oracle.schemes.aw11_decrypt on group elements:
    c_0 / prod_j ( C1_j e(H, C3_j) / e(K_j, C2_j) )^c_j, on an ordinary item"""
    _n, max_terms, L, C = regimes["small"]
    case = mc.cases(max_terms, L, C)["short"]
    rows, h, a0, x = mc.aw11_item(case, 0)
    egg = bn.pairing(bn.G1_GEN, bn.G2_GEN)
    hp = bn.g1_mul(bn.G1_GEN, h)
    egg_s = bn.GT_ONE
    for (a, u, t, kappa), (_t, w) in zip(rows, case.terms):
        num = bn.gt_mul(bn.gt_pow(egg, a), bn.pairing(hp, bn.g2_mul(bn.G2_GEN, t)))
        dem = bn.pairing(bn.g1_mul(bn.G1_GEN, kappa), bn.g2_mul(bn.G2_GEN, u))
        egg_s = bn.gt_mul(egg_s, bn.gt_pow(bn.gt_mul(num, bn.gt_inv(dem)), w % R))
    assert bn.gt_to_le(bn.gt_mul(bn.gt_pow(egg, a0), bn.gt_inv(egg_s))) == bn.gt_to_le(bn.gt_pow(egg, x))
