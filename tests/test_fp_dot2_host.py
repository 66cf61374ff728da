"""The two-term Montgomery dot product (rabe_amd/csrc/bn254/fp.h: dot2_inl) against Python integers, on the CPU: the host build runs
the loop form that FOLLOWS the carry-capture plan (an uncaptured product's carry is dropped, as on the device), so extreme limbs in the
registers are what can break it.  Operands are RAW Montgomery residues; the expected residue is (a0 b0 + a1 b1) / 2^256 mod m, compared
as canonical 32-byte strings.  Then the G1 mixed addition that ends in it (curve.h: g1_madd_inl), against jac_add_aff<Fp> and the
oracle after the conversion to affine.  No GPU needed."""
import random

import pytest

from oracle import bn254 as bn
from tests import dot2_host as dh
from tests import test_g1_madd_forms as mf

RND = random.Random(0xD072)


def want(mod, q):
    a0, b0, a1, b1 = q
    return dh.le((a0 * b0 + a1 * b1) * pow(1 << 256, -1, mod) % mod)


@pytest.mark.parametrize("field", ["fp", "fr"])
def test_random_operands(field):
    mod = dh.MODS[field]
    quads = [tuple(RND.randrange(mod) for _ in range(4)) for _ in range(4000)]
    rc, got, err = dh.dot2(field, quads)
    assert rc == 0, err
    assert [d for d, _ in got] == [want(mod, q) for q in quads]


@pytest.mark.parametrize("field", ["fp", "fr"])
def test_edge_operands_in_all_four_positions(field):
    mod = dh.MODS[field]
    edge = dh.edge_residues(mod, RND, n_random=60)
    quads = []
    for e in edge:                                             # one edge value in each position, the others random / edge
        for pos in range(4):
            for others in (lambda: RND.randrange(mod), lambda: RND.choice(edge)):
                q = [others() for _ in range(4)]
                q[pos] = e
                quads.append(tuple(q))
        quads += [(e, e, e, e), (e, mod - 1, mod - 1, e), (e, e, 0, 0), (0, 0, e, e)]
    named = edge[:10]                                          # 0, 1, 2, m - 1, m - 2, R mod m, saturated patterns: every combination
    quads += [(a, b, c, d) for a in named for b in named for c in named for d in named]
    rc, got, err = dh.dot2(field, quads)
    assert rc == 0, err
    assert [d for d, _ in got] == [want(mod, q) for q in quads]
    assert want(mod, (mod - 1, mod - 1, mod - 1, mod - 1)) in [d for d, _ in got]      # the largest sum, 2 (m - 1)^2, was among them


def test_cancelling_terms_give_zero_not_the_modulus():
    """a0 b0 + (m - a0) b0 = m b0: the reduced value is 0, never the limbs of m"""
    mod = bn.P
    quads = []
    for _ in range(200):
        a, b = RND.randrange(1, mod), RND.randrange(1, mod)
        quads.append((a, b, mod - a, b))
    rc, got, err = dh.dot2("fp", quads)
    assert rc == 0, err
    assert all(d == bytes(32) for d, _ in got)


def test_the_program_refuses_a_truncated_record():
    import subprocess
    res = subprocess.run([dh.build_program(), "fp"], input=bytes(127), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert res.returncode == 2


# ---- the addition that ends in the dot product -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool():
    pts = [bn.g1_mul(bn.G1_GEN, RND.randrange(1, bn.R)) for _ in range(4)]
    while len(pts) < 64:
        pts.append(bn.g1_add(pts[-1], pts[RND.randrange(len(pts) - 1)]))
    return pts


def test_addition_random_and_special_cases(pool):
    z = lambda: RND.randrange(1, bn.P)
    cases = [(RND.choice(pool), RND.choice(pool), z()) for _ in range(1500)]
    for p in pool[:10]:
        cases += [(None, p, 1), (p, None, 1), (p, None, z()), (None, None, 1),                   # accumulator / entry at infinity
                  (p, p, 1), (p, p, z()), (p, p, bn.P - 1),                                      # P + P
                  (p, bn.g1_neg(p), 1), (p, bn.g1_neg(p), z())]                                  # P + (-P)
    rc, got, err = mf.run([mf.jac(p, zz) + mf.aff(q) for p, q, zz in cases])
    assert rc == 0, err
    for (p, q, _z), (madd, ref) in zip(cases, got):
        assert madd == ref == bn.g1_to_le(bn.g1_add(p, q))


def test_addition_with_extreme_limb_coordinates(pool):
    """accumulators whose Z (on-curve points: the oracle decides) or whose Y1 / any coordinate (raw patterns: both additions are the same
    rational map) has extreme limbs -- Y1 = 0 among them, where neg(Y1) has to be 0 and not the modulus"""
    rinv = pow(1 << 256, -1, bn.P)
    edge = dh.edge_residues(bn.P, RND, n_random=40)
    recs, want_tail = [], []
    for m in edge:                                             # one extreme coordinate on an otherwise honest pair
        p, q, z = RND.choice(pool), RND.choice(pool), RND.randrange(1, bn.P)
        for slot in range(5):
            rec = bytearray(mf.jac(p, z) + mf.aff(q))
            rec[32 * slot:32 * slot + 32] = dh.le(m if (m or slot != 2) else 1)       # Z1 = 0 is infinity: covered above
            recs.append(bytes(rec))
    y1_zero = [i for i, r in enumerate(recs) if r[32:64] == bytes(32)]
    assert y1_zero
    for m in edge:
        if m == 0:
            continue
        p, q = RND.choice(pool), RND.choice(pool)
        recs.append(mf.jac(p, m * rinv % bn.P) + mf.aff(q))   # the canonical Z whose Montgomery form is exactly m
        assert recs[-1][64:96] == dh.le(m)
        want_tail.append(bn.g1_to_le(bn.g1_add(p, q)))
    rc, got, err = mf.run(recs)
    assert rc == 0, err
    assert all(m == r for m, r in got)
    assert [m for m, _ in got[-len(want_tail):]] == want_tail
    assert len(set(m for m, _ in got)) > len(recs) // 2


def test_walk_of_13_additions_compared_at_the_end(pool):
    """the accumulator stays Jacobian from the infinite start through 13 entries, as in the signed 20-bit walk; one entry is infinity
    (a zero digit's entry never reaches the addition on the device, but the routine has to pass it through)"""
    entries = pool[20:26] + [None] + pool[26:32]
    assert len(entries) == 13
    acc = None
    for q in entries:
        acc = bn.g1_add(acc, q)
    rc, madd, ref = dh.walk([mf.aff(q) for q in entries])
    assert rc == 0
    assert madd == ref == bn.g1_to_le(acc)
    # the same entry twice (the copy, then the doubling branch), then its negative twice (back to the entry, then cancellation: the
    # walk goes on from an infinite accumulator)
    p = pool[40]
    entries = [p, p, bn.g1_neg(p), bn.g1_neg(p)] + pool[41:50]
    assert len(entries) == 13
    acc = None
    for q in entries:
        acc = bn.g1_add(acc, q)
    rc, madd, ref = dh.walk([mf.aff(q) for q in entries])
    assert rc == 0
    assert madd == ref == bn.g1_to_le(acc)
