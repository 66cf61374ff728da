"""g1_madd_inl (the Z3 = Z1*H mixed addition the G1 table kernels inline, rabe_amd/csrc/bn254/curve.h) against the generic
jac_add_aff<Fp> of the same header and against the oracle, on the CPU: tests/hostsim/g1_madd_forms.cpp is a stand-alone program
compiled from the engine's headers.  The two additions return different Jacobian representatives (Z differs by a factor 2 per
addition), so everything is compared in affine form.  No GPU needed."""
import os
import random
import subprocess

import pytest

from oracle import bn254 as bn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "g1_madd_forms.cpp")
EXE = os.path.join(ROOT, "build", "g1_madd_forms")
HDR_DIR = os.path.join(ROOT, "rabe_amd", "csrc", "bn254")
RND = random.Random(0x6D616464)
MONT_R = (1 << 256) % bn.P


def build_program():
    deps = [SRC] + [os.path.join(HDR_DIR, f) for f in os.listdir(HDR_DIR)]
    if os.path.exists(EXE) and all(os.path.getmtime(d) <= os.path.getmtime(EXE) for d in deps):
        return EXE
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    # RABE_HOST_SANITIZE=address,undefined builds the program (host code, its own main) with those sanitizers
    san = os.environ.get("RABE_HOST_SANITIZE")
    extra = ["-fsanitize=" + san, "-fno-sanitize-recover=all", "-g"] if san else []
    subprocess.run(["hipcc", "-O2", "-std=c++17", "-x", "hip", "--cuda-host-only", "-o", EXE, SRC] + extra, check=True, timeout=600)
    return EXE


def mont(x):
    return (x * MONT_R) % bn.P


def limbs(m):
    return int(m).to_bytes(32, "little")


def jac(pt, z):
    """Montgomery limbs of the Jacobian (x z^2, y z^3, z) of an affine oracle point; None is infinity (Z = 0, X = Y = 1 as jac_inf)"""
    if pt is None:
        return limbs(mont(1)) + limbs(mont(1)) + limbs(0)
    z %= bn.P
    return limbs(mont(pt[0] * z * z)) + limbs(mont(pt[1] * z * z * z)) + limbs(mont(z))


def aff(pt):
    return bytes(64) if pt is None else limbs(mont(pt[0])) + limbs(mont(pt[1]))


def run(records):
    exe = build_program()
    res = subprocess.run([exe], input=b"".join(records), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = res.stdout
    assert len(out) == 128 * len(records), res.stderr.decode()
    pairs = [(out[128 * i:128 * i + 64], out[128 * i + 64:128 * i + 128]) for i in range(len(records))]
    return res.returncode, pairs, res.stderr.decode()


@pytest.fixture(scope="module")
def pool():
    """on-curve points with cheap oracle work: a chain of additions from a few scalar multiples"""
    pts = [bn.g1_mul(bn.G1_GEN, RND.randrange(1, bn.R)) for _ in range(4)]
    while len(pts) < 96:
        pts.append(bn.g1_add(pts[-1], pts[RND.randrange(len(pts) - 1)]))
    return pts


def rand_z():
    return RND.randrange(1, bn.P)


def test_random_pairs_with_random_z(pool):
    cases = [(RND.choice(pool), RND.choice(pool), rand_z()) for _ in range(3000)]
    rc, got, err = run([jac(p, z) + aff(q) for p, q, z in cases])
    assert rc == 0, err
    for (p, q, _z), (madd, ref) in zip(cases, got):
        assert madd == ref == bn.g1_to_le(bn.g1_add(p, q))


def test_special_cases(pool):
    cases = []
    for p in pool[:12]:
        cases += [(None, p, 1), (p, None, 1), (p, None, rand_z()), (None, None, 1),              # p infinite, q infinite, both
                  (p, p, 1), (p, p, rand_z()), (p, p, bn.P - 1),                                   # p == q: the doubling branch
                  (p, bn.g1_neg(p), 1), (p, bn.g1_neg(p), rand_z()),                               # p == -q: infinity
                  (p, pool[20], 1), (p, pool[21], 1)]                                              # Z1 = 1 (the step after the copy)
    rc, got, err = run([jac(p, z) + aff(q) for p, q, z in cases])
    assert rc == 0, err
    for (p, q, _z), (madd, ref) in zip(cases, got):
        assert madd == ref == bn.g1_to_le(bn.g1_add(p, q))


def test_chain_of_additions_changes_only_the_representative(pool):
    """a 13-window walk as the table kernels do it, through the oracle; every intermediate goes back in with a fresh random Z"""
    acc, recs, want = None, [], []
    for q in pool[30:43]:
        recs.append(jac(acc, rand_z()) + aff(q))
        acc = bn.g1_add(acc, q)
        want.append(bn.g1_to_le(acc))
    rc, got, err = run(recs)
    assert rc == 0, err
    assert [m for m, _ in got] == want


def test_extreme_limbs_in_every_coordinate(pool):
    """the limb patterns of tests/carry_vectors.py (saturated limbs, the modulus' own limbs +-1, p - 1, ...) as raw Montgomery forms
    of X1, Y1, Z1, x2, y2.  Such points are not on the curve; both additions are the same rational map of their coordinates (neither
    uses the curve equation), so the affine results still have to agree -- and the doubling formulas are never reached (H != 0)
    except where a pattern repeats, which both handle alike."""
    from tests import test_gpu_field_edge as fe                  # mont_patterns: what carry_vectors.py feeds the device with
    state = fe.RND.getstate()
    pats = fe.mont_patterns(bn.P, 160)
    fe.RND.setstate(state)                                       # that module's own tests keep their inputs
    recs = []
    for i in range(len(pats)):                                   # sliding window: every pattern meets every coordinate
        five = [pats[(i + 7 * k) % len(pats)] for k in range(5)]
        if five[2] == 0:
            five[2] = 1                                          # Z1 = 0 is infinity: covered above
        recs.append(b"".join(limbs(m) for m in five))
    for m in pats[:40]:                                          # one extreme coordinate on an otherwise honest pair
        p, q, z = RND.choice(pool), RND.choice(pool), rand_z()
        for slot in range(5):
            rec = bytearray(jac(p, z) + aff(q))
            rec[32 * slot:32 * slot + 32] = limbs(m if (m or slot != 2) else 1)
            recs.append(bytes(rec))
    want = []
    for m in pats[:40]:                                          # extreme Z1 on an ON-CURVE point: the oracle decides
        if m == 0:
            continue
        p, q = RND.choice(pool), RND.choice(pool)
        z = (m * pow(MONT_R, -1, bn.P)) % bn.P                   # the canonical value whose Montgomery form is exactly m
        recs.append(jac(p, z) + aff(q))
        assert recs[-1][64:96] == limbs(m)
        want.append(bn.g1_to_le(bn.g1_add(p, q)))
    rc, got, err = run(recs)
    assert rc == 0, err
    assert all(m == r for m, r in got)
    assert [m for m, _ in got[-len(want):]] == want
    assert len(set(m for m, _ in got)) > len(recs) // 2          # real results, not a wall of zeros


def test_the_program_refuses_a_truncated_record():
    """the checker itself: a short read cannot pass as agreement"""
    exe = build_program()
    res = subprocess.run([exe], input=bytes(159), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert res.returncode == 2
