"""rhip_dnf_decrypt_batch_one_uk (include/rabe_hip.h) called directly through the ctypes engine wrapper: the four-pair form of the BDABE / MKE08
decrypt, out[i] = lead[i] * e(e2, S2[c]) * e(S1[c], e3) * e(-e4, u2) * e(-u1, e5).

Every argument is a known multiple of a generator, so the expected element is E^x with E = e(G1, G2) and
    x = l + e2 s2[c] + s1[c] e3 - e4 u2 - u1 e5   (mod r; a term drops out where one of its arguments is the identity).
E comes from oracle.bn254's pairing; for the first three items of every batch E^x is oracle.bn254's gt_pow as well, and for all items it is
rhip_gt_pow of the oracle's E -- a kernel the launch under test does not touch.  Sizes 1, 63, 64, 65 and 130 (below, at and above one 64-lane
wave of the uniform pair map; two tiles and a ragged tail), once per family of pairing kernels.  Item i takes case i % 8: the two ordinary
classes, a class whose S1 is the identity (skip bit 0; its S1 slot holds a point that must not be read), a class whose S2 is (skip bit 1 and a
line block of the identity), and a ciphertext element at infinity in each of the four positions.  The walk verdicts
(rhip_ctx_collect_walk_verdicts) count the walked arguments that were examined: pairs 1 and 3 of an item -- two of its four pairs -- less
those that were skipped."""
import ctypes
import random

import pytest

from rabe_amd import Engine
from rabe_amd import engine as E

pytestmark = pytest.mark.gpu
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
SIZES = (1, 63, 64, 65, 130)
FAMILIES = (1, 6, 29, 58)
N_CLASSES = 4          # 0, 1 ordinary; 2: S1 = O; 3: S2 = O


def le(x):
    return int(x % R).to_bytes(32, "little")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.set_pairing_mode(0)
    e.close()


@pytest.fixture(scope="module")
def world(eng):
    """everything the cases share, computed once: the key side, and per size the inputs and the expected elements"""
    from oracle import bn254 as bn
    rnd = random.Random(0x646E66)
    g1, g2 = bn.g1_to_le(bn.G1_GEN), bn.g2_to_le(bn.G2_GEN)
    e_gen = bn.pairing(bn.G1_GEN, bn.G2_GEN)
    u1, u2 = rnd.randrange(1, R), rnd.randrange(1, R)
    s1 = [rnd.randrange(1, R) for _ in range(N_CLASSES)]
    s2 = [rnd.randrange(1, R) for _ in range(N_CLASSES)]
    s2[3] = 0                                                             # the identity: its line block has q_inf set
    p_s1 = eng.g1_mul([g1] * N_CLASSES, [le(x) for x in s1])          # class 2's slot holds an ordinary point that skip bit 0 hides
    p_q = eng.g2_mul([g2] * (1 + N_CLASSES), [le(x) for x in [u2] + s2])
    assert p_q[4] == bytes(128)
    d_q = eng.upload(b"".join(p_q))
    lines = E.G2Lines(eng, 1 + N_CLASSES, d_q)
    key = {"lines": lines, "d_s1": eng.upload(b"".join(p_s1)), "d_skip": eng.upload(bytes([0, 0, 1, 2])),
           "d_nu1": eng.upload(eng.g1_neg(eng.g1_mul([g1], [le(u1)]))[0])}
    out = {"key": key, "e_gen": e_gen, "batches": {}}
    for n in SIZES:
        cls, xs, c1, c2, ls, walked = [], [], [], [], [], []
        for i in range(n):
            case = i % 8
            c = case if case < 4 else i % 2
            e2, e3, e4, e5, l = (rnd.randrange(1, R) for _ in range(5))
            if case >= 4:
                e2, e3, e4, e5 = (0 if case - 4 == k else v for k, v in enumerate((e2, e3, e4, e5)))
            t_s1 = 0 if c == 2 else s1[c]
            xs.append((l + e2 * s2[c] + t_s1 * e3 - e4 * u2 - u1 * e5) % R)
            walked.append((1 if t_s1 and e3 else 0) + (1 if e5 else 0))
            cls.append(c)
            c1 += [e2, e4]
            c2 += [e3, e5]
            ls.append(l)
        e_le = bn.gt_to_le(e_gen)
        out["batches"][n] = {
            "d_class": eng.upload_u32(cls), "d_g1": eng.upload(b"".join(eng.g1_mul([g1] * (2 * n), [le(x) for x in c1]))),
            "d_g2": eng.upload(b"".join(eng.g2_mul([g2] * (2 * n), [le(x) for x in c2]))),
            "d_lead": eng.upload(b"".join(eng.gt_pow([e_le] * n, [le(x) for x in ls]))), "xs": xs, "walked": walked,
            "expect": eng.gt_pow([e_le] * n, [le(x) for x in xs])}
    yield out
    lines.destroy()


def test_expected_elements_are_the_oracles(world):
    """the first three items of every batch: E^x by oracle.bn254 alone"""
    from oracle import bn254 as bn
    for n in SIZES:
        b = world["batches"][n]
        for i in range(min(n, 3)):
            assert b["expect"][i] == bn.gt_to_le(bn.gt_pow(world["e_gen"], b["xs"][i])), (n, i)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n", SIZES)
def test_four_pair_decrypt(eng, world, n, family):
    k, b = world["key"], world["batches"][n]
    d_out, d_verdicts = eng.alloc(n * 384), eng.upload(bytes(8 * n))
    eng.set_pairing_mode(family)
    try:
        eng._check(eng.lib.rhip_ctx_collect_walk_verdicts(eng.ctx, d_verdicts.ptr, ctypes.c_void_p(d_verdicts.ptr.value + 4 * n)))
        E.dnf_decrypt_one_uk_dev(eng, n, N_CLASSES, b["d_class"], k["d_s1"], k["d_skip"], k["d_nu1"], k["lines"], b["d_g1"], b["d_g2"], b["d_lead"], d_out)
        raw = eng.download(d_out, n * 384)
    finally:
        eng.set_pairing_mode(0)
    got = [raw[384 * i:384 * i + 384] for i in range(n)]
    bad = [i for i in range(n) if got[i] != b["expect"][i]]
    assert not bad, (n, family, bad[:8])
    v = eng.download(d_verdicts, 8 * n)
    fail = [int.from_bytes(v[4 * i:4 * i + 4], "little") for i in range(n)]
    count = [int.from_bytes(v[4 * (n + i):4 * (n + i) + 4], "little") for i in range(n)]
    assert fail == [0] * n
    assert count == b["walked"], (n, family)          # pairs 1 and 3 walk; pairs 0 and 2 replay the key's lines


def test_arguments_are_checked(eng, world):
    k, b = world["key"], world["batches"][1]
    d_out = eng.alloc(384)
    args = [b["d_class"], k["d_s1"], k["d_skip"], k["d_nu1"], k["lines"], b["d_g1"], b["d_g2"], b["d_lead"], d_out]
    for missing in (0, 1, 2, 3, 4, 5, 6, 8):
        a = list(args)
        a[missing] = None
        with pytest.raises(Exception):
            E.dnf_decrypt_one_uk_dev(eng, 1, N_CLASSES, *a)
    with pytest.raises(Exception):          # more classes than the lines have blocks for
        E.dnf_decrypt_one_uk_dev(eng, 1, N_CLASSES + 1, *args)
    E.dnf_decrypt_one_uk_dev(eng, 0, N_CLASSES, *args)          # nothing to do
