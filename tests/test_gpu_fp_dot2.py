"""GPU: the two-term Montgomery dot product that closes the G1 mixed addition (rabe_amd/csrc/bn254/fp.h: mont_dot2_raw, on the device the
generated mont_dot2_fp), and the fixed-base walks that run through it, byte for byte against Python integers and oracle.bn254.

* the routine itself through the diagnostic entry rhip_fp_dot2: operands whose MONTGOMERY residues -- the limbs in the registers -- are
  extreme (tests/dot2_host.py: edge_residues), in all four positions, plus one wave of random ones;
* the AC17 row kernel at 1, 63, 64, 65 and 257 rows (items of 1, 2 and 5 rows) on the 16-bit table and on the signed 20-bit table of g,
  with a row scalar of 0 and one of r - 1 in every launch;
* the 8-bit table at the same row counts through rhip_g1_table_mul: an AC17 key always carries its 16-bit table, so the row kernel
  never walks the 8-bit one -- k_table_mul_g1 is the kernel that does, through the same table_mul_g1 and the same addition;
* one AC17 encrypt -> decrypt round trip at 64 items."""
import random

import pytest

from oracle import bn254 as bn
from oracle import policy as pol
from oracle import schemes as sch
from oracle.tape import SeededRng
from tests import ac17_host as host
from tests import dot2_host as dh
from tests import test_gpu_g1_walk_forms as wf

pytestmark = pytest.mark.gpu
R = bn.R
RND = random.Random(0xD072)
ROW_COUNTS = (1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def env():
    from rabe_amd import Engine
    from rabe_amd import engine as E
    eng = Engine(0)
    pk, msk = sch.ac17_setup(SeededRng(0xD072))
    dpk = {w: E.Ac17Pk(eng, bn.g1_to_le(pk["g"]), [bn.g2_to_le(x) for x in pk["h_a"]], [bn.gt_to_le(x) for x in pk["e_gh_ka"]]) for w in (16, 20)}
    dpk[20].set_g_window(20)
    yield eng, E, pk, msk, dpk, wf.Oracle(pk["g"])
    for h in dpk.values():
        h.destroy()
    eng.close()


def test_dot2_on_device_against_python_integers(env):
    eng = env[0]
    rinv = pow(1 << 256, -1, bn.P)
    canon = lambda m: m * rinv % bn.P                          # the canonical value whose Montgomery residue is exactly m
    edge = [canon(m) for m in dh.edge_residues(bn.P, RND, n_random=40)]
    quads = []
    for e in edge:
        for pos in range(4):
            q = [RND.choice(edge) for _ in range(4)]
            q[pos] = e
            quads.append(q)
        b = RND.randrange(1, bn.P)
        quads += [[e, e, e, e], [e, bn.P - 1, bn.P - 1, e], [e, b, (bn.P - e) % bn.P, b]]      # the last: a b + (-a) b = 0, not p
    quads += [[RND.randrange(bn.P) for _ in range(4)] for _ in range(64)]          # one wave of random operands
    got = eng.fp_dot2(*[[dh.le(q[j]) for q in quads] for j in range(4)])
    assert got == [dh.le((q[0] * q[1] + q[2] * q[3]) % bn.P) for q in quads]
    assert bytes(32) in got


def row_scalars(n_rows):
    """3 n_rows scalars: 0 and r - 1 first (slots 0 and 1 of row 0), the edge words of the signed walk, random ones"""
    edge = [k % R for k, _why in wf.edge_scalars()]
    rnd = random.Random(n_rows)
    ks = [0, R - 1] + edge + [rnd.randrange(R) for _ in range(3 * n_rows)]
    return ks[:3 * n_rows]


def items_of(n_rows):
    """row offsets of items of 1, 2 and 5 rows (cycled; the last item takes what is left)"""
    off, sizes = [0], (1, 2, 5)
    while off[-1] < n_rows:
        off.append(min(n_rows, off[-1] + sizes[(len(off) - 1) % 3]))
    return off


@pytest.mark.parametrize("n_rows", ROW_COUNTS)
def test_ac17_rows_on_the_16_bit_and_signed_20_bit_tables(env, n_rows):
    eng, E, _pk, _msk, dpk, ora = env
    rnd = random.Random(1000 + n_rows)
    ks = row_scalars(n_rows)
    off = items_of(n_rows)
    n_items = len(off) - 1
    s = [(rnd.randrange(1, R), rnd.randrange(1, R)) for _ in range(n_items)]
    A = []
    for i in range(n_items):
        s0, s1 = s[i]
        for t in range(off[i], off[i + 1]):
            for l in range(3):
                a1 = rnd.randrange(R)
                A += [wf.word((ks[3 * t + l] - s1 * a1) * bn.fr_inv(s0) % R), wf.word(a1)]
    want = [ora.mul(k) for k in ks]
    assert want[0] == bytes(64) and want[1] == bn.g1_to_le(bn.g1_neg(env[2]["g"]))
    args = (n_items, b"".join(A), off[:-1], off, [wf.word(x) for it in s for x in it])
    c16, c0_16, cp_16 = wf.encrypt_rows(eng, E, dpk[16], *args)
    assert wf.differing(c16, want) == []
    c20, c0_20, cp_20 = wf.encrypt_rows(eng, E, dpk[20], *args)
    assert wf.differing(c20, want) == []
    assert (c0_20, cp_20) == (c0_16, cp_16)


def test_the_8_bit_table_at_the_same_row_counts(env):
    eng, _E, pk, _msk, _dpk, ora = env
    tab = eng.g1_table(bn.g1_to_le(pk["g"]))
    try:
        for n_rows in ROW_COUNTS:
            ks = row_scalars(n_rows)
            assert wf.differing(tab.mul([wf.word(k) for k in ks]), [ora.mul(k) for k in ks]) == []
    finally:
        tab.destroy()


def test_ac17_round_trip_at_64_items(env):
    eng, E, pk, msk, dpk, _ora = env
    policy, attrs = '"A" and "B"', ["A", "B"]
    pi, A = host.policy_table(policy, pol.HUMAN)
    n, n_rows = 64, len(pi)
    rng = SeededRng(64)
    s = [(rng.fr(), rng.fr()) for _ in range(n)]
    msgs = [bn.gt_pow(pk["e_gh_ka"][0], rng.fr_nonzero()) for _ in range(4)]
    msg_bytes = [bn.gt_to_le(msgs[i % 4]) for i in range(n)]
    sk = sch.ac17_cp_keygen(msk, attrs, rng)
    ok, ct_sel, sk_sel = host.decrypt_selection(sk["attr"], pi, policy, pol.HUMAN)
    assert ok
    row_off = [n_rows * i for i in range(n + 1)]
    dc0, dc, dcp = eng.alloc(n * 384), eng.alloc(n * n_rows * 192), eng.alloc(n * 384)
    E.ac17_encrypt_dev(eng, dpk[20], n, eng.upload(A), eng.upload_u32([0] * n), eng.upload_u32(row_off), n * n_rows,
                       eng.upload(b"".join(host.le(x) for it in s for x in it)), eng.upload(b"".join(msg_bytes)), dc0, dc, dcp)
    dout = eng.alloc(n * 384)
    # one secret key for all 64 items; every item brings its own copy of the selection
    E.ac17_decrypt_dev(eng, n, dc0, dc, eng.upload_u32(row_off), dcp,
                       eng.upload(b"".join(bn.g2_to_le(x) for x in sk["sk"]["k_0"])),
                       eng.upload(b"".join(bn.g1_to_le(p) for _, vec in sk["sk"]["k"] for p in vec)),
                       eng.upload_u32([0, len(attrs)]), eng.upload(b"".join(bn.g1_to_le(p) for p in sk["sk"]["k_p"])),
                       eng.upload_u32([0] * n), eng.upload_u32(list(ct_sel) * n), eng.upload_u32([len(ct_sel) * i for i in range(n + 1)]),
                       eng.upload_u32(list(sk_sel) * n), eng.upload_u32([len(sk_sel) * i for i in range(n + 1)]), dout)
    back = eng.download(dout, n * 384)
    assert [back[384 * i:384 * i + 384] for i in range(n)] == msg_bytes
