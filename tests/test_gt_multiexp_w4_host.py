"""The Gt multi-exponentiation over width-4 signed windows (rabe_amd/csrc/bn254/gtmexp4.h: the recoding, the odd-power table, the chunk walk
and the finish that rhip_gt_multiexp_rows runs per lane) on the CPU: tests/hostsim/gt_multiexp_w4.cpp is a stand-alone program compiled from
the engine's headers with -DRB_COUNT_MULS.  It also runs the plain NAF walk of k_gt_multiexp_partial + k_gt_lead on the same inputs, so the
instrumented Fp-multiplication counts of the two are compared here, routine against routine.  No GPU needed.

`python tests/test_gt_multiexp_w4_host.py` prints the counts quoted in docs/kernels.md."""
import os
import random
import re
import struct
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import bn254 as bn  # noqa: E402
from tests import gt_pow_cases as gc  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hostsim", "gt_multiexp_w4.cpp")
HDR_DIR = os.path.join(ROOT, "rabe_amd", "csrc", "bn254")
EXE = os.path.join(ROOT, "build", "gt_multiexp_w4_count")
RND = random.Random(0x6d657870)


def build_program():
    deps = [SRC] + [os.path.join(HDR_DIR, f) for f in os.listdir(HDR_DIR)]
    if os.path.exists(EXE) and all(os.path.getmtime(d) <= os.path.getmtime(EXE) for d in deps):
        return EXE
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    # RABE_HOST_SANITIZE=address,undefined builds the program (host code, its own main) with those sanitizers
    san = os.environ.get("RABE_HOST_SANITIZE")
    extra = ["-fsanitize=" + san, "-fno-sanitize-recover=all", "-g"] if san else []
    subprocess.run(["hipcc", "-O2", "-std=c++17", "-DRB_COUNT_MULS", "-x", "hip", "--cuda-host-only", "-o", EXE, SRC] + extra, check=True, timeout=600)
    return EXE


def run(payload):
    res = subprocess.run([build_program()], input=payload, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    return res.returncode, res.stdout, res.stderr.decode()


# ------------------------------------------------------------------------------------------------------------------------------ recoding
RECODE_SCALARS = gc.SCALARS + [0, 1, bn.R - 1, bn.R, (1 << 256) - 1, 7, 8, 9] + [15 * 16 ** j for j in range(0, 63)]


def digits_of(words):
    """{position: signed digit} of the 32 digit words"""
    out = {}
    for w, word in enumerate(words):
        for b in range(8):
            nib = (word >> (4 * b)) & 15
            if nib:
                assert nib & 7, "a sign bit without a magnitude"
                out[8 * w + b] = -(nib & 7) if nib & 8 else (nib & 7)
    return out


def test_recoding_of_every_scalar():
    """odd digits within +-7, non-zero digits at least four positions apart, and sum d_j 2^j = k mod r as an exact integer (-k with the flag)"""
    cases = [(k, inv) for k in RECODE_SCALARS for inv in (False, True)]
    rc, out, err = run(struct.pack("<I", 0) + b"".join(gc.le(k) + struct.pack("<I", 1 if inv else 0) for k, inv in cases))
    assert rc == 0, err
    assert len(out) == 128 * len(cases)
    seen_top = 0
    for i, (k, inv) in enumerate(cases):
        d = digits_of(struct.unpack("<32I", out[128 * i:128 * i + 128]))
        pos = sorted(d)
        assert all(v % 2 == 1 and -7 <= v <= 7 for v in d.values()), hex(k)
        assert all(b - a >= 4 for a, b in zip(pos, pos[1:])), hex(k)
        assert not pos or pos[-1] <= 254, hex(k)
        value = sum(v << p for p, v in d.items())
        want = -(k % bn.R) if inv else k % bn.R
        assert (value - want) % bn.R == 0, hex(k)          # congruent to k (to -k when inverted), in exact integers
        assert value in (want, want - bn.R, want + bn.R) and 2 * abs(value) <= bn.R, hex(k)          # the representative of smaller magnitude
        if k % bn.R == 0:
            assert not d
        seen_top = max(seen_top, pos[-1] if pos else 0)
    assert seen_top >= 252          # scalars near r / 2 are among the cases: the longest chains the shortened form leaves


# ------------------------------------------------------------------------------------------------------------------- products and counts
def item_record(terms, chunk, invert, mul):
    flags = (1 if invert else 0) | (2 if mul is not None else 0)
    body = struct.pack("<III", len(terms), chunk, flags) + bn.gt_to_le(mul if mul is not None else bn.GT_ONE)
    return body + b"".join(bn.gt_to_le(a) + gc.le(k) for a, k in terms)


def expected(terms, invert, mul):
    acc = mul if mul is not None else bn.GT_ONE
    for a, k in terms:
        acc = bn.gt_mul(acc, bn.gt_pow(a, (-k if invert else k) % bn.R))
    return bn.gt_to_le(acc)


def term_lists():
    """items of 1, 2, 3 and 13 terms; among the bases the identity, a pair (x, k), (x, r - k) that cancels, the same base twice"""
    b = gc.bases()
    k = [RND.randrange(1, bn.R) for _ in range(16)]
    return [
        [(b[1], k[0])],
        [(b[0], k[1])],                                                    # the identity alone
        [(b[2], k[2]), (b[2], bn.R - k[2])],                               # cancels to 1
        [(b[3], k[3]), (b[3], k[4])],                                      # the same base twice
        [(b[1], k[5]), (b[0], k[6]), (b[4], (1 << 256) - 1)],
        [(b[1 + j % 4], k[j]) for j in range(11)] + [(b[0], k[11]), (b[2], 0)],
    ]


def test_products_against_the_oracle():
    cases = []
    for terms in term_lists():
        for chunk in (1, 2, 13):
            for invert in (False, True):
                for mul in (None, gc.bases()[4]):
                    cases.append((terms, chunk, invert, mul))
    rc, out, err = run(struct.pack("<I", 1) + b"".join(item_record(*c) for c in cases))
    assert rc == 0, err          # the windowed routine and the NAF walk agree on every item
    assert len(out) == 768 * len(cases)
    want = {}
    for i, (terms, chunk, invert, mul) in enumerate(cases):
        key = (id(terms), invert, mul is not None)
        if key not in want:
            want[key] = expected(terms, invert, mul)
        assert out[768 * i:768 * i + 384] == want[key], (len(terms), chunk, invert, mul is not None)
    one = bn.gt_to_le(bn.GT_ONE)
    assert out[768 * 24:768 * 24 + 384] == one          # the cancelling pair, C = 1, plain


def counts(err):
    rows = []
    for line in err.splitlines():
        if line.startswith("muls "):
            rows.append({k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", line)})
    return rows


def count_run():
    b = gc.bases()
    terms = [(b[1 + j % 4], RND.randrange(1 << 253, bn.R)) for j in range(13)]          # 13 random 254-bit scalars
    rc, _out, err = run(struct.pack("<I", 1) + item_record(terms, 13, True, b[2]) + item_record(terms, 1, True, b[2]))
    assert rc == 0, err
    rows = counts(err)
    assert [r["C"] for r in rows] == [13, 1]
    return rows


def test_fewer_fp_multiplications_than_the_naf_walk():
    """per item of 13 terms, at C = 13 and at C = 1: the windowed routine (tables and finish included) against the NAF walk on the same
    scalars, both instrumented in the one program"""
    for r in count_run():
        assert r["w4"] == r["w4_table"] + r["w4_walk"] + r["w4_finish"] and r["naf"] == r["naf_walk"] + r["naf_finish"]
        assert r["w4"] < r["naf"], r
        assert r["w4_walk"] < r["naf_walk"], r


def test_the_program_refuses_malformed_input():
    """the checker itself: a short read cannot pass as agreement"""
    assert run(b"")[0] == 2
    assert run(struct.pack("<I", 1) + item_record(term_lists()[0], 1, False, None)[:-1])[0] == 2
    assert run(struct.pack("<I", 0) + bytes(35))[0] == 2


if __name__ == "__main__":
    for r in count_run():
        per_term = (r["w4_walk"], r["naf_walk"])
        print("13 terms, C = %2d: windowed %6d (table %5d, walk %6d, finish %5d)   NAF walk %6d (walk %6d, finish %5d)" % (
            r["C"], r["w4"], r["w4_table"], r["w4_walk"], r["w4_finish"], r["naf"], r["naf_walk"], r["naf_finish"]))
