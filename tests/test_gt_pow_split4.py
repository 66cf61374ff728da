"""gt_pow_split4 (the Gt power over a four-way Frobenius split that k_gt_pow_rows runs per lane, rabe_amd/csrc/bn254/gtpow4.h) against
gt_pow_window of the same headers and against the oracle, on the CPU: tests/hostsim/gt_pow_split4.cpp is a stand-alone program compiled
from the engine's headers.  No GPU needed.

`python tests/test_gt_pow_split4.py` prints the instrumented Fp-multiplication counts of the two routines (docs/kernels.md)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import bn254 as bn  # noqa: E402
from tests import gt_pow_cases as gc  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hostsim", "gt_pow_split4.cpp")
HDR_DIR = os.path.join(ROOT, "rabe_amd", "csrc", "bn254")


def build_program(count=False):
    exe = os.path.join(ROOT, "build", "gt_pow_split4" + ("_count" if count else ""))
    deps = [SRC] + [os.path.join(HDR_DIR, f) for f in os.listdir(HDR_DIR)]
    if os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in deps):
        return exe
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    # RABE_HOST_SANITIZE=address,undefined builds the program (host code, its own main) with those sanitizers
    san = os.environ.get("RABE_HOST_SANITIZE")
    extra = ["-fsanitize=" + san, "-fno-sanitize-recover=all", "-g"] if san else []
    if count:
        extra.append("-DRB_COUNT_MULS")
    subprocess.run(["hipcc", "-O2", "-std=c++17", "-x", "hip", "--cuda-host-only", "-o", exe, SRC] + extra, check=True, timeout=600)
    return exe


def record(a, k, invert, mul):
    flags = (1 if invert else 0) | (2 if mul is not None else 0)
    return bn.gt_to_le(a) + bn.gt_to_le(mul if mul is not None else bn.GT_ONE) + gc.le(k) + flags.to_bytes(4, "little")


def run(records, count=False):
    exe = build_program(count)
    res = subprocess.run([exe], input=b"".join(records), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out = res.stdout
    assert len(out) == 768 * len(records), res.stderr.decode()
    pairs = [(out[768 * i:768 * i + 384], out[768 * i + 384:768 * i + 768]) for i in range(len(records))]
    return res.returncode, pairs, res.stderr.decode()


def test_every_scalar_on_every_base_agrees_with_the_window_routine():
    """all 46 scalars x 5 bases, plain: the program compares the two routines; the oracle decides the special scalars on e(g1, g2) and
    every scalar's answer on the base 1"""
    bases = gc.bases()
    cases = [(a, k) for a in bases for k in gc.SCALARS]
    rc, got, err = run([record(a, k, False, None) for a, k in cases])
    assert rc == 0, err
    assert all(s == w for s, w in got)
    for (a, k), (s, _w) in zip(cases, got):
        if a is bases[0]:
            assert s == bn.gt_to_le(bn.GT_ONE)
        elif a is bases[1] and k in gc.SPECIAL_SCALARS:
            assert s == gc.expected(a, k, False, None), hex(k)
    assert len(set(s for s, _ in got)) > len(cases) // 2          # real results, not a wall of ones


def test_invert_flag_and_mul_operand_against_the_oracle():
    bases = gc.bases()
    cases = []
    for i, k in enumerate(gc.SCALARS):
        a, mul = bases[1 + i % 4], bases[1 + (i + 1) % 4]
        cases += [(a, k, True, None), (a, k, False, mul), (a, k, True, mul)]
    cases += [(bases[0], gc.LAMBDA, True, bases[2]), (bases[2], 0, True, bases[0])]
    rc, got, err = run([record(*c) for c in cases])
    assert rc == 0, err
    assert all(s == w for s, w in got)
    for c, (s, _w) in list(zip(cases, got))[::5] + list(zip(cases, got))[-2:]:
        assert s == gc.expected(*c)
    # a^-k * a^k = 1 through the program's own outputs: k and its inverse power on one base, the second with the first as `mul`
    a, k = bases[3], gc.RANDOM_SCALARS[1]
    _rc, first, _ = run([record(a, k, False, None)])
    rc, second, err = run([record(a, k, True, bn.gt_from_le(first[0][0]))])
    assert rc == 0, err
    assert second[0][0] == bn.gt_to_le(bn.GT_ONE)


def test_the_program_refuses_a_truncated_record():
    """the checker itself: a short read cannot pass as agreement"""
    exe = build_program()
    res = subprocess.run([exe], input=bytes(803), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert res.returncode == 2


if __name__ == "__main__":
    recs = [record(a, k, False, None) for a in gc.bases()[1:] for k in gc.RANDOM_SCALARS if k < bn.R]
    rc, _got, err = run(recs, count=True)
    print(err.strip())
    sys.exit(rc)
