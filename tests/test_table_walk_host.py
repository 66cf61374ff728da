"""The fixed-base table walks (rabe_amd/csrc/bn254/table_walk.h: digit cutters, signed recoder, table geometry, the loops) on the
CPU, on exact integers: tests/hostsim/table_walk.cpp runs the header's own code and checks, for every scalar it is given, that the
digits of each walk sum to the scalar, stay in range, index inside their table and leave no carry.  This file makes the scalars: the
edge constructions for every window width the engine uses (8, 16; signed 8 .. 14; wide 20, 24, 26) and seeded random ones.  No GPU
needed."""
import os
import random
import subprocess

from tests import walk_scalars as ws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "table_walk.cpp")
SAN = os.environ.get("RABE_HOST_SANITIZE")          # address,undefined: the program (host code, its own main) built with those sanitizers
EXE = os.path.join(ROOT, "build", "table_walk" + ("_" + SAN.replace(",", "_") if SAN else ""))          # one executable per setting
HDR_DIR = os.path.join(ROOT, "rabe_amd", "csrc", "bn254")
WIDTHS = [8, 9, 10, 11, 12, 13, 14, 16, 20, 24, 26]


def build_program():
    deps = [SRC] + [os.path.join(HDR_DIR, f) for f in os.listdir(HDR_DIR)]
    if os.path.exists(EXE) and all(os.path.getmtime(d) <= os.path.getmtime(EXE) for d in deps):
        return EXE
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    extra = ["-fsanitize=" + SAN, "-fno-sanitize-recover=all", "-g"] if SAN else []
    subprocess.run(["hipcc", "-O2", "-std=c++17", "-x", "hip", "--cuda-host-only", "-o", EXE, SRC] + extra, check=True, timeout=600)
    return EXE


def run(scalars):
    res = subprocess.run([build_program()], input=b"".join(int(k).to_bytes(32, "little") for k in scalars), stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300)
    return res.returncode, res.stdout.decode().split(), res.stderr.decode()


def test_every_walk_reconstructs_the_edge_and_random_scalars():
    rnd = random.Random("table walks")
    ks = ws.common() + [k for w in WIDTHS for k in ws.edge(w) + ws.dense(w)] + [rnd.randrange(ws.R) for _ in range(400)]
    assert len(set(ks)) > 400 + 7 and all(0 <= k < ws.R for k in ks)
    rc, out, err = run(ks)
    assert rc == 0, err
    assert int(out[0]) == len(ks) and int(out[1]) > 100 * len(ks)          # every scalar went through all the walks


def test_the_carry_chain_scalars_are_what_they_claim():
    """in integers: every digit at half + 1 makes every signed digit below the top negative, every digit at half none"""
    for w in WIDTHS:
        half, n = 1 << (w - 1), (254 + w - 1) // w
        for base, negative in ((half, False), (half + 1, True)):
            k, carry, signs = sum(base << (w * i) for i in range(n - 1)), 0, []
            for i in range(n):
                raw = ((k >> (w * i)) & ((1 << w) - 1)) + carry
                carry = 1 if raw > half else 0
                signs.append(carry == 1)
            assert k in ws.edge(w) and signs[:n - 1] == [negative] * (n - 1) and carry == 0


def test_zero_takes_no_step_and_a_truncated_record_is_refused():
    rc, out, err = run([0])
    assert rc == 0 and out == ["1", "0"], err
    res = subprocess.run([build_program()], input=bytes(33), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert res.returncode == 2
