"""The LSW row routine (rabe_amd/csrc/bn254/lsw_rows.h: what a lane of k_lsw_enc_rows runs, host + device code) on the CPU against the
oracle's point arithmetic, with the scalar cases and the degenerate keys of tests/lsw_row_cases.py: tests/hostsim/lsw_enc_rows.cpp is a
stand-alone program compiled from the engine's headers, which also restates today's path (four window walks, each converted, plus the
addition kernel) and counts the Montgomery multiplications of both.  No GPU needed."""
import os
import re
import subprocess

import pytest

from tests import lsw_row_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "lsw_enc_rows.cpp")
EXE = os.path.join(ROOT, "build", "lsw_enc_rows")
HDR_DIR = os.path.join(ROOT, "rabe_amd", "csrc", "bn254")


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


def le(x):
    return int(x).to_bytes(32, "little")


def run(call):
    """(exit code, fused bytes, four-walk bytes, stderr) of one call's rows"""
    data = b"".join(call.key.points()) + b"".join(le(h) + le(secret) + le(sx) for _i, h, secret, sx in call.rows())
    res = subprocess.run([build_program()], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = res.stdout
    assert len(out) == 384 * call.n_rows, res.stderr.decode()
    fused = b"".join(out[384 * t:384 * t + 192] for t in range(call.n_rows))
    four = b"".join(out[384 * t + 192:384 * t + 384] for t in range(call.n_rows))
    return res.returncode, fused, four, res.stderr.decode()


def check(call):
    rc, fused, four, err = run(call)
    want = call.want_bytes()
    for t in range(call.n_rows):
        assert fused[192 * t:192 * t + 192] == want[192 * t:192 * t + 192], (call.key.name, t, call.note[t])
    assert four == want and rc == 0, err
    return err


@pytest.fixture(scope="module")
def keys():
    return {k.name: k for k in lc.keys()}


def test_scalar_cases_against_the_oracle(keys):
    call = lc.scalar_call(keys["random"], 65, "host")
    assert set(lc.KINDS) <= set(call.note)
    check(call)


@pytest.mark.parametrize("name", ["random", "same", "opposite"])
def test_e5_special_cases_against_the_oracle(keys, name):
    call = lc.special_call(keys[name])
    lc.check_special(call)
    check(call)


def test_the_fused_row_takes_fewer_multiplications(keys):
    """the instrumented count per row (docs/kernels.md quotes it): random scalars, so every walk has its 16 digits"""
    call = lc.Call(keys["random"])
    import random
    rnd = random.Random("lsw mul count")
    for _ in range(8):
        call.add_item(rnd.randrange(1, lc.R), [rnd.randrange(1, lc.R)], [rnd.randrange(1, lc.R)])
    err = check(call)
    m = re.search(r"muls_per_row fused=([0-9.]+) four_walks_plus_add=([0-9.]+)", err)
    assert m, err
    fused, four = float(m.group(1)), float(m.group(2))
    print("Montgomery multiplications per row: fused %.1f, four walks + addition %.1f" % (fused, four))
    assert fused < four
