"""The bounds of a device-planned Miller launch (rabe_amd/csrc/miller_plan.h: rb_miller_plan_bounds, what run_pair_lists_mode of engine_jobs.hip
sizes its plan, work list and workspace with) on the CPU: tests/hostsim/miller_plan_bounds.cpp is built once plain and once with the address
and undefined-behaviour sanitizers -- a program of its own, nothing loaded into Python -- and run.  It checks, for the ragged shapes of
tests/decrypt_launch_cases.py and for the extremes (one item, one pair, max_pairs of 1, of 64 and above, total_pairs just under
n_items * max_pairs, the largest counts 32-bit offsets allow): 1 <= c_lo <= c_hi <= 64, the work list and the workspace hold what any C of
[c_lo, c_hi] can produce, and no size computation wraps (each is recomputed in 128 bits).  No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "miller_plan_bounds.cpp")
HDR = os.path.join(ROOT, "rabe_amd", "csrc", "miller_plan.h")


def build_program(sanitize):
    exe = os.path.join(ROOT, "build", "miller_plan_bounds" + ("_" + sanitize.replace(",", "_") if sanitize else ""))
    if os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in (SRC, HDR)):
        return exe
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    extra = ["-fsanitize=" + sanitize, "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["hipcc", "-O2", "-std=c++17", "-x", "hip", "--cuda-host-only", "-o", exe, SRC] + extra, check=True, timeout=600)
    return exe


@pytest.mark.parametrize("sanitize", ["", "address,undefined"], ids=["plain", "asan-ubsan"])
def test_the_bounds_hold(sanitize):
    res = subprocess.run([build_program(sanitize)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert res.returncode == 0, res.stderr.decode()
    assert int(res.stdout.decode().split()[0]) > 1000          # every family of checks ran
