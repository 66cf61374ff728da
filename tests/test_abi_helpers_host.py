"""The pure helpers of the C interface (rabe_amd/csrc/host/abi_helpers.h: attr_sets, record_span, key_ptrs) on the CPU:
tests/hostsim/abi_helpers_check.cpp is built once plain and once with the address and undefined-behaviour sanitizers -- a program of its own,
nothing loaded into Python -- and run.  Its cases: no list at all, a list of zero names between two non-empty ones, counts that sum to the
flat array's length exactly, record_span on decreasing offsets, on an offset past the blob and with n = 0.  No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "abi_helpers_check.cpp")
HDR = os.path.join(ROOT, "rabe_amd", "csrc", "host", "abi_helpers.h")


def build_program(sanitize):
    exe = os.path.join(ROOT, "build", "abi_helpers_check" + ("_" + sanitize.replace(",", "_") if sanitize else ""))
    if os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in (SRC, HDR)):
        return exe
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    extra = ["-fsanitize=" + sanitize, "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["hipcc", "-O2", "-std=c++17", "-x", "hip", "--cuda-host-only", "-o", exe, SRC] + extra, check=True, timeout=600)
    return exe


@pytest.mark.parametrize("sanitize", ["", "address,undefined"], ids=["plain", "asan-ubsan"])
def test_the_helpers_pass_their_cases(sanitize):
    res = subprocess.run([build_program(sanitize)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert res.returncode == 0, res.stderr.decode()
    assert int(res.stdout.decode().split()[0]) == 21          # every check ran
