"""The source table of the record writers (rabe_amd/csrc/host/record_layout.h: RecordSources, with RecordLayout and record_offsets) on the CPU:
tests/hostsim/record_sources_check.cpp is built once plain and once with the address and undefined-behaviour sanitizers -- a program of its
own, nothing loaded into Python -- and run.  Its cases: n = 0, one item, three items over rows [1, 2, 1], the three indexing kinds in one list,
both prefix-array types, a row offset of 3e9 at stride 384 (no 32-bit wrap), arrays of the wrong length refused, and a layout's map applied to
small host buffers through the table against records laid out by hand.  No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "record_sources_check.cpp")
HDRS = [os.path.join(ROOT, "rabe_amd", "csrc", "host", h) for h in ("record_layout.h", "bytes.h")]


def build_program(sanitize):
    exe = os.path.join(ROOT, "build", "record_sources_check" + ("_" + sanitize.replace(",", "_") if sanitize else ""))
    if os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in [SRC] + HDRS):
        return exe
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    extra = ["-fsanitize=" + sanitize, "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["hipcc", "-O2", "-std=c++17", "-x", "hip", "--cuda-host-only", "-o", exe, SRC] + extra, check=True, timeout=600)
    return exe


@pytest.mark.parametrize("sanitize", ["", "address,undefined"], ids=["plain", "asan-ubsan"])
def test_the_source_table_passes_its_cases(sanitize):
    res = subprocess.run([build_program(sanitize)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert res.returncode == 0, res.stderr.decode()
    assert int(res.stdout.decode().split()[0]) == 39          # every check ran
