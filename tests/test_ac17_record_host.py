"""The reader of one AC17 ciphertext record (rabe_amd/csrc/host/ac17_record.h: check_offsets, Cursor, read_record) on the CPU:
tests/hostsim/ac17_record_check.cpp is built once plain and once with the address and undefined-behaviour sanitizers -- a program of its own,
nothing loaded into Python -- and run.  Its cases: a CP and a KP record of 3 rows, every prefix of each, every u32 field overwritten by 0, 3,
0xffffffff and twice the record's length; the reader throws RabeError or its View lies inside the record.  No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "ac17_record_check.cpp")
HDRS = [os.path.join(ROOT, "rabe_amd", "csrc", "host", h) for h in ("ac17_record.h", "bytes.h")]


def build_program(sanitize):
    exe = os.path.join(ROOT, "build", "ac17_record_check" + ("_" + sanitize.replace(",", "_") if sanitize else ""))
    if os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in [SRC] + HDRS):
        return exe
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    extra = ["-fsanitize=" + sanitize, "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["hipcc", "-O2", "-std=c++17", "-x", "hip", "--cuda-host-only", "-o", exe, SRC] + extra, check=True, timeout=600)
    return exe


@pytest.mark.parametrize("sanitize", ["", "address,undefined"], ids=["plain", "asan-ubsan"])
def test_the_reader_stays_inside_its_record(sanitize):
    res = subprocess.run([build_program(sanitize)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert res.returncode == 0, res.stderr.decode()
    assert int(res.stdout.decode().split()[0]) > 3000          # both records, every prefix
