#!/usr/bin/env python3
"""Writes tests/golden/packed_abi_contract.json: the records tests/test_gpu_packed_abi_contract.py expects, from the table of
tests/packed_abi_cases.py run on a plain host and on the device group [0, 0].  Needs a GPU.

Run it on the commit whose behaviour is to be kept, BEFORE the change that must not alter it, and commit the file with that change:
    python tools/record_packed_abi_contract.py [output path]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from rabe_amd import build
    from rabe_amd import hostlib as hl
    from tests import packed_abi_cases as cases
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "packed_abi_contract.json")
    hosts = {"single": hl.Host(0), "group": hl.Host(devices=[0, 0])}
    entries, keep = cases.build_entries(hosts["single"])
    packed = sorted(s for s in build.declared_symbols() if s.startswith("rabe_") and s.endswith("_packed"))
    assert sorted(entries) == packed, sorted(set(entries) ^ set(packed))
    golden = {}
    for fn in packed:
        golden[fn] = {kind: cases.run_entry(hosts[kind], entries[fn]) for kind in ("single", "group")}
        print(fn, {kind: [r["rc"] for r in golden[fn][kind].values()] for kind in golden[fn]}, flush=True)
    del keep
    for h in hosts.values():
        h.close()
    write(golden, out)


def write(golden, out):
    """one line per case; under "group" only the cases whose record differs from the plain host's (the test reads the others from "single")"""
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    small = {fn: {"single": g["single"], "group": {c: r for c, r in g["group"].items() if r != g["single"][c]}} for fn, g in golden.items()}
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(
            '"%s": {\n' % fn + ",\n".join(
                ' "%s": {\n' % kind + ",\n".join('  "%s": %s' % (case, json.dumps(rec, separators=(",", ":"))) for case, rec in small[fn][kind].items()) + "\n }"
                for kind in small[fn]) + "\n}"
            for fn in sorted(small)) + "\n}\n")
    assert json.load(open(out)) == small
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
