#!/usr/bin/env python3
"""Writes tests/golden/encrypt_tail_contract.json: the records tests/test_gpu_encrypt_tail_contract.py expects, from the table of
tests/encrypt_tail_cases.py.  Needs a GPU.

Run it on the commit whose behaviour is to be kept, BEFORE the change that must not alter it, and commit the file with that change:
    python tools/record_encrypt_tail_contract.py [output path]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from rabe_amd import hostlib as hl
    from tests import encrypt_tail_cases as cases
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "encrypt_tail_contract.json")
    host = hl.Host(0)
    entries, keep = cases.build_entries(host)
    golden = {}
    for name in sorted(entries):
        golden[name] = cases.run(host, entries[name])
        print(name, golden[name]["rc"], golden[name]["err"], flush=True)
    del keep
    host.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join('"%s": %s' % (name, json.dumps(rec, separators=(",", ":"), sort_keys=True)) for name, rec in golden.items()) + "\n}\n")
    assert json.load(open(out)) == golden
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
