#!/usr/bin/env python3
"""Writes tests/golden/decrypt_launch_contract.json: the records tests/test_gpu_decrypt_launch_contract.py expects, from the table of
tests/decrypt_launch_cases.py -- every decrypt entry point of the device library in pairing modes 0 and 99.  Needs a GPU; the launch counts of
mode 0 follow the device's compute-unit count (the kernel families are chosen by it), so the file is for the device named in its header.

Run it on the commit whose behaviour is to be kept, BEFORE the change that must not alter it, and commit the file with that change:
    python tools/record_decrypt_launch_contract.py [output path]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from rabe_amd.engine import Engine
    from tests import decrypt_launch_cases as cases
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "decrypt_launch_contract.json")
    eng = Engine(0)
    n_cu, name = eng.device_info()
    world = cases.World(eng)
    golden = {}
    for entry, shape in cases.CASES:
        rec = cases.run_case(world, entry, shape)
        golden.setdefault(entry, {})[shape] = rec
        print(entry, shape, {mode: (r["rc"], sum(r["launches"].values())) for mode, r in rec.items()}, flush=True)
    eng.close()
    write({"device": name, "compute_units": n_cu}, golden, out)


def write(header, golden, out):
    """one line per (case, mode)"""
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write('{\n"header": %s,\n"cases": {\n' % json.dumps(header, separators=(",", ":")) + ",\n".join(
            '"%s": {\n' % entry + ",\n".join(
                ' "%s": {\n' % shape + ",\n".join('  "%s": %s' % (mode, json.dumps(rec, separators=(",", ":"))) for mode, rec in modes.items()) + "\n }"
                for shape, modes in shapes.items()) + "\n}"
            for entry, shapes in golden.items()) + "\n}\n}\n")
    assert json.load(open(out)) == {"header": header, "cases": golden}
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
