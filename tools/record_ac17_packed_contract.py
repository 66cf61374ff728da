#!/usr/bin/env python3
"""Writes tests/golden/ac17_packed_contract.json: the records tests/test_gpu_ac17_packed_contract.py expects, from the table of
tests/ac17_packed_cases.py.  Needs a GPU.

Run it on the commit whose behaviour is to be kept, BEFORE the change that must not alter it, and commit the file with that change:
    python tools/record_ac17_packed_contract.py [output path] [--only CASE ...]
With --only, the named cases alone are run and take their place in the existing file; every other record stays as it was written."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from rabe_amd import hostlib as hl
    from tests import ac17_packed_cases as cases
    from tests.test_gpu_ac17_packed_contract import check_invariants
    argv = sys.argv[1:]
    only = argv[argv.index("--only") + 1:] if "--only" in argv else None
    argv = argv[:argv.index("--only")] if only is not None else argv
    out = argv[0] if argv else os.path.join(ROOT, "tests", "golden", "ac17_packed_contract.json")
    host = hl.Host(0)
    setup = cases.Setup(host)
    golden, broken = {}, []
    for leg in reversed(cases.LEGS):          # not the test's order: the records do not depend on it
        t0 = time.time()
        got = cases.run_leg(host, setup, leg) if only is None else {name: cases.run(host, setup, leg, name) for name in ["clean"] + only}
        try:
            check_invariants(setup, leg, got)
        except AssertionError as ex:          # still written, for the diagnosis; the run fails
            broken.append((cases.leg_name(leg), str(ex)))
        golden[cases.leg_name(leg)] = {name: rec for name, (rec, _st, _out) in got.items()}
        if only is not None:
            kept = json.load(open(out))[cases.leg_name(leg)]
            assert kept["clean"] == golden[cases.leg_name(leg)]["clean"], "this library is not the one the file was written with"
            golden[cases.leg_name(leg)] = {name: golden[cases.leg_name(leg)][name] if name in only else rec for name, rec in kept.items()}
        print(cases.leg_name(leg), len(got), "cases, %.2f s" % (time.time() - t0), flush=True)
    host.close()
    write(golden, out)
    for leg, what in broken:
        print("INVARIANT BROKEN", leg, what)
    sys.exit(1 if broken else 0)


def write(golden, out):
    """one line per case"""
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(
            '"%s": {\n' % leg + ",\n".join(' "%s": %s' % (case, json.dumps(rec, separators=(",", ":"))) for case, rec in golden[leg].items()) + "\n}"
            for leg in sorted(golden)) + "\n}\n")
    assert json.load(open(out)) == golden
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
