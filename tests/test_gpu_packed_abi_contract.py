"""The C ABI of every rabe_*_packed entry point, frozen call by call (tests/packed_abi_cases.py has the table and says which arguments may be
null): the full call, the sizing call, a capacity one byte short, n_items = 0 and each refusable array null in turn -- on a plain host and on
the device group [0, 0].  Per call: the return code, the text left in rabe_host_last_error, which sentinel-filled output arrays were written,
the offsets and a SHA-256 of what was written.

The expected records (tests/golden/packed_abi_contract.json) were written by tools/record_packed_abi_contract.py on the commit BEFORE the
wrappers of host/host_abi.cpp were folded into one function per call shape; they are not regenerated from the code under test."""
import json
import os

import pytest

from rabe_amd import build
from rabe_amd import hostlib as hl
from tests import packed_abi_cases as cases

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "packed_abi_contract.json")
PACKED = sorted(s for s in build.declared_symbols() if s.startswith("rabe_") and s.endswith("_packed"))


@pytest.fixture(scope="module")
def golden():
    """{entry point: {"single": {case: record}, "group": {case: record}}}; the file lists under "group" only what differs from "single" """
    g = json.load(open(GOLDEN))
    return {fn: {"single": r["single"], "group": {case: r["group"].get(case, rec) for case, rec in r["single"].items()}} for fn, r in g.items()}


@pytest.fixture(scope="module")
def hosts():
    hs = {"single": hl.Host(0), "group": hl.Host(devices=[0, 0])}
    yield hs
    for h in hs.values():
        h.close()


@pytest.fixture(scope="module")
def table(hosts):
    entries, keep = cases.build_entries(hosts["single"])
    yield entries
    del keep


@pytest.fixture(scope="module")
def seen():
    return {}


def test_the_table_covers_every_packed_entry_point(table, golden):
    assert sorted(table) == PACKED
    assert sorted(golden) == PACKED
    for fn in PACKED:
        assert sorted(golden[fn]) == ["group", "single"]
        for kind in ("single", "group"):
            assert list(golden[fn][kind]) == table[fn].cases(), (fn, kind)


@pytest.mark.parametrize("kind", ["single", "group"])
@pytest.mark.parametrize("fn", PACKED)
def test_records_are_the_parents(hosts, table, golden, seen, fn, kind):
    got = cases.run_entry(hosts[kind], table[fn])
    seen[fn, kind] = got
    for case, rec in got.items():
        print(fn, kind, case, json.dumps(rec, sort_keys=True))
    if "short" in got:          # one byte short of what the full call wrote is a refusal: 1, the buffer untouched -- never the full call's record
        assert got["short"]["rc"] == 1 and "buf" not in got["short"]["touched"] and got["short"] != got["full"], (fn, kind)
    for case, rec in got.items():
        assert rec == golden[fn][kind][case], (fn, kind, case)


@pytest.mark.parametrize("fn", PACKED)
def test_the_group_writes_the_single_hosts_bytes(hosts, table, seen, fn):
    """include/rabe_host.h: over a device group the outputs land where the unsplit call puts them and the bytes do not depend on the split --
    the full call and the empty one give one record on both hosts"""
    for kind in ("single", "group"):
        if (fn, kind) not in seen:
            seen[fn, kind] = cases.run_entry(hosts[kind], table[fn])
    for case in ("full", "n0"):
        group, single = dict(seen[fn, "group"][case]), dict(seen[fn, "single"][case])
        del group["tail_clean"], single["tail_clean"]          # behind the last record the buffer is the call's to use
        assert group == single, (fn, case)
    assert seen[fn, "single"]["full"]["rc"] == 0
