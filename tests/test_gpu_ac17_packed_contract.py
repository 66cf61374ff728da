"""rabe_ac17_{cp,kp}_{decrypt,decaps}_packed, checked and trusted, frozen batch by batch (tests/ac17_packed_cases.py has the table): damaged
offsets, records cut at and inside every field, every count and length field overwritten, policies that panic or are not satisfied, renamed /
permuted / additional rows, elements that are no group members, a flipped tag bit, and the shapes of the call itself (n = 0, n = 1, every item
failing, the same call again, another key in between, six damages in one batch).  Per call: the return code, the whole status vector, the text
left in rabe_host_last_error where an item failed, and a SHA-256 over what was written (plaintexts + pt_off; decaps: the key array).

The expected records (tests/golden/ac17_packed_contract.json) were written by tools/record_ac17_packed_contract.py on the commit BEFORE
ac17::decrypt_packed_core moved to host/packed.cpp and onto its helpers; they are not regenerated from the code under test.

Statuses, messages and plaintexts do not depend on whether a record went through its plan's shared row layout or through a selection of its own,
nor on what the cross-call plan cache holds: the golden file is independent of the order of the cases and of the legs.  Keep it that way -- a
case that only passes behind another one is measuring the cache, not the call.  The one case that is ABOUT a new plan (victim_at_0: the
plan learns its row names from a non-standard record) brings a key text of its own in every leg, so it finds no plan whatever ran before."""
import json
import os

import pytest

from rabe_amd import hostlib as hl
from tests import ac17_packed_cases as cases

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ac17_packed_contract.json")


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


@pytest.fixture(scope="module")
def host():
    h = hl.Host(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def setup(host):
    return cases.Setup(host)


def check_invariants(setup, leg, got):
    """what holds whatever the golden file says: an untouched item comes back whole, `ok` damage decrypts, `dead` damage does not"""
    side, op, _mode = leg
    clean = got["clean"][2]
    if op == "decrypt":
        assert clean == cases.PTS
    for name, (rec, st, out) in got.items():
        b = setup.cases[side][name]
        assert rec["rc"] == 0 and len(st) == b.n, (leg, name)
        for i in range(b.n):
            if i not in b.victims or i in b.ok:
                assert st[i] == 0 and out[i] == clean[i], (leg, name, i)
            elif i in b.dead:
                assert st[i] == -1, (leg, name, i)
            else:
                assert st[i] in (0, -1), (leg, name, i)
                if st[i] == 0 and op == "decrypt":          # the seal held: then it is the plaintext
                    assert out[i] == clean[i], (leg, name, i)
            if st[i] != 0 and op == "decaps":
                assert out[i] == bytes(32), (leg, name, i)


def test_the_table_and_the_golden_file_agree(setup, golden):
    assert sorted(golden) == sorted(cases.leg_name(leg) for leg in cases.LEGS)
    for leg in cases.LEGS:
        assert list(golden[cases.leg_name(leg)]) == list(setup.cases[leg[0]]), leg


@pytest.mark.parametrize("leg", cases.LEGS, ids=cases.leg_name)
def test_records_are_the_parents(host, setup, golden, leg):
    got = cases.run_leg(host, setup, leg)
    for name, (rec, _st, _out) in got.items():
        print(cases.leg_name(leg), name, json.dumps(rec, sort_keys=True))
    check_invariants(setup, leg, got)
    for name, (rec, _st, _out) in got.items():
        assert rec == golden[cases.leg_name(leg)][name], (leg, name)
