"""The bytes of every packed encrypt, encaps and issuing call whose records are written from a source table (host/record_layout.h:
RecordSources; host/records.h: finish_encrypt), frozen at a shape that shows a wrong index array, a wrong stride or a misplaced seal: 5 items
over 3 policies / lists of 1, 2 and 3 rows in the order [2, 0, 1, 2, 0], payloads of 1, 15, 16, 17 and 33 bytes (tests/encrypt_tail_cases.py).
Per call: the return code, the error text, the offsets and a SHA-256 of the records and of the keys.

The expected records (tests/golden/encrypt_tail_contract.json) were written by tools/record_encrypt_tail_contract.py on the commit BEFORE the
encrypt side of host/packed.cpp was folded onto one source table and one tail; they are not regenerated from the code under test."""
import json
import os

import pytest

from rabe_amd import hostlib as hl
from tests import encrypt_tail_cases as cases

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encrypt_tail_contract.json")
SCHEMES = ["ac17_cp", "ac17_kp", "bsw", "lsw", "aw11", "ghw11", "bdabe", "mke08"]
ISSUERS = ["ac17_kp_keygen", "bsw_delegate", "lsw_keygen", "lsw_keygen_negative", "ghw11_keygen", "ghw11_provision", "bdabe_keygen", "mke08_keygen",
           "bdabe_request_sk", "mke08_request_sk"]
NAMES = sorted([s + "_encrypt" for s in SCHEMES] + [s + "_encaps" for s in SCHEMES] + ISSUERS)


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


@pytest.fixture(scope="module")
def host():
    h = hl.Host(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def table(host):
    entries, keep = cases.build_entries(host)
    yield entries
    del keep


def test_the_table_and_the_golden_file_cover_the_same_calls(table, golden):
    assert sorted(table) == NAMES
    assert sorted(golden) == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_records_are_the_parents(host, table, golden, name):
    got = cases.run(host, table[name])
    print(name, json.dumps(got, sort_keys=True))
    assert got["rc"] == 0 and got["err"] == "", name
    assert got == golden[name], name


@pytest.mark.parametrize("scheme", SCHEMES)
def test_encaps_writes_the_header_of_encrypt(golden, scheme):
    """the same draws without the nonce: an encaps record is the encrypt record up to its sealed part, whose length field is zero -- so record i
    of the one is 28 bytes and payload i shorter than record i of the other"""
    enc, kem = golden[scheme + "_encrypt"]["off"]["off"], golden[scheme + "_encaps"]["off"]["off"]
    for i, pt in enumerate(cases.PTS):
        assert (enc[i + 1] - enc[i]) - (kem[i + 1] - kem[i]) == len(pt) + 28, (scheme, i)
