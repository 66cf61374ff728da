"""The launch sets of the decrypt entry points of the device library, frozen case by case (tests/decrypt_launch_cases.py has the table and the
shapes): in pairing mode 0 and in the cross-check mode 99, the return code, how often each kernel was launched (the engine's own timing read)
and a SHA-256 of the outputs.

The expected records (tests/golden/decrypt_launch_contract.json) were written by tools/record_decrypt_launch_contract.py on the commit BEFORE
the host-side launch code of engine_jobs.hip was folded (one sum stage, one Miller dispatch, named arenas); they are not regenerated from the
code under test.  Mode 0 chooses its kernel families by the device's compute-unit count: the file is for the device its header names."""
import json
import os

import pytest

from rabe_amd.engine import Engine
from tests import decrypt_launch_cases as cases

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decrypt_launch_contract.json")


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


@pytest.fixture(scope="module")
def world(golden):
    eng = Engine(0)
    n_cu, name = eng.device_info()
    assert {"device": name, "compute_units": n_cu} == golden["header"], "the golden file was recorded on another device"
    yield cases.World(eng)
    eng.close()


def test_the_golden_file_holds_the_table(golden):
    assert [(entry, shape) for entry, shapes in golden["cases"].items() for shape in shapes] == cases.CASES
    assert all(list(modes) == [str(m) for m in cases.MODES] for shapes in golden["cases"].values() for modes in shapes.values())


@pytest.mark.parametrize("entry,shape", cases.CASES, ids=["%s-%s" % c for c in cases.CASES])
def test_records_are_the_parents(world, golden, entry, shape):
    got = cases.run_case(world, entry, shape)
    for mode, rec in got.items():
        print(entry, shape, mode, json.dumps(rec, sort_keys=True))
    for mode, rec in got.items():
        assert rec == golden["cases"][entry][shape][mode], (entry, shape, mode)
    # the cross-check mode returns the automatic selection's result
    assert got["99"]["sha256"] == got["0"]["sha256"] and got["99"]["rc"] == got["0"]["rc"]
