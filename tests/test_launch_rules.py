"""Launch-selection rules of the convolution hooks against tests/golden/launch_rules.{npz,json}
(recorded by tests/golden/record_launch_rules.py).  Only handles and choice hooks: no convolution is launched."""
import json
import os
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import record_launch_rules as rules   # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def default_environment():
    with pytest.MonkeyPatch.context() as mp:
        for var in rules.ENV:
            mp.delenv(var, raising=False)
        yield


@pytest.fixture(scope="module")
def recorded():
    with open(rules.OUT + ".json") as f:
        return np.load(rules.OUT + ".npz"), json.load(f)


@pytest.fixture(scope="module")
def handles():
    return {}


def get_handle(handles, sf):
    if sf not in handles:
        handles[sf] = rules.handle(sf)
    return handles[sf]


@pytest.mark.parametrize("sf,rows,H", rules.GRID_CASES)
def test_set_conv_choice_admits_and_resolves_as_recorded(recorded, handles, sf, rows, H):
    arrays, _ = recorded
    tag = f"sf{sf}_{rows}x{H}"
    status, slot_rep, skip_rep = rules.choice_grid(get_handle(handles, sf), rows, H)
    assert np.array_equal(status, arrays[f"status_{tag}"]), np.argwhere(status != arrays[f"status_{tag}"])[:8]
    assert np.array_equal(slot_rep, arrays[f"slot_{tag}"]), np.argwhere(slot_rep != arrays[f"slot_{tag}"])[:8]
    assert np.array_equal(skip_rep, arrays[f"skip_{tag}"]), np.argwhere(skip_rep != arrays[f"skip_{tag}"])[:8]


@pytest.mark.parametrize("sf", rules.SIZES)
def test_conv_choices_of_baseline_shapes_as_recorded(recorded, handles, sf):
    _, meta = recorded
    got = rules.plan_reports(get_handle(handles, sf))
    want = meta["plans"][str(sf)]
    assert got.keys() == want.keys()
    for key in want:
        assert got[key] == want[key], key


def test_plan_table_entries_are_accepted_unchanged(handles):
    seen = set()
    bad = [key for sf in rules.SIZES for key in rules.table_mismatches(get_handle(handles, sf), seen)]
    assert not bad
    assert seen == set(rules.engine._Plans.table())
