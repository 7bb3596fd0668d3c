"""The planners' public methods against tests/golden/planner_calls.json (tools/gen_golden_planner.py recorded it; the cases
are tests/planner_cases.py's): every call returns the recorded bits, makes the recorded sequence of library entry points
-- no launch added, dropped or reordered -- and synchronises the context no more often than it did."""
import json
import os

import pytest

import planner_cases as pc

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "planner_calls.json")))


@pytest.fixture(scope="module")
def requests():
    fs = pc.setup()
    yield fs
    pc.drop(fs)


def test_the_fixture_holds_every_case():
    assert set(GOLDEN["cases"]) == set(pc.CASES)
    assert GOLDEN["recorded_twice"]


@pytest.mark.parametrize("name", list(pc.CASES))
def test_a_call_is_the_recorded_one(requests, name):
    want = GOLDEN["cases"][name]
    got, out = pc.run(requests, name)
    print(f"{name}: digest {got['digest'][:12]} (recorded {want['digest'][:12]}), {got['synchronizes']} synchronisations "
          f"(recorded {want['synchronizes']})")
    assert got["digest"] == want["digest"]
    assert got["calls"] == want["calls"]
    assert got["synchronizes"] <= want["synchronizes"]
    for k in ("launch_sizes", "group_launch_sizes", "error"):
        assert got.get(k) == want.get(k), k
    assert name not in pc.BRANCHES or pc.BRANCHES[name](out)
