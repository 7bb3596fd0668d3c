"""Whole fleet flights against tests/golden/fleet_flights.json (tools/gen_golden_fleet.py recorded it; the configurations
are tests/fleet_flight_cases.py's): every flight produces the recorded bits, run() calls the recorded sequence of library
entry points -- no launch added, dropped or reordered -- and synchronises the context no more often than it did."""
import json
import os

import pytest

import fleet_flight_cases as fc

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fleet_flights.json")))


@pytest.fixture(scope="module")
def fleet():
    import neo_planner_amd as npa
    fs = fc.setup()
    neo = fc.make_neo(fs, npa.BatchPlanner())
    yield fs, neo, fc.weights_digest(neo)
    fc.drop(fs)


def test_the_fixture_holds_the_configurations():
    assert set(GOLDEN["flights"]) | set(GOLDEN["left_out"]) == set(fc.CONFIGS)
    assert set(GOLDEN["left_out"]) <= set(fc.NETWORK)


@pytest.mark.parametrize("name", [k for k in fc.CONFIGS if k in GOLDEN["flights"]])
def test_a_flight_is_the_recorded_one(fleet, name):
    fs, neo, weights = fleet
    if name in fc.NETWORK and weights != GOLDEN["weights"]:
        pytest.skip("this torch build initialised other network weights than the one the fixture was recorded with "
                    f"(head weights {weights[:12]}, fixture {GOLDEN['weights'][:12]}): the flight is another flight")
    want = GOLDEN["flights"][name]
    got = fc.fly(fs, name, neo if name in fc.NETWORK else None)
    print(f"{name}: digest {got['digest'][:12]} (recorded {want['digest'][:12]}), {got['synchronizes']} synchronisations "
          f"(recorded {want['synchronizes']}), replans {got['replans']}, failed attempts {got['failed_attempts']}")
    assert got["digest"] == want["digest"]
    assert got["calls"] == want["calls"]
    assert got["synchronizes"] <= want["synchronizes"]
    for k in ("replans", "failed_attempts", "fallback_missions", "failed_ticks"):
        assert got.get(k) == want.get(k), k
