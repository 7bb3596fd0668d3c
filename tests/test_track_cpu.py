"""Fleet goal routes, the parts that need no GPU: the route model of csrc/neo_track.hpp compiled by the host compiler
(tests/host_harness/track_host.cpp) against its NumPy model goal_routes.GoalRoutes bit for bit, header and exports, the
argument errors of GoalRoutes and FleetReplanLoop, and the tracker node's loop (replan.TrackerLoop) on the CPU oracle."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO

import neo_planner_amd as npa
from neo_planner_amd import _lib, build, synth
from neo_planner_amd.goal_routes import GoalRoutes
from neo_planner_amd.replan import ReplanLoop, TrackerLoop
from oracle import minco_np as onp

import track_cases as tc

INC = os.path.join(REPO, "neo-planner_amd", "csrc")
SRC = os.path.join(REPO, "tests", "host_harness", "track_host.cpp")
ORIGIN = (0.0, -15.0)


# ------------------------------------------------------------------ header against model
def _hex(a):
    return " ".join("%016x" % w for w in np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64))


def test_header_equals_model_bit_for_bit(tmp_path):
    exe = str(tmp_path / "track_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-I", INC, SRC,
                           "-o", exe])
    routes = tc.route_set()
    lines, want = [], []
    on_vertex = past_end = laps = 0
    for b in range(routes.B):
        v = routes.route(b)
        lines.append("R %d %d 0x%s %s" % (len(v), routes.closed[b], _hex(routes.speed[b]),
                                          " ".join("0x" + h for h in _hex(v).split())))
        want.append(_hex(routes.cum[b]))
        one = routes.take([b])
        for t in tc.route_times(routes, b):
            p = one.at(t)[0]
            lines.append("T 0x%s" % _hex(t))
            want.append(_hex(p) + " " + _hex(p))      # route_point and route_point_cum
            s, total = routes.speed[b] * t, routes.cum[b][-1]
            on_vertex += bool(np.any(routes.cum[b][:-1] == (np.fmod(s, total) if routes.closed[b] and total > 0 else s)))
            past_end += bool(not routes.closed[b] and s > total)
            laps += bool(routes.closed[b] and total > 0 and s > 2.0 * total)
    assert on_vertex >= 20 and past_end >= 10 and laps >= 10, (on_vertex, past_end, laps)
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[-1] == "" and len(out) == len(lines) + 1
    bad = [(l[:60], g, w) for l, g, w in zip(lines, out, want) if g != w]
    assert not bad, (len(bad), bad[:5])


def test_route_points_are_what_the_rule_says():
    r = tc.route_set()
    b = r.B - 1                                  # lengths 5 and 12 and the closing 3-16 side, speed 1, closed
    one = r.take([b])
    total = 5.0 + 12.0 + np.sqrt(3.0 * 3.0 + 16.0 * 16.0)
    assert np.array_equal(one.cum[0], [0.0, 5.0, 17.0, total])
    assert np.array_equal(one.at(0.0)[0], [0.0, 0.0]) and np.array_equal(one.at(5.0)[0], [3.0, 4.0])
    assert np.array_equal(one.at(17.0)[0], [3.0, 16.0]) and np.array_equal(one.at(11.0)[0], [3.0, 10.0])
    assert np.allclose(one.at(2.0 * total + 5.0)[0], [3.0, 4.0], atol=1e-12)
    # open: past the end the goal stays on the last vertex; a zero-length segment and a route without length give v_k
    z_open = r.take([8])
    assert np.allclose(z_open.at(1e6)[0], [9.0, -3.5], atol=1e-12) and np.array_equal(z_open.at(10.0)[0], [4.0, 6.0])
    for k in (10, 11):
        assert np.array_equal(r.take([k]).at(123.4)[0], [3.25, -1.5])
    assert np.array_equal(r.take([12]).at(55.0)[0], [2.0, 2.0])      # speed 0
    # one time per route
    t = np.linspace(0.0, 30.0, r.B)
    assert np.array_equal(r.at(t), np.stack([r.take([k]).at(t[k])[0] for k in range(r.B)]))


# ------------------------------------------------------------------ header and exports
NEW = {"neo_fleet_goal_route": 11, "neo_fleet_goal_route_dev": 11, "neo_fleet_hold_dev": 10, "neo_fleet_track_audit": 18,
       "neo_fleet_track_audit_dev": 18}


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(REPO, "include", "neo_planner.h")).read()
    build.build()
    lib = _lib.load()
    for name, nargs in NEW.items():
        m = re.search(r"^int %s\(neo_ctx \*ctx,([^)]*)\)\s*;" % name, header, re.M)
        assert m, name
        assert len(m.group(1).split(",")) + 1 == nargs, name
        assert name in _lib.EXPORTS
        assert len(getattr(lib, name).argtypes) == nargs, name
    assert not re.search(r"\bneo_fleet_hold\s*\(", header)      # the hold exists only on resident arrays
    assert re.search(r"^#define NEO_FLEET_ROUTE_MAX 256\b", header, re.M) and _lib.NEO_FLEET_ROUTE_MAX == 256
    assert re.search(r"^#define NEO_TRACK_FIELDS 8\b", header, re.M) and _lib.NEO_TRACK_FIELDS == 8
    for k, name in enumerate(_lib.TRACK_FIELDS):
        assert re.search(r"^\s*NEO_TRACK_%s = %d\b" % (name.upper(), k), header, re.M), name
    assert npa.GoalRoutes is GoalRoutes and "GoalRoutes" in npa.__all__


# ------------------------------------------------------------------ argument errors
def test_goal_routes_argument_errors():
    v = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [2.0, 2.0]])
    ok = GoalRoutes(v, [0, 2, 4], [1.0, 0.0], closed=[0, 1])
    assert ok.B == 2 and np.array_equal(ok.closed, [0, 1]) and np.array_equal(GoalRoutes(v, [0, 4], [1.0]).closed, [0])
    bad_v = v.copy()
    bad_v[1, 0] = np.nan
    for args in ((bad_v, [0, 2, 4], [1.0, 1.0]),                       # not finite
                 (v, [0, 2, 4], [1.0, np.inf]),
                 (v, [0, 2, 4], [1.0, -0.5]),                          # negative speed
                 (v, [0, 1, 4], [1.0, 1.0]),                           # fewer than 2 vertices
                 (v, [1, 4], [1.0]),                                   # not from 0
                 (v, [0, 3, 2, 4], [1.0, 1.0, 1.0]),                   # not ascending
                 (v, [0, 2], [1.0]),                                   # not all the vertices
                 (v, [0, 2, 4], [1.0]),                                # one speed per route
                 (np.zeros((257, 2)), [0, 257], [1.0])):               # more than 256 vertices
        with pytest.raises(ValueError):
            GoalRoutes(*args)
    with pytest.raises(ValueError):
        GoalRoutes(v, [0, 2, 4], [1.0, 1.0], closed=[1])
    GoalRoutes(np.zeros((256, 2)), [0, 256], [1.0])


def test_fleet_loop_argument_errors_without_a_device():
    class Cfg:
        v_max, init_wpts_num = 1.0, 2

    class FakePlanner:
        cfg = Cfg()
    routes = tc.flight_routes()
    sig = inspect.signature(npa.FleetReplanLoop.__init__).parameters
    assert sig["goal_routes"].default is None and sig["track_radius"].default == 1.0 and sig["metric_weights"].default is None
    loop = npa.FleetReplanLoop(FakePlanner(), None, None, goal_routes=routes)
    assert loop.B == 3 and np.array_equal(loop.goals, routes.at(0.0)) and np.array_equal(loop.metric_weights, [1.0, 1.0, 1.0])
    assert npa.FleetReplanLoop(FakePlanner(), None, [[30.0, 0.0]]).metric_weights is None
    assert np.array_equal(npa.FleetReplanLoop(FakePlanner(), None, None, goal_routes=routes, metric_weights=(1, 2, 3)).metric_weights,
                          [1.0, 2.0, 3.0])
    for kw in (dict(goal_routes=routes, mode="geo"),                    # the tracker node has no geo planner
               dict(),                                                  # no goals at all
               dict(goal_routes=[[0.0, 0.0], [1.0, 1.0]]),
               dict(goal_routes=routes, track_radius=float("nan")),
               dict(goal_routes=routes, track_radius=-1.0),
               dict(goal_routes=routes, metric_weights=(1.0, 1.0)),
               dict(goal_routes=routes, mission_ids=[0, 1])):
        with pytest.raises(ValueError):
            npa.FleetReplanLoop(FakePlanner(), None, None, **kw)
    with pytest.raises(ValueError):
        npa.FleetReplanLoop(FakePlanner(), None, np.zeros((2, 2)), goal_routes=routes)


# ------------------------------------------------------------------ the tracker node's loop on the CPU oracle
@pytest.fixture(scope="module")
def oracle_flights():
    routes = tc.flight_routes()
    grid = onp.GridESDF(synth.occupancy_2d(3), synth.RES, 300, 300, ORIGIN)
    np.random.seed(503)
    state = np.random.get_state()
    flights = [TrackerLoop(onp.OraclePlanner(onp.PlannerParams()), grid).run_tracking(routes.take([b]), tc.FLIGHT_TICKS, (0.0, 0.0))
               for b in range(routes.B)]
    after = np.random.get_state()
    untouched = np.array_equal(after[1], state[1]) and after[2:] == state[2:]
    return routes, flights, untouched


def test_tracker_loop_chases_the_three_routes(oracle_flights):
    routes, flights, untouched = oracle_flights
    assert untouched, "an oracle flight drew random numbers: not comparable"
    for b, f in enumerate(flights):
        gap = np.linalg.norm(f["path"][::60] - f["goals"], axis=1)
        print(f"route {b}: {f['replans']} plans, {f['failed_attempts']} failed attempts, {f['failed_ticks']} failed ticks, "
              f"{f['iter_num']} iterations, {f['n_flown']} flown rows of {len(f['commands'])}, gap at the ticks min "
              f"{gap.min():.3f} final {gap[-1]:.3f} m")
        assert f["replans"] == 31 and f["failed_attempts"] == 0 and f["failed_ticks"] == 0
        assert f["n_flown"] == 1801 and f["path"].shape == (1801, 2) and f["goals"].shape == (31, 2)
        assert np.array_equal(f["goals"][0], routes.route(b)[0])
        # row i is the command at i / cmd_hz: the row of every tick is where the plan made a tick before put it
        assert len(f["commands"]) >= 1801
    # the third goal reaches the end of its route and stays: the drone arrives and replans from on top of it
    f = flights[2]
    assert np.allclose(f["goals"][-1], routes.route(2)[-1], atol=1e-12)
    assert np.linalg.norm(f["path"][-1] - f["goals"][-1]) < ReplanLoop(None, None).target_reach_threshold


def test_tracker_loop_leaves_replan_loop_as_it_is():
    loop = TrackerLoop(None, None)
    assert isinstance(loop, ReplanLoop) and ReplanLoop.run is TrackerLoop.run
    loop.global_target = np.array([1.0, 1.0])
    loop.set_local_target(np.array([0.0, 0.0]))
    assert np.array_equal(loop.target_state, [[1.0, 1.0], [0.0, 0.0]]) and not loop.near_global_target      # :319-321
    base = ReplanLoop(None, None)
    base.global_target = np.array([1.0, 1.0])
    base.set_local_target(np.array([0.0, 0.0]))
    assert base.near_global_target
