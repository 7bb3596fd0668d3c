"""Fleet replan loop, the parts that need no GPU: the C ABI declares and exports the fleet entry points, and the random
streams of a mission (target jitter, BatchPlanner.plan's retry noise) do not depend on the fleet it flies in."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO
from helpers import _code_lines

import neo_planner_amd as npa
from neo_planner_amd import _lib, build, fleet
from neo_planner_amd.goal_routes import GoalRoutes

ENTRY_POINTS = ("neo_fleet_target_batch", "neo_fleet_target_batch_dev", "neo_fleet_advance_dev", "neo_fleet_splice_dev",
                "neo_fleet_audit_batch", "neo_fleet_audit_batch_dev")
FLAGS = dict(NEO_FLEET_FLAG_TARGET_CAPPED=1, NEO_FLEET_FLAG_CMD_FULL=2, NEO_FLEET_FLAG_BAD_SCENE=4,
             NEO_FLEET_FLAG_SPLICE_FAILED=8, NEO_FLEET_FLAG_ABANDONED=16)


def test_header_declares_the_fleet_entry_points_and_flags():
    header = open(os.path.join(REPO, "include", "neo_planner.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"^int %s\(neo_ctx \*ctx," % name, header, re.M), name
        assert name in _lib.EXPORTS
    # advance and splice exist only on resident arrays
    assert not re.search(r"\bneo_fleet_(advance|splice)(_batch)?\s*\(", header)
    for name, value in FLAGS.items():
        assert re.search(r"^#define %s %d\b" % (name, value), header, re.M), name
        assert getattr(_lib, name) == value


def test_library_exports_the_fleet_entry_points():
    build.build()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert getattr(lib, name) is not None
        assert getattr(lib, name).argtypes, name     # bound with a signature, not called through ctypes' defaults


def test_fleet_is_exported():
    assert npa.FleetReplanLoop is fleet.FleetReplanLoop
    sig = inspect.signature(npa.FleetReplanLoop.__init__)
    for name, default in dict(mode="basic", cmd_hz=60, replan_period=1.0, planning_time_ahead=1.0, longitu_step_dis=5.0,
                              lateral_step_length=1.0, target_reach_threshold=0.2, max_cmd_seconds=120, seed=0,
                              scene_ids=None).items():
        assert sig.parameters[name].default == default, name
    assert inspect.signature(npa.FleetReplanLoop.run).parameters["max_replans"].default == 60


def test_target_jitter_of_a_mission_is_the_same_in_any_fleet():
    seed = 7
    all64 = {(t, r): fleet.target_jitter(seed, np.arange(64), t, r) for t in (0, 3, 17) for r in (0, 1, 10)}
    for (t, r), j in all64.items():
        assert j.shape == (64, 2)
        if r == 0:
            assert not j.any()          # the first target of a tick is the deterministic one
            continue
        for i in (0, 1, 37, 63):
            assert np.array_equal(fleet.target_jitter(seed, [i], t, r)[0], j[i])
            assert np.array_equal(j[i], np.random.default_rng([seed, i, t, r]).normal(0.0, 1.0, 2))
        # a subset in another order: still each mission's own draws
        sub = np.array([40, 3, 12])
        assert np.array_equal(fleet.target_jitter(seed, sub, t, r), j[sub])
    assert not np.array_equal(all64[(3, 1)], all64[(3, 10)]) and not np.array_equal(all64[(3, 1)], all64[(17, 1)])
    assert not np.array_equal(fleet.target_jitter(seed + 1, np.arange(64), 3, 1), all64[(3, 1)])
    # the plans of one (tick, target) share a seed that differs between them
    seeds = {fleet.plan_seed(seed, t, r) for t in range(5) for r in range(11)}
    assert len(seeds) == 55 and all(0 <= s < 2 ** 62 for s in seeds)


def test_fleet_loop_passes_mission_ids_as_streams():
    class Cfg:
        v_max, init_wpts_num = 1.0, 2
    class FakePlanner:
        cfg = Cfg()
    goals = np.array([[30.0, 0.0], [28.0, 3.0]])
    a = npa.FleetReplanLoop(FakePlanner(), None, goals)
    assert np.array_equal(a.mission_ids, [0, 1]) and a.cap == 7200 and a.stride == 6 and a.move_vel == 0.8
    b = npa.FleetReplanLoop(FakePlanner(), None, goals[1:], mission_ids=[1])
    assert np.array_equal(b.mission_ids, [1])
    with pytest.raises(ValueError):
        npa.FleetReplanLoop(FakePlanner(), None, goals, mission_ids=[1])
    with pytest.raises(ValueError):
        npa.FleetReplanLoop(FakePlanner(), None, goals, mode="nn")


# the constructor's refusals, as they read before its checks moved into one function
MESSAGES = (
    "FleetReplanLoop: mode must be 'basic', 'geo', 'batch', 'neo', 'nn' or 'warmstart'",
    "FleetReplanLoop: goal_routes must be a GoalRoutes",
    "FleetReplanLoop: goal routes need a mode other than 'geo' (the tracker node has no geo planner)",
    "FleetReplanLoop: one goal route per mission",
    "FleetReplanLoop: goals may be None only with goal_routes",
    "FleetReplanLoop: track_radius must be finite and >= 0",
    "FleetReplanLoop: metric_weights must be three finite numbers",
    "FleetReplanLoop: modes 'neo' and 'nn' need neo=BatchNeoPlanner",
    "FleetReplanLoop: neo's planner must be the loop's batch_planner",
    "FleetReplanLoop: the network plans M = 3 pieces: modes 'neo' and 'nn' need init_wpts_num = 2",
    "FleetReplanLoop: neo's camera renders %d x %d, its network takes %d x %d",
    "FleetReplanLoop: modes 'neo' and 'nn' need scenes=(boxes, box_begin), what the cameras see",
    "FleetReplanLoop: resident=True needs mode 'basic' or 'batch' (geo_plan has no resident form)",
    "FleetReplanLoop: onboard maps need mode 'basic' or 'batch' (geo on onboard maps is not built)",
    "FleetReplanLoop: onboard and record need scenes=(boxes, box_begin), what the cameras see",
    "FleetReplanLoop: one mission id and one scene id per goal",
    "FleetReplanLoop: the onboard mapper must have one entry per goal",
    "FleetReplanLoop: scene_index must have one entry per goal",
    "FleetReplanLoop: the recorder's M must be the planner's init_wpts_num + 1",
    "FleetReplanLoop: the recorder and the planner must share one context",
    "FleetReplanLoop: a scene id without a map",
    "FleetReplanLoop.x: no flight yet",
)


def test_the_loop_keeps_its_structure():
    """run() asks neither for the mode nor for `resident` -- __init__ chose the plan step --, the pose and the state kernel
    have one call site each, the refusals read as they did, and the file stays below what it was before the loop was
    taken apart (1 stage per duplicated one, 1 helper per hand-written call)"""
    run = inspect.getsource(fleet.FleetReplanLoop.run)
    assert "self.mode" not in run and "self.resident" not in run
    source = inspect.getsource(fleet)
    code = re.sub(r'""".*?"""', "", source, flags=re.S)
    for name in ("neo_fleet_pose_dev", "neo_record_state_dev"):
        assert len(re.findall(r"\b%s\b" % name, code)) == 1, name
    assert not re.search(r"\blib\.neo_(?!scene_slot\b)", code)      # every launch goes through the one helper
    for m in MESSAGES:
        assert source.count('"%s"' % m) == 1, m
    assert _code_lines('x = 1\n\n# c\ndef f():\n    """doc\n    more"""\n    return (1,\n            2)  # c\n') == 4
    assert _code_lines(source) < 558      # what fleet.py had before


def test_the_constructor_refuses_in_the_same_order():
    """the first refusal and its message, for the arguments the suite's tests provoke one with"""
    class Cfg:
        v_max, init_wpts_num = 1.0, 2
    class FakePlanner:
        cfg, ctx = Cfg(), object()
    class Cam:
        height, width = 48, 64
    class Neo:
        pass
    class Sized:
        def __init__(self, **kw):
            self.__dict__.update(kw)
    bp = FakePlanner()
    goals = np.array([[30.0, 0.0], [28.0, 3.0]])
    routes = GoalRoutes.from_lists([[[1.0, 0.0], [2.0, 0.0]]] * 2, [1.0, 1.0])
    neo = Sized(bp=bp, init=Sized(net=Sized(img_height=48, img_width=64)), camera=Cam())
    scenes = (np.zeros((0, 6)), np.zeros(1, np.int32))
    cases = [
        (dict(mode="Warmstart"), MESSAGES[0]),
        (dict(mode="geo", jitter="device"), "jitter"),                                   # counter_rng's own refusal comes first
        (dict(goals=None, goal_routes=[[0.0, 0.0], [1.0, 1.0]]), MESSAGES[1]),
        (dict(goals=None, goal_routes=routes, mode="geo"), MESSAGES[2]),
        (dict(goals=np.zeros((3, 2)), goal_routes=routes), MESSAGES[3]),
        (dict(goals=None), MESSAGES[4]),
        (dict(goals=None, goal_routes=routes, track_radius=float("nan"), metric_weights=(1.0, 1.0)), MESSAGES[5]),
        (dict(goals=None, goal_routes=routes, track_radius=-1.0), MESSAGES[5]),
        (dict(goals=None, goal_routes=routes, metric_weights=(1.0, 1.0), mission_ids=[0]), MESSAGES[6]),
        (dict(mode="nn", mission_ids=[1]), MESSAGES[7]),
        (dict(mode="neo", neo=Sized(bp=FakePlanner())), MESSAGES[8]),
        (dict(mode="neo", neo=Sized(bp=bp, init=Sized(net=Sized(img_height=96, img_width=64)), camera=Cam())),
         "FleetReplanLoop: neo's camera renders 48 x 64, its network takes 96 x 64"),
        (dict(mode="nn", neo=neo), MESSAGES[11]),
        (dict(mode="geo", resident=True, onboard=Sized(B=2)), MESSAGES[12]),
        (dict(mode="geo", onboard=Sized(B=2), scenes=scenes), MESSAGES[13]),
        (dict(mode="warmstart", record=object()), MESSAGES[14]),
        (dict(onboard=Sized(B=2)), MESSAGES[14]),
        (dict(mission_ids=[1]), MESSAGES[15]),
        (dict(scene_ids=[1, 2, 3]), MESSAGES[15]),
        (dict(goals=None, goal_routes=routes, mission_ids=[0, 1, 2]), MESSAGES[15]),
        (dict(jitter="counter", seed=-3), "seed"),
        (dict(jitter="counter", mission_ids=[0, 2 ** 31]), "id"),
        (dict(onboard=Sized(B=3), scenes=scenes, scene_index=[0]), MESSAGES[16]),
        (dict(onboard=Sized(B=2, scene_ids=None), scenes=scenes, scene_index=[0]), MESSAGES[17]),
        (dict(record=Sized(M=5, ctx=bp.ctx), scenes=scenes), MESSAGES[18]),
        (dict(record=Sized(M=3, ctx=object()), scenes=scenes), MESSAGES[19]),
    ]
    for kw, message in cases:
        kw = dict(dict(goals=goals), **kw)
        with pytest.raises(ValueError) as e:
            npa.FleetReplanLoop(bp, None, kw.pop("goals"), **kw)
        assert message in str(e.value), (kw, str(e.value))
        if message.startswith("FleetReplanLoop"):
            assert str(e.value) == message, kw
    five = FakePlanner()
    five.cfg = Sized(v_max=1.0, init_wpts_num=4)
    with pytest.raises(ValueError) as e:
        npa.FleetReplanLoop(five, None, goals, mode="neo", neo=Sized(bp=five))
    assert str(e.value) == MESSAGES[9]
    with pytest.raises(_lib.NeoError) as e:
        npa.FleetReplanLoop(bp, None, goals).x
    assert str(e.value) == MESSAGES[21]
    # the plan step is chosen once, by mode and `resident`
    step = lambda **kw: npa.FleetReplanLoop(bp, None, goals, **kw)._plan_step.__name__
    assert [step(), step(resident=True), step(mode="geo"), step(mode="batch"), step(mode="batch", resident=True), step(mode="warmstart"),
            step(mode="neo", neo=neo, scenes=scenes), step(mode="nn", neo=neo, scenes=scenes)] == \
        ["_plan_host", "_plan_resident", "_plan_geo", "_plan_batch", "_plan_batch", "_plan_warm", "_plan_neo", "_plan_nn"]


def test_plan_has_stream_ids_and_its_default_is_the_position():
    p = inspect.signature(npa.BatchPlanner.plan).parameters
    assert "stream_ids" in p and p["stream_ids"].default is None
    seed, D, count = 123456789, 2, 2
    todo = np.array([3, 5, 40])
    for attempt in (1, 2, 4):
        # the expression plan() used before it had stream_ids: the request's position keys its stream
        before = np.stack([np.random.default_rng([int(seed), int(i), attempt]).normal(0.0, 0.5, (D, count)) for i in todo])
        assert np.array_equal(npa.BatchPlanner.retry_noise(seed, np.arange(64)[todo], attempt, D, count), before)
        # with mission ids as streams, a request's noise is its mission's wherever it sits in the batch
        ids = np.array([900, 7, 12])
        got = npa.BatchPlanner.retry_noise(seed, ids, attempt, D, count)
        for k, i in enumerate(ids):
            assert np.array_equal(got[k], np.random.default_rng([seed, int(i), attempt]).normal(0.0, 0.5, (D, count)))
