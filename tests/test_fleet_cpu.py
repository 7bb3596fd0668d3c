"""Fleet replan loop, the parts that need no GPU: the C ABI declares and exports the fleet entry points, and the random
streams of a mission (target jitter, BatchPlanner.plan's retry noise) do not depend on the fleet it flies in."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO

import neo_planner_amd as npa
from neo_planner_amd import _lib, build, fleet

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
