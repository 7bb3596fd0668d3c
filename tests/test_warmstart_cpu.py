"""Mode "warmstart", the parts that need no GPU: the C ABI declares and binds the two entry points, FleetReplanLoop takes
the mode, ReplanLoop(mode="warmstart") flies the CPU oracle from its previous plans -- fewer iterations than mode
"basic", no random draw -- and the NumPy model of the two fleet kernels (tests/warm_oracle_np.py), fed that flight's
plans, reproduces the first guesses the oracle planner was started from."""
import os
import re

import numpy as np
import pytest

from conftest import REPO

import neo_planner_amd as npa
import warm_oracle_np as won
from neo_planner_amd import _lib, build, synth
from neo_planner_amd.replan import ReplanLoop
from oracle import minco_np as onp

ORIGIN = (0.0, -15.0)
ENTRY_POINTS = {"neo_fleet_warm_guess_dev": 9, "neo_fleet_warm_carry_dev": 13}


def test_header_declares_and_lib_binds_the_entry_points():
    build.build()
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "neo_planner.h")).read()
    for name, count in ENTRY_POINTS.items():
        assert name in _lib.EXPORTS
        decl = re.search(r"^int " + name + r"\(neo_ctx \*ctx,([^)]*)\)", header, re.M)
        assert decl, name
        assert len(getattr(lib, name).argtypes) == len(decl.group(1).split(",")) + 1 == count, name
    assert re.search(r"#define\s+NEO_ABI_VERSION\s+1\b", header)
    assert callable(npa.BatchPlanner.warm_guess_dev) and callable(npa.BatchPlanner.warm_carry_dev)


class _Cfg:
    v_max, init_wpts_num = 1.0, 2


class FakePlanner:
    cfg = _Cfg()


def test_fleet_loop_takes_the_mode_without_a_device():
    goals = np.array([[30.0, 0.0], [28.0, 3.0]])
    loop = npa.FleetReplanLoop(FakePlanner(), None, goals, mode="warmstart")
    assert loop.resident and loop.mode == "warmstart" and loop.neo is None and loop._dev is None
    assert npa.FleetReplanLoop(FakePlanner(), None, goals, mode="warmstart", jitter="counter").counter
    assert not npa.FleetReplanLoop(FakePlanner(), None, goals).resident          # the default stays basic, on the host
    for bad in ("warm", "warmstart ", "Warmstart", ""):
        with pytest.raises(ValueError, match="mode must be"):
            npa.FleetReplanLoop(FakePlanner(), None, goals, mode=bad)
    with pytest.raises(ValueError, match="scenes"):         # onboard and record still want to know what the cameras see
        npa.FleetReplanLoop(FakePlanner(), None, goals, mode="warmstart", record=object())
    # the refusals of geo stay
    with pytest.raises(ValueError):
        npa.FleetReplanLoop(FakePlanner(), None, goals, mode="geo", resident=True)


class _Watched(onp.OraclePlanner):
    """the oracle planner, noting what every plan call was started from and what it left"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.calls = []

    def warm_start_plan(self, map, head_state, tail_state, int_wpts, ts):
        call = dict(head=np.array(head_state), wpts0=np.array(int_wpts), ts0=np.array(ts))
        self.calls.append(call)
        super().warm_start_plan(map, head_state, tail_state, int_wpts, ts)
        call.update(wpts=np.array(self.int_wpts), tau=np.array(self.tau), ts=np.array(self.ts))


@pytest.fixture(scope="module")
def flights():
    """scene 3, (0, 0) to (30, 0), on the CPU oracle: mode "warmstart" (watched) and mode "basic\""""
    grid = onp.GridESDF(synth.occupancy_2d(3), synth.RES, 300, 300, ORIGIN)
    np.random.seed(503)
    state = np.random.get_state()
    planner = _Watched(onp.PlannerParams())
    warm = ReplanLoop(planner, grid, mode="warmstart").run()
    after = np.random.get_state()
    drew = not (np.array_equal(after[1], state[1]) and after[2:] == state[2:])
    basic = ReplanLoop(onp.OraclePlanner(onp.PlannerParams()), grid).run()
    return warm, basic, planner, drew


def test_replan_loop_flies_the_oracle_from_its_previous_plans(flights):
    warm, basic, planner, drew = flights
    print(f"warmstart: {warm['replans']} plans, {warm['failed_attempts']} failed, {warm['iter_num']} iterations, "
          f"{warm['opt_runs']} runs, {len(warm['path'])} commands, clearance {warm['min_clearance']:.3f}; basic: "
          f"{basic['replans']} plans, {basic['failed_attempts']} failed, {basic['iter_num']} iterations, {basic['opt_runs']} runs")
    assert not drew, "the warm-started oracle flight drew random numbers"
    assert warm["success"] and basic["success"]
    assert (warm["replans"], warm["failed_attempts"], warm["iter_num"], warm["opt_runs"], len(warm["path"])) == \
        (25, 0, 134, 25, 1788)
    assert basic["iter_num"] == 381 and warm["iter_num"] < basic["iter_num"]
    # the first plan is a basic plan: the straight line and the init durations; every later one is not
    first = planner.calls[0]
    assert np.array_equal(first["ts0"], [3.75, 2.5, 3.75])
    assert all(not np.array_equal(c["ts0"], first["ts0"]) for c in planner.calls[1:])


def test_the_model_reproduces_the_oracle_planners_first_guesses(flights):
    """carry after plan k, guess before plan k + 1, one mission: the waypoints bit for bit and tau bit for bit map_T2tau's
    of the durations the planner held (both are NumPy / libm here)"""
    warm, basic, planner, drew = flights
    P = onp.PlannerParams()
    T_min, T_max = float(P.T_min), float(P.T_max)
    calls = planner.calls
    assert len(calls) == 25
    count = calls[0]["wpts"].shape[1]
    M = count + 1
    init_ts = np.array([3.75, 2.5, 3.75])
    wl, tc = np.zeros((1, 2, count)), np.zeros((1, M))
    one = np.ones(1, np.int32)
    for k in range(len(calls) - 1):
        c, nxt = calls[k], calls[k + 1]
        x = np.concatenate([c["wpts"].reshape(-1), c["tau"]])[None]
        head = np.zeros((1, 3, 2))
        head[0, :2] = c["head"]
        wl, tc = won.carry(x, head, one, 0 * one, one, init_ts, wl, tc, T_min, T_max)
        assert np.array_equal(tc[0], c["ts"])           # what planner.ts held
        head_n = np.zeros((1, 3, 2))
        head_n[0, :2] = nxt["head"]
        x0 = won.guess(head_n, wl, tc, T_min, T_max)[0]
        assert np.array_equal(x0[:2 * count].reshape(2, count), nxt["wpts0"]), k
        probe = onp.OraclePlanner(P)
        probe.M = M
        assert np.array_equal(x0[2 * count:], probe.map_T2tau(nxt["ts0"])), k
        assert np.isfinite(x0).all()


def test_the_model_where_map_T2tau_raises():
    T_min, T_max = 0.5, 5.0
    probe = onp.OraclePlanner(onp.PlannerParams())
    probe.M = 1
    for t in (T_max, 0.0, 7.0, np.inf, -np.inf):
        with pytest.raises(Exception):
            probe.map_T2tau(np.array([t]))
        assert np.isnan(won.tau_of(t, T_min, T_max)), t
    # exactly T_min: NumPy's division by zero does not raise, the reference goes on with tau = -inf and a NaN gradient;
    # the mode's definition ends that attempt like the others
    with np.errstate(divide="ignore"):
        assert probe.map_T2tau(np.array([T_min]))[0] == -np.inf
    assert np.isnan(won.tau_of(T_min, T_min, T_max))
    assert np.isnan(won.tau_of(np.nan, T_min, T_max))
    assert won.tau_of(2.75, T_min, T_max) == 0.0
    # a duration saturates from |tau| of about 37 on, and the guess made of it is NaN
    ts = won.durations_of([-40.0, 40.0, -800.0, 800.0, 36.0, np.nan], T_min, T_max)
    assert list(ts[:4]) == [T_min, T_max, T_min, T_max] and T_min < ts[4] < T_max and np.isnan(ts[5])
    assert all(np.isnan(won.tau_of(float(t), T_min, T_max)) for t in ts[:4])
