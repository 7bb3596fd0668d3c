"""The fleet's flight model, the parts that need no GPU: csrc/neo_flight.hpp compiled by the host compiler
(tests/host_harness/flight_host.cpp) against its NumPy model and definition flight_model.py bit for bit, the independence
of a flight from how launches cut it, the edge cases of a launch, the settle rows, exact following, the tracking-error
record against a plain loop, the gust draws, header and exports, the refusals, and replan.ReplanLoop and TrackerLoop on the
CPU oracle with and without a model."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO

import neo_planner_amd as npa
from neo_planner_amd import _lib, build, counter_rng, synth
from neo_planner_amd import flight_model as fm
from neo_planner_amd.replan import ReplanLoop
from oracle import minco_np as onp

import flight_cases as fc

INC = os.path.join(REPO, "neo-planner_amd", "csrc")
SRC = os.path.join(REPO, "tests", "host_harness", "flight_host.cpp")
ORIGIN = (0.0, -15.0)


# ------------------------------------------------------------------ header against model
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("flight") / "flight_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-I", INC, SRC,
                           "-o", exe])
    return exe


def _hex(a):
    return " ".join("0x%016x" % w for w in np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64))


def _floats(words):
    return np.array([int(w, 16) for w in words], dtype=np.uint64).view(np.float64)


def host_launch(exe, fl, d, step, ahead=5, first=0, settle=0, reach=0.2):
    """the header's flight_fly for every mission of the fleet `fl`, in place: what fleet_fly_kernel does with the words"""
    cap = fl["cap"]
    lines = ["M %s %d %d" % (_hex([d.h, d.kp, d.kv, d.a_max, d.alpha, d.drag, d.rho, d.scale]), d.gust_every, d.seed)]
    for b in range(fl["B"]):
        n = max(min(int(fl["cmd_len"][b]), cap), 0)
        lines.append("F %d %d %d %d %d %d %d %d %d %s %s %s %s" % (
            fl["mission_ids"][b], cap, fl["cmd_len"][b], fl["cmd_index"][b], fl["flown_len"][b], step, ahead, first, settle,
            _hex(reach), _hex(fl["goal"][b]), _hex(fl["drone"][b]), _hex(fl["cmd"][b, :n])))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0] == "ok" and out[-1] == "" and len(out) == len(lines) + 1
    for b, line in enumerate(out[1:-1]):
        if line == "skip":
            assert fl["cmd_len"][b] < 1
            continue
        w = line.split()
        idx, fut, flen, sat, full = (int(x) for x in w[:5])
        fl["cmd_index"][b], fl["future_index"][b], fl["flown_len"][b] = idx, fut, flen
        fl["saturated"][b] += sat
        if full:
            fl["flags"][b] |= _lib.NEO_FLEET_FLAG_CMD_FULL
        fl["drone"][b] = _floats(w[5:13])
        fl["cur_pos"][b] = fl["drone"][b, :2]
        fl["head"][b].reshape(6)[:4] = _floats(w[13:17])
        fl["head"][b].reshape(6)[4:] = 0.0
        rows = _floats(w[17:]).reshape(cap, 3, 2)
        wrote = rows.reshape(cap, 6).view(np.uint64)[:, 0] != np.float64(fc.CANARY).view(np.uint64)
        fl["flown"][b, :cap][wrote] = rows[wrote]


@pytest.mark.parametrize("name", list(fc.MODELS))
def test_header_equals_model_bit_for_bit(host_exe, name):
    d = fc.MODELS[name].derived(fc.HZ)
    a, b = fc.fleet(5, 11), fc.fleet(5, 11)
    sat0 = a["saturated"].copy()
    for k, (step, first) in enumerate([(7, 1), (3, 0), (60, 0)]):
        fc.model_launch(a, d, step, first=first)
        host_launch(host_exe, b, d, step, first=first)
        assert not fc.differing(a, b), (name, k, fc.differing(a, b))
    flew = a["cmd_len"] >= 1
    assert np.all(np.isfinite(a["drone"])) and np.array_equal(a["cur_pos"][flew], a["drone"][flew, :2])
    assert np.isnan(a["cur_pos"][~flew]).all()
    sat = a["saturated"] - sat0
    if name == "saturating":
        assert sat[flew].sum() > 30
    elif name == "default":
        assert sat.sum() == 0
    # the flown rows are not the command rows, and the head comes from the command array
    for m in np.flatnonzero(flew):
        fut = a["future_index"][m]
        assert np.array_equal(a["head"][m, :2], a["cmd"][m, fut, :2]) and np.all(a["head"][m, 2] == 0.0)
        assert a["future_index"][m] == min(a["cmd_index"][m] + 5, min(a["cmd_len"][m], fc.CAP) - 1)
    assert not np.array_equal(a["flown"][2, 1:fc.CAP, 0], a["cmd"][2, 1:fc.CAP, 0])


# ------------------------------------------------------------------ partition independence
@pytest.mark.parametrize("name", ["default", "gust1", "gust6"])
def test_a_flight_does_not_depend_on_how_launches_cut_it(name):
    d = fc.MODELS[name].derived(fc.HZ)
    base = fc.fleet(5, 23)
    base["cmd_len"][:], base["cmd_index"][:], base["flown_len"][:] = fc.CAP, 2, 3      # (rows 3 .. 15: a draw of gust6 at 6 and 12)
    whole = fc.copy_of(base)
    fc.model_launch(whole, d, 13)
    for cuts in ((6, 7), (5, 1, 7)):
        part = fc.copy_of(base)
        for s in cuts:
            fc.model_launch(part, d, s)
        assert not fc.differing(whole, part), (name, cuts, fc.differing(whole, part))
    assert np.all(whole["cmd_index"] == 15) and np.all(whole["flown_len"] == 16)
    if name != "default":      # the gusts moved the drones
        calm = fc.copy_of(base)
        fc.model_launch(calm, fc.MODELS["default"].derived(fc.HZ), 13)
        assert not np.array_equal(calm["drone"], whole["drone"])


# ------------------------------------------------------------------ edge cases
def test_edge_cases_of_a_launch(host_exe):
    d = fc.MODELS["default"].derived(fc.HZ)
    fl = fc.fleet(8, 5)
    before = fc.copy_of(fl)
    fc.model_launch(fl, d, 60, first=1)
    # cmd_len = 0: every row and word stays
    for k in fc.STATE:
        assert fc.same_bits(fl[k][0], before[k][0]), k
    # one command: nothing to fly, row 0 is the start state as it stands, the words are those of the last row
    assert fl["cmd_index"][1] == 0 and fl["future_index"][1] == 0 and fl["flown_len"][1] == 1
    assert fc.same_bits(fl["drone"][1], before["drone"][1]) and fc.same_bits(fl["flown"][1, 0].reshape(6), fm.out_row(d, before["drone"][1]))
    assert np.isnan(fl["flown"][1, 1:]).all()
    # clamping at the array's last row, with cmd_len == cap and cmd_len > cap alike: nothing at or past cap
    for b in (2, 3):
        assert fl["cmd_index"][b] == fc.CAP - 1 == fl["future_index"][b] and fl["flown_len"][b] == fc.CAP
        assert np.all(np.isfinite(fl["flown"][b, max(before["cmd_index"][b], 0):fc.CAP]))
    # an index below 0 counts as 0; one past the array goes back to its last row without flying
    assert fl["cmd_index"][4] == 19 and np.all(np.isfinite(fl["flown"][4, :20])) and np.isnan(fl["flown"][4, 20:]).all()
    assert fl["cmd_index"][6] == 19 and fc.same_bits(fl["drone"][6], before["drone"][6])
    assert fl["flags"].sum() == 0
    # `first` writes the row the drone is on; without it (and with rows flown before) that row stays
    again = fc.copy_of(before)
    again["flown_len"][:] = np.where(again["cmd_len"] > 0, 1, 0)
    fc.model_launch(again, d, 60, first=0)
    assert np.isnan(again["flown"][2, 0]).all() and np.isfinite(fl["flown"][2, 0]).all()
    assert fc.same_bits(again["flown"][2, 1:], fl["flown"][2, 1:])
    # the header does the same
    host = fc.copy_of(before)
    host_launch(host_exe, host, d, 60, first=1)
    assert not fc.differing(fl, host)


# ------------------------------------------------------------------ settle
def test_settle_ends_at_the_reach_test_at_settle_and_at_cap(host_exe):
    d = fc.MODELS["default"].derived(fc.HZ)
    cap = 240
    base = fc.fleet(5, 31, cap=cap)
    base["cmd_len"][:], base["cmd_index"][:], base["flown_len"][:] = 20, 10, 11
    base["cmd"][:, 19, 1:] = 0.0                                   # the arrays end at rest ...
    base["goal"][:] = base["cmd"][:, 19, 0]                        # ... on their goals
    base["drone"][:, :2] = base["cmd"][:, 10, 0] + [0.3, -0.2]     # the drones lag
    got = {}
    for what, settle, reach in (("reach", 1000, 0.05), ("settle", 4, 1e-9), ("cap", 1000, 1e-9), ("none", 0, 0.05)):
        fl = fc.copy_of(base)
        fc.model_launch(fl, d, cap, settle=settle, reach=reach)
        host = fc.copy_of(base)
        host_launch(host_exe, host, d, cap, settle=settle, reach=reach)
        assert not fc.differing(fl, host), (what, fc.differing(fl, host))
        got[what] = fl
        assert np.all(fl["cmd_index"] == 19)
    assert np.all(got["none"]["flown_len"] == 20) and np.all(got["settle"]["flown_len"] == 24)
    assert np.all(got["cap"]["flown_len"] == cap) and np.all(got["cap"]["flags"] == _lib.NEO_FLEET_FLAG_CMD_FULL)
    assert np.isfinite(got["cap"]["flown"][:, cap - 1]).all()
    r = got["reach"]
    print("settle rows until within reach:", (r["flown_len"] - 20).tolist())
    assert np.all(r["flags"] == 0) and np.all(r["flown_len"] > 20) and np.all(r["flown_len"] < cap)
    for b in range(5):      # the first sub-step that starts within reach is not flown: the row before it is the first within
        n = r["flown_len"][b]
        dist = np.linalg.norm(r["flown"][b, :n, 0] - r["goal"][b], axis=1)
        assert dist[n - 1] < 0.05 and np.all(dist[19:n - 1] >= 0.05) and np.isnan(r["flown"][b, n:]).all()
    assert np.all(got["settle"]["flags"] == 0) and np.all(got["none"]["flags"] == 0)


# ------------------------------------------------------------------ exact following
def test_a_matched_start_on_a_straight_line_is_followed_exactly():
    d = fm.FlightModel(drag=0.0, gust_sigma=0.0).derived(fc.HZ)
    v = np.array([0.75, -0.5])
    rows = np.zeros((120, 3, 2))
    p = np.array([1.0, 2.0])
    for t in range(120):      # rows built as the model integrates: p += h * v
        if t:
            p = p + np.float64(d.h) * v
        rows[t, 0], rows[t, 1] = p, v
    f = fm.fly(fm.FlightModel(drag=0.0), fc.HZ, rows, rows[0, 0], rows[0, 1])
    assert f.n == 120 and fc.same_bits(f.rows(), rows) and not f.saturated_rows
    rec, count, flags = fm.fly_error(f.rows(), rows, 1)
    assert count == 120 and flags == 0 and rec[0] == 0.0 and rec[1] == 0.0 and rec[3] == 0.0 and rec[5] == 0.0
    # and a drag or a start that is off shows
    g = fm.fly(fm.FlightModel(), fc.HZ, rows, rows[0, 0], rows[0, 1])
    assert fm.fly_error(g.rows(), rows, 1)[0][1] > 0.0


# ------------------------------------------------------------------ the tracking-error record
@pytest.mark.parametrize("stride", [1, 6])
@pytest.mark.parametrize("n", [0, 1, 7])
def test_fly_error_equals_the_plain_loop(n, stride):
    rng = np.random.default_rng([n, stride])
    flown, cmds = rng.normal(0.0, 1.0, (n, 3, 2)), rng.normal(0.0, 1.0, (max(n - 2, 1), 3, 2))      # (the last rows: settle rows)
    rec, count, flags = fm.fly_error(flown, cmds, stride)
    want = fc.error_restated(flown, cmds, stride)
    assert count == want["count"] == len(range(0, n, stride)) and flags == want["flags"] == 0
    if n == 0:
        assert np.isnan(rec).all()
        return
    for k, name in enumerate(_lib.FLY_FIELDS):
        if name.endswith("_rms"):
            assert abs(rec[k] - want[name]) <= 1e-12 * want[name], name
        else:
            assert rec[k] == want[name], name
    bad = flown.copy()
    bad[0, 1, 0] = np.inf
    rec, count, flags = fm.fly_error(bad, cmds, stride)
    assert np.isnan(rec).all() and count == 0 and flags == _lib.NEO_AUDIT_FLAG_NONFINITE


# ------------------------------------------------------------------ the gust draws
def test_gust_draws_are_the_counter_streams_of_domain_4():
    assert fm.DOMAIN_GUST == 4 and fm.DOMAIN_GUST not in (counter_rng.DOMAIN_RETRY, counter_rng.DOMAIN_TARGET, 3)
    seed, mid = 2 ** 40 + 5, 12345
    got = fm.gust_draws(seed, mid, [0, 1, 9, 2 ** 20])
    for k, a in enumerate([0, 1, 9, 2 ** 20]):
        assert fc.same_bits(got[k], counter_rng.stream_normals(seed, [mid], a, 0, 4, 2)[0])
    # and they are what a sub-step adds: g = rho * g + scale * z at t % gust_every == 0, nothing between
    d = fc.MODELS["gust6"].derived(fc.HZ)
    assert d.gust_every == 6 and d.rho == np.exp(-0.1) and d.scale == 0.3 * np.sqrt(1.0 - d.rho * d.rho)
    s = np.zeros(8)
    for t in range(1, 13):
        g = s[6:8].copy()
        fm.substep(d, mid, t, np.zeros(6), s)
        want = np.float64(d.rho) * g + np.float64(d.scale) * fm.gust_draws(d.seed, mid, [t // 6])[0] if t % 6 == 0 else g
        assert fc.same_bits(s[6:8], want), t
    assert fm.FlightModel().derived(60).gust_every == 6 and fm.FlightModel().derived(300).gust_every == 30
    assert fm.FlightModel().derived(4).gust_every == 1 and fm.FlightModel().derived(60).scale == 0.0


# ------------------------------------------------------------------ header and exports
NEW = {"neo_fleet_fly_dev": 24, "neo_fleet_fly_error_dev": 13}


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(REPO, "include", "neo_planner.h")).read()
    build.build()
    lib = _lib.load()
    for name, nargs in NEW.items():
        m = re.search(r"^int %s\(neo_ctx \*ctx,([^)]*)\)\s*;" % name, header, re.M)
        assert m, name
        assert len(m.group(1).split(",")) + 1 == nargs, name
        assert not re.search(r"int B,\s*const int32_t \*subset,\s*int n_subset", m.group(1)), name
        assert name in _lib.EXPORTS
        assert len(getattr(lib, name).argtypes) == nargs, name
    assert re.search(r"^#define NEO_FLY_FIELDS 6\b", header, re.M) and _lib.NEO_FLY_FIELDS == 6
    for k, name in enumerate(_lib.FLY_FIELDS):
        assert re.search(r"^\s*NEO_FLY_%s = %d\b" % (name.upper(), k), header, re.M), name
    fields = re.search(r"typedef struct neo_flight_model \{(.*?)\} neo_flight_model;", header, re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [f[0] for f in _lib.NeoFlightModel._fields_] == list(fm.Derived._fields)
    for h in ("neo_flight.hpp", "neo_track.hpp", "neo_legs.hpp", "neo_fleet.hpp"):   # the fleet unit's alone
        assert [s for s in build.SOURCES if h in build.headers_of(s)] == ["neo_disp_fleet.hip"], h
    assert npa.FlightModel is fm.FlightModel and "FlightModel" in npa.__all__


# ------------------------------------------------------------------ refusals
def test_flight_model_refusals():
    ok = fm.FlightModel()
    assert (ok.kp, ok.kv, ok.tau, ok.a_max, ok.drag, ok.gust_sigma, ok.gust_tau, ok.gust_every, ok.seed) == \
        (8.0, 5.0, 0.08, 6.0, 0.1, 0.0, 1.0, None, 0)
    fm.FlightModel(kp=0.0, kv=0.0, tau=0.0, drag=0.0, gust_every=1, seed=2 ** 64 - 1)
    for kw in (dict(kp=float("nan")), dict(kv=float("inf")), dict(tau=float("nan")), dict(a_max=float("inf")),
               dict(drag=float("nan")), dict(gust_sigma=float("inf")), dict(gust_tau=float("nan")),
               dict(kp=-1.0), dict(kv=-0.1), dict(drag=-0.1), dict(gust_sigma=-0.3), dict(tau=-0.01), dict(a_max=0.0),
               dict(a_max=-1.0), dict(gust_tau=0.0), dict(gust_every=0), dict(gust_every=-3), dict(gust_every=1.5),
               dict(seed=-1), dict(seed=2 ** 64)):
        with pytest.raises(ValueError):
            fm.FlightModel(**kw)
    for hz in (0.0, -60.0, float("nan")):
        with pytest.raises(ValueError):
            ok.derived(hz)


def test_fleet_loop_refuses_campaigns_with_a_model_before_any_device_use():
    class Cfg:
        v_max, init_wpts_num = 1.0, 2

    class FakePlanner:      # (no context: anything that touched the device would raise AttributeError)
        cfg = Cfg()
    sig = inspect.signature(npa.FleetReplanLoop.__init__).parameters
    assert sig["flight"].default is None and sig["settle_seconds"].default == 2.0
    seq = npa.GoalSequences.from_lists([[[3.0, 0.0], [6.0, 1.0]]])
    with pytest.raises(ValueError, match="goal_sequences"):
        npa.FleetReplanLoop(FakePlanner(), None, None, goal_sequences=seq, flight=fm.FlightModel())
    with pytest.raises(ValueError):
        npa.FleetReplanLoop(FakePlanner(), None, [[3.0, 0.0]], flight="px4")
    with pytest.raises(ValueError):
        npa.FleetReplanLoop(FakePlanner(), None, [[3.0, 0.0]], flight=fm.FlightModel(), settle_seconds=-1.0)
    loop = npa.FleetReplanLoop(FakePlanner(), None, [[3.0, 0.0]], flight=fm.FlightModel(gust_sigma=0.3, seed=9), cmd_hz=60)
    assert tuple(getattr(loop._fly_model, k) for k in fm.Derived._fields) == tuple(fm.FlightModel(gust_sigma=0.3, seed=9).derived(60))
    assert npa.FleetReplanLoop(FakePlanner(), None, [[3.0, 0.0]])._fly_model is None


# ------------------------------------------------------------------ the CPU loop
KEYS_TODAY = {"success", "replans", "failed_attempts", "iter_num", "opt_runs", "path", "min_clearance", "duration", "max_speed"}


def _oracle_run(**kw):
    grid = onp.GridESDF(synth.occupancy_2d(3), synth.RES, 300, 300, ORIGIN)
    np.random.seed(503)
    loop = ReplanLoop(onp.OraclePlanner(onp.PlannerParams()), grid, **kw)
    return loop, loop.run(max_replans=3)


def test_cpu_loop_flies_the_model_and_is_what_it_was_without_one():
    model = fm.FlightModel(gust_sigma=0.3, seed=5)
    loop, out = _oracle_run(flight=model, mission_id=4)
    cmds, path = out["commands"], out["path"]
    assert out["replans"] == 4 and cmds.shape[0] == path.shape[0] > 400 and cmds is loop.des_state_array
    err = np.linalg.norm(path - cmds[:, 0], axis=1)
    print(f"flown against commanded over {len(path)} rows: rms {np.sqrt(np.mean(err ** 2)):.4f} max {err.max():.4f} m; record rms "
          f"{out['fly_pos_err_rms']:.4f} max {out['fly_pos_err_max']:.4f} final {out['fly_pos_err_final']:.4f}, "
          f"{out['fly_saturated']} saturated")
    assert err.max() > 1e-3 and np.array_equal(path[0], [0.0, 0.0])
    again = fm.fly(model, 60, cmds, (0.0, 0.0), mission_id=4)
    assert fc.same_bits(again.rows()[:, 0], path) and fc.same_bits(again.rows(), out["flown"])
    assert out["fly_count"] == len(range(0, len(path), 6)) and out["fly_flags"] == 0
    assert out["fly_pos_err_max"] == err[::6].max() and out["fly_saturated"] == len(again.saturated_rows)
    # without a model: today's keys and today's values -- the path is the command array's positions
    plain_loop, plain = _oracle_run()
    none_loop, none = _oracle_run(flight=None)
    assert set(plain) == set(none) == KEYS_TODAY
    for k in KEYS_TODAY:
        assert np.array_equal(plain[k], none[k]), k
    assert np.array_equal(plain["path"], plain_loop.des_state_array[:, 0, :])
    assert np.array_equal(plain_loop.des_state_array, none_loop.des_state_array)
    # the drone's lag moved the local targets: the plans are other plans
    assert not np.array_equal(plain_loop.des_state_array[:len(cmds)], cmds[:len(plain_loop.des_state_array)])


def test_tracker_loop_flies_the_model_too():
    import track_cases as tc
    from neo_planner_amd.replan import TrackerLoop
    grid = onp.GridESDF(synth.occupancy_2d(3), synth.RES, 300, 300, ORIGIN)
    model = fm.FlightModel(gust_sigma=0.3, seed=5)
    route = tc.flight_routes().take([0])
    np.random.seed(503)
    out = TrackerLoop(onp.OraclePlanner(onp.PlannerParams()), grid, flight=model, mission_id=2).run_tracking(route, 3, (0.0, 0.0))
    assert out["replans"] == 4 and out["n_flown"] == 181 and out["path"].shape == (181, 2) and len(out["commands"]) > 181
    again = fm.fly(model, 60, out["commands"][:181], (0.0, 0.0), mission_id=2)
    assert fc.same_bits(again.rows()[:, 0], out["path"]) and not np.array_equal(out["path"], out["commands"][:181, 0])
    assert out["fly_count"] == 31 and out["fly_flags"] == 0 and 0.0 < out["fly_pos_err_max"] < 0.5
    plain = TrackerLoop(onp.OraclePlanner(onp.PlannerParams()), grid).run_tracking(route, 3, (0.0, 0.0))
    assert not [k for k in plain if k.startswith("fly_")] and np.array_equal(plain["path"], plain["commands"][:181, 0])
