"""Fleet goal routes on the GPU (csrc/neo_track.hpp, neo_fleet_goal_route / neo_fleet_hold_dev / neo_fleet_track_audit,
FleetReplanLoop(goal_routes=...)): the goal kernel against goal_routes.GoalRoutes bit for bit, the hold against NumPy row
copies, the track audit against a NumPy restatement, a fleet of one against replan.TrackerLoop on the CPU oracle, a
mission's independence of the fleet it chases in, a tick whose every target fails, and a fixed-goal control."""
import ctypes
import functools

import numpy as np
import pytest

import depth_oracle_np as don
import neo_planner_amd as npa
from neo_planner_amd import _lib, synth
from neo_planner_amd.depth import DepthCamera
from neo_planner_amd.goal_routes import GoalRoutes
from neo_planner_amd.record import DemoRecorder
from neo_planner_amd.replan import TrackerLoop
from oracle import minco_np as onp

import track_cases as tc

pytestmark = pytest.mark.gpu

ORIGIN = (0.0, -15.0)
SENTINEL = 777.0
NAN_FLAG = _lib.NEO_AUDIT_FLAG_NONFINITE


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run(ctx, fn, *args):
    """a `_dev` call between torch's stream and the context's"""
    torch, dev = _torch()
    torch.cuda.synchronize(dev)
    ctx.check(fn(ctx.h, *args))
    ctx.synchronize()


def _tiled(B):
    """B routes: the CPU test's route set, over and over"""
    rs = tc.route_set()
    return rs.take(np.arange(B) % rs.B)


@pytest.fixture(scope="module")
def map3():
    m = npa.ESDF()
    m.occupancy_map_cb(synth.OccupancyGridMsg(synth.occupancy_2d(3)))
    return m


# ------------------------------------------------------------------ 1. the goal kernel
@pytest.mark.parametrize("B", [1, 64, 65, 257])
def test_goal_kernel_equals_the_model_bit_for_bit(B):
    torch, dev = _torch()
    ctx = _lib.default_context()
    routes = _tiled(B)
    rng = np.random.default_rng(B)
    d_v, d_rb, d_sp, d_cl = _dev(routes.vertices), _dev(routes.route_begin), _dev(routes.speed), _dev(routes.closed)
    nv = len(routes.vertices)
    times = [0.0, 1.0, 5.0, 17.0, 30.0 + 1.0 / 60.0, 12345.678]
    for k, t in enumerate(times):
        want = routes.at(t)
        goal = torch.full((B, 2), SENTINEL, dtype=torch.float64, device=dev)
        _run(ctx, ctx.lib.neo_fleet_goal_route_dev, B, None, 0, _p(d_v), nv, _p(d_rb), _p(d_sp), _p(d_cl), t, _p(goal))
        got = goal.cpu().numpy()
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (t, np.flatnonzero((got != want).any(axis=1))[:5])
        # a subset that skips missions, in another order, with indices outside 0 .. B - 1: the same bits, the rest untouched
        pick = rng.permutation(B)[:max(1, (2 * B) // 3)]
        sub = (np.concatenate([[B], pick, [-1, B + 9]]) if B > 1 else pick).astype(np.int32)      # (at most B entries)
        goal2 = torch.full((B, 2), SENTINEL, dtype=torch.float64, device=dev)
        d_sub = _dev(sub)
        _run(ctx, ctx.lib.neo_fleet_goal_route_dev, B, _p(d_sub), len(sub), _p(d_v), nv, _p(d_rb), _p(d_sp), _p(d_cl), t, _p(goal2))
        got2 = goal2.cpu().numpy()
        on = np.isin(np.arange(B), pick)
        assert np.array_equal(got2[on].view(np.uint64), want[on].view(np.uint64)) and np.all(got2[~on] == SENTINEL)
        if k < 2:      # the host form
            gh = np.full((B, 2), SENTINEL)
            ctx.check(ctx.lib.neo_fleet_goal_route(ctx.h, B, _lib.ptr(sub), len(sub), _lib.ptr(routes.vertices), nv,
                                                   _lib.ptr(routes.route_begin), _lib.ptr(routes.speed), _lib.ptr(routes.closed),
                                                   t, _lib.ptr(gh)))
            assert np.array_equal(gh.view(np.uint64), got2.view(np.uint64))


def test_goal_kernel_at_the_times_that_sit_on_vertices():
    """every route of the set at its own special times (s exactly on a vertex, past the end, several laps): one mission a
    launch through a subset"""
    torch, dev = _torch()
    ctx = _lib.default_context()
    routes = tc.route_set()
    B, nv = routes.B, len(routes.vertices)
    d_v, d_rb, d_sp, d_cl = _dev(routes.vertices), _dev(routes.route_begin), _dev(routes.speed), _dev(routes.closed)
    goal = torch.full((B, 2), SENTINEL, dtype=torch.float64, device=dev)
    n = 0
    for b in range(B):
        d_sub = _dev(np.array([b], np.int32))
        one = routes.take([b])
        for t in tc.route_times(routes, b)[7:22]:
            _run(ctx, ctx.lib.neo_fleet_goal_route_dev, B, _p(d_sub), 1, _p(d_v), nv, _p(d_rb), _p(d_sp), _p(d_cl), float(t), _p(goal))
            assert np.array_equal(goal[b].cpu().numpy().view(np.uint64), one.at(float(t))[0].view(np.uint64)), (b, t)
            n += 1
    assert n > 100


def test_a_bad_route_gets_nan_and_touches_no_other_row():
    torch, dev = _torch()
    ctx = _lib.default_context()
    v = np.random.default_rng(4).uniform(0.0, 20.0, (260, 2))
    rb = np.array([0, 1, 3, 260], np.int32)          # 1, 2 and 257 vertices
    sp = np.ones(3)
    goal = torch.full((3, 2), SENTINEL, dtype=torch.float64, device=dev)
    d_v, d_rb, d_sp = _dev(v), _dev(rb), _dev(sp)
    _run(ctx, ctx.lib.neo_fleet_goal_route_dev, 3, None, 0, _p(d_v), 260, _p(d_rb), _p(d_sp), None, 0.5, _p(goal))
    got = goal.cpu().numpy()
    assert np.isnan(got[[0, 2]]).all()
    assert np.array_equal(got[1], GoalRoutes(v[1:3], [0, 2], [1.0]).at(0.5)[0])
    # a table shorter than route_begin says: no read past it
    _run(ctx, ctx.lib.neo_fleet_goal_route_dev, 3, None, 0, _p(d_v), 2, _p(d_rb), _p(d_sp), None, 0.5, _p(goal))
    assert np.isnan(goal.cpu().numpy()).all()
    cmd = _dev(np.zeros((3, 8, 3, 2)))
    nf = _dev(np.full(3, 8, np.int32))
    track = torch.full((3, _lib.NEO_TRACK_FIELDS), SENTINEL, dtype=torch.float64, device=dev)
    count = torch.full((3,), -1, dtype=torch.int32, device=dev)
    flags = count.clone()
    _run(ctx, ctx.lib.neo_fleet_track_audit_dev, 3, None, 0, _p(cmd), 8, _p(nf), 1, 60.0, _p(d_v), 260, _p(d_rb), _p(d_sp), None,
         1.0, _p(track), _p(count), _p(flags))
    tr = track.cpu().numpy()
    assert np.isnan(tr[[0, 2]]).all() and not np.isnan(tr[1]).any()
    assert count.cpu().numpy().tolist() == [0, 8, 0] and flags.cpu().numpy().tolist() == [NAN_FLAG, 0, NAN_FLAG]


def test_track_argument_errors():
    torch, dev = _torch()
    ctx = _lib.default_context()
    L = ctx.lib
    z = torch.zeros(256, dtype=torch.float64, device=dev)
    zi = torch.zeros(8, dtype=torch.int32, device=dev)
    goal = lambda v=_p(z), nv=4, t=0.0, out=_p(z), n_sub=0, sub=None: L.neo_fleet_goal_route_dev(
        ctx.h, 2, sub, n_sub, v, nv, _p(zi), _p(z), None, t, out)
    assert goal() == 0
    assert goal(v=None) == 1 and goal(out=None) == 1 and goal(nv=-1) == 1 and goal(t=float("inf")) == 1
    assert goal(sub=_p(zi), n_sub=3) == 1
    hold = lambda cmd=_p(z), cap=4, step=2, fl=_p(zi): L.neo_fleet_hold_dev(ctx.h, 2, None, 0, cmd, cap, _p(zi), _p(zi), step, fl)
    assert hold() == 0
    assert hold(cmd=None) == 1 and hold(cap=0) == 1 and hold(step=0) == 1 and hold(fl=None) == 1
    assert hold(cmd=ctypes.c_void_p(z.data_ptr() + 8)) == 1 and b"aligned" in L.neo_last_error(ctx.h)
    aud = lambda cap=4, stride=1, hz=60.0, radius=1.0, out=_p(z): L.neo_fleet_track_audit_dev(
        ctx.h, 2, None, 0, _p(z), cap, _p(zi), stride, hz, _p(z), 4, _p(zi), _p(z), None, radius, out, _p(zi), _p(zi))
    assert aud() == 0
    assert aud(cap=0) == 1 and aud(stride=0) == 1 and aud(hz=0.0) == 1 and aud(hz=float("nan")) == 1 and aud(out=None) == 1
    assert aud(radius=float("nan")) == 1
    ctx.synchronize()


# ------------------------------------------------------------------ 2. the hold kernel
@pytest.mark.parametrize("step", [7, 60])
def test_hold_equals_numpy_row_copies(step):
    torch, dev = _torch()
    ctx = _lib.default_context()
    rng = np.random.default_rng(step)
    cap, guard = 3 * step + 11, 512
    # (cmd_index, cmd_len): pads of 0, 1, step and step + 1 rows, nothing planned, need == cap, need == cap + 1, a full array,
    # an array far behind, and one that is long enough by far
    cases = [(5, 5 + step + 1), (5, 5 + step), (5, 6), (5, 5), (0, 0), (cap - step - 1, cap - step), (cap - step, cap - step + 1),
             (cap - 1, cap), (2 * step, 3), (0, cap - 2), (0, 1), (-4, 2)]
    B = len(cases)
    cmd = rng.normal(0, 1, (B, cap, 3, 2))
    idx = np.array([c[0] for c in cases], np.int32)
    ln = np.array([c[1] for c in cases], np.int32)
    want, want_len, want_flags = cmd.copy(), ln.copy(), np.zeros(B, np.int32)
    for b in range(B):
        need = max(int(idx[b]), 0) + step + 1
        if ln[b] >= 1 and ln[b] < need:
            upto = min(need, cap)
            want[b, ln[b]:upto] = cmd[b, ln[b] - 1]
            want_len[b] = upto
            if need > cap:
                want_flags[b] = _lib.NEO_FLEET_FLAG_CMD_FULL
    assert want_flags.tolist().count(_lib.NEO_FLEET_FLAG_CMD_FULL) == 2 and want_len[5] == cap and want_flags[5] == 0
    for sub in (None, np.array([B + 1, 7, 2, 0, 6, -1, 9], np.int32)):
        buf = torch.full((B * cap * 6 + guard,), SENTINEL, dtype=torch.float64, device=dev)
        buf[:B * cap * 6] = _dev(cmd).reshape(-1)
        d_len, d_idx = _dev(ln), _dev(idx)
        d_flags = torch.full((B,), 16, dtype=torch.int32, device=dev)      # (OR-ed in: what was there stays)
        d_sub = None if sub is None else _dev(sub)
        _run(ctx, ctx.lib.neo_fleet_hold_dev, B, _p(d_sub), 0 if sub is None else len(sub), _p(buf), cap, _p(d_len), _p(d_idx), step,
             _p(d_flags))
        out = buf.cpu().numpy()
        assert np.all(out[B * cap * 6:] == SENTINEL), "written past the buffer"
        got = out[:B * cap * 6].reshape(B, cap, 3, 2)
        on = np.ones(B, bool) if sub is None else np.isin(np.arange(B), sub)
        assert np.array_equal(got[on], want[on]) and np.array_equal(got[~on], cmd[~on])      # rows beyond the pad keep theirs
        assert np.array_equal(d_len.cpu().numpy(), np.where(on, want_len, ln))
        assert np.array_equal(d_flags.cpu().numpy(), 16 | np.where(on, want_flags, 0))
        assert np.array_equal(d_idx.cpu().numpy(), idx)


# ------------------------------------------------------------------ 3. the track audit
COUNTS = (0, 1, 63, 64, 65, 256, 257)      # 257: one past a full round of four samples a lane


def _audit_cases():
    rng = np.random.default_rng(31)
    rs = tc.route_set()
    hz, radius = 60.0, 1.0
    cap = 256 * 6 + 8
    spec = [(c, s) for s in (1, 6) for c in COUNTS] + [(70, 6), (70, 1), (40, 6)]      # then: two ties, a NaN row
    B = len(spec)
    routes = rs.take((np.arange(B) * 3 + 1) % rs.B)
    cmd = rng.normal(0, 1, (B, cap, 3, 2))
    n_flown = np.zeros(B, np.int32)
    stride = np.array([s for _, s in spec])
    for b, (cnt, s) in enumerate(spec):
        n_flown[b] = 0 if cnt == 0 else (cnt - 1) * s + 1 + (int(rng.integers(0, s)) if b % 2 else 0)
        one = routes.take([b])
        t = np.arange(cap) / hz
        goal = np.stack([one.at(float(tt))[0] for tt in t[:max(int(n_flown[b]), 1)]])
        cmd[b, :len(goal), 0] = goal + rng.normal(0, 0.8, goal.shape)
    tie_a, tie_b, nan_b = B - 3, B - 2, B - 1
    for b, (j0, j1) in ((tie_a, (5, 38)), (tie_b, (5, 69))):      # gap exactly 0 twice: on two lanes, and on one lane
        for j in (j0, j1):
            r = j * stride[b]
            cmd[b, r, 0] = routes.take([b]).at(r / hz)[0]
    cmd[nan_b, 12 * 6, 1, 0] = np.nan
    return dict(B=B, cap=cap, hz=hz, radius=radius, routes=routes, cmd=cmd, n_flown=n_flown, stride=stride, spec=spec,
                ties=(tie_a, tie_b), nan_b=nan_b)


@pytest.fixture(scope="module")
def audit_cases():
    cs = _audit_cases()
    cs["ref"] = [tc.track_restated(cs["cmd"][b], int(cs["n_flown"][b]), int(cs["stride"][b]), cs["hz"], cs["routes"].take([b]),
                                   cs["radius"]) for b in range(cs["B"])]
    return cs


@pytest.mark.parametrize("stride", [1, 6])
def test_track_audit_equals_the_restatement(audit_cases, stride):
    torch, dev = _torch()
    ctx = _lib.default_context()
    cs = audit_cases
    B, cap, hz, radius, routes = cs["B"], cs["cap"], cs["hz"], cs["radius"], cs["routes"]
    mine = np.flatnonzero(cs["stride"] == stride).astype(np.int32)
    assert sorted(cs["ref"][b]["count"] for b in mine if b < 14) == list(COUNTS)
    d_cmd, d_nf = _dev(cs["cmd"]), _dev(cs["n_flown"])
    d_v, d_rb, d_sp, d_cl = _dev(routes.vertices), _dev(routes.route_begin), _dev(routes.speed), _dev(routes.closed)
    nv = len(routes.vertices)

    def device(sub):
        track = torch.full((B, _lib.NEO_TRACK_FIELDS), SENTINEL, dtype=torch.float64, device=dev)
        count = torch.full((B,), -1, dtype=torch.int32, device=dev)
        flags = count.clone()
        d_sub = _dev(sub)
        _run(ctx, ctx.lib.neo_fleet_track_audit_dev, B, _p(d_sub), len(sub), _p(d_cmd), cap, _p(d_nf), stride, hz, _p(d_v), nv,
             _p(d_rb), _p(d_sp), _p(d_cl), radius, _p(track), _p(count), _p(flags))
        return track.cpu().numpy(), count.cpu().numpy(), flags.cpu().numpy()

    track, count, flags = device(mine)
    F = {name: k for k, name in enumerate(_lib.TRACK_FIELDS)}
    for b in mine:
        r = cs["ref"][b]
        assert count[b] == r["count"] and flags[b] == r["flags"], (b, count[b], r["count"], flags[b], r["flags"])
        if r["count"] == 0:
            assert np.isnan(track[b]).all()
            continue
        for f in ("gap_max", "t_gap_max", "gap_min", "t_gap_min", "gap_final", "t_first_within", "frac_within"):
            assert track[b, F[f]] == r[f], (b, f, track[b, F[f]], r[f])
        assert abs(track[b, F["gap_mean"]] - r["gap_mean"]) <= 1e-12 * abs(r["gap_mean"]), (b, track[b, F["gap_mean"]], r["gap_mean"])
    within = [cs["ref"][b]["frac_within"] for b in mine if cs["ref"][b]["count"] > 1]
    assert min(within) < 0.9 and max(within) > 0.1 and any(cs["ref"][b].get("t_first_within", 0) > 0 for b in mine)
    for b in cs["ties"]:      # a tie in the minimum goes to the first sample
        if b in mine:
            assert track[b, F["gap_min"]] == 0.0 and track[b, F["t_gap_min"]] == (5 * stride) / hz
            assert np.count_nonzero(cs["ref"][b]["gaps"] == 0.0) == 2
    if cs["nan_b"] in mine:      # a row that is not finite: the NaN record
        assert np.isnan(track[cs["nan_b"]]).all() and count[cs["nan_b"]] == 0 and flags[cs["nan_b"]] == NAN_FLAG
    other = ~np.isin(np.arange(B), mine)
    assert np.all(track[other] == SENTINEL) and np.all(count[other] == -1) and np.all(flags[other] == -1)
    # the same bits for another order with indices to skip, and from host arrays
    order2 = np.concatenate([[B + 2], mine[::-1], [-1]]).astype(np.int32)
    t2, c2, f2 = device(order2)
    assert np.array_equal(t2, track, equal_nan=True) and np.array_equal(c2, count) and np.array_equal(f2, flags)
    th = np.full((B, _lib.NEO_TRACK_FIELDS), SENTINEL)
    ch = np.full(B, -1, np.int32)
    fh = np.full(B, -1, np.int32)
    ctx.check(ctx.lib.neo_fleet_track_audit(ctx.h, B, _lib.ptr(mine), len(mine), _lib.ptr(cs["cmd"]), cap, _lib.ptr(cs["n_flown"]),
                                            stride, hz, _lib.ptr(routes.vertices), nv, _lib.ptr(routes.route_begin),
                                            _lib.ptr(routes.speed), _lib.ptr(routes.closed), radius, _lib.ptr(th), _lib.ptr(ch),
                                            _lib.ptr(fh)))
    assert np.array_equal(th, track, equal_nan=True) and np.array_equal(ch, count) and np.array_equal(fh, flags)


# ------------------------------------------------------------------ 4. a fleet of one against the CPU oracle
@functools.lru_cache(maxsize=None)
def _oracle_flight(b):
    grid = onp.GridESDF(synth.occupancy_2d(3), synth.RES, 300, 300, ORIGIN)
    np.random.seed(503)
    state = np.random.get_state()
    ref = TrackerLoop(onp.OraclePlanner(onp.PlannerParams()), grid).run_tracking(tc.flight_routes().take([b]), tc.FLIGHT_TICKS,
                                                                                 (0.0, 0.0))
    after = np.random.get_state()
    assert np.array_equal(after[1], state[1]) and after[2:] == state[2:], "the oracle flight drew random numbers: not comparable"
    return ref


def _check_track_fields(loop, out, i, route_of_one):
    r = tc.track_restated(loop.commands(i), int(out["n_flown"][i]), loop.stride, float(loop.cmd_hz), route_of_one, loop.track_radius)
    assert out["track_count"][i] == r["count"] and out["track_flags"][i] == 0
    for f in ("gap_max", "t_gap_max", "gap_min", "t_gap_min", "gap_final", "t_first_within", "frac_within"):
        assert out["track_" + f][i] == r[f], (f, out["track_" + f][i], r[f])
    assert abs(out["track_gap_mean"][i] - r["gap_mean"]) <= 1e-12 * abs(r["gap_mean"])


@pytest.mark.parametrize("b", [0, 1, 2])
def test_fleet_of_one_flies_the_tracker_oracle_flight(map3, b):
    ref = _oracle_flight(b)
    route = tc.flight_routes().take([b])
    loop = npa.FleetReplanLoop(npa.BatchPlanner(), map3, None, goal_routes=route)
    out = loop.run([[0.0, 0.0]], max_replans=tc.FLIGHT_TICKS)
    cmd = loop.commands(0)
    n = min(len(cmd), len(ref["commands"]))
    diff = np.max(np.linalg.norm(cmd[:n, 0] - ref["commands"][:n, 0], axis=1))
    print(f"route {b}: fleet {out['replans'][0]} plans, {out['failed_attempts'][0]} failed, {out['failed_ticks'][0]} failed ticks, "
          f"iterations {out['iter_num'][0]}, {out['n_flown'][0]} flown of {out['n_cmd'][0]}; oracle {ref['replans']} plans, "
          f"{ref['failed_attempts']} failed, {ref['failed_ticks']} failed ticks, iterations {ref['iter_num']}, {ref['n_flown']} flown "
          f"of {len(ref['commands'])}; max position difference {diff:.4f} m; gap mean {out['track_gap_mean'][0]:.3f} min "
          f"{out['track_gap_min'][0]:.3f} final {out['track_gap_final'][0]:.3f}, within {out['track_frac_within'][0]:.2f}")
    assert out["replans"][0] == ref["replans"] == 31 and out["failed_attempts"][0] == ref["failed_attempts"]
    assert out["failed_ticks"][0] == ref["failed_ticks"]
    assert out["n_flown"][0] == ref["n_flown"] == 1801 and out["n_cmd"][0] == len(cmd)
    assert diff < 0.25
    assert abs(out["iter_num"][0] - ref["iter_num"]) <= 0.2 * ref["iter_num"] + 5
    assert bool(out["success"][0]) and out["flags"][0] == 0 and not out["abandoned"][0]
    assert np.array_equal(out["goal_final"][0], route.at(tc.FLIGHT_TICKS * 60 / 60.0)[0])
    assert abs(out["final_dist"][0] - np.linalg.norm(cmd[1800, 0] - out["goal_final"][0])) <= 1e-12
    assert out["count"][0] == (1801 + 5) // 6 == out["track_count"][0]
    # metric weights (1, 1, 1) (:175)
    assert out["weighted"][0] == 1.0 * out["path_length"][0] + 1.0 * out["feasibility"][0] + 1.0 * out["collision"][0]
    _check_track_fields(loop, out, 0, route)
    if b == 2:      # the goal stopped at the end of its route: the drone arrived and holds there
        assert out["final_dist"][0] < loop.target_reach_threshold and out["track_gap_final"][0] < loop.target_reach_threshold


# ------------------------------------------------------------------ 5. a mission chases the same alone and in a fleet
def _fleet_of_8():
    fr = tc.flight_routes()
    extra = [([[20.0, -5.0], [10.0, -9.0], [25.0, 3.0]], 0.7, True), ([[12.0, 6.0], [26.0, -2.0]], 0.3, False),
             ([[5.0, -3.0], [9.0, -4.0], [16.0, 2.0], [22.0, 1.0]], 1.2, False), ([[27.0, 9.0], [18.0, -10.0]], 0.9, True),
             ([[6.0, 4.5], [6.0, 4.5], [15.0, 0.0]], 0.4, False)]
    routes = GoalRoutes.from_lists([fr.route(b) for b in range(3)] + [e[0] for e in extra],
                                   list(fr.speed) + [e[1] for e in extra], list(fr.closed) + [e[2] for e in extra])
    start = np.array([[0.0, 0.0]] * 3 + [[0.5, -2.0], [0.5, 3.0], [1.0, -6.0], [0.5, 1.0], [0.5, 0.5]])
    return routes, start


@pytest.mark.parametrize("mode,resident", [("basic", False), ("basic", True), ("warmstart", True)])
def test_a_mission_chases_the_same_alone_and_in_a_fleet(map3, mode, resident):
    routes, start = _fleet_of_8()
    ticks = 10
    kw = dict(mode=mode, resident=resident, seed=41, max_cmd_seconds=60)
    loop = npa.FleetReplanLoop(npa.BatchPlanner(), map3, None, goal_routes=routes, **kw)
    out = loop.run(start, max_replans=ticks)
    print(f"{mode} resident={resident}: plans {out['replans'].tolist()}, failed attempts {out['failed_attempts'].tolist()}, failed "
          f"ticks {out['failed_ticks'].tolist()}, flags {out['flags'].tolist()}, gap mean {np.round(out['track_gap_mean'], 2).tolist()}")
    assert np.array_equal(out["n_flown"][out["n_cmd"] > 0], np.full(int((out["n_cmd"] > 0).sum()), ticks * 60 + 1))
    assert np.array_equal(out["replans"] + out["failed_ticks"], np.full(8, ticks + 1))
    for i in (0, 2, 5):
        one = npa.FleetReplanLoop(npa.BatchPlanner(), map3, None, goal_routes=routes.take([i]), mission_ids=[i], **kw)
        o1 = one.run(start[i:i + 1], max_replans=ticks)
        assert set(o1) == set(out)
        for k in out:
            assert np.array_equal(np.asarray(o1[k])[0], np.asarray(out[k])[i], equal_nan=True), (i, k, o1[k][0], out[k][i])
        assert np.array_equal(one.commands(0), loop.commands(i)), i
        _check_track_fields(loop, out, i, routes.take([i]))


def test_batch_mode_with_counter_jitter_and_a_recorder_chases(map3):
    routes, start = _fleet_of_8()
    scenes = [don.boxes_of(synth.forest_boxes(3))]
    rec = DemoRecorder(DepthCamera(width=64, height=48), capacity=8 * 8)
    loop = npa.FleetReplanLoop(npa.BatchPlanner(), map3, None, goal_routes=routes, mode="batch", jitter="counter", record=rec,
                               scenes=DepthCamera.pack_scenes(scenes), seed=3, max_cmd_seconds=60)
    out = loop.run(start, max_replans=6)
    print(f"batch/counter/record: plans {out['replans'].tolist()}, failed ticks {out['failed_ticks'].tolist()}, flags "
          f"{out['flags'].tolist()}")
    assert np.all(out["flags"] == 0)
    assert np.array_equal(out["replans"] + out["failed_ticks"], np.full(8, 7))
    assert np.array_equal(out["n_flown"][out["n_cmd"] > 0], np.full(int((out["n_cmd"] > 0).sum()), 361))
    assert np.array_equal(out["goal_final"], routes.at(6.0))


# ------------------------------------------------------------------ 6. a tick whose every target fails
def test_a_tick_whose_targets_all_fail_leaves_the_mission_flying(map3):
    """the goal passes (6, 4.5), a vertex on an occupied cell, exactly at tick 2 (5 m of route at 2.5 m/s); the drone is closer
    than longitu_step_dis then, so all 11 targets are the goal itself, inside the obstacle.  The CPU oracle's TrackerLoop
    flies the same: 3 plans, 11 failed attempts, 1 failed tick."""
    route = GoalRoutes.from_lists([[[3.0, 0.5], [6.0, 4.5], [7.5, 6.5]]], [2.5])
    assert np.array_equal(route.at(2.0)[0], [6.0, 4.5]) and map3.query(np.array([[6.0, 4.5]]))[0][0] < 0.05
    assert all(map3.query(route.at(float(k)))[0][0] >= 1.2 for k in (0, 1, 3))
    loop = npa.FleetReplanLoop(npa.BatchPlanner(), map3, None, goal_routes=route)
    out = loop.run([[3.9, 1.7]], max_replans=3)
    assert [t["active"] for t in loop.timings] == [1, 1, 1, 1] and [t["plans"] for t in loop.timings] == [1, 1, 11, 1]
    assert out["failed_ticks"][0] == 1 and out["failed_attempts"][0] == 11 and out["replans"][0] == 3
    assert not out["abandoned"][0] and out["flags"][0] == 0 and out["n_flown"][0] == 181
    assert np.array_equal(out["goal_final"][0], route.at(3.0)[0])


# ------------------------------------------------------------------ 7. a fixed-goal control
def test_a_fixed_goal_flight_is_what_it_was(map3):
    loop = npa.FleetReplanLoop(npa.BatchPlanner(), map3, [[30.0, 0.0]])
    out = loop.run([[0.0, 0.0]])
    assert not [k for k in out if k.startswith("track_")] and "failed_ticks" not in out and "goal_final" not in out
    assert loop.routes is None and not [k for k in loop._dev if k in ("vertices", "route_begin", "speed", "closed", "track")]
    assert bool(out["success"][0]) and out["n_flown"][0] == out["n_cmd"][0] == len(loop.commands(0))
    assert out["final_dist"][0] < 0.2 and out["flags"][0] == 0
