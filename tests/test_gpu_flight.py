"""The fleet's flight model on the GPU (csrc/neo_flight.hpp, neo_fleet_fly_dev / neo_fleet_fly_error_dev,
FleetReplanLoop(flight=...)): fleet_fly_kernel against flight_model.fly_launch bit for bit, launches that cut a flight,
the settle launch, the row past cap, fleet_fly_error_kernel against a plain loop, the refusals of both entries, a fleet of
one against replan.ReplanLoop on the CPU oracle, a mission's independence of the fleet it flies in, the model next to goal
routes, a recorder and mode "batch", and a control without a model."""
import ctypes
import functools

import numpy as np
import pytest

import depth_oracle_np as don
import neo_planner_amd as npa
from neo_planner_amd import _lib, synth
from neo_planner_amd import flight_model as fm
from neo_planner_amd.depth import DepthCamera
from neo_planner_amd.record import DemoRecorder
from neo_planner_amd.replan import ReplanLoop
from oracle import minco_np as onp

import fleet_flight_cases as ffc
import flight_cases as fc
import track_cases as tc

pytestmark = pytest.mark.gpu

ORIGIN = (0.0, -15.0)
SENTINEL = 777.0
NAN_FLAG = _lib.NEO_AUDIT_FLAG_NONFINITE
INT_KEYS = ("cmd_len", "cmd_index", "future_index", "flown_len", "saturated", "flags", "mission_ids")
F64_KEYS = ("cmd", "goal", "drone", "flown", "cur_pos", "head")


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


def _model_struct(d):
    return _lib.NeoFlightModel(*d)


def to_device(fl):
    return {k: _dev(fl[k]) for k in INT_KEYS + F64_KEYS}


def dev_launch(ctx, D, fl, d, step, ahead=5, first=0, settle=0, reach=0.2, subset=None, cap=None):
    m = _model_struct(d)
    sub = None if subset is None else _dev(np.asarray(subset, np.int32))
    _run(ctx, ctx.lib.neo_fleet_fly_dev, fl["B"], ctypes.byref(m), _p(sub), 0 if subset is None else len(subset), _p(D["cmd"]),
         fl["cap"] if cap is None else cap, _p(D["cmd_len"]), _p(D["cmd_index"]), _p(D["future_index"]), step, ahead, first, settle,
         reach, _p(D["mission_ids"]), _p(D["goal"]), _p(D["drone"]), _p(D["flown"]), _p(D["flown_len"]), _p(D["saturated"]),
         _p(D["flags"]), _p(D["cur_pos"]), _p(D["head"]))


def differing(D, fl):
    return [k for k in fc.STATE if not fc.same_bits(D[k].cpu().numpy(), fl[k])]


@pytest.fixture(scope="module")
def map3():
    m = npa.ESDF()
    m.occupancy_map_cb(synth.OccupancyGridMsg(synth.occupancy_2d(3)))
    yield m
    c = _lib.default_context()      # the context's map table is the session's: leave it as long as it was
    c.check(c.lib.neo_esdf_drop(c.h, m.scene_id))


# ------------------------------------------------------------------ 1. the fly kernel against the model
@pytest.mark.parametrize("name", list(fc.MODELS))
@pytest.mark.parametrize("B", [1, 64, 65, 257])
def test_fly_kernel_equals_the_model_bit_for_bit(B, name):
    ctx = _lib.default_context()
    d = fc.MODELS[name].derived(fc.HZ)
    fl = fc.fleet(B, 100 + B)
    D = to_device(fl)
    rng = np.random.default_rng(B)
    pick = rng.permutation(B)[:max(1, (2 * B) // 3)]
    sub = (np.concatenate([[B], pick, [-1, B + 9]]) if B > 1 else pick).astype(np.int32)      # (at most B entries)
    sat0 = fl["saturated"].copy()
    # a subset that skips missions, in another order, with indices outside 0 .. B - 1; then everybody, twice
    for k, (step, first, subset) in enumerate([(7, 1, sub), (7, 0, None), (60, 0, None)]):
        fc.model_launch(fl, d, step, first=first, subset=subset)
        dev_launch(ctx, D, fl, d, step, first=first, subset=subset)
        assert not differing(D, fl), (B, name, k, differing(D, fl))
        if k == 0 and B > 1:      # the canary rows of every mission that was not launched stay
            off = ~np.isin(np.arange(B), pick)
            assert np.isnan(D["flown"].cpu().numpy()[off]).all() and np.isnan(D["cur_pos"].cpu().numpy()[off]).all()
            assert np.all(D["future_index"].cpu().numpy()[off] == -7)
    flew = fl["cmd_len"] >= 1
    assert np.array_equal(fl["cur_pos"][flew], fl["drone"][flew, :2])
    if name == "saturating" and B > 1:
        assert (fl["saturated"] - sat0).sum() > 5 * B
    if name == "default":
        assert (fl["saturated"] - sat0).sum() == 0


# ------------------------------------------------------------------ 2. two launches equal one
def test_two_launches_equal_one():
    ctx = _lib.default_context()
    d = fc.MODELS["gust6"].derived(fc.HZ)
    base = fc.fleet(65, 23)
    base["cmd_len"][:], base["cmd_index"][:], base["flown_len"][:] = fc.CAP, 2, 3      # rows 3 .. 15: draws at 6 and 12
    whole = to_device(base)
    dev_launch(ctx, whole, base, d, 13)
    want = fc.copy_of(base)
    fc.model_launch(want, d, 13)
    assert not differing(whole, want)
    for cuts in ((6, 7), (5, 1, 7)):
        part = to_device(base)
        for s in cuts:
            dev_launch(ctx, part, base, d, s)
        assert not differing(part, want), (cuts, differing(part, want))


# ------------------------------------------------------------------ 3. the settle launch
def test_the_settle_launch():
    ctx = _lib.default_context()
    d = fc.MODELS["default"].derived(fc.HZ)
    cap = 240
    base = fc.fleet(5, 31, cap=cap)
    base["cmd_len"][:], base["cmd_index"][:], base["flown_len"][:] = 20, 10, 11
    base["cmd"][:, 19, 1:] = 0.0
    base["goal"][:] = base["cmd"][:, 19, 0]
    base["drone"][:, :2] = base["cmd"][:, 10, 0] + [0.3, -0.2]
    lens = {}
    for what, settle, reach in (("reach", 1000, 0.05), ("settle", 4, 1e-9), ("cap", 1000, 1e-9), ("none", 0, 0.05)):
        fl = fc.copy_of(base)
        fc.model_launch(fl, d, cap, settle=settle, reach=reach)
        D = to_device(base)
        dev_launch(ctx, D, base, d, cap, settle=settle, reach=reach)
        assert not differing(D, fl), (what, differing(D, fl))
        lens[what] = fl["flown_len"].copy()
        assert np.all(fl["flags"] == (_lib.NEO_FLEET_FLAG_CMD_FULL if what == "cap" else 0))
    assert np.all(lens["none"] == 20) and np.all(lens["settle"] == 24) and np.all(lens["cap"] == cap)
    assert np.all(lens["reach"] > 20) and np.all(lens["reach"] < cap)


# ------------------------------------------------------------------ 4. nothing at or past cap
def test_nothing_is_written_at_or_past_cap():
    """one mission whose arrays have cap + 1 rows: the settle steps run into cap, raise CMD_FULL, and row cap stays"""
    ctx = _lib.default_context()
    d = fc.MODELS["gust1"].derived(fc.HZ)
    cap = 24
    fl = fc.fleet(1, 7, cap=cap, rows=cap + 1)
    fl["cmd"] = np.concatenate([fl["cmd"], np.full((1, 1, 3, 2), fc.CANARY)], axis=1)      # (the kernel's cap stays 24)
    fl["cmd_len"][:], fl["cmd_index"][:], fl["flown_len"][:] = cap + 5, 3, 4
    D = to_device(fl)
    dev_launch(ctx, D, fl, d, 1000, settle=50, reach=1e-9, cap=cap)
    got = D["flown"].cpu().numpy()
    assert np.isfinite(got[0, 4:cap]).all() and fc.same_bits(got[0, cap], np.full((3, 2), fc.CANARY))
    assert D["flown_len"].cpu().numpy()[0] == cap and D["cmd_index"].cpu().numpy()[0] == cap - 1
    assert D["flags"].cpu().numpy()[0] == _lib.NEO_FLEET_FLAG_CMD_FULL
    want = fc.copy_of(fl)
    want["cmd"], want["flown"] = fl["cmd"][:, :cap], fl["flown"][:, :cap].copy()
    fc.model_launch(want, d, 1000, settle=50, reach=1e-9)
    assert fc.same_bits(got[:, :cap], want["flown"]) and fc.same_bits(D["drone"].cpu().numpy(), want["drone"])


# ------------------------------------------------------------------ 5. the tracking-error kernel
COUNTS = (0, 1, 63, 64, 65, 129)


@pytest.mark.parametrize("stride", [1, 6])
def test_fly_error_kernel_equals_the_restatement(stride):
    torch, dev = _torch()
    ctx = _lib.default_context()
    cap = 129 * 6
    B = len(COUNTS) + 3
    rng = np.random.default_rng(stride)
    flown_len = np.array([0 if c == 0 else (c - 1) * stride + 1 + (stride > 1) * 2 for c in COUNTS] + [200, 200, 300], np.int32)
    cmd_len = np.minimum(flown_len + 5, cap).astype(np.int32)
    cmd_len[2], cmd_len[-1] = max(flown_len[2] - 20, 1), 0      # settle rows: the last command; and a mission without commands
    cmd = rng.normal(0.0, 1.0, (B, cap, 3, 2))
    flown = cmd + rng.normal(0.0, 0.05, (B, cap, 3, 2))
    nan_b = len(COUNTS)
    flown[nan_b, 7 * stride, 1, 1] = np.nan
    cmd[3, [5 * stride, 9 * stride], 0] = 0.0      # a tie in the maximum goes to the first sample
    flown[3, [5 * stride, 9 * stride], 0] = [3.0, 4.0]
    want = [fc.error_restated(flown[b, :flown_len[b]], cmd[b, :max(cmd_len[b], 0)], stride) for b in range(B)]
    assert [w["count"] for w in want[:len(COUNTS)]] == list(COUNTS)
    d_fl, d_cmd, d_n, d_cl = _dev(flown), _dev(cmd), _dev(flown_len), _dev(cmd_len)

    def device(sub):
        rec = torch.full((B, _lib.NEO_FLY_FIELDS), SENTINEL, dtype=torch.float64, device=dev)
        count = torch.full((B,), -1, dtype=torch.int32, device=dev)
        flags = count.clone()
        d_sub = None if sub is None else _dev(sub)
        _run(ctx, ctx.lib.neo_fleet_fly_error_dev, B, _p(d_n), _p(d_sub), 0 if sub is None else len(sub), _p(d_fl), _p(d_cmd), cap,
             _p(d_cl), stride, _p(rec), _p(count), _p(flags))
        return rec.cpu().numpy(), count.cpu().numpy(), flags.cpu().numpy()

    rec, count, flags = device(None)
    F = {name: k for k, name in enumerate(_lib.FLY_FIELDS)}
    for b, w in enumerate(want):
        assert count[b] == w["count"] and flags[b] == w["flags"], (b, count[b], w["count"], flags[b], w["flags"])
        if w["count"] == 0:
            assert np.isnan(rec[b]).all()
            continue
        for f in ("pos_err_max", "pos_err_max_at", "vel_err_max", "pos_err_final"):
            assert rec[b, F[f]] == w[f], (b, f, rec[b, F[f]], w[f])
        for f in ("pos_err_rms", "vel_err_rms"):
            assert abs(rec[b, F[f]] - w[f]) <= 1e-12 * w[f], (b, f, rec[b, F[f]], w[f])
    assert flags[nan_b] == NAN_FLAG and want[nan_b]["flags"] == NAN_FLAG and flags[-1] == 0 and count[-1] == 0
    assert rec[3, F["pos_err_max"]] == 5.0 and rec[3, F["pos_err_max_at"]] == 5 * stride
    # the NumPy model says the same
    for b in range(B):
        r, c, f = fm.fly_error(flown[b, :flown_len[b]], cmd[b, :max(cmd_len[b], 0)], stride)
        assert c == count[b] and f == flags[b] and np.allclose(r, rec[b], rtol=1e-12, atol=0.0, equal_nan=True)
    # a subset in another order with indices to skip: the same bits, the other missions untouched
    mine = np.array([B + 2, 4, nan_b, 1, -1], np.int32)
    r2, c2, f2 = device(mine)
    on = np.isin(np.arange(B), mine)
    assert np.array_equal(r2[on], rec[on], equal_nan=True) and np.array_equal(c2[on], count[on]) and np.array_equal(f2[on], flags[on])
    assert np.all(r2[~on] == SENTINEL) and np.all(c2[~on] == -1) and np.all(f2[~on] == -1)


# ------------------------------------------------------------------ 6. refusals
def test_refusals_of_both_entries():
    torch, dev = _torch()
    ctx = _lib.default_context()
    fl = fc.fleet(2, 3)
    D = to_device(fl)
    sub = _dev(np.zeros(1, np.int32))
    good = dict(B=2, model=fc.MODELS["gust6"].derived(fc.HZ), subset=None, n_subset=0, cmd=D["cmd"], cap=fc.CAP, cmd_len=D["cmd_len"],
                cmd_index=D["cmd_index"], future_index=D["future_index"], step=7, ahead=5, first=0, settle=0, reach=0.2,
                mission_ids=D["mission_ids"], goal=D["goal"], drone=D["drone"], flown=D["flown"], flown_len=D["flown_len"],
                saturated=D["saturated"], flags=D["flags"], cur_pos=D["cur_pos"], head=D["head"])

    def fly(**kw):
        a = dict(good, **kw)
        m = None if a["model"] is None else _model_struct(a["model"])
        vals = [a[k] for k in good]
        vals[1] = None if m is None else ctypes.byref(m)
        vals = [_p(v) if hasattr(v, "data_ptr") else v for v in vals]
        torch.cuda.synchronize(dev)
        rc = ctx.lib.neo_fleet_fly_dev(ctx.h, *vals)
        return int(rc), ctx.lib.neo_last_error(ctx.h).decode() if rc else ""

    before = {k: D[k].cpu().numpy().copy() for k in fc.STATE}
    d = good["model"]
    bad_model = "fleet fly: the model has a field that is not finite"
    for kw, text in ((dict(B=-1), "fleet fly: B must be >= 0"),
                     (dict(subset=sub, n_subset=3), "fleet fly: bad subset size"),
                     (dict(subset=sub, n_subset=-1), "fleet fly: bad subset size"),
                     (dict(cap=0), "fleet fly: cap must be > 0"),
                     (dict(step=-1), "fleet fly: step, ahead and settle must be in 0 .. 2^30"),
                     (dict(ahead=-1), "fleet fly: step, ahead and settle must be in 0 .. 2^30"),
                     (dict(settle=-1), "fleet fly: step, ahead and settle must be in 0 .. 2^30"),
                     (dict(step=2 ** 30 + 1), "fleet fly: step, ahead and settle must be in 0 .. 2^30"),
                     (dict(ahead=2 ** 30 + 1), "fleet fly: step, ahead and settle must be in 0 .. 2^30"),
                     (dict(settle=2 ** 30 + 1), "fleet fly: step, ahead and settle must be in 0 .. 2^30"),
                     (dict(reach=float("nan")), "fleet fly: reach must be finite"),
                     (dict(model=None), "fleet fly: null buffer"),
                     (dict(model=d._replace(kp=float("nan"))), bad_model),
                     (dict(model=d._replace(rho=float("inf"))), bad_model),
                     (dict(model=d._replace(h=0.0)), "fleet fly: the model's h, a_max and alpha must be > 0"),
                     (dict(model=d._replace(a_max=-1.0)), "fleet fly: the model's h, a_max and alpha must be > 0"),
                     (dict(model=d._replace(gust_every=0)), "fleet fly: the model's gust_every must be >= 1")) + \
            tuple((dict({k: None}), "fleet fly: null buffer") for k in ("cmd", "cmd_len", "cmd_index", "future_index", "goal", "drone",
                                                                       "flown", "flown_len", "saturated", "flags", "cur_pos", "head")):
        rc, msg = fly(**kw)
        assert (rc, msg) == (1, text), (kw, rc, msg)
    ctx.synchronize()
    assert all(fc.same_bits(D[k].cpu().numpy(), before[k]) for k in fc.STATE)      # nothing was launched
    assert fly(mission_ids=None) == (0, "") and fly(B=0) == (0, "") and fly(subset=sub, n_subset=0) == (0, "")
    ctx.synchronize()

    rec = torch.full((2, _lib.NEO_FLY_FIELDS), SENTINEL, dtype=torch.float64, device=dev)
    count = torch.full((2,), -1, dtype=torch.int32, device=dev)
    eflags = count.clone()
    egood = dict(B=2, flown_len=D["flown_len"], subset=None, n_subset=0, flown=D["flown"], cmd=D["cmd"], cap=fc.CAP,
                 cmd_len=D["cmd_len"], stride=6, fly=rec, count=count, flags=eflags)

    def err(**kw):
        vals = [_p(v) if hasattr(v, "data_ptr") else v for v in dict(egood, **kw).values()]
        torch.cuda.synchronize(dev)
        rc = ctx.lib.neo_fleet_fly_error_dev(ctx.h, *vals)
        return int(rc), ctx.lib.neo_last_error(ctx.h).decode() if rc else ""

    for kw, text in ((dict(B=-1), "fleet fly error: B must be >= 0"),
                     (dict(subset=sub, n_subset=3), "fleet fly error: bad subset size"),
                     (dict(cap=0), "fleet fly error: cap must be > 0"),
                     (dict(stride=0), "fleet fly error: stride must be >= 1")) + \
            tuple((dict({k: None}), "fleet fly error: null buffer") for k in ("flown_len", "flown", "cmd", "cmd_len", "fly", "count", "flags")):
        rc, msg = err(**kw)
        assert (rc, msg) == (1, text), (kw, rc, msg)
    ctx.synchronize()
    assert np.all(rec.cpu().numpy() == SENTINEL) and np.all(count.cpu().numpy() == -1)
    assert err() == (0, "")
    ctx.synchronize()
    assert np.all(count.cpu().numpy() >= 0)


# ------------------------------------------------------------------ 7. a fleet of one against the CPU oracle
GOAL_ONE = [7.1, 2.5]
MODEL_ONE = dict(gust_sigma=0.3, seed=5)


@functools.lru_cache(maxsize=None)
def _oracle_flight():
    grid = onp.GridESDF(synth.occupancy_2d(3), synth.RES, 300, 300, ORIGIN)
    np.random.seed(503)
    state = np.random.get_state()
    loop = ReplanLoop(onp.OraclePlanner(onp.PlannerParams()), grid, goal=GOAL_ONE, flight=fm.FlightModel(**MODEL_ONE), mission_id=4)
    ref = loop.run(max_replans=4)
    after = np.random.get_state()
    assert np.array_equal(after[1], state[1]) and after[2:] == state[2:], "the oracle flight drew random numbers: not comparable"
    return ref


def test_fleet_of_one_flies_the_cpu_oracle_flight(map3):
    """the default model with gusts, scene 3, (0, 0) to (7.1, 2.5): plans, rows and saturated sub-steps equal, flown positions
    within 1e-4 m (measured on the MI355X: 5 plans, 582 rows, 5.9e-14 m)"""
    ref = _oracle_flight()
    loop = npa.FleetReplanLoop(npa.BatchPlanner(), map3, [GOAL_ONE], flight=fm.FlightModel(**MODEL_ONE), mission_ids=[4])
    out = loop.run([[0.0, 0.0]], max_replans=4)
    flown, cmd = loop.flown_rows(0), loop.commands(0)
    n = min(len(flown), len(ref["path"]))
    diff = np.max(np.linalg.norm(flown[:n, 0] - ref["path"][:n], axis=1))
    cdiff = np.max(np.linalg.norm(cmd[:min(len(cmd), len(ref["commands"])), 0] - ref["commands"][:min(len(cmd), len(ref["commands"])), 0], axis=1))
    sat_ref = sum(1 for r in ref["fly_saturated_rows"] if r < n)
    print(f"fleet {out['replans'][0]} plans, {out['failed_attempts'][0]} failed, {out['n_cmd'][0]} commands, {out['n_flown'][0]} flown, "
          f"{out['fly_saturated'][0]} saturated, landed success {bool(out['success'][0])}; oracle {ref['replans']} plans, "
          f"{ref['failed_attempts']} failed, {len(ref['commands'])} commands, {len(ref['path'])} flown, {ref['fly_saturated']} saturated "
          f"({sat_ref} below row {n}); max flown position difference {diff:.3e} m, max commanded {cdiff:.3e} m; fly rms "
          f"{out['fly_pos_err_rms'][0]:.4f} max {out['fly_pos_err_max'][0]:.4f} final {out['fly_pos_err_final'][0]:.4f} (oracle "
          f"{ref['fly_pos_err_rms']:.4f} {ref['fly_pos_err_max']:.4f} {ref['fly_pos_err_final']:.4f})")
    assert out["replans"][0] == ref["replans"] and out["failed_attempts"][0] == ref["failed_attempts"] == 0
    assert out["n_cmd"][0] == len(cmd) == len(ref["commands"])
    # a landed mission flies its array out and settles, on both sides; another stops on the row its last tick left it on
    assert out["n_flown"][0] == len(flown) == (len(ref["path"]) if ref["landed"] else ref["n_flown_planned"])
    assert diff < 1e-4
    assert out["fly_saturated"][0] == sat_ref
    assert bool(out["success"][0]) == ref["success"] or not ref["landed"]
    # the flown rows are the model's flight over the fleet's own commands, bit for bit
    mine = fm.fly(fm.FlightModel(**MODEL_ONE), 60, cmd, (0.0, 0.0), mission_id=4, settle=max(len(flown) - len(cmd), 0),
                  reach=loop.target_reach_threshold, goal=GOAL_ONE)
    assert fc.same_bits(mine.rows()[:len(flown)], flown)


# ------------------------------------------------------------------ 8. a mission flies the same alone and in a fleet
@pytest.mark.parametrize("mode", ["basic", "warmstart"])
def test_a_mission_flies_the_same_alone_and_in_a_fleet(map3, mode):
    B = 64
    rng = np.random.default_rng(8)
    goals = np.stack([rng.uniform(9.0, 14.0, B), rng.uniform(-6.0, 6.0, B)], axis=1)
    start = np.stack([np.full(B, 0.5), rng.uniform(-3.0, 3.0, B)], axis=1)
    model = fm.FlightModel(gust_sigma=0.3, seed=12)
    kw = dict(mode=mode, seed=41, max_cmd_seconds=40, flight=model)
    loop = npa.FleetReplanLoop(npa.BatchPlanner(), map3, goals, **kw)
    out = loop.run(start, max_replans=3)
    print(f"{mode}: plans {out['replans'].sum()}, failed attempts {out['failed_attempts'].sum()}, abandoned {int(out['abandoned'].sum())}, "
          f"fly rms {np.nanmean(out['fly_pos_err_rms']):.3f} max {np.nanmax(out['fly_pos_err_max']):.3f}, saturated "
          f"{out['fly_saturated'].sum()}")
    assert np.nanmax(out["fly_pos_err_max"]) > 0.01
    for i in (0, 17, 63):
        one = npa.FleetReplanLoop(npa.BatchPlanner(), map3, goals[i:i + 1], mission_ids=[i], **kw)
        o1 = one.run(start[i:i + 1], max_replans=3)
        assert set(o1) == set(out)
        for k in out:
            assert np.array_equal(np.asarray(o1[k])[0], np.asarray(out[k])[i], equal_nan=True), (i, k, o1[k][0], out[k][i])
        assert np.array_equal(one.commands(0), loop.commands(i)) and fc.same_bits(one.flown_rows(0), loop.flown_rows(i)), i


# ------------------------------------------------------------------ 9. with goal routes, a recorder and mode "batch"
def test_the_model_next_to_goal_routes_a_recorder_and_mode_batch(map3):
    routes = tc.flight_routes()
    scenes = [don.boxes_of(synth.forest_boxes(3))]
    rec = DemoRecorder(DepthCamera(width=64, height=48), capacity=64)
    model = fm.FlightModel(gust_sigma=0.3, seed=3)
    loop = npa.FleetReplanLoop(npa.BatchPlanner(), map3, None, goal_routes=routes, mode="batch", record=rec,
                               scenes=DepthCamera.pack_scenes(scenes), seed=3, max_cmd_seconds=30, flight=model)
    out = loop.run(np.zeros((3, 2)), max_replans=2)
    assert np.all(out["flags"] == 0) and np.array_equal(out["n_flown"], [121] * 3) and np.all(out["fly_count"] == 21)
    vel = rec.cur_vel.cpu().numpy()
    for i in range(3):
        flown, cmd = loop.flown_rows(i), loop.commands(i)
        assert len(flown) == 121
        # the recorder's velocity now is the flown one: the model's over the mission's commands, not the commanded one
        mine = fm.fly(model, 60, cmd[:121], (0.0, 0.0), mission_id=i)
        assert fc.same_bits(mine.rows(), flown)
        assert fc.same_bits(vel[i], flown[120, 1]) and not np.array_equal(vel[i], cmd[120, 1])
        # the tracking audit and the flight metric ran on the flown rows
        r = tc.track_restated(flown, 121, loop.stride, float(loop.cmd_hz), routes.take([i]), loop.track_radius)
        assert out["track_count"][i] == r["count"] == 21 and out["track_gap_max"][i] == r["gap_max"] and out["track_gap_final"][i] == r["gap_final"]
        rc = tc.track_restated(cmd, 121, loop.stride, float(loop.cmd_hz), routes.take([i]), loop.track_radius)
        assert rc["gap_final"] != r["gap_final"]
        assert abs(out["final_dist"][i] - np.linalg.norm(flown[120, 0] - out["goal_final"][i])) <= 1e-12
        e = fc.error_restated(flown, cmd, loop.stride)
        assert out["fly_pos_err_max"][i] == e["pos_err_max"] and out["fly_pos_err_final"][i] == e["pos_err_final"]


# ------------------------------------------------------------------ 10. without a model
def test_without_a_model_nothing_of_it_is_called(map3):
    bp = npa.BatchPlanner()
    loop = npa.FleetReplanLoop(bp, map3, [[30.0, 0.0], [25.0, 3.0]])
    ctx = bp.ctx
    lib, proxy = ctx.lib, ffc.RecordingLib(ctx.lib)
    ctx.lib = proxy
    try:
        out = loop.run(np.zeros((2, 2)), max_replans=2)
    finally:
        ctx.lib = lib
    assert "neo_fleet_advance_dev" in proxy.names and not [n for n in proxy.names if n.startswith("neo_fleet_fly")]
    assert not [k for k in out if k.startswith("fly_")] and not [k for k in loop._dev if k in ("drone", "flown", "flown_len", "fly")]
    # and with one, the fly launch stands where the advance stood
    loop = npa.FleetReplanLoop(bp, map3, [[30.0, 0.0], [25.0, 3.0]], flight=fm.FlightModel())
    proxy = ffc.RecordingLib(lib)
    ctx.lib = proxy
    try:
        out = loop.run(np.zeros((2, 2)), max_replans=2)
    finally:
        ctx.lib = lib
    assert "neo_fleet_advance_dev" not in proxy.names and proxy.names.count("neo_fleet_fly_dev") == 2
    assert proxy.names.count("neo_fleet_fly_error_dev") == 1 and {"fly_" + f for f in _lib.FLY_FIELDS} <= set(out)
