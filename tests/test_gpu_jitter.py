"""The counter-based jitter on the GPU (csrc/neo_counter_rng.hpp; neo_plan_jitter*, neo_fleet_jitter*): the two kernels
against the NumPy model (neo_planner_amd/counter_rng.py) bit for bit, plan_dev(jitter="counter") against its oracle
plan(jitter="counter") -- every returned array and the launch sizes -- without a host draw, and the fleet with
jitter="counter": the resident form against the host form flight by flight, a mission alone against its row in the fleet."""
import ctypes

import numpy as np
import pytest

import neo_planner_amd as npa
from neo_planner_amd import _lib, fleet, synth
from neo_planner_amd.fleet import draw_missions
from oracle import minco_np as onp

pytestmark = pytest.mark.gpu

ORIGIN = (0.0, -15.0)
SENTINEL = 777.0
INVALID = 1          # NEO_ERR_INVALID
IDS = np.arange(48) * 3 + 500          # the requests' stream ids: not their positions
# the first seed from 11 upwards whose host plan(jitter="counter") over the request set exercises the chain in both modes
# (test_plan_dev_counter_is_plan_counter_bit_for_bit asserts it): with 11, f64 launches [48, 14, 11, 10, 10] requests and
# solves 4 by a retry, f32x [48, 14, 12, 11, 11] and 3; 34 requests are solved at once
SEED = 11


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------ 1. the two kernels against the model
def _lists():
    """(name, B, subset or None, rows of the noise array) -- rows past the list keep the sentinel"""
    rng = np.random.default_rng(4)
    return [("six", 7, np.array([3, -1, 0, 9, 6, 2], np.int32), 8),            # one index below 0, one >= B
            ("all", 7, None, 9),
            ("300", 301, rng.permutation(301)[:300].astype(np.int32), 301)]    # more than one workgroup of 256 lanes


def _ids(B):
    ids = (np.arange(B, dtype=np.int64) * 7919 + 13) % (2 ** 31)
    ids[0], ids[min(3, B - 1)], ids[B - 1] = 2 ** 31 - 1, 0, 500
    return ids.astype(np.int32)


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("count", [1, 2, 5])
def test_plan_jitter_kernel_is_the_model_bit_for_bit(count, D):
    torch, dev = _torch()
    ctx = _lib.default_context()
    L, M = ctx.lib, count + 1
    for name, B, sub, rows in _lists():
        ids = _ids(B)
        P = B if sub is None else len(sub)
        at = np.arange(B) if sub is None else sub
        valid = (at >= 0) & (at < B)
        d_sub, d_ids = (None if sub is None else _dev(sub)), _dev(ids)
        for seed in (0, 11, 2 ** 62 - 1):
            for attempt in (1, 4):
                ref = npa.BatchPlanner.retry_noise_counter(seed, ids[at[valid]], attempt, D, count)

                def check(noise):
                    assert np.array_equal(noise[:P][valid], ref), (name, seed, attempt)
                    assert np.all(noise[:P][~valid] == SENTINEL) and np.all(noise[P:] == SENTINEL), (name, seed, attempt)

                noise = np.full((rows, D, count), SENTINEL)
                ctx.check(L.neo_plan_jitter(ctx.h, B, _lib.ptr(sub), P if sub is not None else 0, M, D, seed, attempt,
                                            _lib.ptr(ids), _lib.ptr(noise)))
                check(noise)
                d_noise = torch.full((rows, D, count), SENTINEL, dtype=torch.float64, device=dev)
                torch.cuda.synchronize(dev)
                ctx.check(L.neo_plan_jitter_dev(ctx.h, B, _p(d_sub), P if sub is not None else 0, M, D, seed, attempt,
                                                _p(d_ids), _p(d_noise)))
                ctx.synchronize()
                check(d_noise.cpu().numpy())
        # without stream_ids a request's stream is its index
        noise = np.full((rows, D, count), SENTINEL)
        ctx.check(L.neo_plan_jitter(ctx.h, B, _lib.ptr(sub), P if sub is not None else 0, M, D, 11, 2, None, _lib.ptr(noise)))
        assert np.array_equal(noise[:P][valid], npa.BatchPlanner.retry_noise_counter(11, at[valid], 2, D, count)), name
        assert np.all(noise[:P][~valid] == SENTINEL) and np.all(noise[P:] == SENTINEL)


def test_fleet_jitter_kernel_is_the_model_bit_for_bit():
    torch, dev = _torch()
    ctx = _lib.default_context()
    L, B = ctx.lib, 70
    ids = _ids(B)
    sub = np.arange(30, 70).astype(np.int32)                 # 40 missions on both sides of lane 64
    sub[[5, 33]] = sub[[33, 5]]
    rest = np.setdiff1d(np.arange(B), sub)
    d_sub, d_ids = _dev(sub), _dev(ids)
    for seed, tick in ((0, 0), (5, 9), (2 ** 64 - 1, 60)):
        for target in (0, 3):
            ref = fleet.target_jitter_counter(seed, ids[sub], tick, target)
            assert ref.any() == (target != 0)
            jit = np.full((B, 2), SENTINEL)
            ctx.check(L.neo_fleet_jitter(ctx.h, B, _lib.ptr(sub), len(sub), seed, tick, target, _lib.ptr(ids), _lib.ptr(jit)))
            assert np.array_equal(jit[sub], ref) and np.all(jit[rest] == SENTINEL), (seed, tick, target)
            d_jit = torch.full((B, 2), SENTINEL, dtype=torch.float64, device=dev)
            torch.cuda.synchronize(dev)
            ctx.check(L.neo_fleet_jitter_dev(ctx.h, B, _p(d_sub), len(sub), seed, tick, target, _p(d_ids), _p(d_jit)))
            ctx.synchronize()
            got = d_jit.cpu().numpy()
            assert np.array_equal(got[sub], ref) and np.all(got[rest] == SENTINEL), (seed, tick, target)
    # no subset: every mission; no mission_ids: the index
    jit = np.full((B, 2), SENTINEL)
    ctx.check(L.neo_fleet_jitter(ctx.h, B, None, 0, 5, 9, 3, None, _lib.ptr(jit)))
    assert np.array_equal(jit, fleet.target_jitter_counter(5, np.arange(B), 9, 3))


def test_jitter_entry_point_argument_errors():
    ctx = _lib.default_context()
    L = ctx.lib
    noise = np.zeros((4, 2, 2)); ids = np.zeros(4, np.int32); sub5 = np.zeros(5, np.int32)
    plan = lambda B=4, sub=None, n_sub=0, M=3, D=2, attempt=1, out=_lib.ptr(noise): L.neo_plan_jitter(
        ctx.h, B, sub, n_sub, M, D, 7, attempt, _lib.ptr(ids), out)
    assert plan() == 0
    for kw in (dict(out=None), dict(B=-1), dict(M=1), dict(M=65), dict(D=1), dict(D=4), dict(attempt=-1),
               dict(sub=_lib.ptr(sub5), n_sub=5), dict(sub=_lib.ptr(sub5), n_sub=-1)):
        assert plan(**kw) == INVALID and L.neo_last_error(ctx.h), kw
    assert L.neo_plan_jitter_dev(ctx.h, 4, None, 0, 3, 2, 7, 1, None, None) == INVALID
    assert L.neo_plan_jitter_dev(ctx.h, 4, None, 0, 3, 2, 7, -1, None, _lib.ptr(noise)) == INVALID       # (refused before any launch)
    jit = np.zeros((4, 2))
    fl = lambda B=4, sub=None, n_sub=0, tick=1, target=1, out=_lib.ptr(jit): L.neo_fleet_jitter(
        ctx.h, B, sub, n_sub, 7, tick, target, _lib.ptr(ids), out)
    assert fl() == 0
    for kw in (dict(out=None), dict(B=-1), dict(tick=-1), dict(target=-1), dict(sub=_lib.ptr(sub5), n_sub=5)):
        assert fl(**kw) == INVALID and L.neo_last_error(ctx.h), kw
    assert L.neo_fleet_jitter_dev(ctx.h, 4, None, 0, 7, 1, 1, None, None) == INVALID
    assert plan(B=0) == 0 and fl(B=0) == 0


# ------------------------------------------------------------------ 2. plan_dev against plan, both with the counter streams
@pytest.fixture(scope="module")
def scenes():
    """scene -> (device map, the oracle's host grid) for the scenes the tests fly on"""
    out = {}
    for s in (1, 2, 7):
        occ = synth.occupancy_2d(s)
        m = npa.ESDF()
        m.occupancy_map_cb(synth.OccupancyGridMsg(occ))
        out[s] = (m, onp.GridESDF(occ, synth.RES, 300, 300, ORIGIN))
    return out


@pytest.fixture(scope="module")
def requests(scenes):
    """the request set of tests/test_gpu_plan_dev.py, built the same way: 24 requests on each of scenes 1 (14 m long) and
    7 (11 m) -- head (48, 3, 2), tail, scene ids, map-table slots"""
    head = np.zeros((48, 3, 2)); tail = np.zeros((48, 3, 2)); which = np.zeros(48, int)
    k = 0
    for s, dist in ((1, 14.0), (7, 11.0)):
        grid = scenes[s][1]
        rng = np.random.default_rng([2024, s])
        for _ in range(24):
            while True:
                x = rng.uniform(1.0, 24.0); y = rng.uniform(-9.0, 9.0); th = rng.uniform(-np.pi, np.pi)
                p, d = np.array([x, y]), np.array([np.cos(th), np.sin(th)])
                if grid.get_edt_dis(p) >= 0.7 and grid.get_edt_dis(p + dist * d) >= 0.0:
                    break
            head[k, 0], head[k, 1] = p, 0.5 * d
            tail[k, 0], tail[k, 1] = p + dist * d, 0.8 * d
            which[k] = s
            k += 1
    sids = np.array([scenes[s][0].scene_id for s in which], np.int32)
    c = _lib.default_context()
    slots = np.array([c.lib.neo_scene_slot(c.h, int(s)) for s in sids], np.int32)
    return head, tail, sids, slots


PLAN_KEYS = ("x", "costs", "costs_last", "nit", "nfev", "status", "collision", "attempts", "nit_total", "solved")


def _as_plan(bufs, rows=None):
    """plan_dev's resident results in the form of plan's dict"""
    h = {k: bufs[k].cpu().numpy() for k in ("x", "costs", "costs_last", "nit", "nfev", "status", "attempts", "nit_total",
                                             "solved")}
    st = h["status"]
    out = dict(h, status=st & 0xff, collision=(st & _lib.NEO_TRAJ_FLAG_COLLISION) != 0, solved=h["solved"] != 0)
    return out if rows is None else {k: v[rows] for k, v in out.items()}


def _equal(got, ref):
    for k in PLAN_KEYS:
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k], equal_nan=True), k


@pytest.fixture(scope="module")
def planned(scenes, requests):
    """plan(jitter="counter") over the request set in both modes, once, and plan_dev(jitter="counter") over the same"""
    torch, dev = _torch()
    head, tail, sids, slots = requests
    out = {}
    for mode in ("f64", "f32x"):
        bp = npa.BatchPlanner(sample_dtype=mode)
        ref = bp.plan(scenes[1][0], head, tail, scene_ids=sids, seed=SEED, stream_ids=IDS, return_launch_sizes=True,
                      jitter="counter")
        d_head, d_tail, d_slots = _dev(head), _dev(tail), _dev(slots)
        torch.cuda.synchronize(dev)
        bufs = bp.plan_dev(scenes[1][0], d_head, d_tail, slots=d_slots, seed=SEED, stream_ids=IDS, jitter="counter")
        out[mode] = (bp, ref, bufs, (d_head, d_tail, d_slots))
    return out


@pytest.mark.parametrize("mode", ["f64", "f32x"])
def test_plan_dev_counter_is_plan_counter_bit_for_bit(planned, scenes, requests, mode, capsys):
    bp, ref, bufs, _ = planned[mode]
    hist = np.bincount(ref["attempts"], minlength=6).tolist()
    spent = int(((ref["attempts"] == 5) & ~ref["solved"]).sum())
    first = int(((ref["attempts"] == 1) & ref["solved"]).sum())
    with capsys.disabled():
        print(f"\n{mode}: requests by attempts {hist[1:]}, unsolved after all five {spent}, solved at the first {first}; "
              f"launch sizes {ref['launch_sizes']}")
    # the inputs exercise the chain: retries, retries that got somewhere, a request that uses every attempt, and a
    # majority that needs none
    assert (ref["attempts"] >= 2).sum() >= 3 and spent >= 1 and first >= 24
    assert ((ref["attempts"] >= 2) & ref["solved"]).sum() >= 2
    _equal(_as_plan(bufs), ref)
    assert bufs["launch_sizes"] == ref["launch_sizes"] and len(ref["launch_sizes"]) == 5
    # the counter streams fly other flights than the NumPy generators: the switch does switch
    head, tail, sids, _ = requests
    other = bp.plan(scenes[1][0], head, tail, scene_ids=sids, seed=SEED, stream_ids=IDS)
    assert not np.array_equal(other["x"], ref["x"])


def test_plan_dev_counter_over_a_subset_with_device_stream_ids(scenes, requests, planned):
    torch, dev = _torch()
    head, tail, sids, _ = requests
    bp, full, _, (d_head, d_tail, d_slots) = planned["f32x"]
    rng = np.random.default_rng(5)
    sub = rng.permutation(48)[:31]
    assert (full["attempts"][sub] >= 2).sum() >= 2
    ref = bp.plan(scenes[1][0], head[sub], tail[sub], scene_ids=sids[sub], seed=23, stream_ids=IDS[sub], return_launch_sizes=True,
                  jitter="counter")
    assert (ref["attempts"] >= 2).sum() >= 2
    d_sub = _dev(sub.astype(np.int32))
    d_ids = _dev(IDS.astype(np.int32))
    for ids in (IDS, d_ids):                       # a host array, uploaded by the call; an int32 device tensor, used where it lies
        bufs = bp.plan_buffers(48, dev)
        for k in ("x", "costs", "costs_last"):
            bufs[k].fill_(SENTINEL)
        for k in ("nit", "nfev", "status", "attempts", "nit_total", "solved"):
            bufs[k].fill_(-9)
        torch.cuda.synchronize(dev)
        assert bp.plan_dev(scenes[1][0], d_head, d_tail, bufs=bufs, slots=d_slots, subset=d_sub, seed=23, stream_ids=ids,
                           jitter="counter") is bufs
        _equal(_as_plan(bufs, sub), ref)
        assert bufs["launch_sizes"] == ref["launch_sizes"]
        rest = np.setdiff1d(np.arange(48), sub)
        assert np.all(bufs["x"].cpu().numpy()[rest] == SENTINEL)
        for k in ("nit", "status", "attempts", "nit_total", "solved"):
            assert np.all(bufs[k].cpu().numpy()[rest] == -9), k
    assert torch.equal(d_ids, _dev(IDS.astype(np.int32)))          # only read


def test_plan_dev_counter_from_a_callers_first_guess(scenes, requests, planned):
    torch, dev = _torch()
    head, tail, sids, _ = requests
    bp, _, _, (d_head, d_tail, d_slots) = planned["f64"]
    cand, ts = bp.batch_init_guess(head, tail, K=2)               # the guess shifted sideways by 0.6 m
    ts = np.tile(ts, (48, 1))
    ref = bp.plan(scenes[1][0], head, tail, int_wpts=cand[:, 1], ts=ts, scene_ids=sids, seed=31, stream_ids=IDS,
                  return_launch_sizes=True, jitter="counter")
    assert (ref["attempts"] >= 2).sum() >= 3
    d_x0 = _dev(bp.pack_x(cand[:, 1], ts))
    torch.cuda.synchronize(dev)
    bufs = bp.plan_dev(scenes[1][0], d_head, d_tail, x0=d_x0, slots=d_slots, seed=31, stream_ids=IDS, jitter="counter")
    _equal(_as_plan(bufs), ref)
    assert bufs["launch_sizes"] == ref["launch_sizes"]


def test_a_request_planned_alone_with_the_counter_equals_its_row_in_the_batch(scenes, requests, planned):
    torch, dev = _torch()
    bp, ref, _, (d_head, d_tail, d_slots) = planned["f64"]
    spent = np.flatnonzero((ref["attempts"] == 5) & ~ref["solved"])          # never solved: every attempt's jitter is used
    retried = np.flatnonzero((ref["attempts"] >= 2) & ref["solved"])
    for i in (int(spent[0]), int(retried[0]), int(retried[-1])):
        one = bp.plan_dev(scenes[1][0], d_head[i:i + 1].clone(), d_tail[i:i + 1].clone(), slots=d_slots[i:i + 1].clone(),
                          seed=SEED, stream_ids=IDS[i:i + 1], jitter="counter")
        _equal(_as_plan(one), {k: ref[k][i:i + 1] for k in PLAN_KEYS})
        assert one["launch_sizes"] == [1] * int(ref["attempts"][i])


def test_plan_dev_counter_draws_nothing_on_the_host(scenes, requests, planned, monkeypatch):
    torch, dev = _torch()
    bp, ref, _, (d_head, d_tail, d_slots) = planned["f64"]

    def no_draws(*a, **kw):
        raise AssertionError("a NumPy generator was made")

    monkeypatch.setattr(np.random, "default_rng", no_draws)
    monkeypatch.setattr(npa.BatchPlanner, "retry_noise", staticmethod(no_draws))
    monkeypatch.setattr(npa.BatchPlanner, "retry_noise_counter", staticmethod(no_draws))      # nor the model
    bufs = bp.plan_dev(scenes[1][0], d_head, d_tail, slots=d_slots, seed=SEED, stream_ids=IDS, jitter="counter")
    monkeypatch.undo()
    _equal(_as_plan(bufs), ref)
    assert len(bufs["launch_sizes"]) == 5


# ------------------------------------------------------------------ 3. fleet
@pytest.mark.parametrize("mode", ["basic", "batch"])
def test_the_counter_fleet_flies_the_same_resident_and_alone(scenes, mode, capsys, monkeypatch):
    maps = [scenes[1][0], scenes[2][0]]
    start, goals, sids = draw_missions(maps, 12, seed=3)
    mission_ids = np.arange(24) + 100
    drawn = []
    model = npa.BatchPlanner.retry_noise_counter

    def spy(seed, ids, attempt, D, count):
        drawn.append(len(ids))
        return model(seed, ids, attempt, D, count)

    runs = {}
    for resident in (False, True):
        if not resident:
            monkeypatch.setattr(npa.BatchPlanner, "retry_noise_counter", staticmethod(spy))
        loop = npa.FleetReplanLoop(npa.BatchPlanner(), maps[0], goals, mode=mode, scene_ids=sids, seed=5,
                                   mission_ids=mission_ids, resident=resident, jitter="counter")
        runs[resident] = (loop, loop.run(start, max_replans=6))
        monkeypatch.undo()
    (host_loop, host), (res_loop, res) = runs[False], runs[True]
    with capsys.disabled():
        print(f"\n{mode}: plans {int(host['replans'].sum())}, failed attempts (re-targeted rounds) {int(host['failed_attempts'].sum())}, "
              f"retry rows drawn by the host form {sum(drawn)}")
    # the flights exercise both jitters: a mission re-targeted (a target round > 0) and a request retried
    assert host["failed_attempts"].max() >= 1 and sum(drawn) >= 1
    assert host["replans"].sum() >= 24 * 4
    assert res_loop._plan is not None and host_loop._plan is None        # the resident chain ran, and only there
    assert set(res) == set(host)
    for k in host:
        assert np.array_equal(np.asarray(res[k]), np.asarray(host[k]), equal_nan=True), k
    for i in range(24):
        assert np.array_equal(res_loop.commands(i), host_loop.commands(i)), i
    assert np.array_equal(res_loop.uncounted_candidates, host_loop.uncounted_candidates)
    # a mission that re-targeted, alone with its id: the flight it flies in the fleet
    i = int(np.argmax(host["failed_attempts"]))
    alone = npa.FleetReplanLoop(npa.BatchPlanner(), maps[0], goals[i:i + 1], mode=mode, scene_ids=sids[i:i + 1], seed=5,
                                mission_ids=mission_ids[i:i + 1], resident=True, jitter="counter")
    out = alone.run(start[i:i + 1], max_replans=6)
    for k in host:
        assert np.array_equal(np.asarray(out[k]), np.asarray(host[k])[i:i + 1], equal_nan=True), k
    assert np.array_equal(alone.commands(0), host_loop.commands(i))
    # and the switch does switch: the NumPy generators fly other flights
    other = npa.FleetReplanLoop(npa.BatchPlanner(), maps[0], goals, mode=mode, scene_ids=sids, seed=5, mission_ids=mission_ids)
    other.run(start, max_replans=6)
    assert not np.array_equal(other.commands(i), host_loop.commands(i))
