"""The resident geo warm start on the GPU: neo_geo_guess_dev (search, prune and pack over a launch list, masked and
direct), BatchGeoPlanner.plan_dev against BatchPlanner.geo_plan, and FleetReplanLoop(mode="geo", geo=...) against the
host form and on onboard maps.  Everything is compared for equality: the resident forms are defined to give the host
form's bits."""
import ctypes

import numpy as np
import pytest

import depth_oracle_np as don
import neo_planner_amd as npa
from neo_planner_amd import _lib, synth
from neo_planner_amd.depth import DepthCamera
from neo_planner_amd.fleet import draw_missions
from neo_planner_amd.geo_resident import BatchGeoPlanner, pack_guess
from neo_planner_amd.onboard import OnboardMapper

pytestmark = pytest.mark.gpu

ORIGIN = (0.0, -15.0)
SENTINEL = 777.0
GEO_KEYS = ("key_pts", "path_cost", "path_len", "expansions", "flags")
# two workspace slots of the 400 x 400 expanded grid (32 bytes a cell and slot), and a little: the workgroups loop
TWO_SLOTS = 2 * 400 * 400 * 32 + 4096
DEFAULT_BUDGET = 2 << 30


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _dev(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _slot(c, scene_id):
    return int(c.lib.neo_scene_slot(c.h, int(scene_id)))


def _rebuild(c, m, occ):
    """scene m rebuilt in place from another occupancy grid (neo_esdf_build_2d_batch_dev)"""
    torch, dev = _torch()
    occ_dev = torch.from_numpy(np.ascontiguousarray(occ, dtype=np.int8)).to(dev)
    torch.cuda.synchronize(dev)
    H, W = occ.shape
    ids = np.array([m.scene_id], dtype=np.int32)
    c.check(c.lib.neo_esdf_build_2d_batch_dev(c.h, _lib.ptr(ids), 1, ctypes.c_void_p(occ_dev.data_ptr()), W, H, synth.RES,
                                              _lib.ptr(np.array([ORIGIN], dtype=np.float64))))


@pytest.fixture(scope="module")
def world():
    """two synth scenes, B = 72 requests on them through slots -- 5 m local targets from free starts, the velocity and
    acceleration rows of head / tail filled with numbers that must not matter -- and, among them, the special ones.  The
    host form's answers (geo_init with scene_ids) are computed once.  A context of its own: its scene table holds these two
    maps and nothing else, so the workspace budget and the count of mask builds mean what the tests say."""
    c = _lib.Context(0)
    maps = []
    for s in (0, 1):
        m = npa.ESDF(ctx=c)
        m.occupancy_map_cb(synth.OccupancyGridMsg(synth.occupancy_2d(s)))
        maps.append(m)
    B = 72
    rng = np.random.default_rng(21)
    which = (np.arange(B) % 2).astype(int)
    head = rng.normal(0.0, 1.0, (B, 3, 2))
    tail = rng.normal(0.0, 1.0, (B, 3, 2))
    blocked = None
    for b in range(B):
        esdf = maps[which[b]].esdf_map
        dist = lambda p: esdf[int((p[1] - ORIGIN[1]) / synth.RES), int((p[0] - ORIGIN[0]) / synth.RES)]
        while True:
            s = np.array([rng.uniform(0.5, 29.5), rng.uniform(-14.5, 14.5)])
            if dist(s) >= 0.6:
                break
        a = rng.uniform(-np.pi, np.pi)
        head[b, 0] = s
        tail[b, 0] = s + 5.0 * np.array([np.cos(a), np.sin(a)])
        if which[b] == 0 and blocked is None:
            ys, xs = np.nonzero(esdf < 0.2)
            blocked = np.array([ORIGIN[0] + (xs[0] + 0.5) * synth.RES, ORIGIN[1] + (ys[0] + 0.5) * synth.RES])
    tail[10, 0] = head[10, 0]                   # start == target
    tail[12, 0] = blocked                       # a target inside an obstacle (request 12 is on scene 0)
    head[14, 0] = (3.0, -100.0)                 # a start outside the expanded grid (its key is negative)
    sids = np.array([maps[w].scene_id for w in which], dtype=np.int32)
    slots = np.array([_slot(c, s) for s in sids], dtype=np.int32)
    BAD = 16
    slots[BAD] = 1000                           # one slot outside the table
    bp = npa.BatchPlanner(ctx=c)
    ref = bp.geo_init(maps[0], head[:, 0], tail[:, 0], scene_ids=sids)
    assert ref["flags"][12] == _lib.NEO_GEO_FLAG_NO_PATH and ref["flags"][14] == _lib.NEO_GEO_FLAG_START_OUTSIDE
    assert ref["path_len"][10] == 1 and ref["flags"][10] == 0 and (ref["path_len"] > 20).sum() > B // 2
    w = dict(c=c, maps=maps, B=B, bp=bp, head=head, tail=tail, sids=sids, slots=slots, bad=BAD, ref=ref,
             d_head=_dev(head), d_tail=_dev(tail), d_slots=_dev(slots))
    _torch()[0].cuda.synchronize()
    yield w
    c.synchronize()
    c.close()


def _expected(w, ref=None):
    """the host form's arrays with the bad-slot request's rows as the device form leaves them, and x0 = pack_x of them"""
    ref = w["ref"] if ref is None else ref
    e = {k: np.array(ref[k]) for k in GEO_KEYS}
    b = w["bad"]
    e["key_pts"][b] = np.nan; e["path_cost"][b] = np.nan
    e["path_len"][b] = 0; e["expansions"][b] = 0; e["flags"][b] = _lib.NEO_GEO_FLAG_BAD_SCENE
    bp = w["bp"]
    int_wpts = e["key_pts"][:, 1:3, :].transpose(0, 2, 1).copy()
    e["x0"] = bp.pack_x(int_wpts, np.asarray(ref["ts"]))
    assert np.array_equal(e["x0"], pack_guess(e["key_pts"], bp._plan_frac_tau(2)[1]), equal_nan=True)
    return e


def _sentinels(g, B, x0):
    """every result array of the planner filled with sentinels (allocating them first)"""
    torch, dev = _torch()
    if g.key_pts is None:
        g.key_pts = torch.zeros((B, 4, 2), dtype=torch.float64, device=dev)
        g.path_cost = torch.zeros(B, dtype=torch.float64, device=dev)
        g.path_len, g.expansions, g.flags = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3))
    g.key_pts.fill_(SENTINEL); g.path_cost.fill_(SENTINEL); x0.fill_(SENTINEL)
    for t in (g.path_len, g.expansions, g.flags):
        t.fill_(-9)
    torch.cuda.synchronize(dev)


def _got(g, x0):
    g.bp.ctx.synchronize()
    out = {k: getattr(g, k).cpu().numpy() for k in GEO_KEYS}
    out["x0"] = x0.cpu().numpy()
    return out


def _check_rows(got, want, rows, B):
    rows = np.asarray(rows, dtype=int)
    rest = np.setdiff1d(np.arange(B), rows)
    for k in GEO_KEYS + ("x0",):
        assert np.array_equal(got[k][rows], want[k][rows], equal_nan=True), k
        if k in ("key_pts", "path_cost", "x0"):
            assert np.all(got[k][rest] == SENTINEL), k
        else:
            assert np.all(got[k][rest] == -9), k


@pytest.mark.parametrize("direct", [False, True])
def test_the_list_form_equals_the_dense_form(world, direct):
    """counts 1, 3 and 70 with two workspace slots, a scrambled subset with an index of -1 and one of B, the empty
    subset and the whole batch: the rows of the list are geo_init's and pack_x's, every other row keeps its sentinel --
    for the masked and for the direct search (so: direct equals masked, x0 included)"""
    torch, dev = _torch()
    w = world
    c, B = w["c"], w["B"]
    want = _expected(w)
    g = BatchGeoPlanner(w["bp"], direct=direct)
    x0 = torch.zeros((B, 7), dtype=torch.float64, device=dev)
    c.check(c.lib.neo_geo_workspace_budget(c.h, TWO_SLOTS))
    rng = np.random.default_rng(5)
    for count in (1, 3, 70):
        rows = np.sort(rng.choice(B, count, replace=False)) if count < 70 else np.setdiff1d(np.arange(B), [3, 40])
        if count == 3:
            rows = np.array([10, 12, w["bad"]])
        _sentinels(g, B, x0)
        sub = _dev(rows.astype(np.int32))
        torch.cuda.synchronize(dev)
        assert g.warm_start_dev(w["maps"][0], w["d_head"], w["d_tail"], slots=w["d_slots"], subset=sub, x0=x0) is x0
        _check_rows(_got(g, x0), want, rows, B)
    # scrambled, with one index of -1 and one of B
    rows = rng.permutation(B)[:31]
    sub = _dev(np.concatenate([rows[:7], [-1], rows[7:20], [B], rows[20:]]).astype(np.int32))
    _sentinels(g, B, x0)
    g.warm_start_dev(w["maps"][0], w["d_head"], w["d_tail"], slots=w["d_slots"], subset=sub, x0=x0)
    _check_rows(_got(g, x0), want, rows, B)
    # the empty subset writes nothing
    _sentinels(g, B, x0)
    g.warm_start_dev(w["maps"][0], w["d_head"], w["d_tail"], slots=w["d_slots"], subset=torch.zeros((0,), dtype=torch.int32, device=dev),
                     x0=x0)
    _check_rows(_got(g, x0), want, [], B)
    # no subset: all B; and without slots every request is on `map`
    c.check(c.lib.neo_geo_workspace_budget(c.h, DEFAULT_BUDGET))
    _sentinels(g, B, x0)
    g.warm_start_dev(w["maps"][0], w["d_head"], w["d_tail"], slots=w["d_slots"], x0=x0)
    _check_rows(_got(g, x0), want, np.arange(B), B)
    on0 = np.flatnonzero(w["sids"] == w["maps"][0].scene_id)
    on0 = on0[on0 != w["bad"]]
    _sentinels(g, B, x0)
    g.warm_start_dev(w["maps"][0], w["d_head"], w["d_tail"], subset=_dev(on0.astype(np.int32)))
    own = _got(g, g.x0)
    for k in GEO_KEYS + ("x0",):
        assert np.array_equal(own[k][on0], want[k][on0], equal_nan=True), k
    assert np.all(x0.cpu().numpy() == SENTINEL)          # the planner's own x0 was written, not the caller's last one


def test_direct_builds_no_mask_and_follows_a_rebuilt_map(world):
    """one scene rebuilt in place from another occupancy grid: both forms give geo_init's answers on the new map, the
    masked one by rebuilding that scene's mask, the direct one without building any"""
    torch, dev = _torch()
    w = world
    c, B = w["c"], w["B"]
    masked, direct = BatchGeoPlanner(w["bp"], direct=False), BatchGeoPlanner(w["bp"], direct=True)
    x0 = torch.zeros((B, 7), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    call = lambda g: g.warm_start_dev(w["maps"][0], w["d_head"], w["d_tail"], slots=w["d_slots"], x0=x0)
    call(masked)                                 # (every mask of the table is up to date from here)
    before = _expected(w)
    try:
        _rebuild(c, w["maps"][1], synth.occupancy_2d(2))
        n0 = direct.mask_builds()
        call(direct)
        got_direct = _got(direct, x0)
        assert direct.mask_builds() == n0        # the map changed, and the direct search built nothing
        call(masked)
        got_masked = _got(masked, x0)
        assert masked.mask_builds() == n0 + 1    # the one scene that changed
        ref = w["bp"].geo_init(w["maps"][0], w["head"][:, 0], w["tail"][:, 0], scene_ids=w["sids"])
        want = _expected(w, ref)
        on1 = np.flatnonzero((w["sids"] == w["maps"][1].scene_id) & (np.arange(B) != w["bad"]))
        assert not np.array_equal(want["key_pts"][on1], before["key_pts"][on1])      # the new map gives other paths
        for k in GEO_KEYS + ("x0",):
            assert np.array_equal(got_direct[k], want[k], equal_nan=True), k
            assert np.array_equal(got_masked[k], want[k], equal_nan=True), k
    finally:
        _rebuild(c, w["maps"][1], synth.occupancy_2d(1))
    call(direct)
    now = _got(direct, x0)
    for k in GEO_KEYS + ("x0",):
        assert np.array_equal(now[k], before[k], equal_nan=True), k


# ------------------------------------------------------------------ plan_dev against geo_plan
PLAN_KEYS = ("x", "costs", "costs_last", "nit", "nfev", "status", "collision", "attempts", "nit_total", "solved")
IDS = np.arange(64) * 3 + 500          # the requests' stream ids: not their positions


def _as_plan(bufs):
    """plan_dev's resident results as plan's dict has them"""
    h = {k: bufs[k].cpu().numpy() for k in ("x", "costs", "costs_last", "nit", "nfev", "status", "attempts", "nit_total", "solved")}
    st = h["status"]
    return dict(h, status=st & 0xff, collision=(st & _lib.NEO_TRAJ_FLAG_COLLISION) != 0, solved=h["solved"] != 0)


@pytest.mark.parametrize("jitter", ["numpy", "counter"])
def test_plan_dev_is_geo_plan_bit_for_bit(world, jitter):
    torch, dev = _torch()
    w = world
    rows = np.setdiff1d(np.arange(w["B"]), [w["bad"]])[:64]       # 64 requests on the two scenes
    head, tail, sids = w["head"][rows].copy(), w["tail"][rows].copy(), w["sids"][rows]
    head[:, 1] *= 0.3; head[:, 2] = 0.0; tail[:, 1:] = 0.0         # starts in motion, targets at rest
    bp = w["bp"]
    host = bp.geo_plan(w["maps"][0], head, tail, scene_ids=sids, seed=77, stream_ids=IDS, jitter=jitter)
    assert host["attempts"].max() > 1 and host["solved"].sum() > 32      # some retries re-seeded, most requests solved
    d_head, d_tail, d_slots = _dev(head), _dev(tail), _dev(w["slots"][rows])
    torch.cuda.synchronize(dev)
    g = BatchGeoPlanner(bp)
    bufs = g.plan_dev(w["maps"][0], d_head, d_tail, slots=d_slots, seed=77, stream_ids=IDS, jitter=jitter)
    got = _as_plan(bufs)
    for k in PLAN_KEYS:
        assert np.array_equal(got[k], host[k], equal_nan=True), k
    assert np.array_equal(g.key_pts.cpu().numpy(), host["geo"]["key_pts"])
    assert np.array_equal(g.x0.cpu().numpy(), bp.pack_x(host["geo"]["int_wpts"], host["geo"]["ts"]))
    # over a subset of 20 of them: the others keep what they had
    sub = np.sort(np.random.default_rng(9).choice(64, 20, replace=False))
    rest = np.setdiff1d(np.arange(64), sub)
    for k in ("x", "costs", "costs_last"):
        bufs[k].fill_(SENTINEL)
    for k in ("nit", "nfev", "status", "attempts", "nit_total", "solved"):
        bufs[k].fill_(-9)
    g.x0.fill_(SENTINEL)
    d_sub = _dev(sub.astype(np.int32))
    torch.cuda.synchronize(dev)
    g.plan_dev(w["maps"][0], d_head, d_tail, slots=d_slots, subset=d_sub, bufs=bufs, seed=77, stream_ids=IDS, jitter=jitter)
    part = _as_plan(bufs)
    for k in PLAN_KEYS:
        assert np.array_equal(part[k][sub], host[k][sub], equal_nan=True), k
    for k in ("x", "costs", "costs_last"):
        assert np.all(bufs[k].cpu().numpy()[rest] == SENTINEL), k
    for k in ("nit", "nfev", "status", "attempts", "nit_total", "solved"):
        assert np.all(bufs[k].cpu().numpy()[rest] == -9), k
    assert np.all(g.x0.cpu().numpy()[rest] == SENTINEL)


# ------------------------------------------------------------------ the fleet
def test_the_resident_geo_fleet_flies_the_host_geo_fleets_flights():
    """the set-up of test_the_resident_fleet_flies_the_host_fleets_flights, mode "geo" without and with geo="""
    c = _lib.default_context()
    maps = []
    for s in (1, 2):
        m = npa.ESDF()
        m.occupancy_map_cb(synth.OccupancyGridMsg(synth.occupancy_2d(s)))
        maps.append(m)
    try:
        start, goals, sids = draw_missions(maps, 12, seed=3)
        runs = {}
        for resident in (False, True):
            bp = npa.BatchPlanner()
            loop = npa.FleetReplanLoop(bp, maps[0], goals, mode="geo", scene_ids=sids, seed=5, mission_ids=np.arange(24) + 100,
                                       geo=BatchGeoPlanner(bp) if resident else None)
            runs[resident] = (loop, loop.run(start, max_replans=6))
        (host_loop, host), (res_loop, res) = runs[False], runs[True]
        assert host["replans"].sum() >= 24 * 4
        assert res_loop._plan is not None and host_loop._plan is None        # the resident chain ran, and only there
        assert set(res) == set(host)
        for k in host:
            assert np.array_equal(np.asarray(res[k]), np.asarray(host[k]), equal_nan=True), k
        for i in range(24):
            assert np.array_equal(res_loop.commands(i), host_loop.commands(i)), i
        assert np.array_equal(res_loop.x, host_loop.x)
    finally:
        for m in maps:
            c.check(c.lib.neo_esdf_drop(c.h, m.scene_id))


FLEET_CAM = dict(width=64, height=48)


def _onboard_setup():
    """tests/test_gpu_onboard.py's fleet: 8 missions, a 64 x 48 camera, two forests"""
    scenes = [don.boxes_of(synth.forest_boxes(s)) for s in (0, 1)]
    maps = []
    for s in (0, 1):
        m = npa.ESDF()
        m.occupancy_map_cb(synth.OccupancyGridMsg(synth.occupancy_2d(s)))
        maps.append(m)
    B = 8
    scene_index = (np.arange(B) % 2).astype(np.int32)
    rng = np.random.default_rng(42)
    start = np.stack([np.full(B, 0.5), np.linspace(-3.0, 3.0, B)], 1)
    th = rng.uniform(-0.3, 0.3, B)
    goals = start + rng.uniform(10.0, 12.0, B)[:, None] * np.stack([np.cos(th), np.sin(th)], 1)
    sids = np.array([maps[s].scene_id for s in scene_index], dtype=np.int32)
    return dict(packed=DepthCamera.pack_scenes(scenes), maps=maps, B=B, scene_index=scene_index, start=start, goals=goals, sids=sids)


def _fly_onboard(fs, mappers, direct, pick=None, max_replans=25):
    idx = np.arange(fs["B"]) if pick is None else np.asarray(pick)
    mapper = OnboardMapper(_lib.default_context(), DepthCamera(**FLEET_CAM), len(idx))
    mappers.append(mapper)
    bp = npa.BatchPlanner()
    loop = npa.FleetReplanLoop(bp, fs["maps"][0], fs["goals"][idx], mode="geo", geo=BatchGeoPlanner(bp, direct=direct),
                               scene_ids=fs["sids"][idx], mission_ids=idx, onboard=mapper, scenes=fs["packed"],
                               scene_index=fs["scene_index"][idx])
    return loop, mapper, loop.run(fs["start"][idx], max_replans=max_replans)


@pytest.fixture(scope="module")
def onboard_fleet():
    """the fleet in mode geo on its onboard maps, the search in the form `direct=None` chooses for an OnboardMapper"""
    fs = _onboard_setup()
    mappers = []
    loop, mapper, out = _fly_onboard(fs, mappers, None)
    yield fs, mappers, loop, mapper, out
    for m in mappers:
        m.close()
    c = _lib.default_context()
    for m in fs["maps"]:
        c.check(c.lib.neo_esdf_drop(c.h, m.scene_id))


def test_the_direct_search_on_a_live_map_is_geo_init_on_that_map(onboard_fleet):
    """after the first plan the planner's resident key nodes and flags are the host geo_init's on the mapper's own scenes,
    from the resident look-ahead positions and targets: the form the reference fixtures pin, on a map the fleet built"""
    fs, mappers = onboard_fleet[:2]
    g0 = BatchGeoPlanner(npa.BatchPlanner())
    n0 = g0.mask_builds()
    loop, mapper, out = _fly_onboard(fs, mappers, None, max_replans=0)
    assert g0.mask_builds() == n0                # direct=None on an OnboardMapper: the direct form, no mask built
    head, tail = loop._dev["head"].cpu().numpy(), loop._dev["tail"].cpu().numpy()
    ref = loop.bp.geo_init(mapper, head[:, 0], tail[:, 0], scene_ids=mapper.scene_ids)
    g = loop.geo
    for k in GEO_KEYS:
        assert np.array_equal(getattr(g, k).cpu().numpy(), ref[k], equal_nan=True), k
    assert np.array_equal(loop._dev["x0"].cpu().numpy(), loop.bp.pack_x(ref["int_wpts"], ref["ts"]))
    assert (ref["path_len"] > 1).any() and out["replans"].sum() > 0


def test_masked_and_direct_fly_the_same_on_onboard_maps(onboard_fleet):
    fs, mappers, loop, mapper, out = onboard_fleet
    m_loop, m_map, m_out = _fly_onboard(fs, mappers, False)
    for i in range(fs["B"]):
        assert np.array_equal(m_loop.commands(i), loop.commands(i)), i
    assert np.array_equal(m_map.occupancy.cpu().numpy(), mapper.occupancy.cpu().numpy())
    for k in out:
        assert np.array_equal(np.asarray(m_out[k]), np.asarray(out[k]), equal_nan=True), k
    # the run was not vacuous: somebody arrived, and some map holds an obstacle
    assert out["success"].any() and (mapper.occupancy.cpu().numpy() == 100).any()
    print(f"geo on onboard maps, {fs['B']} missions: success {out['success'].mean():.2f}, unsafe "
          f"{np.mean((out['audit_flags'] & _lib.NEO_AUDIT_FLAG_UNSAFE) != 0):.2f}, ticks {len(loop.timings)}")


def test_mission_3_flies_the_same_alone_on_its_onboard_map(onboard_fleet):
    fs, mappers, loop, mapper, out = onboard_fleet
    one, mapper1, o1 = _fly_onboard(fs, mappers, None, pick=[3])
    assert np.array_equal(one.commands(0), loop.commands(3))
    assert np.array_equal(mapper1.occupancy[0].cpu().numpy(), mapper.occupancy[3].cpu().numpy())
    for k in ("success", "replans", "n_flown", "min_clearance", "weighted"):
        assert np.array_equal(np.asarray(o1[k])[0:1], np.asarray(out[k])[3:4], equal_nan=True), k
