"""Onboard maps on the GPU: neo_onboard_integrate_batch[_dev] and OnboardMapper against the NumPy model
(tests/onboard_oracle_np.py) bit for bit, the batched 2-D ESDF build against neo_esdf_build_2d scene by scene, and
FleetReplanLoop(onboard=...) against a replay of its recorded poses through the two oracles."""
import ctypes

import numpy as np
import pytest

import depth_oracle_np as don
import onboard_oracle_np as oon
import neo_planner_amd as npa
from neo_planner_amd import _lib, synth
from neo_planner_amd.depth import DepthCamera
from neo_planner_amd.onboard import OnboardMapper

pytestmark = pytest.mark.gpu

NEO_ERR_INVALID = 1
ORIGIN = (0.0, -15.0)
DEFAULTS = dict(grid=(300, 300), res=0.1, origin=ORIGIN, rng=6.0, band=synth.PROJECT_Z_RANGE, lodds=oon.LOGODDS)
# a 4 m x 3 m grid a metre ahead of every mission's first eye: most of the window lies outside it
SMALL = dict(DEFAULTS, grid=(40, 30), origin="ahead")
COARSE = dict(DEFAULTS, res=0.25, grid=(120, 120), rng=4.0, band=(0.5, 3.0), lodds=(20, -5, -30, 40))


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


_SCENES = {}


def three_scenes():
    """a forest with canopy, a scene WITHOUT boxes between the two others, a second forest"""
    if not _SCENES:
        _SCENES["s"] = [don.boxes_of(synth.forest_boxes(0), synth.canopy_boxes(0, 80)), np.zeros((0, 6)),
                        don.boxes_of(synth.forest_boxes(1), synth.canopy_boxes(1, 20))]
    return _SCENES["s"]


def mission_scans(b, count=3):
    """mission b's scene and `count` successive poses (eye, yaw), a step and a turn apart: they depend on b alone, so a
    batch of 3 is the head of a batch of 70"""
    rng = np.random.default_rng(100 + b)
    eye = np.array([rng.uniform(0.5, 20.0), rng.uniform(-4.0, 4.0), 2.0])
    yaw = rng.uniform(-1.0, 1.0)
    return b % 3, [(eye + k * np.array([0.4, 0.15, 0.0]), yaw + 0.12 * k) for k in range(count)]


def origin_of(cfg, b):
    if cfg["origin"] == "ahead":
        _, scans = mission_scans(b)
        eye, yaw = scans[0]
        return (float(eye[0] + 1.0 * np.cos(yaw) - 1.5), float(eye[1] + 1.0 * np.sin(yaw) - 1.0))
    return cfg["origin"]


_REF = {}


def reference(cam, cfg_name, cfg, b):
    """the oracle's three scans of mission b: per scan (depth_m, pose row, logodds, occupancy, changed, hit, passed);
    computed once per (camera, configuration, mission) and shared"""
    key = (cam.width, cam.height, cfg_name, b)
    if key not in _REF:
        scene, scans = mission_scans(b)
        u, v = oon.camera_tables(cam.width, cam.height, cam.focal_px)
        L = oon.empty(*cfg["grid"])
        out = []
        for eye, yaw in scans:
            depth = don.render(three_scenes()[scene], eye, yaw, cam.width, cam.height, cam.hfov_deg, cam.max_range)["depth_m"]
            c, s = np.cos(yaw), np.sin(yaw)
            L, occ, ch, hit, passed = oon.integrate(L, depth, u, v, np.float32(c), np.float32(s), eye, cfg["res"],
                                                    origin_of(cfg, b), cfg["rng"], cfg["band"], cfg["lodds"])
            out.append((depth, np.array([eye[0], eye[1], eye[2], c, s]), L, occ, ch, hit, passed))
        _REF[key] = out
    return _REF[key]


_MAPPERS = []


@pytest.fixture(autouse=True)
def _close_the_tests_mappers():
    """the default context is shared with the other test files: a test leaves none of its scenes behind (the module's
    fleet fixture, made before this one starts, closes its own)"""
    first = len(_MAPPERS)
    yield
    while len(_MAPPERS) > first:
        _MAPPERS.pop().close()


def make_mapper(cam, cfg, B):
    origins = np.array([origin_of(cfg, b) for b in range(B)])
    _MAPPERS.append(OnboardMapper(_lib.default_context(), cam, B, cfg["grid"][0], cfg["grid"][1], cfg["res"], origins,
                                  sensor_range=cfg["rng"], z_band=cfg["band"], logodds=cfg["lodds"]))
    return _MAPPERS[-1]


def run_scans(cam, cfg_name, cfg, B):
    """three scans of missions 0 .. B - 1 on the GPU, each checked against the oracle; returns the references"""
    torch, dev = _torch()
    mp = make_mapper(cam, cfg, B)
    refs = [reference(cam, cfg_name, cfg, b) for b in range(B)]
    for k in range(3):
        depth = torch.from_numpy(np.stack([r[k][0] for r in refs])).to(dev)
        pose = torch.from_numpy(np.stack([r[k][1] for r in refs])).to(dev)
        changed = mp.integrate(depth, pose).cpu().numpy()
        L, occ = mp.logodds.cpu().numpy(), mp.occupancy.cpu().numpy()
        for b in range(B):
            assert np.array_equal(L[b], refs[b][k][2]), f"logodds of mission {b}, scan {k}"
            assert np.array_equal(occ[b], refs[b][k][3]), f"occupancy of mission {b}, scan {k}"
            assert changed[b] == refs[b][k][4], f"changed of mission {b}, scan {k}"
    return refs


def hit_wins_occurred(refs):
    return any((r[k][5] & r[k][6]).any() for r in refs for k in range(3))


@pytest.mark.parametrize("B", [1, 3, 70])
@pytest.mark.parametrize("size", [(64, 48), (61, 37), (5, 3)])
def test_integrate_equals_the_oracle(size, B):
    """three successive scans of 1, 3 and 70 missions over three scenes (the middle one empty) on the 300 x 300 grid:
    logodds, occupancy and changed after every scan"""
    cam = DepthCamera(width=size[0], height=size[1])
    refs = run_scans(cam, "defaults", DEFAULTS, B)
    if B >= 3 and size[0] > 5:
        assert hit_wins_occurred(refs)                                  # a cell hit by one pixel and passed by another
        assert any(r[2][3].max() == 100 for r in refs) and any(r[k][4] for r in refs for k in range(3))


def test_integrate_on_a_small_grid_ahead_of_the_eye():
    """40 x 30 cells whose origin (per mission) leaves most of the window outside the grid"""
    cam = DepthCamera(width=61, height=37)
    refs = run_scans(cam, "small", SMALL, 6)
    known = sum(int((r[2][2] != oon.UNKNOWN).sum()) for r in refs)
    assert known > 300            # (1200 cells a grid against the window's 28 561)
    assert sum(int(r[k][5].sum()) for r in refs for k in range(3)) > 50 and hit_wins_occurred(refs)


def test_integrate_away_from_the_default_parameters():
    """res 0.25, range 4.0, band (0.5, 3.0), logodds (20, -5, -30, 40): three hits clamp at hi"""
    cam = DepthCamera(width=61, height=37)
    refs = run_scans(cam, "coarse", COARSE, 6)
    clamped = sum(int((r[0][5] & r[1][5] & r[2][5] & (r[2][2] == 40)).sum()) for r in refs)
    assert clamped > 0 and hit_wins_occurred(refs)


def test_clamping_and_clearing_over_nine_scans():
    """Three scans cannot clear a cell or reach hi at octomap's constants (17 - 2 * 8 > 0, 3 * 17 < 70), so: one scan of
    a forest, three of the empty scene from the same pose (the cells hit are passed three times: cleared), five of the
    forest again (- 7 + 5 * 17 clamps at 70), against the oracle after every scan"""
    torch, dev = _torch()
    cam = DepthCamera(width=64, height=48)
    B = 3
    mp = make_mapper(cam, DEFAULTS, B)
    u, v = oon.camera_tables(cam.width, cam.height, cam.focal_px)
    poses = [mission_scans(b)[1][0] for b in range(B)]
    images = {}
    for b, (eye, yaw) in enumerate(poses):
        for scene in (2 * (b % 2), 1):
            images[b, scene] = don.render(three_scenes()[scene], eye, yaw, cam.width, cam.height)["depth_m"]
    L = [oon.empty(300, 300) for _ in range(B)]
    pose = torch.from_numpy(np.array([[e[0], e[1], e[2], np.cos(y), np.sin(y)] for e, y in poses])).to(dev)
    cleared = clamped = 0
    for k in range(9):
        occ_before = [l >= 0 for l in L]                                # (unknown is -128)
        depth = np.stack([images[b, 1 if 1 <= k <= 3 else 2 * (b % 2)] for b in range(B)])
        changed = mp.integrate(torch.from_numpy(depth).to(dev), pose).cpu().numpy()
        got_L, got_occ = mp.logodds.cpu().numpy(), mp.occupancy.cpu().numpy()
        for b, (eye, yaw) in enumerate(poses):
            before = L[b]
            L[b], occ, ch, hit, _ = oon.integrate(before, depth[b], u, v, np.float32(np.cos(yaw)), np.float32(np.sin(yaw)),
                                                  eye, 0.1, ORIGIN)
            assert np.array_equal(got_L[b], L[b]) and np.array_equal(got_occ[b], occ) and changed[b] == ch, (b, k)
            cleared += int((occ_before[b] & (L[b] < 0)).sum())
            clamped += int((hit & (before.astype(int) + 17 > 70) & (L[b] == 70)).sum())
    assert cleared > 0 and clamped > 0


def test_a_subset_leaves_the_other_missions_alone_and_nan_images_mark_nothing():
    torch, dev = _torch()
    cam = DepthCamera(width=61, height=37)
    B = 5
    mp = make_mapper(cam, DEFAULTS, B)
    refs = [reference(cam, "defaults", DEFAULTS, b) for b in range(B)]
    depth = torch.from_numpy(np.stack([r[0][0] for r in refs])).to(dev)
    pose = torch.from_numpy(np.stack([r[0][1] for r in refs])).to(dev)
    mp.integrate(depth, pose)
    L0, occ0 = mp.logodds.cpu().numpy(), mp.occupancy.cpu().numpy()
    mp.changed.fill_(7)
    # missions 3 and 1, in that order, with the second scan's images by position in the subset
    sub = np.array([3, 1], dtype=np.int32)
    depth = torch.from_numpy(np.stack([refs[b][1][0] for b in sub])).to(dev)
    pose = torch.from_numpy(np.stack([refs[b][1][1] for b in sub])).to(dev)
    changed = mp.integrate(depth, pose, subset=sub).cpu().numpy()
    L1, occ1 = mp.logodds.cpu().numpy(), mp.occupancy.cpu().numpy()
    for b in range(B):
        k = 1 if b in sub else 0
        assert np.array_equal(L1[b], refs[b][k][2]) and np.array_equal(occ1[b], refs[b][k][3])
        assert changed[b] == (refs[b][1][4] if b in sub else 7)
    assert np.array_equal(L1[[0, 2, 4]], L0[[0, 2, 4]]) and np.array_equal(occ1[[0, 2, 4]], occ0[[0, 2, 4]])
    # the renderer's NaN image of a request with a bad scene index marks nothing
    boxes, begin = DepthCamera.pack_scenes(three_scenes())
    sidx = np.array([0, 7, 2, 1, 0], dtype=np.int32)
    pose_all = torch.from_numpy(np.stack([r[2][1] for r in refs])).to(dev)
    img = cam.render_dev(torch.from_numpy(boxes).to(dev), torch.from_numpy(begin).to(dev), pose_all,
                         torch.from_numpy(sidx).to(dev))["depth_m"]
    assert torch.isnan(img[1]).all() and not torch.isnan(img[0]).any()
    changed = mp.integrate(img, pose_all).cpu().numpy()
    assert np.array_equal(mp.logodds[1].cpu().numpy(), L1[1]) and changed[1] == 0
    assert not np.array_equal(mp.logodds[0].cpu().numpy(), L1[0])


def test_indices_to_skip_and_the_empty_subset_in_the_device_form():
    """subset [3, -1, 1, B, B + 7] of 5 missions (5 x 3 images, the 40 x 30 grid): missions 3 and 1 get the bits of the
    call without a subset, every other grid keeps its sentinel; a subset of no entries returns 0 and writes nothing"""
    torch, dev = _torch()
    cam = DepthCamera(width=5, height=3)
    cfg, B = SMALL, 5
    gw, gh = cfg["grid"]
    scans = [reference(cam, "small", cfg, b)[0] for b in range(B)]
    origins = torch.from_numpy(np.array([origin_of(cfg, b) for b in range(B)])).to(dev)
    sub = np.array([3, -1, 1, B, B + 7], dtype=np.int32)
    c = _lib.default_context()

    def run(subset, n):
        at = list(range(B)) if subset is None else [int(b) if 0 <= b < B else 0 for b in subset]   # rows by launch position
        depth = torch.from_numpy(np.stack([scans[b][0] for b in at])).to(dev)
        pose = torch.from_numpy(np.stack([scans[b][1] for b in at])).to(dev)
        L = torch.full((B, gh, gw), oon.UNKNOWN, dtype=torch.int8, device=dev)
        occ = torch.full((B, gh, gw), -1, dtype=torch.int8, device=dev)
        changed = torch.full((B,), 9, dtype=torch.int32, device=dev)
        d_sub = None if subset is None else torch.from_numpy(subset).to(dev)
        torch.cuda.synchronize(dev)
        assert c.lib.neo_onboard_integrate_batch_dev(
            c.h, B, _p(d_sub), n, _p(depth), _p(pose), cam.width, cam.height, cam.focal_px, cam.max_range, gw, gh, cfg["res"],
            _p(origins), cfg["rng"], cfg["band"][0], cfg["band"][1], 17, -8, -40, 70, _p(L), _p(occ), _p(changed)) == 0
        c.synchronize()
        return L.cpu().numpy(), occ.cpu().numpy(), changed.cpu().numpy()

    full, part, none = run(None, 0), run(sub, len(sub)), run(sub, 0)
    on = np.isin(np.arange(B), [3, 1])
    assert np.all(full[2] != 9) and all((full[0][b] != oon.UNKNOWN).any() for b in (3, 1))
    for f, p, e, sentinel in zip(full, part, none, (oon.UNKNOWN, -1, 9)):
        assert np.array_equal(p[on], f[on])
        assert np.all(p[~on] == sentinel)
        assert np.all(e == sentinel)


def test_host_twin_equals_the_device_form():
    cam = DepthCamera(width=61, height=37)
    cfg = SMALL
    B = 4
    refs = [reference(cam, "small", cfg, b) for b in range(B)]
    gw, gh = cfg["grid"]
    origins = np.array([origin_of(cfg, b) for b in range(B)])
    L = np.full((B, gh, gw), oon.UNKNOWN, dtype=np.int8)
    occ = np.full((B, gh, gw), -1, dtype=np.int8)
    changed = np.full(B, 9, dtype=np.int32)
    sub = np.array([2, 0, 3], dtype=np.int32)
    c = _lib.default_context()
    for k in range(3):
        depth = np.ascontiguousarray(np.stack([refs[b][k][0] for b in sub]))
        pose = np.ascontiguousarray(np.stack([refs[b][k][1] for b in sub]))
        c.check(c.lib.neo_onboard_integrate_batch(c.h, B, _lib.ptr(sub), len(sub), _lib.ptr(depth), _lib.ptr(pose), cam.width,
                                                  cam.height, cam.focal_px, cam.max_range, gw, gh, cfg["res"],
                                                  _lib.ptr(origins), cfg["rng"], cfg["band"][0], cfg["band"][1], 17, -8, -40,
                                                  70, _lib.ptr(L), _lib.ptr(occ), _lib.ptr(changed)))
        for b in sub:
            assert np.array_equal(L[b], refs[b][k][2]) and np.array_equal(occ[b], refs[b][k][3]) and changed[b] == refs[b][k][4]
    assert np.all(L[1] == oon.UNKNOWN) and np.all(occ[1] == -1) and changed[1] == 9
    # a mission listed twice would be updated by two workgroups at once: refused, nothing written
    twice = np.array([2, 0, 2], dtype=np.int32)
    before = L.copy()
    rc = c.lib.neo_onboard_integrate_batch(c.h, B, _lib.ptr(twice), 3, _lib.ptr(depth), _lib.ptr(pose), cam.width, cam.height,
                                           cam.focal_px, cam.max_range, gw, gh, cfg["res"], _lib.ptr(origins), cfg["rng"],
                                           cfg["band"][0], cfg["band"][1], 17, -8, -40, 70, _lib.ptr(L), _lib.ptr(occ),
                                           _lib.ptr(changed))
    assert rc == NEO_ERR_INVALID and b"twice" in c.lib.neo_last_error(c.h) and np.array_equal(L, before)


def test_argument_errors():
    """a window beyond LDS, a camera that does not reach sensor_range, log-odds outside a byte: NEO_ERR_INVALID with a
    message, nothing written"""
    c = _lib.default_context()
    cam = DepthCamera(width=5, height=3)
    depth = np.zeros((1, 3, 5), dtype=np.float32)
    pose = np.array([[0.55, 0.55, 2.0, 1.0, 0.0]])
    origins = np.zeros((1, 2))
    L = np.full((1, 10, 10), oon.UNKNOWN, dtype=np.int8)
    occ = np.full((1, 10, 10), -1, dtype=np.int8)
    changed = np.full(1, 5, dtype=np.int32)

    def call(res=0.1, rng=6.0, max_range=20.0, lodds=(17, -8, -40, 70)):
        return c.lib.neo_onboard_integrate_batch(c.h, 1, None, 0, _lib.ptr(depth), _lib.ptr(pose), cam.width, cam.height,
                                                 cam.focal_px, max_range, 10, 10, res, _lib.ptr(origins), rng, 1.8, 10.0,
                                                 lodds[0], lodds[1], lodds[2], lodds[3], _lib.ptr(L), _lib.ptr(occ),
                                                 _lib.ptr(changed))

    assert call(res=0.01) == NEO_ERR_INVALID and b"LDS" in c.lib.neo_last_error(c.h)
    assert call(res=0.02) == NEO_ERR_INVALID                # 2 * 415 + 1 cells a side: 172 KB of marks
    assert call(max_range=5.9) == NEO_ERR_INVALID and b"max_range" in c.lib.neo_last_error(c.h)
    assert call(lodds=(17, -8, -128, 70)) == NEO_ERR_INVALID and call(lodds=(17, -8, -40, 128)) == NEO_ERR_INVALID
    assert np.all(L == oon.UNKNOWN) and np.all(occ == -1) and changed[0] == 5
    assert call() == 0 and changed[0] == 1 and L[0, 5, 5] == 17 and occ[0, 5, 5] == 100    # depth 0: a hit in the eye's own cell
    assert (L != oon.UNKNOWN).sum() == 1
    with pytest.raises(ValueError):
        OnboardMapper(c, DepthCamera(width=5, height=3, max_range=5.0), 1)


# ------------------------------------------------------------------ the batched ESDF build
def _occupancies(n, W, H, seed):
    """n grids: random blocks of occupied and unknown cells; among five, the second all free and the fourth all occupied"""
    rng = np.random.default_rng(seed)
    occ = np.zeros((n, H, W), dtype=np.int8)
    for k in range(n):
        for _ in range(6):
            x, y = rng.integers(0, W), rng.integers(0, H)
            occ[k, y:y + rng.integers(1, 8), x:x + rng.integers(1, 8)] = 100
        occ[k][rng.random((H, W)) < 0.05] = -1
    if n >= 5:
        occ[1] = np.where(rng.random((H, W)) < 0.3, -1, 0)
        occ[3] = 100
    return occ


def _cell_centres(W, H, res, origin):
    ix, iy = np.meshgrid(np.arange(W), np.arange(H))
    return np.stack([origin[0] + (ix.ravel() + 0.5) * res, origin[1] + (iy.ravel() + 0.5) * res], 1)


def _query(c, scene_id, pts):
    d, g = np.empty(len(pts)), np.empty((len(pts), 2))
    c.check(c.lib.neo_esdf_query(c.h, scene_id, len(pts), _lib.ptr(pts), _lib.ptr(d), _lib.ptr(g)))
    return d, g


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("size", [(300, 300), (37, 23), (1, 1), (520, 40)])
def test_batched_build_equals_build_2d(size, n):
    """scene by scene through neo_esdf_query on every cell centre, bit for bit (520 x 40 takes the sweeps); a second
    build of changed occupancy keeps every slot and serves the new distances"""
    torch, dev = _torch()
    c = _lib.default_context()
    W, H = size
    res = 0.1
    origins = np.stack([np.linspace(0.0, 2.0, n), np.linspace(-15.0, -14.0, n)], 1)
    ids = np.array([c.new_scene_id() for _ in range(n)], dtype=np.int32)
    for round_ in range(2):
        occ = _occupancies(n, W, H, seed=10 * W + n + round_)
        occ_dev = torch.from_numpy(occ).to(dev)
        torch.cuda.synchronize(dev)
        slots = [c.lib.neo_scene_slot(c.h, int(s)) for s in ids]
        c.check(c.lib.neo_esdf_build_2d_batch_dev(c.h, _lib.ptr(ids), n, _p(occ_dev), W, H, res, _lib.ptr(origins)))
        now = [c.lib.neo_scene_slot(c.h, int(s)) for s in ids]
        assert min(now) >= 0 and len(set(now)) == n
        if round_ == 1:
            assert now == slots                                 # rewritten in place: no slot moved
        for k in range(n):
            single = c.new_scene_id()
            dist = np.empty((H, W))
            c.check(c.lib.neo_esdf_build_2d(c.h, single, _lib.ptr(occ[k]), W, H, res, origins[k, 0], origins[k, 1],
                                            _lib.ptr(dist), None, None))
            pts = _cell_centres(W, H, res, origins[k])
            d1, g1 = _query(c, single, pts)
            c.check(c.lib.neo_esdf_drop(c.h, single))
            d0, g0 = _query(c, int(ids[k]), pts)
            assert np.array_equal(d0.view(np.uint64), d1.view(np.uint64)), f"distances of map {k}"
            assert np.array_equal(g0.view(np.uint64), g1.view(np.uint64)), f"gradients of map {k}"
            assert np.array_equal(d0.reshape(H, W), dist)
    for s in ids:
        c.check(c.lib.neo_esdf_drop(c.h, int(s)))


def test_rebuild_in_place_keeps_a_loops_slots_valid():
    """OnboardMapper: scans and rebuilds leave `slots` and neo_scene_slot as they were, and query() serves the new map"""
    torch, dev = _torch()
    cam = DepthCamera(width=64, height=48)
    B = 4
    mp = make_mapper(cam, DEFAULTS, B)
    c = mp.ctx
    slots = mp.slots.cpu().numpy().copy()
    refs = [reference(cam, "defaults", DEFAULTS, b) for b in range(B)]
    probe = _cell_centres(300, 300, 0.1, ORIGIN)
    before = [mp.query(b, probe)[0] for b in range(B)]
    depth = torch.from_numpy(np.stack([r[0][0] for r in refs])).to(dev)
    pose = torch.from_numpy(np.stack([r[0][1] for r in refs])).to(dev)
    changed = mp.integrate(depth, pose).cpu().numpy()
    rebuilt = mp.rebuild()
    assert np.array_equal(rebuilt, np.flatnonzero(changed)) and 0 < len(rebuilt) < B       # (mission 1 sees the empty scene)
    assert [c.lib.neo_scene_slot(c.h, int(s)) for s in mp.scene_ids] == slots.tolist()
    for b in range(B):
        occ = refs[b][0][3]
        m = npa.ESDF()
        m.occupancy_map_cb(synth.OccupancyGridMsg(occ))
        d, _ = mp.query(b, probe)
        assert np.array_equal(d.reshape(300, 300), m.esdf_map)
        assert np.array_equal(d, before[b]) == (changed[b] == 0)
        c.check(c.lib.neo_esdf_drop(c.h, m.scene_id))


# ------------------------------------------------------------------ the fleet
FLEET_CAM = dict(width=64, height=48)


def _fleet_setup():
    scenes = [don.boxes_of(synth.forest_boxes(s)) for s in (0, 1)]
    boxes, begin = DepthCamera.pack_scenes(scenes)
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
    return dict(scenes=scenes, packed=(boxes, begin), maps=maps, B=B, scene_index=scene_index, start=start, goals=goals,
                sids=sids)


def _fly(fs, pick=None, **kw):
    idx = np.arange(fs["B"]) if pick is None else np.asarray(pick)
    cam = DepthCamera(**FLEET_CAM)
    mapper = OnboardMapper(_lib.default_context(), cam, len(idx))
    _MAPPERS.append(mapper)
    loop = npa.FleetReplanLoop(npa.BatchPlanner(), fs["maps"][0], fs["goals"][idx], scene_ids=fs["sids"][idx],
                               mission_ids=idx, onboard=mapper, scenes=fs["packed"], scene_index=fs["scene_index"][idx],
                               record_poses=True, **kw)
    out = loop.run(fs["start"][idx], max_replans=25)
    return loop, mapper, out


@pytest.fixture(scope="module")
def fleet():
    fs = _fleet_setup()
    loop, mapper, out = _fly(fs)
    print(f"onboard fleet of {fs['B']}: success {out['success'].mean():.2f}, unsafe "
          f"{np.mean((out['audit_flags'] & _lib.NEO_AUDIT_FLAG_UNSAFE) != 0):.2f}, ticks {len(loop.timings)}, sensing "
          f"{sum(t['sense_s'] for t in loop.timings) / sum(t['tick_s'] for t in loop.timings):.2f} of the tick time")
    _MAPPERS.remove(mapper)             # (kept for the module's tests)
    yield fs, loop, mapper, out
    mapper.close()
    c = _lib.default_context()
    for m in fs["maps"]:
        c.check(c.lib.neo_esdf_drop(c.h, m.scene_id))


def test_fleet_maps_equal_a_replay_of_the_recorded_poses(fleet):
    fs, loop, mapper, out = fleet
    poses, sensed = out["poses"], out["sensed"]
    assert poses.shape[1:] == (fs["B"], 5) and sensed.shape == poses.shape[:2] and sensed[0].all()
    cam = mapper.camera
    u, v = oon.camera_tables(cam.width, cam.height, cam.focal_px)
    got = mapper.occupancy.cpu().numpy()
    for b in range(fs["B"]):
        L = oon.empty(300, 300)
        occ = np.full((300, 300), -1, dtype=np.int8)
        for t in np.flatnonzero(sensed[:, b]):
            ex, ey, ez, c, s = poses[t, b]
            assert ez == 2.0 and abs(c * c + s * s - 1.0) < 1e-12
            depth = don.render(fs["scenes"][fs["scene_index"][b]], (ex, ey, ez), oon.yaw_of(c, s), cam.width, cam.height)["depth_m"]
            L, occ, _, _, _ = oon.integrate(L, depth, u, v, np.float32(c), np.float32(s), (ex, ey, ez), 0.1, ORIGIN)
        assert np.array_equal(got[b], occ), f"mission {b}"
    assert (got == 100).any()
    # the first pose looks at the goal from the start; the pose of tick t stands on row t * step of the command array
    # (rows before a splice point never change) and looks along the step that led there
    want = np.array([oon.heading((0.0, 0.0), d) for d in fs["goals"] - fs["start"]])
    assert np.array_equal(poses[0][:, 3:], want) and np.array_equal(poses[0][:, :2], fs["start"])
    step = int(round(loop.replan_period * loop.cmd_hz))
    checked = 0
    for b in range(fs["B"]):
        cmd = loop.commands(b)
        for t in np.flatnonzero(sensed[:, b]):
            k = t * step
            if t == 0 or k >= len(cmd) - 1:
                continue
            assert np.array_equal(poses[t, b, :2], cmd[k, 0])
            assert tuple(poses[t, b, 3:]) == oon.heading(cmd[k, 0] - cmd[k - 1, 0], fs["goals"][b] - cmd[k, 0])
            checked += 1
    assert checked > fs["B"]


def test_mission_3_flies_the_same_alone(fleet):
    fs, loop, mapper, out = fleet
    one, mapper1, o1 = _fly(fs, pick=[3])
    assert np.array_equal(one.commands(0), loop.commands(3))
    assert np.array_equal(mapper1.occupancy[0].cpu().numpy(), mapper.occupancy[3].cpu().numpy())
    assert np.array_equal(mapper1.logodds[0].cpu().numpy(), mapper.logodds[3].cpu().numpy())
    for k in ("success", "replans", "n_flown", "min_clearance", "weighted"):
        assert np.array_equal(np.asarray(o1[k])[0:1], np.asarray(out[k])[3:4], equal_nan=True), k


@pytest.mark.parametrize("mode", ["basic", "batch"])
def test_resident_flies_the_same_flights(fleet, mode):
    fs = fleet[0]
    pick = [0, 1, 2, 3]
    a_loop, a_map, a = _fly(fs, pick=pick, mode=mode, resident=False)
    b_loop, b_map, b = _fly(fs, pick=pick, mode=mode, resident=True)
    for i in range(len(pick)):
        assert np.array_equal(a_loop.commands(i), b_loop.commands(i)), (mode, i)
    assert np.array_equal(a_map.occupancy.cpu().numpy(), b_map.occupancy.cpu().numpy())
    assert np.array_equal(a["success"], b["success"]) and np.array_equal(a["poses"], b["poses"])
    print(f"{mode}: success {a['success'].mean():.2f}")
    if mode == "basic":
        for i in range(len(pick)):
            assert np.array_equal(a_loop.commands(i), fleet[1].commands(pick[i]))


def test_without_onboard_nothing_changes(fleet):
    fs = fleet[0]
    pick = [0, 1]
    outs = []
    for kw in (dict(), dict(onboard=None, scenes=None, scene_index=None, record_poses=False)):
        loop = npa.FleetReplanLoop(npa.BatchPlanner(), fs["maps"][0], fs["goals"][pick], scene_ids=fs["sids"][pick], **kw)
        out = loop.run(fs["start"][pick], max_replans=25)
        outs.append((out, [loop.commands(i) for i in range(len(pick))]))
        assert "poses" not in out and all("sense_s" not in t for t in loop.timings)
    for k in outs[0][0]:
        assert np.array_equal(np.asarray(outs[0][0][k]), np.asarray(outs[1][0][k]), equal_nan=True), k
    for a, b in zip(outs[0][1], outs[1][1]):
        assert np.array_equal(a, b)


def test_a_second_run_starts_from_nothing_and_from_the_tables_slots(fleet):
    """run() resets the mapper and reads its slots again: a second run of the same loop, after a scene with a lower id
    was dropped (the map table is renumbered), flies the first run's flights"""
    fs = fleet[0]
    c = _lib.default_context()
    early = npa.ESDF()
    early.occupancy_map_cb(synth.OccupancyGridMsg(synth.occupancy_2d(5)))
    pick = [2, 3]
    loop, mapper, first = _fly(fs, pick=pick)
    cmds = [loop.commands(i) for i in range(len(pick))]
    occ = mapper.occupancy.cpu().numpy()
    slots = mapper.slots.cpu().numpy().copy()
    c.check(c.lib.neo_esdf_drop(c.h, early.scene_id))
    second = loop.run(fs["start"][pick], max_replans=25)
    assert not np.array_equal(mapper.slots.cpu().numpy(), slots)           # renumbered, and followed
    for i in range(len(pick)):
        assert np.array_equal(loop.commands(i), cmds[i])
        assert np.array_equal(loop.commands(i), fleet[1].commands(pick[i]))
    assert np.array_equal(mapper.occupancy.cpu().numpy(), occ)
    assert np.array_equal(first["success"], second["success"]) and np.array_equal(first["poses"], second["poses"])


def test_geo_mode_refuses_onboard_maps(fleet):
    fs = fleet[0]
    with pytest.raises(ValueError):
        npa.FleetReplanLoop(npa.BatchPlanner(), fs["maps"][0], fs["goals"], mode="geo", onboard=fleet[2], scenes=fs["packed"])
