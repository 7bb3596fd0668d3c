"""The batched depth camera on the GPU (neo_depth_render_batch[_dev], DepthCamera, BatchNeoPlanner) against the NumPy
float32 restatement of its arithmetic (tests/depth_oracle_np.py): depth_m through its uint32 view, depth_max and depth_u8
equal bit for bit, not close."""
import math

import numpy as np
import pytest

import depth_oracle_np as don
import neo_planner_amd as npa
from neo_planner_amd import _lib, synth
from neo_planner_amd.depth import DepthCamera

pytestmark = pytest.mark.gpu

NEO_ERR_INVALID = 1


def forest(scene, canopy=80):
    return don.boxes_of(synth.forest_boxes(scene), synth.canopy_boxes(scene, canopy) if canopy else ())


_SCENES = {}


def three_scenes():
    """a forest with canopy, a scene WITHOUT boxes (ground and sky only) between two others in box_begin, a second forest"""
    if not _SCENES:
        _SCENES["s"] = [forest(0, 80), np.zeros((0, 6)), forest(1, 20)]
    return _SCENES["s"]


def requests(B, seed=0):
    rng = np.random.default_rng(100 + seed)
    eye = np.stack([rng.uniform(0.5, 20.0, B), rng.uniform(-4.0, 4.0, B), np.full(B, 2.0)], axis=1)
    yaw = rng.uniform(-1.0, 1.0, B)
    yaw[0] = 0.0                    # an odd width then has a centre column with dy = 0
    return eye, yaw, (np.arange(B) % 3).astype(np.int32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_image(out, b, boxes, eye, yaw, cam):
    ref = don.render(boxes, eye, yaw, cam.width, cam.height, cam.hfov_deg, cam.max_range)
    assert np.array_equal(bits(out["depth_m"][b]), bits(ref["depth_m"])), f"depth_m of image {b}"
    assert bits(out["depth_max"][b:b + 1])[0] == bits(np.array([ref["depth_max"]]))[0], f"depth_max of image {b}"
    assert np.array_equal(out["depth_u8"][b], ref["depth_u8"]), f"depth_u8 of image {b}"
    return ref


@pytest.mark.parametrize("B", [1, 3, 70])
@pytest.mark.parametrize("size", [(64, 48), (61, 37), (5, 3)])
def test_sizes_and_batches(size, B):
    """64 x 48, 61 x 37 and 5 x 3 (odd widths: a packed-store tail and a centre column with dy = 0 at yaw 0) for 1, 3 and
    70 requests over three scenes, the middle one empty"""
    cam = DepthCamera(width=size[0], height=size[1])
    scenes = three_scenes()
    eye, yaw, sidx = requests(B)
    out = cam.render(scenes, eye, yaw, sidx)
    assert out["depth_m"].shape == (B, size[1], size[0]) and out["depth_u8"].dtype == np.uint8
    for b in range(B):
        check_image(out, b, scenes[sidx[b]], eye[b], yaw[b], cam)


def test_full_size_image():
    cam = DepthCamera()
    assert (cam.width, cam.height) == (640, 480)
    boxes = forest(0, 80)
    eye, yaw = np.array([[1.5, 0.3, 2.0]]), np.array([0.2])
    out = cam.render(boxes, eye, yaw)
    ref = check_image(out, 0, boxes, eye[0], yaw[0], cam)
    assert 0 < ref["depth_u8"].min() < 255 == ref["depth_u8"].max()


def test_edge_poses():
    W, H = 61, 37
    cam = DepthCamera(width=W, height=H)
    woods = forest(2, 80)

    def one(boxes, eye, yaw, camera=cam):
        out = camera.render(np.asarray(boxes, dtype=np.float64).reshape(-1, 6), np.array([eye], dtype=np.float64),
                            np.array([yaw]))
        return out, check_image(out, 0, boxes, eye, yaw, camera)

    # the eye inside a box: depth 0 wherever the box is seen -- from inside, everywhere
    inside = np.concatenate([woods, [[4.0, -1.0, 0.0, 6.0, 1.0, 4.0]]])
    out, ref = one(inside, (5.0, 0.0, 2.0), 0.3)
    assert out["depth_max"][0] == 0.0 and not out["depth_m"].any() and not out["depth_u8"].any()
    assert bits(out["depth_m"]).max() == 0                                      # +0, never -0
    # the eye on a face, looking across it: rays that enter and rays that only touch it at t = 0 (a far side of -0)
    out, ref = one([[5.0, -1.0, 0.0, 6.0, 1.0, 4.0]], (5.0, 0.0, 2.0), 2.0)
    assert not ref["depth_m"].any() and bits(out["depth_m"]).max() == 0
    # max_range in front of everything: all 255
    near = DepthCamera(width=W, height=H, max_range=0.5)
    out, ref = one(woods, (1.0, 0.0, 2.0), 0.0, near)
    assert np.all(out["depth_u8"] == 255) and np.all(out["depth_m"] == np.float32(0.5))
    # high above the ground, looking level
    one(woods, (3.0, 1.0, 25.0), -0.4)
    # yaw 0 with the eye's y exactly on a face's plane: the centre column's dy is 0 and 0 * inf is a miss
    out, ref = one([[3.0, 0.0, 0.0, 4.0, 1.0, 4.0], [6.0, -2.0, 0.0, 7.0, 0.0, 4.0]], (0.0, 0.0, 2.0), 0.0)
    assert ref["depth_m"][H // 2, W // 2] == np.float32(20.0) and ref["depth_m"][H // 2, W // 2 - 1] == np.float32(3.0)
    # quarter and half turns, cos and sin from NumPy (6e-17, not 0)
    for yaw in (np.pi / 2, -np.pi / 2, np.pi):
        one(woods, (15.0, 0.5, 2.0), yaw)
    # every box behind the camera
    out, ref = one(forest(2, 0), (29.5, 0.0, 2.0), 0.0)
    assert ref["depth_m"].max() == np.float32(20.0)
    # a scene of exactly NEO_DEPTH_MAX_BOXES small boxes at 5 x 3
    n = int(math.isqrt(_lib.NEO_DEPTH_MAX_BOXES))
    assert n * n == _lib.NEO_DEPTH_MAX_BOXES == 1024
    gx, gy = np.meshgrid(2.0 + 0.3 * np.arange(n), -4.8 + 0.3 * np.arange(n), indexing="ij")
    lo = np.stack([gx.ravel(), gy.ravel(), np.full(n * n, 1.9)], axis=1)
    many = np.concatenate([lo, lo + 0.2], axis=1)
    out, ref = one(many, (0.0, 0.1, 2.0), 0.1, DepthCamera(width=5, height=3))
    assert ref["depth_m"].min() < 3.0


def test_images_do_not_depend_on_the_batch():
    """rows {2, 5, 11} of a 16-image batch over two scenes, rendered alone and in reverse order, equal their rows of the
    full batch; the _dev form equals the host form; render_dev in chunks of 3 equals one launch of 8"""
    import torch
    cam = DepthCamera(width=61, height=37)
    scenes = [forest(0, 80), forest(3, 40)]
    rng = np.random.default_rng(7)
    B = 16
    eye = np.stack([rng.uniform(0.5, 20.0, B), rng.uniform(-4.0, 4.0, B), np.full(B, 2.0)], axis=1)
    yaw = rng.uniform(-1.0, 1.0, B)
    sidx = rng.integers(0, 2, B).astype(np.int32)
    full = cam.render(scenes, eye, yaw, sidx)
    rows = [11, 5, 2]
    # alone, reversed, and with the scenes packed the other way round
    part = cam.render(scenes[::-1], eye[rows], yaw[rows], 1 - sidx[rows])
    for k in ("depth_u8", "depth_max", "depth_m"):
        assert np.array_equal(part[k].view(np.uint8), full[k][rows].view(np.uint8)), k
    boxes, begin = cam.pack_scenes(scenes)
    t = lambda a: torch.as_tensor(a, device="cuda")
    dev = cam.render_dev(t(boxes), t(begin), t(cam.poses(eye, yaw)), t(sidx))
    for k in ("depth_u8", "depth_max", "depth_m"):
        assert np.array_equal(dev[k].cpu().numpy().view(np.uint8), full[k].view(np.uint8)), k
    a = cam.render_dev(t(boxes), t(begin), t(cam.poses(eye[:8], yaw[:8])), t(sidx[:8]), chunk=3, want_m=False)
    b8 = cam.render_dev(t(boxes), t(begin), t(cam.poses(eye[:8], yaw[:8])), t(sidx[:8]), chunk=8)
    assert "depth_m" not in a
    for k in ("depth_u8", "depth_max"):
        assert np.array_equal(a[k].cpu().numpy().view(np.uint8), b8[k].cpu().numpy().view(np.uint8)), k
        assert np.array_equal(a[k].cpu().numpy().view(np.uint8), full[k][:8].view(np.uint8)), k


def test_errors_leave_the_outputs_alone():
    cam = DepthCamera(width=16, height=8)
    c = cam.ctx
    W, H, B = 16, 8, 2
    boxes = forest(0, 0)
    nb = boxes.shape[0]
    begin = np.array([0, nb], dtype=np.int32)
    pose = cam.poses(np.array([[1.0, 0.0, 2.0], [2.0, 1.0, 2.0]]), np.array([0.0, 0.3]))
    sidx = np.zeros(B, dtype=np.int32)
    m = np.full((B, H, W), -7.0, dtype=np.float32)
    u8 = np.full((B, H, W), 77, dtype=np.uint8)
    mx = np.full(B, -7.0, dtype=np.float32)
    base = dict(width=W, height=H, focal=cam.focal_px, max_range=20.0, boxes=boxes, begin=begin, n_scenes=1, sidx=sidx,
                B=B, pose=pose, m=m)

    def call(**kw):
        a = dict(base, **kw)
        return c.lib.neo_depth_render_batch(c.h, a["width"], a["height"], float(a["focal"]), float(a["max_range"]),
                                            _lib.ptr(a["boxes"]), _lib.ptr(a["begin"]), a["n_scenes"], _lib.ptr(a["sidx"]),
                                            a["B"], _lib.ptr(a["pose"]), _lib.ptr(a["m"]), _lib.ptr(u8), _lib.ptr(mx))

    one_too_many = np.tile(boxes[:1], (_lib.NEO_DEPTH_MAX_BOXES + 1, 1))
    bad = [dict(B=0), dict(B=-1), dict(width=0), dict(width=4097), dict(height=0), dict(height=4097),
           dict(focal=0.0), dict(focal=-3.0), dict(focal=np.nan), dict(focal=np.inf),
           dict(max_range=0.0), dict(max_range=-1.0), dict(max_range=np.nan), dict(max_range=np.inf),
           dict(n_scenes=0), dict(boxes=None), dict(begin=None), dict(pose=None), dict(m=None),
           dict(begin=np.array([1, nb], dtype=np.int32)),
           dict(begin=np.array([0, nb, nb - 1], dtype=np.int32), n_scenes=2),
           dict(boxes=one_too_many, begin=np.array([0, _lib.NEO_DEPTH_MAX_BOXES + 1], dtype=np.int32)),
           dict(sidx=np.array([0, 1], dtype=np.int32)), dict(sidx=np.array([-1, 0], dtype=np.int32))]
    for kw in bad:
        assert call(**kw) == NEO_ERR_INVALID, kw
        assert c.lib.neo_last_error(c.h).decode().startswith("depth:"), kw
        assert np.all(m == -7.0) and np.all(u8 == 77) and np.all(mx == -7.0), kw
    # exactly the maximum is fine, and the context is still usable
    most = np.tile(boxes[:1], (_lib.NEO_DEPTH_MAX_BOXES, 1))
    assert call(boxes=most, begin=np.array([0, _lib.NEO_DEPTH_MAX_BOXES], dtype=np.int32)) == _lib.NEO_OK
    assert call() == _lib.NEO_OK
    ref = don.render(boxes, pose[1, :3], 0.3, W, H)
    assert np.array_equal(bits(m[1]), bits(ref["depth_m"])) and np.array_equal(u8[1], ref["depth_u8"])


def test_dev_form_marks_a_request_with_a_scene_out_of_range():
    import torch
    cam = DepthCamera(width=61, height=37)
    scenes = [forest(0, 80), forest(3, 40)]
    eye = np.array([[1.0, 0.0, 2.0], [2.0, 1.0, 2.0], [3.0, -1.0, 2.0]])
    yaw = np.array([0.0, 0.3, -0.2])
    sidx = np.array([1, 2, 0], dtype=np.int32)           # the middle request names scene n_scenes
    boxes, begin = cam.pack_scenes(scenes)
    t = lambda a: torch.as_tensor(a, device="cuda")
    out = {k: v.cpu().numpy() for k, v in cam.render_dev(t(boxes), t(begin), t(cam.poses(eye, yaw)), t(sidx)).items()}
    assert np.all(np.isnan(out["depth_m"][1])) and not out["depth_u8"][1].any() and np.isnan(out["depth_max"][1])
    for b in (0, 2):
        check_image(out, b, scenes[sidx[b]], eye[b], yaw[b], cam)


def test_batch_neo_planner():
    """NeoPlanner.enhanced_traj_plan for 5 requests over two camera scenes of one 2-D map, against the per-request path"""
    import torch
    from neo_planner_amd import initializer as ini
    from test_initializer import _net
    H, W, B = 48, 64, 5
    net = _net(H, W)
    ref_net = _net(H, W)                                     # the same seeded weights, kept on the CPU
    binit = ini.BatchInitializer(net=net, device="cuda")
    cam = DepthCamera(width=W, height=H)
    bp = npa.BatchPlanner()
    neo = ini.BatchNeoPlanner(bp, binit, cam, des_pos_z=2.0)
    occ = synth.occupancy_2d(0)
    m = npa.ESDF()
    m.occupancy_map_cb(synth.OccupancyGridMsg(occ))
    pillars = [synth.forest_boxes(0), synth.forest_boxes(1)]
    scenes = [don.boxes_of(p) for p in pillars]
    head, tail, _, _ = synth.replan_requests(0, B, 2, D=2, length_range=(4.0, 6.0))
    sidx = np.array([0, 1, 0, 1, 1], dtype=np.int32)
    pos = np.concatenate([head[:, 0], np.full((B, 1), 2.0)], axis=1)
    vel = np.concatenate([head[:, 1], np.zeros((B, 1))], axis=1)
    d = tail[:, 0] - head[:, 0]
    yaw = np.arctan2(d[:, 1], d[:, 0])
    lvel = np.stack([ini.Quat.from_yaw(y).inverse.rotate(v) for y, v in zip(yaw, vel)])
    out = neo.plan(m, scenes, pos, vel, lvel, yaw, head, tail, scene_index=sidx, seed=5)

    # the images: raycast_depth of each request, under the cap of tests/test_depth_cpu.py
    got_u8 = out["depth_u8"].cpu().numpy()
    want_u8 = [ini.raycast_depth(pillars[sidx[b]], eye=pos[b], yaw=yaw[b], height=H, width=W) for b in range(B)]
    diff = sum(int(np.count_nonzero(got_u8[b] != want_u8[b])) for b in range(B))
    print(f"BatchNeoPlanner images vs raycast_depth: {diff} of {B * H * W} pixels differ")
    assert diff <= math.ceil(B * H * W / 100000)

    # the warm starts: form_nn_input -> net -> get_wpts_world per request, durations clamped like warm_start's.
    # Tolerance: tests/test_initializer.py test_initializer_on_gpu_feeds_the_optimiser holds the GPU's fp32 forward of
    # this network to its reference within 2e-3 * max(1, max |reference output|); the same bound here on the 9
    # outputs.  A waypoint's world coordinate is a row of the yaw rotation times two of them plus the position:
    # |cos| + |sin| <= sqrt(2) times the bound; a duration is an output itself (clamping does not widen it).
    eps = 1e-3 * (binit.T_max - binit.T_min)
    for b in range(B):
        ds = ini.DroneState()
        ds.global_pos, ds.global_vel, ds.local_vel = pos[b], vel[b], lvel[b]
        ds.attitude = ini.Quat.from_yaw(yaw[b])
        st = ini.DroneState()
        st.global_pos = np.array([head[b, 0, 0], head[b, 0, 1], 0.0])
        st.global_vel = np.array([head[b, 1, 0], head[b, 1, 1], 0.0])
        _, motion = ini.form_nn_input(np.ones((H, W)), ds, 2.0, st, tail[b, :2])
        with torch.no_grad():
            o = ref_net(torch.from_numpy(ini.process_input_np(want_u8[b], motion))[None])[0].numpy()
        tol = 2e-3 * max(1.0, float(np.abs(o).max()))
        local, ts = ini.split_output(o)
        nn_pl = ini.NNPlanner(des_pos_z=2.0, net=ref_net, device="cpu")
        nn_pl.drone_state = ds
        wp = nn_pl.get_wpts_world(local)[:2]
        ts = np.clip(ts, binit.T_min + eps, binit.T_max - eps)
        err_w, err_t = np.abs(out["int_wpts0"][b] - wp).max(), np.abs(out["ts0"][b] - ts).max()
        print(f"request {b}: warm start off by {err_w:.2e} (waypoints), {err_t:.2e} (durations); bound {tol:.2e}")
        assert err_w <= math.sqrt(2.0) * tol and err_t <= tol

    # the plan: BatchPlanner.plan from the same warm start and seed, bit for bit
    again = bp.plan(m, head, tail, int_wpts=out["int_wpts0"], ts=out["ts0"], seed=5)
    for k in ("x", "costs", "costs_last", "nit", "nfev", "status", "collision", "final_cost", "attempts", "nit_total", "solved"):
        assert np.array_equal(np.asarray(out[k]).view(np.uint8), np.asarray(again[k]).view(np.uint8)), k
