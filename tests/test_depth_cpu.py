"""The depth camera off the GPU: the NumPy float32 restatement of its arithmetic (tests/depth_oracle_np.py) against the
float64 definition initializer.raycast_depth, the batched input glue against form_nn_input, and the C ABI's new names."""
import math
import os
import re

import numpy as np
import pytest

import depth_oracle_np as don
from neo_planner_amd import _lib, build, synth
from neo_planner_amd import initializer as ini

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _poses(scene, count):
    """eye x in [0.5, 20], y in [-4, 4], z = 2, yaw in [-1, 1]"""
    rng = np.random.default_rng(500 + scene)
    return [((rng.uniform(0.5, 20.0), rng.uniform(-4.0, 4.0), 2.0), rng.uniform(-1.0, 1.0)) for _ in range(count)]


def _differing(scene, eye, yaw, w, h):
    pillars, canopy = synth.forest_boxes(scene), synth.canopy_boxes(scene, 80)
    want = ini.raycast_depth(pillars, canopy, eye=eye, yaw=yaw, height=h, width=w)
    got = don.render(don.boxes_of(pillars, canopy), eye, yaw, w, h)["depth_u8"]
    assert got.shape == want.shape and got.dtype == np.uint8
    return int(np.count_nonzero(got != want)), want.size


def test_restatement_matches_raycast_depth_small_images():
    """scenes 0..3 with 80 canopy boxes, three poses each, 61 x 37 and 64 x 48: pixels that differ at all <= 1 in
    100 000 of the set's pixels, rounded up (room for a silhouette ray within fp32 rounding of an edge)"""
    diff = total = 0
    for scene in range(4):
        for eye, yaw in _poses(scene, 3):
            for w, h in ((61, 37), (64, 48)):
                d, n = _differing(scene, eye, yaw, w, h)
                diff += d
                total += n
    print(f"restatement vs raycast_depth, small images: {diff} of {total} pixels differ")
    assert diff <= math.ceil(total / 100000)


def test_restatement_matches_raycast_depth_full_size():
    """two 640 x 480 images, the same condition"""
    diff = total = 0
    for scene in (0, 3):
        eye, yaw = _poses(scene, 1)[0]
        d, n = _differing(scene, eye, yaw, 640, 480)
        diff += d
        total += n
    print(f"restatement vs raycast_depth, 640 x 480: {diff} of {total} pixels differ")
    assert diff <= math.ceil(total / 100000)


def test_boxes_of_forms_raycast_depths_rows():
    from neo_planner_amd.depth import DepthCamera
    pillars, canopy = synth.forest_boxes(1), synth.canopy_boxes(1, 5)
    rows = DepthCamera.boxes_of(pillars, canopy)
    assert rows.shape == (len(pillars) + 5, 6) and np.array_equal(rows, don.boxes_of(pillars, canopy))
    cx, cy, sx, sy, sz = pillars[0]
    assert tuple(rows[0]) == (cx - sx / 2, cy - sy / 2, 0.0, cx + sx / 2, cy + sy / 2, sz)
    boxes, begin = DepthCamera.pack_scenes([(pillars, canopy), np.zeros((0, 6)), rows[:3]])
    assert begin.tolist() == [0, len(rows), len(rows), len(rows) + 3] and boxes.shape == (len(rows) + 3, 6)
    cam = DepthCamera(width=64, height=48)
    assert cam.focal_px == (64 / 2) / np.tan(np.radians(87.0) / 2)


def test_form_nn_input_batch_matches_form_nn_input():
    """7 requests with distinct yaws, within 1e-12 absolute: three products and two sums in fp64 of values below 60 m,
    summed in a different order, stay under 1e-13"""
    rng = np.random.default_rng(11)
    B = 7
    yaw = np.linspace(-2.8, 2.9, B)
    pos = np.concatenate([rng.uniform(-20, 20, (B, 2)), rng.uniform(1, 3, (B, 1))], axis=1)
    vel = rng.uniform(-1, 1, (B, 3))
    lvel = rng.uniform(-1, 1, (B, 3))
    start = np.stack([pos[:, :2] + rng.uniform(-0.5, 0.5, (B, 2)), rng.uniform(-1, 1, (B, 2))], axis=1)
    target = np.stack([pos[:, :2] + rng.uniform(-8, 8, (B, 2)), rng.uniform(-1, 1, (B, 2))], axis=1)
    motion, R, gp = ini.form_nn_input_batch(pos, vel, lvel, yaw, 2.0, start, target)
    assert motion.shape == (B, 24) and R.shape == (B, 3, 3) and gp.shape == (B, 3)
    depth = np.linspace(0.5, 9.0, 12).reshape(3, 4)
    for b in range(B):
        ds = ini.DroneState()
        ds.global_pos, ds.global_vel, ds.local_vel = pos[b], vel[b], lvel[b]
        ds.attitude = ini.Quat.from_yaw(yaw[b])
        st = ini.DroneState()
        st.global_pos = np.array([start[b, 0, 0], start[b, 0, 1], 0.0])
        st.global_vel = np.array([start[b, 1, 0], start[b, 1, 1], 0.0])
        _, want = ini.form_nn_input(depth, ds, 2.0, st, target[b])
        assert np.max(np.abs(motion[b] - want)) <= 1e-12
        assert np.max(np.abs(R[b] - ds.attitude.rotation_matrix)) <= 1e-12
        assert np.array_equal(gp[b], pos[b])


def test_depth_entry_points_in_the_abi():
    build.build()
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "neo_planner.h")).read()
    for name in ("neo_depth_render_batch", "neo_depth_render_batch_dev"):
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header)
        assert decl, name
        assert len(fn.argtypes) == len(decl.group(1).split(",")) == 14
    m = re.search(r"#define\s+NEO_DEPTH_MAX_BOXES\s+(\d+)", header)
    assert m and int(m.group(1)) == _lib.NEO_DEPTH_MAX_BOXES
    assert re.search(r"#define\s+NEO_ABI_VERSION\s+1\b", header) and lib.neo_abi_version() == 1
