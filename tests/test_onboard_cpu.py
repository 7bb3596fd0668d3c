"""Onboard mapping off the GPU: the NumPy model (tests/onboard_oracle_np.py) against the scenes' true footprints, the
window a scan can touch, the fleet's heading rule and the C ABI's new names."""
import math
import os
import re

import numpy as np
import pytest

import depth_oracle_np as don
import onboard_oracle_np as oon
from neo_planner_amd import _lib, build, synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 64, 48
GRID, RES, ORIGIN = 300, 0.1, (0.0, -15.0)
RANGE, BAND = 6.0, synth.PROJECT_Z_RANGE


def truth_footprint(boxes):
    """cells overlapped by the boxes whose z extent meets the band, dilated 3 x 3"""
    t = np.zeros((GRID, GRID), dtype=bool)
    for lx, ly, lz, hx, hy, hz in boxes:
        if hz < BAND[0] or lz > BAND[1]:
            continue
        x0, x1 = int(math.floor((lx - ORIGIN[0]) / RES)), int(math.floor((hx - ORIGIN[0]) / RES))
        y0, y1 = int(math.floor((ly - ORIGIN[1]) / RES)), int(math.floor((hy - ORIGIN[1]) / RES))
        t[max(y0 - 1, 0):max(y1 + 2, 0), max(x0 - 1, 0):max(x1 + 2, 0)] = True
    return t


_RUNS = {}


def flown(scene):
    """twelve scans of `scene` from eyes (0.5 + 2 k, U(-2, 2), 2.0) with yaw U(-0.6, 0.6), drawn pose by pose from
    default_rng(scene); computed once"""
    if scene in _RUNS:
        return _RUNS[scene]
    boxes = don.boxes_of(synth.forest_boxes(scene), synth.canopy_boxes(scene, 80) if scene == 2 else ())
    u, v = oon.camera_tables(W, H, don.focal_px(W, 87.0))
    half = oon.window_half(u, RANGE, RES)
    rng = np.random.default_rng(scene)
    L = oon.empty(GRID, GRID)
    ever_hit = np.zeros((GRID, GRID), dtype=bool)
    outside_window = 0
    for k in range(12):
        eye = (0.5 + 2 * k, rng.uniform(-2.0, 2.0), 2.0)
        yaw = rng.uniform(-0.6, 0.6)
        depth = don.render(boxes, eye, yaw, W, H)["depth_m"]
        new, occ, _, hit, _ = oon.integrate(L, depth, u, v, np.float32(np.cos(yaw)), np.float32(np.sin(yaw)), eye, RES,
                                            ORIGIN, RANGE, BAND)
        ever_hit |= hit
        rows, cols = np.nonzero(new != L)
        ecx, ecy = math.floor((eye[0] - ORIGIN[0]) / RES), math.floor((eye[1] - ORIGIN[1]) / RES)
        outside_window += int(np.count_nonzero((np.abs(cols - ecx) > half) | (np.abs(rows - ecy) > half)))
        assert np.array_equal(occ, np.where(new == oon.UNKNOWN, -1, np.where(new >= 0, 100, 0)))
        L = new
    _RUNS[scene] = dict(occupied=occ == 100, ever_hit=ever_hit, truth=truth_footprint(boxes), outside_window=outside_window,
                        half=half)
    return _RUNS[scene]


@pytest.mark.parametrize("scene", [0, 1, 2])
def test_occupied_cells_lie_on_the_true_footprint(scene):
    """soundness: no occupied cell outside the truth (the issue's prototype: 0 of 119 / 165 / 317)"""
    r = flown(scene)
    outside = int(np.count_nonzero(r["occupied"] & ~r["truth"]))
    print(f"scene {scene}: {outside} of {int(r['occupied'].sum())} occupied cells outside the true footprint")
    assert r["occupied"].sum() > 100
    assert outside == 0


@pytest.mark.parametrize("scene", [0, 1, 2])
def test_hit_cells_are_rarely_cleared(scene):
    """cells hit in some scan that end not occupied: at most 1 % of the cells ever hit, rounded up"""
    r = flown(scene)
    ever, cleared = int(r["ever_hit"].sum()), int(np.count_nonzero(r["ever_hit"] & ~r["occupied"]))
    print(f"scene {scene}: {cleared} of {ever} cells ever hit end not occupied")
    assert cleared <= math.ceil(ever / 100)


@pytest.mark.parametrize("scene", [0, 1, 2])
def test_a_scan_stays_inside_the_eyes_window(scene):
    """no cell outside (2 half + 1)^2 cells around the eye's cell changes, half = window_half: a point lies d along the
    optical axis and d u across it, so the window reaches sensor_range sqrt(1 + u_max^2), not sensor_range"""
    r = flown(scene)
    assert r["half"] == 84 and r["outside_window"] == 0


def test_window_half_follows_the_field_of_view():
    u, _ = oon.camera_tables(640, 480, don.focal_px(640, 87.0))
    assert oon.window_half(u, 6.0, 0.1) == 84          # 6 m sqrt(1 + tan(43.5 deg)^2) = 8.27 m
    narrow, _ = oon.camera_tables(5, 3, 1.0e6)
    assert oon.window_half(narrow, 6.0, 0.1) == 62     # a pencil of rays: ceil(6 / 0.1) + 1 (+ the slack's cell)
    assert oon.n_samples(6.0, 0.1) == 120 and oon.n_samples(4.0, 0.25) == 32


def test_update_rules():
    """hit wins over passed, both clamp, unmarked cells keep their state, unknown starts from 0"""
    L = np.array([[oon.UNKNOWN, oon.UNKNOWN, 60, -36, 5, -3, oon.UNKNOWN, -8]], dtype=np.int8)
    hit = np.array([1, 0, 1, 0, 1, 0, 0, 1], dtype=bool)
    passed = np.array([1, 1, 0, 1, 1, 1, 0, 0], dtype=bool)
    new, occ, changed = oon.apply_marks(L, hit, passed)
    assert new.tolist() == [[17, -8, 70, -40, 22, -11, oon.UNKNOWN, 9]]
    assert occ.tolist() == [[100, 0, 100, 0, 100, 0, -1, 100]] and changed == 1
    again, _, changed = oon.apply_marks(new, np.zeros(8, bool), np.zeros(8, bool))
    assert np.array_equal(again, new) and changed == 0


def test_nan_depth_marks_nothing():
    u, v = oon.camera_tables(5, 3, don.focal_px(5, 87.0))
    depth = np.full((3, 5), np.nan, dtype=np.float32)
    new, occ, changed, hit, passed = oon.integrate(oon.empty(40, 30), depth, u, v, 1.0, 0.0, (1.0, 1.0, 2.0), 0.1, (0.0, 0.0))
    assert not hit.any() and not passed.any() and changed == 0 and np.all(new == oon.UNKNOWN) and np.all(occ == -1)


def test_heading_rule_matches_arctan2():
    """(cmd[k] - cmd[k-1]) / |.| against cos / sin of the reference's arctan2 (traj_planner_node.py:685-687), to 1e-12;
    the way to the goal where the step has no length"""
    rng = np.random.default_rng(7)
    for _ in range(200):
        step = rng.normal(0.0, 1.0, 2) * 10.0 ** rng.uniform(-6, 1)
        c, s = oon.heading(step, (1.0, 0.0))
        yaw = np.arctan2(step[1], step[0])
        assert abs(c - np.cos(yaw)) <= 1e-12 and abs(s - np.sin(yaw)) <= 1e-12
    c, s = oon.heading((0.0, 0.0), (3.0, -4.0))
    assert (c, s) == (0.6, -0.8)
    assert oon.heading((0.0, 0.0), (0.0, 0.0)) == (1.0, 0.0)
    assert oon.heading((np.nan, 1.0), (0.0, 2.0)) == (0.0, 1.0)


def test_onboard_entry_points_in_the_abi():
    # the family's header recompiles this unit alone
    assert [s for s in build.SOURCES if "neo_onboard.hpp" in build.headers_of(s)] == ["neo_disp_onboard.hip"]
    build.build()
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "neo_planner.h")).read()
    counts = {"neo_onboard_integrate_batch": 24, "neo_onboard_integrate_batch_dev": 24, "neo_esdf_build_2d_batch_dev": 8,
              "neo_fleet_pose_dev": 12}
    for name, count in counts.items():
        assert name in _lib.EXPORTS
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header)
        assert decl, name
        assert len(getattr(lib, name).argtypes) == len(decl.group(1).split(",")) == count, name


def test_mapper_is_exported():
    import neo_planner_amd as npa
    assert "OnboardMapper" in npa.__all__ and npa.OnboardMapper.__name__ == "OnboardMapper"
