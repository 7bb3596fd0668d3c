"""The resident geo warm start, the parts that need no GPU: the pack of the first guess as a NumPy statement, the new
entry points' bindings, BatchGeoPlanner's refusals before any device use, and FleetReplanLoop(mode="geo", geo=...)'s
refusals and plan step."""
import re
import os

import numpy as np
import pytest

from conftest import REPO

import neo_planner_amd as npa
from neo_planner_amd import _lib, build, fleet_geo
from neo_planner_amd.geo_resident import BatchGeoPlanner, pack_guess


class Cfg:
    v_max, init_wpts_num, init_T, T_min, T_max = 1.0, 2, 2.0, 0.1, 10.0


class FakePlanner:
    """what test_fleet_cpu builds: a planner that never reaches a device"""
    cfg, ctx = Cfg(), object()


class Sized:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_the_pack_is_pack_x_of_geo_inits_layout():
    """x0 = [k1.x, k2.x, k1.y, k2.y, tau0, tau1, tau2] is BatchPlanner.pack_x(int_wpts = key_pts[:, 1:3].T, ts = init_T *
    [1.5, 1, 1.5]) -- the arrays geo_init hands to plan -- bit for bit, a no-path row and a NaN row included"""
    bp = npa.BatchPlanner(ctx=object())      # (pack_x, _start_ts and _plan_frac_tau are host arithmetic)
    rng = np.random.default_rng(3)
    key_pts = rng.uniform(-20.0, 40.0, (9, 4, 2))
    key_pts[4] = key_pts[4, 3]              # no path: four equal nodes, the target cell
    key_pts[6] = np.nan                     # a slot outside the table
    B = key_pts.shape[0]
    # geo_init's own two lines
    int_wpts = key_pts[:, 1:3, :].transpose(0, 2, 1).copy()
    ts = np.tile(bp._start_ts(2), (B, 1))
    want = bp.pack_x(int_wpts, ts)
    tau = bp._plan_frac_tau(2)[1]
    got = pack_guess(key_pts, tau)
    assert got.shape == (B, 7) and tau.shape == (3,)
    assert np.array_equal(got.view(np.uint64)[np.isfinite(got)], want.view(np.uint64)[np.isfinite(want)])
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(got[6, :4]).all() and np.isfinite(got[6, 4:]).all()
    assert np.array_equal(got[4, :4], [key_pts[4, 3, 0]] * 2 + [key_pts[4, 3, 1]] * 2)
    # the layout, written out once
    assert np.array_equal(got[0], [key_pts[0, 1, 0], key_pts[0, 2, 0], key_pts[0, 1, 1], key_pts[0, 2, 1], *tau])


def test_the_new_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "neo_planner.h")).read()
    for name in ("neo_geo_guess_dev", "neo_geo_mask_builds"):
        assert re.search(r"^int %s\(neo_ctx \*ctx," % name, header, re.M), name
        assert name in _lib.EXPORTS
    assert "direct" in header
    build.build()
    lib = _lib.load()
    assert len(lib.neo_geo_guess_dev.argtypes) == 17          # bound with a signature, not ctypes' defaults
    assert len(lib.neo_geo_mask_builds.argtypes) == 2
    assert npa.BatchGeoPlanner is BatchGeoPlanner and "BatchGeoPlanner" in npa.__all__


def test_batch_geo_planner_refuses_before_any_device_use():
    torch = pytest.importorskip("torch")
    bp = FakePlanner()          # its context is a plain object: any call on it would raise AttributeError
    g = BatchGeoPlanner(bp)
    assert g.bp is bp and g.direct is None and g.max_expansions == 0
    with pytest.raises(ValueError, match="max_expansions"):
        BatchGeoPlanner(bp, max_expansions=-1)
    here, other = Sized(ctx=bp.ctx, scene_id=1), Sized(ctx=object(), scene_id=1)
    h2 = torch.zeros((5, 3, 2), dtype=torch.float64)
    h3 = torch.zeros((5, 3, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match="2-D"):
        g.warm_start_dev(here, h3, h3)
    with pytest.raises(ValueError, match="2-D"):
        g.plan_dev(here, h3, h3)
    with pytest.raises(ValueError, match="2-D"):
        g.warm_start_dev(here, h2, h2[:4])
    with pytest.raises(ValueError, match="another context"):
        g.warm_start_dev(other, h2, h2)
    with pytest.raises(ValueError, match="float64"):
        g.warm_start_dev(here, h2.float(), h2.float())
    with pytest.raises(ValueError, match="slots"):
        g.warm_start_dev(here, h2, h2, slots=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="subset"):
        g.warm_start_dev(here, h2, h2, subset=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="subset"):
        g.warm_start_dev(here, h2, h2, subset=torch.zeros(6, dtype=torch.int32))
    with pytest.raises(ValueError, match="x0"):
        g.warm_start_dev(here, h2, h2, x0=torch.zeros((5, 6), dtype=torch.float64))
    assert g.x0 is None and g.key_pts is None       # nothing was allocated on the way


def test_the_fleet_takes_geo_and_refuses_what_it_must():
    bp = FakePlanner()
    goals = np.array([[30.0, 0.0], [28.0, 3.0]])
    scenes = (np.zeros((0, 6)), np.zeros(1, np.int32))
    geo = BatchGeoPlanner(bp)
    cases = [
        (dict(mode="basic", geo=geo), "FleetReplanLoop: geo= needs mode 'geo' (the other modes have their own plan steps)"),
        (dict(mode="batch", geo=geo, resident=True), "FleetReplanLoop: geo= needs mode 'geo' (the other modes have their own plan steps)"),
        (dict(mode="geo", geo=object()), "FleetReplanLoop: geo must be a BatchGeoPlanner"),
        (dict(mode="geo", geo=BatchGeoPlanner(FakePlanner())), "FleetReplanLoop: geo's planner must be the loop's batch_planner"),
        # without geo= the two old refusals read as they did
        (dict(mode="geo", resident=True),
         "FleetReplanLoop: resident=True needs mode 'basic' or 'batch' (geo_plan has no resident form)"),
        (dict(mode="geo", onboard=Sized(B=2), scenes=scenes),
         "FleetReplanLoop: onboard maps need mode 'basic' or 'batch' (geo on onboard maps is not built)"),
        # and with it the checks that follow them still run
        (dict(mode="geo", geo=geo, onboard=Sized(B=2)),
         "FleetReplanLoop: onboard and record need scenes=(boxes, box_begin), what the cameras see"),
        (dict(mode="geo", geo=geo, onboard=Sized(B=3), scenes=scenes),
         "FleetReplanLoop: the onboard mapper must have one entry per goal"),
    ]
    for kw, message in cases:
        with pytest.raises(ValueError) as e:
            npa.FleetReplanLoop(bp, None, goals, **kw)
        assert str(e.value) == message, kw
    five = FakePlanner()
    five.cfg = Sized(v_max=1.0, init_wpts_num=4)
    with pytest.raises(ValueError) as e:
        npa.FleetReplanLoop(five, None, goals, mode="geo", geo=BatchGeoPlanner(five))
    assert str(e.value) == "FleetReplanLoop: the geo plan has M = 3 pieces: geo= needs init_wpts_num = 2"
    # accepted, with and without onboard maps; resident plans always
    plain = npa.FleetReplanLoop(bp, None, goals, mode="geo", geo=geo)
    onb = Sized(B=2, scene_ids=np.array([5, 6], np.int32), scene_id=5)
    flown = npa.FleetReplanLoop(bp, None, goals, mode="geo", geo=geo, onboard=onb, scenes=scenes)
    assert plain.geo is geo and plain.resident and flown.resident and flown.plan_map is onb
    assert np.array_equal(flown.plan_scene_ids, onb.scene_ids)
    assert npa.FleetReplanLoop(bp, None, goals, mode="geo", geo=geo, resident=True).resident
    # the plan step: the resident one with geo=, the host form's without
    assert plain._plan_step is fleet_geo.plan_step and flown._plan_step is fleet_geo.plan_step
    assert plain._plan_step.__name__ != "_plan_geo"
    host = npa.FleetReplanLoop(bp, None, goals, mode="geo")
    assert host._plan_step.__name__ == "_plan_geo" and host.geo is None and not host.resident
    assert npa.FleetReplanLoop(bp, None, goals).geo is None
