"""The `batch` planner mode for B requests (BatchPlanner.batch_plan, neo_batch_*), the parts that need no GPU: the NumPy
form of the candidates against the reference-shaped planner's, the C ABI's declarations and exports, the fleet's new
mode, and the two facts about NumPy's arithmetic that the kernels in neo_batch.hpp restate."""
import inspect
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from conftest import REPO

import neo_planner_amd as npa
from neo_planner_amd import _lib, build

ENTRY_POINTS = ("neo_batch_candidates", "neo_batch_candidates_dev", "neo_batch_select", "neo_batch_select_dev")


def _requests(rng, B):
    start = np.stack([rng.uniform(0.0, 25.0, B), rng.uniform(-10.0, 10.0, B)], 1)
    th = rng.uniform(-np.pi, np.pi, B)
    d = np.stack([np.cos(th), np.sin(th)], 1)
    head = np.zeros((B, 3, 2)); tail = np.zeros((B, 3, 2))
    head[:, 0], head[:, 1] = start, 0.5 * d
    tail[:, 0], tail[:, 1] = start + rng.uniform(0.5, 9.0, B)[:, None] * d, 0.8 * d
    # axis-parallel requests: linspace's step is 0 in one dimension and its other branch is taken for both
    tail[1, 0] = head[1, 0] + [4.0, 0.0]
    tail[2, 0] = head[2, 0] + [0.0, -3.5]
    tail[3, 0] = head[3, 0]                       # start == target
    return head, tail


@pytest.mark.parametrize("count", [2, 3, 5])
def test_batch_init_guess_is_the_reference_shaped_planners_request_by_request(count):
    head, tail = _requests(np.random.default_rng(count), 64)
    cfg = npa.PlannerConfig(init_wpts_num=count)
    bp = npa.BatchPlanner(cfg)
    mj = npa.MinJerkPlanner(cfg)
    wp, ts = bp.batch_init_guess(head, tail)
    assert wp.shape == (64, 3, 2, count) and ts.shape == (count + 1,)
    for b in range(64):
        with np.errstate(invalid="ignore", divide="ignore"):
            ref_wp, ref_ts = mj.batch_generate_init_variables(head[b, :2], tail[b, :2])
        assert np.array_equal(wp[b], ref_wp, equal_nan=True), b
        assert np.array_equal(ts, ref_ts)
    # start == target: candidate 0 finite, the shifted candidates NaN, as in the reference
    assert np.isfinite(wp[3, 0]).all() and np.isnan(wp[3, 1:]).all()
    assert np.isfinite(np.delete(wp, 3, axis=0)).all()
    # more candidates alternate the side at the same distance; explicit offsets; candidate 0 does not depend on K
    wp5, _ = bp.batch_init_guess(head, tail, K=5)
    assert np.array_equal(wp5[:, :3], wp, equal_nan=True)
    assert np.array_equal(wp5[:, 3], wp[:, 1], equal_nan=True) and np.array_equal(wp5[:, 4], wp[:, 2], equal_nan=True)
    wp2, _ = bp.batch_init_guess(head, tail, lateral_offsets=[0.0, -0.6])
    assert np.array_equal(wp2[:, 1], wp[:, 2], equal_nan=True)
    assert np.array_equal(bp.batch_init_guess(head, tail, K=1)[0][:, 0], wp[:, 0])


def test_batch_argument_errors_need_no_gpu():
    bp = npa.BatchPlanner()
    head, tail = _requests(np.random.default_rng(0), 8)
    for kw in (dict(K=0), dict(K=9), dict(K=3, lateral_offsets=[0.0, 0.6]), dict(lateral_offsets=np.zeros(9))):
        with pytest.raises(ValueError):
            bp.batch_init_guess(head, tail, **kw)
        with pytest.raises(ValueError):
            bp.batch_plan(None, head, tail, **kw)
    with pytest.raises(ValueError):
        bp.batch_init_guess(np.zeros((4, 3, 3)), np.zeros((4, 3, 3)))
    with pytest.raises(ValueError):
        bp.batch_plan(None, np.zeros((4, 3, 3)), np.zeros((4, 3, 3)))
    with pytest.raises(ValueError):
        bp.batch_plan(None, head, tail, stream_ids=np.arange(7))
    out = bp.batch_plan(None, np.zeros((0, 3, 2)), np.zeros((0, 3, 2)))     # B = 0: empty arrays, nothing launched
    assert out["x"].shape == (0, 7) and out["candidate_cost"].shape == (0, 3) and out["chosen"].shape == (0,)
    assert set(out) >= {"x", "costs", "costs_last", "nit", "nfev", "status", "collision", "chosen", "candidate_cost",
                        "final_cost", "nit_total", "attempts", "solved"}


def test_header_declares_and_library_exports_the_batch_entry_points():
    header = open(os.path.join(REPO, "include", "neo_planner.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"^int %s\(neo_ctx \*ctx, int B, const int32_t \*subset, int n_subset, int M, int D, int K," % name,
                         header, re.M), name
        assert name in _lib.EXPORTS
    assert re.search(r"^#define NEO_BATCH_MAX_CANDIDATES 8\b", header, re.M) and _lib.NEO_BATCH_MAX_CANDIDATES == 8
    assert re.search(r"^#define NEO_ABI_VERSION 1\b", header, re.M)
    # each family's header recompiles its unit alone
    assert [s for s in build.SOURCES if "neo_batch.hpp" in build.headers_of(s)] == ["neo_disp_batch.hip"]
    assert [s for s in build.SOURCES if "neo_esdf.hpp" in build.headers_of(s)] == ["neo_disp_esdf.hip"]
    build.build()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert getattr(lib, name).argtypes, name     # bound with a signature, not called through ctypes' defaults
    assert len(lib.neo_batch_candidates_dev.argtypes) == 16 and len(lib.neo_batch_select_dev.argtypes) == 27


def test_fleet_accepts_mode_batch():
    class Cfg:
        v_max, init_wpts_num = 1.0, 2

    class FakePlanner:
        cfg = Cfg()
    goals = np.array([[30.0, 0.0], [28.0, 3.0]])
    loop = npa.FleetReplanLoop(FakePlanner(), None, goals, mode="batch")
    assert loop.mode == "batch"
    for mode in ("basic", "geo"):
        assert npa.FleetReplanLoop(FakePlanner(), None, goals, mode=mode).mode == mode
    with pytest.raises(ValueError):
        npa.FleetReplanLoop(FakePlanner(), None, goals, mode="nn")
    p = inspect.signature(npa.BatchPlanner.batch_plan).parameters
    assert [p[k].default for k in ("K", "lateral_offsets", "scene_ids", "seed", "stream_ids", "max_attempts")] == \
        [None, None, None, None, None, 5]


def test_numpy_sums_four_products_from_left_to_right():
    """batch_select_kernel's cost: (costs_last * w).sum() is ((p0 + p1) + p2) + p3, as one row and along an axis"""
    rng = np.random.default_rng(7)
    c = rng.random((20000, 4)) * rng.choice([1e-3, 1.0, 1e3, 1e6], (20000, 4))
    w = rng.random(4) * np.array([1.0, 1.0, 1.0, 1e4])
    p = c * w
    left = ((p[:, 0] + p[:, 1]) + p[:, 2]) + p[:, 3]
    assert np.array_equal(p.sum(axis=1), left)
    assert np.array_equal(np.array([(c[i] * w).sum() for i in range(2000)]), left[:2000])
    assert not np.array_equal((p[:, 0] + p[:, 1]) + (p[:, 2] + p[:, 3]), left)      # the inputs tell the orders apart


def test_numpy_norm_of_a_2_vector_fuses_the_second_square():
    """batch_candidates_kernel's direction: np.linalg.norm([dx, dy]) is sqrt(fma(dy, dy, round(dx * dx))) -- BLAS ddot
    accumulates with a fused multiply-add"""
    rng = np.random.default_rng(8)
    v = rng.normal(0.0, 5.0, (3000, 2))
    got = np.array([np.linalg.norm(a) for a in v])
    fused = np.array([np.sqrt(float(Fraction(y) * Fraction(y) + Fraction(x * x))) for x, y in v])
    assert np.array_equal(got, fused)
    assert not np.array_equal(np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]), fused)  # the inputs tell the two apart
