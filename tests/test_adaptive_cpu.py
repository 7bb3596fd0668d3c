"""Adaptive waypoint counts without a GPU: BatchPlanner.adaptive_counts (the definition adaptive_count_kernel restates)
against the reference's recorded adaptive cases (tests/golden/g4_init.npz), against
MinJerkPlanner(init_wpts_mode='adaptive').generate_init_variables and on the lattice and edge cases; the argument errors
of adaptive_counts, plan, plan_dev and plan_buffers, raised before any device use; adaptive_groups on a hand-made ragged
dict; the entry points in the header and the library."""
import math
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, REPO

import neo_planner_amd as npa
from neo_planner_amd import _lib, build


def _requests(start, target):
    """head / tail (B, 3, D) from positions (B, D)"""
    start, target = np.asarray(start, dtype=np.float64), np.asarray(target, dtype=np.float64)
    head = np.zeros((start.shape[0], 3, start.shape[1])); tail = np.zeros_like(head)
    head[:, 0], tail[:, 0] = start, target
    return head, tail


def _from_origin(targets):
    targets = np.asarray(targets, dtype=np.float64)
    return _requests(np.zeros_like(targets), targets)


def _adaptive(seg=2.0):
    return npa.BatchPlanner(npa.PlannerConfig(init_wpts_mode="adaptive", init_seg_len=seg))


# ------------------------------------------------------------------ the count
def test_counts_of_the_references_recorded_adaptive_cases():
    g = np.load(os.path.join(GOLDEN, "g4_init.npz"))
    cases = [i for i in range(int(g["n_cases"])) if str(g["c%d_mode" % i]) == "adaptive"]
    assert len(cases) == 2
    head = np.stack([g["c%d_head" % i] for i in cases]); tail = np.stack([g["c%d_tail" % i] for i in cases])
    counts, clamped = _adaptive().adaptive_counts(head, tail)
    assert counts.dtype == np.int32 and clamped.dtype == np.bool_
    assert counts.tolist() == [g["c%d_wpts" % i].shape[1] for i in cases] == [4, 1] and not clamped.any()


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("seg", [2.0, 0.5, 3.0])
def test_counts_equal_generate_init_variables(D, seg):
    rng = np.random.default_rng([7, D])
    r = 9.0 * seg                                                    # (the longest diagonal stays below 63 waypoints)
    start, target = rng.uniform(-r, r, (2000, D)), rng.uniform(-r, r, (2000, D))
    target[:50] = start[:50] + rng.integers(-6, 7, (50, D))          # lengths on and next to the lattice
    head, tail = _requests(start, target)
    counts, clamped = _adaptive(seg).adaptive_counts(head, tail)
    one = npa.MinJerkPlanner(npa.PlannerConfig(init_wpts_mode="adaptive", init_seg_len=seg))
    ref = np.array([one.generate_init_variables(head[i], tail[i])[1].shape[0] - 1 for i in range(2000)])
    assert ref.max() <= 63 and len(set(ref.tolist())) >= 8
    assert np.array_equal(counts, ref) and not clamped.any()


def test_lattice_and_edge_cases():
    bp = _adaptive()
    counts, clamped = bp.adaptive_counts(*_from_origin([(4, 0), (3, 4), (6, 8), (0, 0)]))
    assert counts.tolist() == [1, 2, 4, 1] and not clamped.any()
    up = np.nextafter(4.0, 5.0)
    counts, clamped = bp.adaptive_counts(*_from_origin([(4, 0), (up, 0), (0, up), (np.nan, 1.0), (np.inf, 0.0), (1e200, 1e200)]))
    assert counts.tolist() == [1, 2, 2, 1, 1, 1] and not clamped.any()        # (1e200 squared is inf: L is not finite)
    counts, clamped = bp.adaptive_counts(*_from_origin([(128.0, 0), (127.9, 0), (130.0, 0), (1e6, 0), (1e150, 0)]))
    assert counts.tolist() == [63, 63, 63, 63, 63] and clamped.tolist() == [False, False, True, True, True]
    counts, clamped = bp.adaptive_counts(*_from_origin([(2.0, 0), (9.0, 0), (8.0, 0), (8.1, 0)]), max_waypoints=3)
    assert counts.tolist() == [1, 3, 3, 3] and clamped.tolist() == [False, True, False, True]
    for seg, want in ((0.5, [7, 9, 19, 1, 63]), (3.0, [1, 1, 3, 1, 63])):
        counts, clamped = _adaptive(seg).adaptive_counts(*_from_origin([(4, 0), (3, 4), (6, 8), (0, 0), (500.0, 0)]))
        assert counts.tolist() == want and clamped.tolist() == [False] * 4 + [True], seg
    counts, _ = bp.adaptive_counts(*_from_origin([(2, 3, 6), (0, 0, 0), (0, 0, 4.0), (0, 0, up)]))   # D = 3: |(2, 3, 6)| = 7
    assert counts.tolist() == [3, 1, 1, 2]
    assert max(math.ceil(7.0 / 2.0 - 1), 1) == 3


# ------------------------------------------------------------------ argument errors, without a device
class _NoDevice:
    """stands where a map or a context would: any use is a failure"""

    def __getattr__(self, name):
        raise AssertionError("the device was used (%s)" % name)


def test_argument_errors_are_raised_without_a_device():
    import torch
    head, tail = _from_origin([(4, 0), (3, 4), (6, 8)])
    bp = npa.BatchPlanner(ctx=_NoDevice())
    m = _NoDevice()
    for w in (0, 64, -1, 2.5):
        with pytest.raises(ValueError):
            bp.adaptive_counts(head, tail, max_waypoints=w)
        with pytest.raises(ValueError):
            bp.plan(m, head, tail, waypoints="adaptive", max_waypoints=w)
        with pytest.raises(ValueError):
            bp.plan_buffers(3, "cpu", waypoints="adaptive", max_waypoints=w)
    for seg in (0.0, -2.0, math.inf, math.nan):
        bad = npa.BatchPlanner(npa.PlannerConfig(init_seg_len=seg), ctx=_NoDevice())
        with pytest.raises(ValueError):
            bad.adaptive_counts(head, tail)
        with pytest.raises(ValueError):
            bad.plan(m, head, tail, waypoints="adaptive")
    with pytest.raises(ValueError):
        bp.adaptive_counts(np.zeros((3, 3, 4)), np.zeros((3, 3, 4)))
    wp, ts = bp.init_guess(head, tail, 2)
    for kw in (dict(int_wpts=wp, ts=ts), dict(int_wpts=wp), dict(ts=ts), dict(jitter="philox"), dict(stream_ids=[1, 2])):
        with pytest.raises(ValueError):
            bp.plan(m, head, tail, waypoints="adaptive", **kw)
    with pytest.raises(ValueError):
        bp.plan(m, head, tail, waypoints="adaptiv")
    with pytest.raises(ValueError):
        bp.plan_buffers(3, "cpu", waypoints="longest")
    # plan_dev
    d_head, d_tail = torch.from_numpy(head), torch.from_numpy(tail)
    fixed = bp.plan_buffers(3, "cpu", D=2, waypoints=63)
    made = bp.plan_buffers(3, "cpu", D=2, waypoints="adaptive", max_waypoints=5)
    for kw in (dict(x0=torch.zeros((3, 7), dtype=torch.float64)), dict(max_waypoints=0), dict(max_waypoints=64),
               dict(max_attempts=0), dict(jitter="philox"), dict(stream_ids=np.arange(2)), dict(bufs=fixed), dict(bufs=made),
               dict(bufs=made, max_waypoints=4), dict(x=torch.zeros((3, 7), dtype=torch.float64), max_waypoints=5, bufs=made)):
        with pytest.raises(ValueError):
            bp.plan_dev(m, d_head, d_tail, waypoints="adaptive", **kw)
    with pytest.raises(ValueError):
        bp.plan_dev(m, d_head, d_tail, waypoints="adaptiv")


def test_adaptive_buffers():
    bp = npa.BatchPlanner(ctx=_NoDevice())
    b = bp.plan_buffers(10, "cpu", D=3, waypoints="adaptive", max_waypoints=7)
    n_max = 3 * 7 + 7 + 1
    assert b["adaptive"] and b["max_waypoints"] == 7 and b["M"] == 8 and b["D"] == 3
    assert tuple(b["x"].shape) == (10, n_max) and tuple(b["x_k"].shape) == (10, n_max) and tuple(b["noise"].shape) == (10, 3, 7)
    assert tuple(b["counts"].shape) == tuple(b["clamped"].shape) == tuple(b["group_order"].shape) == (10,)
    assert b["table"].numel() == 2 * _lib.NEO_MAX_PIECES + 3 and tuple(b["todo"].shape) == (2, 10)
    plain = bp.plan_buffers(10, "cpu", D=3, waypoints=7)                # the fixed form is what it was
    assert "adaptive" not in plain and tuple(plain["counts"].shape) == (2,) and tuple(plain["x"].shape) == (10, n_max)


# ------------------------------------------------------------------ the ragged result, group by group
def test_adaptive_groups_round_trip():
    rng = np.random.default_rng(3)
    for D, W in ((2, 6), (3, 4)):
        counts = np.array([3, 1, W, 3, 2, 1, 3], dtype=np.int32)
        n_max = D * W + W + 1
        x = np.full((7, n_max), np.nan)
        rows = {}
        for b, c in enumerate(counts):
            rows[b] = rng.normal(size=D * c + c + 1)
            x[b, :rows[b].size] = rows[b]
        result = dict(x=x, counts=counts, max_waypoints=W)
        groups = list(npa.BatchPlanner.adaptive_groups(result))
        assert [g[0] for g in groups] == sorted(set(counts.tolist()))
        seen = []
        for c, idx, dense in groups:
            assert dense.shape == (idx.size, D * c + c + 1) and dense.flags["C_CONTIGUOUS"] and np.isfinite(dense).all()
            assert np.all(counts[idx] == c) and np.all(np.diff(idx) > 0)
            for k, b in enumerate(idx):
                assert np.array_equal(dense[k], rows[int(b)])
            seen += idx.tolist()
        assert sorted(seen) == list(range(7))
        # over a subset: the rows outside may hold anything
        counts2 = counts.copy(); counts2[[0, 5]] = -9
        sub = list(npa.BatchPlanner.adaptive_groups(dict(result, counts=counts2), rows=[6, 1, 2, 3, 4]))
        assert sorted(sum((g[1].tolist() for g in sub), [])) == [1, 2, 3, 4, 6]
        with pytest.raises(ValueError):
            list(npa.BatchPlanner.adaptive_groups(dict(result, counts=counts2)))
        import torch
        as_torch = list(npa.BatchPlanner.adaptive_groups(dict(x=torch.from_numpy(x), counts=torch.from_numpy(counts), max_waypoints=W)))
        assert all(a[0] == g[0] and np.array_equal(a[1], g[1]) and np.array_equal(a[2], g[2]) for a, g in zip(as_torch, groups))


# ------------------------------------------------------------------ header and exports
NEW = {"neo_adaptive_count": 11, "neo_adaptive_count_dev": 11, "neo_adaptive_bucket": 8, "neo_adaptive_bucket_dev": 8,
       "neo_adaptive_merge_dev": 26, "neo_adaptive_compact": 6, "neo_adaptive_compact_dev": 5}


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(REPO, "include", "neo_planner.h")).read()
    build.build()
    lib = _lib.load()
    for name, nargs in NEW.items():
        m = re.search(r"\bint %s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        assert name in _lib.EXPORTS
        assert len(getattr(lib, name).argtypes) == nargs, name
    # the family's header recompiles this unit alone
    assert [s for s in build.SOURCES if "neo_adaptive.hpp" in build.headers_of(s)] == ["neo_disp_adaptive.hip"]
    assert int(re.search(r"#define NEO_MAX_PIECES (\d+)", header).group(1)) == _lib.NEO_MAX_PIECES
    # the existing neighbours keep their signatures
    assert len(lib.neo_plan_guess_dev.argtypes) == 17 and len(lib.neo_plan_merge_dev.argtypes) == 25
