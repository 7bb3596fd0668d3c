"""The resident form of BatchPlanner.plan (plan_dev, neo_plan_*), the parts that need no GPU: the C ABI's declarations
and exports, the argument errors raised before any device use, the host values the guess kernel is handed, and the
NumPy restatement of one attempt's merge (used by tests/test_gpu_plan_dev.py) against `plan`'s own bookkeeping."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO

import neo_planner_amd as npa
from neo_planner_amd import _lib, build

ENTRY_POINTS = ("neo_plan_guess", "neo_plan_guess_dev", "neo_plan_merge", "neo_plan_merge_dev")
MERGED = ("x", "costs4", "costs4_last", "nit", "nfev", "status", "attempts", "nit_total", "solved")


def merge_restated(B, sub, reset, xk, ck, lk, nit, nfev, st, init):
    """one attempt's neo_plan_merge over packed results, with NumPy: (request-indexed arrays, failed list, bad-scene word)"""
    out = {k: v.copy() for k, v in init.items()}
    failed_list, bad = [], 0
    for p, b in enumerate(sub):
        if not 0 <= b < B:
            continue
        code = int(st[p]) & 0xff
        failed = (code > _lib.NEO_TRAJ_MAXITER and code != _lib.NEO_TRAJ_BAD_SCENE) or bool(st[p] & _lib.NEO_TRAJ_FLAG_COLLISION)
        counted = 0 if code >= _lib.NEO_TRAJ_NUMERIC_RANGE else int(nit[p])
        out["x"][b], out["costs4"][b], out["costs4_last"][b] = xk[p], ck[p], lk[p]
        out["nit"][b], out["nfev"][b], out["status"][b] = nit[p], nfev[p], st[p]
        out["attempts"][b] = 1 if reset else out["attempts"][b] + 1
        out["nit_total"][b] = counted if reset else out["nit_total"][b] + counted
        out["solved"][b] = 0 if failed else 1
        if failed:
            failed_list.append(b)
        bad |= code == _lib.NEO_TRAJ_BAD_SCENE
    return out, np.array(failed_list, np.int32), int(bad)


def test_header_declares_and_library_exports_the_plan_entry_points():
    header = open(os.path.join(REPO, "include", "neo_planner.h")).read()
    counts = {}
    for name in ENTRY_POINTS:
        m = re.search(r"^int %s\(neo_ctx \*ctx, int B, const int32_t \*subset, int n_subset, int M, int D,([^;]*)\);" % name,
                      header, re.M)
        assert m, name
        counts[name] = 6 + m.group(1).count(",") + 1
        assert name in _lib.EXPORTS
    # the family's header recompiles this unit alone
    assert [s for s in build.SOURCES if "neo_plan.hpp" in build.headers_of(s)] == ["neo_disp_plan.hip"]
    assert os.path.exists(os.path.join(build.CSRC, "neo_plan.hpp"))
    build.build()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert len(getattr(lib, name).argtypes) == counts[name], name      # bound with the header's argument count
    assert counts["neo_plan_guess"] == counts["neo_plan_guess_dev"] == 17
    assert counts["neo_plan_merge"] == counts["neo_plan_merge_dev"] == 25


def test_plan_dev_and_the_resident_fleet_raise_their_argument_errors_without_a_device():
    bp = npa.BatchPlanner()
    head = np.zeros((4, 3, 2)); tail = np.ones((4, 3, 2))
    for kw in (dict(stream_ids=np.arange(3)), dict(x0=np.zeros((4, 8))), dict(x0=np.zeros((3, 7))),
               dict(x0=np.zeros((4, 7)), waypoints=3), dict(max_attempts=0), dict(bufs=dict(B=3, D=2, M=3)),
               dict(bufs=dict(B=4, D=3, M=3)), dict(bufs=dict(B=4, D=2, M=4))):
        with pytest.raises(ValueError):
            bp.plan_dev(None, head, tail, **kw)
    with pytest.raises(ValueError):
        bp.plan_dev(None, head, np.ones((4, 3, 3)))
    with pytest.raises(ValueError):
        bp.plan_dev(None, np.zeros((4, 2, 2)), np.zeros((4, 2, 2)))
    p = inspect.signature(npa.BatchPlanner.plan_dev).parameters
    names = ("bufs", "x0", "slots", "subset", "x", "solved", "max_attempts", "seed", "rng", "stream_ids", "waypoints")
    assert [p[k].default for k in names] == [None, None, None, None, None, None, 5, None, None, None, None]
    assert list(inspect.signature(npa.BatchPlanner.plan_buffers).parameters)[:3] == ["self", "B", "device"]

    class Cfg:
        v_max, init_wpts_num = 1.0, 2

    class FakePlanner:
        cfg = Cfg()
    goals = np.array([[30.0, 0.0], [28.0, 3.0]])
    with pytest.raises(ValueError):
        npa.FleetReplanLoop(FakePlanner(), None, goals, mode="geo", resident=True)
    for mode in ("basic", "batch"):
        assert npa.FleetReplanLoop(FakePlanner(), None, goals, mode=mode, resident=True).resident is True
    for mode in ("basic", "geo", "batch"):
        assert npa.FleetReplanLoop(FakePlanner(), None, goals, mode=mode).resident is False


@pytest.mark.parametrize("count", [2, 3, 5])
def test_the_host_values_of_the_guess_are_init_guess_and_pack_x_bit_for_bit(count):
    """the guess kernel is handed f[k] and tau by the host: start + (target - start) * f, each operation rounded on its own,
    and a tau that does not depend on how many rows pack_x is given at once"""
    rng = np.random.default_rng(count)
    bp = npa.BatchPlanner(npa.PlannerConfig(init_wpts_num=count, T_min=0.4, init_T=2.3))
    frac, tau = bp._plan_frac_tau(count)
    for B, D in ((1, 2), (7, 3), (48, 2), (4099, 3)):
        head = rng.normal(0, 9, (B, 3, D)); tail = rng.normal(0, 9, (B, 3, D))
        wp, ts = bp.init_guess(head, tail, count)
        x = bp.pack_x(wp, ts)
        assert np.array_equal(x[:, D * count:], np.broadcast_to(tau, (B, count + 1)))
        along = (tail[:, 0] - head[:, 0])[:, :, None] * frac
        assert np.array_equal(x[:, :D * count], (head[:, 0][:, :, None] + along).reshape(B, -1))


def test_the_merge_restatement_is_plans_bookkeeping_on_every_status():
    """every status code 0 .. 7, with and without the collision flag: `plan`'s own `counted` and `failed` lambdas, run the
    way plan runs them over an attempt's dict, against the restatement the GPU test compares the kernel with"""
    codes = np.repeat(np.arange(8), 2).astype(np.int32)
    flag = np.tile([0, _lib.NEO_TRAJ_FLAG_COLLISION], 8).astype(np.int32)
    st = codes | flag
    P = len(st)
    nit = (np.arange(P) * 7 + 3).astype(np.int32)
    r = dict(status=st & 0xff, collision=(st & _lib.NEO_TRAJ_FLAG_COLLISION) != 0, nit=nit)
    # (the two lambdas of BatchPlanner.plan, as its source has them)
    src = inspect.getsource(npa.BatchPlanner.plan)
    assert 'counted = lambda r: np.where(r["status"] >= _lib.NEO_TRAJ_NUMERIC_RANGE, 0, r["nit"]).astype(np.int64)' in src
    assert ('failed = lambda r: ((r["status"] > _lib.NEO_TRAJ_MAXITER) & (r["status"] != _lib.NEO_TRAJ_BAD_SCENE)) | '
            'r["collision"]') in src
    counted = np.where(r["status"] >= _lib.NEO_TRAJ_NUMERIC_RANGE, 0, r["nit"]).astype(np.int64)
    failed = ((r["status"] > _lib.NEO_TRAJ_MAXITER) & (r["status"] != _lib.NEO_TRAJ_BAD_SCENE)) | r["collision"]
    n = 5
    init = dict(x=np.zeros((P, n)), costs4=np.zeros((P, 4)), costs4_last=np.zeros((P, 4)), nit=np.zeros(P, np.int32),
                nfev=np.zeros(P, np.int32), status=np.zeros(P, np.int32), attempts=np.full(P, 2, np.int32),
                nit_total=np.full(P, 1000, np.int64), solved=np.full(P, -1, np.int32))
    xk = np.arange(P * n, dtype=np.float64).reshape(P, n); ck = xk[:, :4] + 0.5; lk = xk[:, :4] + 0.25
    nfev = nit + 1
    sub = np.arange(P, dtype=np.int32)
    out, lst, bad = merge_restated(P, sub, 0, xk, ck, lk, nit, nfev, st, init)
    assert np.array_equal(out["nit_total"], 1000 + counted) and np.array_equal(out["attempts"], np.full(P, 3))
    assert np.array_equal(out["solved"] == 0, failed) and np.array_equal(lst, np.flatnonzero(failed)) and bad == 1
    assert np.array_equal(out["x"], xk) and np.array_equal(out["status"], st) and np.array_equal(out["nfev"], nfev)
    # what the table has to tell apart: answers kept (0 .. 3), overflows (4, 5, 7) retried and not counted, a bad scene (6)
    # neither retried nor counted, and the collision flag failing whatever the code
    assert failed.tolist() == [False, True] * 4 + [True, True] * 2 + [False, True] + [True, True]
    assert (counted == 0).tolist() == [False] * 8 + [True] * 8
    first, lst1, bad1 = merge_restated(P, sub[:12], 1, xk, ck, lk, nit, nfev, st, init)
    assert np.array_equal(first["attempts"][:12], np.ones(12)) and np.array_equal(first["nit_total"][:12], counted[:12])
    assert np.array_equal(first["attempts"][12:], init["attempts"][12:]) and bad1 == 0 and np.array_equal(lst1, lst[lst < 12])
