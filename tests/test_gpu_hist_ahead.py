"""
Once the L-BFGS memory is full (col = m = 10), the search direction of the all-fp32 optimiser kernel under its fixed launch
plan runs the two-loop recursion written out step by step: every (s, y) pair is read from LDS once, one step ahead of its
use in loop 1, and loop 2 works on the registers (csrc/neo_kernels.hpp DevBackend::direction_full, Plan::hist_ahead; the
control flow: csrc/neo_lbfgs_dir.hpp hist_walk_full, tests/test_hist_schedule_cpu.py).  Same pairs, same order, same
expressions, so the run must equal, bit for bit, the same launch through optimize_dyn_kernel -- reached through a trace
buffer, as in tests/test_gpu_gather_ahead.py, whose helpers are imported -- and, in the brick layout (budgeted launches
take no yz4 field), a budgeted run of the same requests (the budgeted members are compiled for the dynamic plan too): x,
both sets of cost terms, iteration and evaluation counts, status and the collision flag, all 96 runs of every case.
neo_optimize_plan_launches shows which kernel served each launch.

Shapes: a 48^3 synthetic field in the brick and the yz4 layout, B = 96 requests a case.
  M = 12   n = 45 variables: one FLAT slot, partly filled (the member with NS = 1)
  M = 17   n = 65: the second FLAT slot holds one lane -- every other lane reads element 0 of the row and must get a zero
  M = 21   n = 81: the bench's shape
Iteration caps (PlannerConfig.maxiter, as tests/test_gpu_params.py sets them): the direction of iteration k runs after
k - 1 updates of the memory, so
  maxiter 1 .. 5        the last direction has col = 0, 1, 2, 3, 4 pairs: the plain loops, which these kernels keep while
                        the memory fills -- none, a single-pair step a loop, one pair of steps, a pair and a single, two pairs
  maxiter 11 .. 14      the memory is full and head = 0, 1, 2, 3: the first directions of the written-out form, slots
                        that wrap inside a step
  none                  runs to termination: every head, over and over
and "restart": goals inside inflated obstacles, pieces too short for v_max (the "violations" construction of the
gather-ahead file, M = 17) -- line searches that fail, after which the run drops its memory and takes the
steepest-descent direction in the same iteration (col = 0 in the middle of a run, then a memory that fills again, the
written-out form entered a second time).  The reference trace must show more than maxls + 1 = 21 evaluations under one
iteration number in at least one run (seed 63: it does in 22 of the 96).
"""
import ctypes

import numpy as np
import pytest

import neo_planner_amd as npa
from neo_planner_amd import _lib, synth
import param_sets as ps
from test_gpu_gather_ahead import B, CAP, KEYS, RES, _launches, _move_goal, dist  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPES = (12, 17, 21)
CAPS = (1, 2, 3, 4, 5, 11, 12, 13, 14, None)
CASES = [(M, cap) for M in SHAPES for cap in CAPS] + [("restart", None)]
BUDGET = 23                 # evaluations a launch of the budgeted run: launches end in the middle of line searches
RESTART_M, RESTART_SEED, MAXLS = 17, 63, 20       # (MAXLS: the default of PlannerConfig)


def requests(case, dist_):
    vol = dict(D=3, length_range=(10.0, 26.0), z_range=(1.5, 26.0), y_range=(-12.0, 12.0), pitch=0.25)
    if case == "restart":
        M = RESTART_M
        head, tail, wp, ts = synth.replan_requests(RESTART_SEED, B, M - 1, **vol)
        zz, yy, xx = np.nonzero(dist_[1:-1, 1:-1, 1:-1] <= 0.1)
        centres = (np.stack([xx, yy, zz], axis=1) + 1.5) * RES + np.asarray(synth.DOMAIN_ORIGIN)
        near = tail[:, 0, :]
        _move_goal(tail, wp, np.stack([centres[np.argmin(((centres - near[b]) ** 2).sum(axis=1))] for b in range(B)]))
        ts = np.random.default_rng(700 + RESTART_SEED).uniform(0.7, 2.0, ts.shape)
    else:
        M = case
        head, tail, wp, ts = synth.replan_requests(240 + M, B, M - 1, **vol)
        ts = np.random.default_rng(2700 + M).uniform(0.7, 4.6, ts.shape)
    return head, tail, wp, ts


def _planner(ctx, opts):
    return npa.BatchPlanner(config=ps.planner_config(None, **opts), ctx=ctx, sample_dtype="f32x", waves_per_simd=2)


@pytest.fixture(scope="module", params=["brick", "yz4"])
def field(request, dist):  # noqa: F811
    import torch
    ctx = _lib.Context(0)
    g3 = npa.ESDF3D(torch.from_numpy(dist).to(torch.device("cuda", 0)), RES, synth.DOMAIN_ORIGIN, store="f32", layout=request.param,
                    ctx=ctx)
    return ctx, g3, request.param


@pytest.fixture(scope="module")
def inputs(dist):  # noqa: F811
    """the requests of a shape, drawn once and shared by its cases"""
    return {case: requests(case, dist) for case in SHAPES + ("restart",)}


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "%s-%s" % c)
def runs(request, field, inputs):
    """the plain launch (fixed plan: the written-out recursion once the memory is full), the same launch with a trace
    (optimize_dyn_kernel: the plain loops throughout) and, in the brick layout, the budgeted run (dynamic plan as well)"""
    import torch
    ctx, g3, layout = field
    shape, cap = request.param
    head, tail, wp, ts = inputs[shape]
    opts = {} if cap is None else dict(maxiter=cap)
    out = {"case": request.param, "M": ts.shape[1], "cap": cap, "count": [_launches(ctx)]}
    new = _planner(ctx, opts)
    x0 = new.pack_x(wp, ts)
    out["new"] = new.optimize(g3, x0, head, tail, order=False)
    out["count"].append(_launches(ctx))
    old = _planner(ctx, opts)
    tr = torch.zeros(B, CAP, 4, dtype=torch.float64, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    ctx.check(ctx.lib.neo_optimize_trace(ctx.h, ctypes.c_void_p(tr.data_ptr()), CAP))
    try:
        out["old"] = old.optimize(g3, x0, head, tail, order=False)
    finally:
        ctx.check(ctx.lib.neo_optimize_trace(ctx.h, None, 0))
    out["count"].append(_launches(ctx))
    out["trace"] = tr.cpu().numpy()
    if layout == "brick":
        out["budgeted"] = _planner(ctx, opts).optimize_budgeted(g3, x0, head, tail, BUDGET)
        out["count"].append(_launches(ctx))
    return out


def test_written_out_recursion_gives_the_plain_loops_bit_for_bit(runs):
    for k in KEYS:
        assert np.array_equal(runs["new"][k], runs["old"][k]), (runs["case"], k, int((runs["new"][k] != runs["old"][k]).sum()))
        if "budgeted" in runs:
            assert np.array_equal(runs["new"][k], runs["budgeted"][k]), (runs["case"], k, int((runs["new"][k] != runs["budgeted"][k]).sum()))


def test_plain_launch_runs_the_fixed_plan_the_references_the_dynamic_one(runs):
    c = runs["count"]
    d = [(b[0] - a[0], b[1] - a[1]) for a, b in zip(c, c[1:])]      # (fixed, dynamic) launches of each step
    assert d[:2] == [(1, 0), (0, 1)], (runs["case"], d)
    if "budgeted" in runs:
        assert d[2][0] == 0 and d[2][1] == len(runs["budgeted"]["launch_sizes"]) >= 1, (runs["case"], d)


def test_the_reference_run_shows_what_the_case_exercises(runs):
    case, M, cap, ref, tr = runs["case"], runs["M"], runs["cap"], runs["old"], runs["trace"]
    nfev, nit = ref["nfev"], ref["nit"]
    assert nfev.min() >= 1 and nfev.max() <= CAP
    assert 4 * M - 3 == {12: 45, 17: 65, 21: 81}[M]
    if cap is not None:
        # runs that reach the cap: their last direction was formed after cap - 1 iterations
        capped = (ref["status"] == 3) & (nit == cap)
        assert capped.sum() >= B // 2, (case, int(capped.sum()))
        assert nit.max() <= cap
    elif case[0] != "restart":
        assert np.median(nit) > 14 and (ref["status"] <= 1).sum() >= B // 2       # converged, long after the memory filled
    else:
        # more than maxls + 1 evaluations under one iteration number: a line search failed and the iteration went on from
        # the steepest-descent direction with the memory dropped (the first iteration has 1 + maxls at the most, and ends
        # the run when its search fails)
        most = [int(np.bincount(tr[b, :nfev[b], 3].astype(np.int64)).max()) for b in range(B)]
        assert max(most) > MAXLS + 1, (case, max(most))
        assert ref["collision"].any()
