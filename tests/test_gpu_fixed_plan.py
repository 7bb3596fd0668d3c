"""
The all-fp32 optimiser kernel compiled for its launch plan (csrc/neo_kernels.hpp: optimize_kernel under PlanFixedX) against
the same run with the plan's selectors tested at run time (optimize_dyn_kernel) and against a budgeted launch: x, both sets
of cost terms, iteration and evaluation counts and status bit for bit -- and the launcher's routing: a plain context runs
the fixed form; a trace buffer or flags bit 4096 (comparison runs) must never reach it.

Shapes: a 48^3 synthetic forest field, brick layout, B = 96 requests at M = 17 and M = 21 pieces -- the smallest and the
largest piece count of cfg2's family member (two FLAT slots: 64 < 4M - 3 <= 128; one lane per (piece, dimension):
3M <= 64).  Durations are drawn per piece, so pieces have different sample counts and a piece's partials are folded over
several sample lanes; the trace of per-evaluation sample totals shows runs whose counts change on the way, i.e. runs that
need a second lane assignment (the cached one no longer fits).
"""
import ctypes

import numpy as np
import pytest

import neo_planner_amd as npa
from neo_planner_amd import _lib, synth

pytestmark = pytest.mark.gpu

B, CAP = 96, 1024
KEYS = ("x", "costs", "costs_last", "nit", "nfev", "status", "collision")


def _launches(ctx):
    fixed, dyn = ctypes.c_int64(), ctypes.c_int64()
    ctx.check(ctx.lib.neo_optimize_plan_launches(ctx.h, ctypes.byref(fixed), ctypes.byref(dyn)))
    return int(fixed.value), int(dyn.value)


def _requests(M):
    head, tail, wp, ts = synth.replan_requests(40 + M, B, M - 1, D=3, length_range=(10.0, 26.0), z_range=(1.5, 26.0),
                                               y_range=(-12.0, 12.0), pitch=0.25)
    ts = np.random.default_rng(700 + M).uniform(0.7, 4.6, ts.shape)      # (T_min 0.5 < T < T_max 5: 7 .. 46 samples a piece)
    return head, tail, wp, ts


@pytest.fixture(scope="module")
def scene():
    import torch
    ctx = _lib.Context(0)
    res = 30.0 / 48
    dist = synth.esdf_3d(6, n=48, res=res, canopy=8)
    g3 = npa.ESDF3D(torch.from_numpy(dist).to(torch.device("cuda", 0)), res, synth.DOMAIN_ORIGIN, store="f32", layout="brick", ctx=ctx)
    return ctx, g3


@pytest.fixture(scope="module", params=[17, 21])
def runs(request, scene):
    """one plain launch, the same launch with trace buffers, the same with flags bit 4096, one budgeted launch: results
    and the launch counters around each"""
    import torch
    ctx, g3 = scene
    M = request.param
    head, tail, wp, ts = _requests(M)
    bp = npa.BatchPlanner(ctx=ctx, sample_dtype="f32x")
    x0 = bp.pack_x(wp, ts)
    n = x0.shape[1]
    assert 64 < n <= 128 and 3 * M <= 64
    out = {"M": M, "count": [_launches(ctx)]}
    out["plain"] = bp.optimize(g3, x0, head, tail, order=False)
    out["count"].append(_launches(ctx))
    dev = torch.device("cuda", 0)
    tr = torch.zeros(B, CAP, 4, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.neo_optimize_trace(ctx.h, ctypes.c_void_p(tr.data_ptr()), CAP))
    try:
        out["traced"] = bp.optimize(g3, x0, head, tail, order=False)
    finally:
        ctx.check(ctx.lib.neo_optimize_trace(ctx.h, None, 0))
    out["count"].append(_launches(ctx))
    out["trace"] = tr.cpu().numpy()
    cmp_ = npa.BatchPlanner(ctx=ctx, sample_dtype="f32x")
    cmp_.flags |= 4096
    out["flag4096"] = cmp_.optimize(g3, x0, head, tail, order=False)
    out["count"].append(_launches(ctx))
    bp._sync()
    out["budgeted"] = bp.optimize_budgeted(g3, x0, head, tail, 1 << 20)
    out["count"].append(_launches(ctx))
    out["plain_again"] = bp.optimize(g3, x0, head, tail, order=False)
    out["count"].append(_launches(ctx))
    return out


def test_the_cases_fold_over_several_lanes_and_reassign_lanes(runs):
    ref, tr = runs["plain"], runs["trace"]
    nfev = ref["nfev"]
    assert nfev.max() <= CAP and nfev.min() >= 1
    # the lane assignment of the drawn durations (csrc/neo_device.hpp balanced_sample_lanes: the fewest rounds R for which
    # sum ceil(ns / R) lanes fit the wavefront): every request has pieces with different numbers of sample lanes, more than
    # one lane for some piece -- the fold over several lanes, per-piece accumulators
    _, _, _, ts = _requests(runs["M"])
    for ns in np.floor(ts / 0.1 + 1e-6).astype(int):
        R = next(R for R in range(1, 64) if (-(-ns // R)).sum() <= 64)
        lanes = -(-ns // R)
        assert lanes.max() >= 2 and lanes.min() < lanes.max() - 1      # (a margin of one: T goes through fp32 on the device)
    assert np.all(tr[:, 0, 2] > 64)
    # a run whose sample total changes between two evaluations has changed a piece's sample count: the cached lane
    # assignment missed and a second one was made
    changed = [b for b in range(B) if nfev[b] >= 2 and np.unique(tr[b, :nfev[b], 2]).size > 1]
    assert changed, "no run needed a second lane assignment"
    for b in range(B):      # (every counted evaluation left its record, none beyond)
        assert np.all(tr[b, :nfev[b], 2] > 0) and not tr[b, nfev[b]:].any()


def test_fixed_plan_kernel_is_the_dynamic_kernel_bit_for_bit(runs):
    for k in KEYS:
        assert np.array_equal(runs["plain"][k], runs["traced"][k]), (runs["M"], k, int((runs["plain"][k] != runs["traced"][k]).sum()))
        assert np.array_equal(runs["plain"][k], runs["plain_again"][k]), (runs["M"], k)


def test_fixed_plan_kernel_is_the_budgeted_launch_bit_for_bit(runs):
    assert runs["budgeted"]["launch_sizes"] == [B]
    for k in KEYS:
        assert np.array_equal(runs["plain"][k], runs["budgeted"][k]), (runs["M"], k, int((runs["plain"][k] != runs["budgeted"][k]).sum()))


def test_routing_plain_launches_run_the_fixed_form_traces_and_comparison_runs_never(runs):
    c = runs["count"]
    d = [(b[0] - a[0], b[1] - a[1]) for a, b in zip(c, c[1:])]      # (fixed, dynamic) launches of each step
    assert d[0] == (1, 0), d          # a plain context
    assert d[1] == (0, 1), d          # a trace buffer
    assert d[2] == (0, 1), d          # flags bit 4096
    assert d[3] == (0, 1), d          # a budgeted launch (its kernels keep the run-time selectors)
    assert d[4] == (1, 0), d          # and plain again, with the trace gone and the flag cleared
