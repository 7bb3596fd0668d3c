"""
The fp32 L-BFGS pairs of the optimiser kernels lie in LDS as records: element e of the pair in a slot is (s_e, y_e) at
hist[(slot * n + e) * 2 + {0, 1}] (csrc/neo_lbfgs_dir.hpp hist_index; tests/test_hist_layout_cpu.py).  A lane moves s and y
of its element with one 8-byte access; under the fixed launch plan the written-out recursion (DevBackend::DirFull::read)
fetches a whole pair from ONE per-lane address with no condition, so a lane beyond n in the partly filled FLAT slot reads
the records that follow -- behind the last pair the cyclic reduction's multipliers -- and `settle` replaces what it read
by zeros.  Everywhere else (optimize_dyn_kernel, the budgeted members, the loops while the memory fills) such a lane reads
record 0 of the pair and takes zeros, or reads its record under its mask (DevBackend::kMaskedRead).  fp64 pairs keep their
rows [2][m][n] (hist_index_rows).  Placement changes no arithmetic: the plain launch, the same launch with a trace buffer
(optimize_dyn_kernel) and, in the brick layout (budgeted launches take no yz4 field), a budgeted run of 23 evaluations a
launch -- whose suspended state carries the region as it stands -- must agree bit for bit: x, both sets of cost terms,
iteration and evaluation counts, status and the collision flag, all 96 runs of every case.  neo_optimize_plan_launches
shows which kernel served each launch.

Shapes (a 48^3 synthetic field, B = 96 requests a case; tests/test_gpu_hist_ahead.py is the model):
  M = 12   n = 45: one FLAT slot, partly filled
  M = 17   n = 65: the second FLAT slot holds ONE element -- a wrong record offset or a missing `settle` shows at once
  M = 21   n = 81: the bench's shape
  M = 32   n = 125: lane = piece, no fixed plan -- the plain loops with the new layout in optimize_kernel itself
  M = 2, 3 n = 5, 9: the reads behind the last pair (472, 440 bytes) exceed the multipliers (48 bytes at M = 2): the
           launcher must send the plain launch to optimize_dyn_kernel
each with maxiter 1 .. 5 (the last direction has col = 0 .. 4 pairs), 11 .. 14 (the memory is full, head = 0 .. 3) and no
cap; "restart": goals inside inflated obstacles, pieces too short for v_max (M = 17) -- line searches that fail, the memory
dropped and filled again in the middle of a run; and M = 21 once each in the f32 and the f64 mode, whose pairs are doubles.
"""
import ctypes

import numpy as np
import pytest

import neo_planner_amd as npa
from neo_planner_amd import _lib, synth
import param_sets as ps
from test_gpu_gather_ahead import B, CAP, KEYS, RES, _launches, dist  # noqa: F401
from test_gpu_hist_ahead import BUDGET, MAXLS, requests

pytestmark = pytest.mark.gpu

FIXED_SHAPES = (12, 17, 21)          # the plain launch runs the fixed plan
SHAPES = FIXED_SHAPES + (32, 2, 3)
CAPS = (1, 2, 3, 4, 5, 11, 12, 13, 14, None)
CASES = [(M, cap, "f32x") for M in SHAPES for cap in CAPS] + [("restart", None, "f32x"), (21, None, "f32"), (21, None, "f64")]


def _planner(ctx, opts, mode):
    return npa.BatchPlanner(config=ps.planner_config(None, **opts), ctx=ctx, sample_dtype=mode, waves_per_simd=2)


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


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "%s-%s-%s" % c)
def runs(request, field, inputs):
    """the plain launch, the same launch with a trace (optimize_dyn_kernel) and, in the brick layout, the budgeted run"""
    import torch
    ctx, g3, layout = field
    shape, cap, mode = request.param
    head, tail, wp, ts = inputs[shape]
    opts = {} if cap is None else dict(maxiter=cap)
    out = {"case": request.param, "M": ts.shape[1], "cap": cap, "mode": mode, "count": [_launches(ctx)]}
    new = _planner(ctx, opts, mode)
    x0 = new.pack_x(wp, ts)
    out["new"] = new.optimize(g3, x0, head, tail, order=False)
    out["count"].append(_launches(ctx))
    old = _planner(ctx, opts, mode)
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
        out["budgeted"] = _planner(ctx, opts, mode).optimize_budgeted(g3, x0, head, tail, BUDGET)
        out["count"].append(_launches(ctx))
    return out


def test_plain_traced_and_budgeted_runs_agree_bit_for_bit(runs):
    for k in KEYS:
        assert np.array_equal(runs["new"][k], runs["old"][k]), (runs["case"], k, int((runs["new"][k] != runs["old"][k]).sum()))
        if "budgeted" in runs:
            assert np.array_equal(runs["new"][k], runs["budgeted"][k]), (runs["case"], k, int((runs["new"][k] != runs["budgeted"][k]).sum()))


def test_which_kernel_served_each_launch(runs):
    c = runs["count"]
    d = [(b[0] - a[0], b[1] - a[1]) for a, b in zip(c, c[1:])]      # (fixed, dynamic) launches of each step
    fixed = runs["mode"] == "f32x" and runs["M"] in FIXED_SHAPES
    # M = 2, 3: the reads behind the last pair do not fit the multipliers; M = 32 and the fp64-solve modes have no fixed plan
    assert d[:2] == [(1, 0) if fixed else (0, 1), (0, 1)], (runs["case"], d)
    if "budgeted" in runs:
        assert d[2][0] == 0 and d[2][1] == len(runs["budgeted"]["launch_sizes"]) >= 1, (runs["case"], d)


def test_the_reference_run_shows_what_the_case_exercises(runs):
    case, M, cap, ref, tr = runs["case"], runs["M"], runs["cap"], runs["old"], runs["trace"]
    nfev, nit = ref["nfev"], ref["nit"]
    assert nfev.min() >= 1 and nfev.max() <= CAP
    assert 4 * M - 3 == {2: 5, 3: 9, 12: 45, 17: 65, 21: 81, 32: 125}[M]
    if "budgeted" in runs and cap is None:
        assert len(runs["budgeted"]["launch_sizes"]) > 1            # runs were suspended and resumed: the state carried the pairs
    if cap is not None:
        assert nit.max() <= cap
        if M >= 12:
            # runs that reach the cap: their last direction was formed after cap - 1 iterations
            capped = (ref["status"] == 3) & (nit == cap)
            assert capped.sum() >= B // 2, (case, int(capped.sum()))
        else:
            assert nit.max() >= min(cap, 5), (case, int(nit.max()))      # some run has a memory of four pairs at the least
    elif case[0] != "restart":
        if M >= 12:
            assert np.median(nit) > 14 and (ref["status"] <= 1).sum() >= B // 2   # converged, long after the memory filled
        else:
            assert nit.max() > 10                                   # some run fills the memory (the plain loops at col = m)
    else:
        most = [int(np.bincount(tr[b, :nfev[b], 3].astype(np.int64)).max()) for b in range(B)]
        assert max(most) > MAXLS + 1, (case, max(most))             # a failed line search: memory dropped, filled again
        assert ref["collision"].any()
