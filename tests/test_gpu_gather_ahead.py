"""
The sample loop of the all-fp32 optimiser kernel under its fixed launch plan issues the ESDF gathers of round i + 1 before
it consumes round i (csrc/neo_device.hpp minco_sample, Plan::gather_ahead).  Rounds are consumed in the same order by the
same expressions, so the run must equal, bit for bit, the same launch through optimize_dyn_kernel, whose sample loop is the
one every other kernel has: x, both sets of cost terms, iteration and evaluation counts, status and the collision flag.
The reference launch reaches optimize_dyn_kernel through a trace buffer: the same launch plan with its selectors tested at
run time.  (Flags bit 4096 reaches it too, but asks for ANOTHER plan -- no kept multipliers of the cyclic reduction -- whose
bits differ from the plain launch's with or without this loop; that run is made, and only its routing is asserted.)
A third run, BatchPlanner's default launch, is compared as well.  (In the all-fp32 mode every 3-D launch is served by the
same family member, whatever waves_per_simd says -- csrc/neo_abi.hip -- so the third run checks that the flag changes
nothing; a one-wave kernel with four samples in flight exists only for the fp64 solve, whose bits differ by construction.)

Shapes: a 48^3 synthetic forest field in the brick and the yz4 layout, B = 96 requests a case.  The cases are the smallest
at which a rolling loop can go wrong, and each states what it exercises as an assertion on the reference (dynamic) run
alone -- its trace of per-evaluation sample totals, its collision flags -- or on the start point x0, which is the first
point any run evaluates:

  varied17 / varied21   durations drawn per piece from U(0.7, 4.6): the round count changes along a run
  one_round             every piece five samples and M = 12 pieces: 60 samples in 64 lanes, ONE round -- the loop body
                        never runs, nothing is prefetched.  (M = 21 cannot get there: T > T_min = 0.5 s means five samples
                        a piece at least, 105 in all; twelve pieces is the most that fit one round, and the member
                        with one FLAT slot that serves it runs under the same fixed plan.)
  two_rounds            the same durations at M = 21: 105 samples, lanes for ceil(5 / 2) = 3 samples a piece: exactly two
                        rounds at the first evaluation -- one prefetch, consumed after the loop
  border                start and goal within 0.3 m of the field's y border: the waypoints' scatter puts samples outside,
                        a prefetched round carries lanes with inside == false next to valid ones
  violations            goals inside inflated obstacles, pieces too short for v_max: sample_accumulate runs in most rounds
                        while the next round's gathers are in flight
"""
import ctypes

import numpy as np
import pytest

import neo_planner_amd as npa
from neo_planner_amd import _lib, synth

pytestmark = pytest.mark.gpu

B, CAP = 96, 1024
N, RES = 48, 30.0 / 48
KEYS = ("x", "costs", "costs_last", "nit", "nfev", "status", "collision")
CASES = ("varied17", "varied21", "one_round", "two_rounds", "border", "violations")
DT = 0.1


def field():
    return synth.esdf_3d(6, n=N, res=RES, canopy=8)


def _move_goal(tail, wp, goal):
    """the goal positions to `goal` [B][3]; the waypoints follow in proportion (their scatter about the line is kept)"""
    M = wp.shape[2] + 1
    wp += (goal - tail[:, 0, :])[:, :, None] * (np.arange(1, M)[None, None, :] / M)
    tail[:, 0, :] = goal


def requests(case, dist=None):
    """head, tail, waypoints, durations of a case (see the module's docstring)"""
    vol = dict(D=3, length_range=(10.0, 26.0), z_range=(1.5, 26.0), y_range=(-12.0, 12.0), pitch=0.25)
    if case in ("varied17", "varied21"):
        M = int(case[-2:])
        head, tail, wp, ts = synth.replan_requests(40 + M, B, M - 1, **vol)
        ts = np.random.default_rng(700 + M).uniform(0.7, 4.6, ts.shape)
    elif case in ("one_round", "two_rounds"):
        M = 12 if case == "one_round" else 21
        head, tail, wp, ts = synth.replan_requests(90 + M, B, M - 1, **vol)
        ts = np.random.default_rng(800 + M).uniform(0.52, 0.58, ts.shape)      # int(T / 0.1) = 5, in fp32 as in fp64
    elif case == "border":
        M = 17
        vol.update(y_range=(-14.95, -14.7))
        head, tail, wp, ts = synth.replan_requests(57, B, M - 1, **vol)
        # the goal back to the border (replan_requests clips it to 0.5 m inside): the straight line stays within 0.3 m of it
        goal = tail[:, 0, :].copy()
        goal[:, 1] = np.random.default_rng(857).uniform(-14.95, -14.7, B)
        _move_goal(tail, wp, goal)
        ts = np.random.default_rng(757).uniform(0.7, 4.6, ts.shape)
    elif case == "violations":
        M = 17
        head, tail, wp, ts = synth.replan_requests(63, B, M - 1, **vol)
        # goals on voxels well inside the inflated obstacles (distance <= 0.1 m against safe_dis = 0.7 m), nearest to the
        # drawn goal; waypoints rescaled onto the new straight line, their scatter kept
        dist = field() if dist is None else dist
        zz, yy, xx = np.nonzero(dist[1:-1, 1:-1, 1:-1] <= 0.1)
        cells = np.stack([xx, yy, zz], axis=1) + 1
        centres = (cells + 0.5) * RES + np.asarray(synth.DOMAIN_ORIGIN)
        near = tail[:, 0, :]
        _move_goal(tail, wp, np.stack([centres[np.argmin(((centres - near[b]) ** 2).sum(axis=1))] for b in range(B)]))
        ts = np.random.default_rng(763).uniform(0.7, 2.0, ts.shape)
    else:
        raise KeyError(case)
    return head, tail, wp, ts


def samples_of_x0(head, tail, wp, ts, dist):
    """positions [B][M][S][3] of the quadrature samples of the START trajectory and their mask [B][M][S] (sample j of a
    piece exists for j < int(T / delta_t)), from the fp64 coefficients of oracle/cpu_native"""
    from oracle import cpu_native
    M = ts.shape[1]
    S = int(np.floor(ts.max() / DT + 1e-9)) + 1
    pos = np.zeros((ts.shape[0], M, S, 3))
    mask = np.zeros((ts.shape[0], M, S), dtype=bool)
    grid = cpu_native.NativeMap.from_field3d(dist, RES, synth.DOMAIN_ORIGIN)
    pl = cpu_native.NativePlanner()
    for b in range(ts.shape[0]):
        pl.read_planning_conditions(grid, head[b], tail[b], wp[b], ts[b])
        x = np.concatenate([wp[b].reshape(-1), pl.map_T2tau(ts[b])])
        pl.get_grad(x)
        c = pl.coeffs.reshape(M, 6, 3)
        for p in range(M):
            ns = int(np.floor(ts[b, p] / DT + 1e-9))
            s = np.arange(ns) * DT
            pos[b, p, :ns] = sum(c[p, k][None, :] * s[:, None] ** k for k in range(6))
            mask[b, p, :ns] = True
    return pos, mask


def _launches(ctx):
    fixed, dyn = ctypes.c_int64(), ctypes.c_int64()
    ctx.check(ctx.lib.neo_optimize_plan_launches(ctx.h, ctypes.byref(fixed), ctypes.byref(dyn)))
    return int(fixed.value), int(dyn.value)


@pytest.fixture(scope="module")
def dist():
    return field()


@pytest.fixture(scope="module", params=["brick", "yz4"])
def scene(request, dist):
    import torch
    ctx = _lib.Context(0)
    g3 = npa.ESDF3D(torch.from_numpy(dist).to(torch.device("cuda", 0)), RES, synth.DOMAIN_ORIGIN, store="f32", layout=request.param,
                    ctx=ctx)
    return ctx, g3


@pytest.fixture(scope="module", params=CASES)
def runs(request, scene, dist):
    """the fixed form (the new loop), the dynamic form with its trace (the old loop), flags bit 4096, the default launch"""
    import torch
    ctx, g3 = scene
    case = request.param
    head, tail, wp, ts = requests(case, dist)
    M = ts.shape[1]
    out = {"case": case, "M": M, "req": (head, tail, wp, ts), "count": [_launches(ctx)]}
    new = npa.BatchPlanner(ctx=ctx, sample_dtype="f32x", waves_per_simd=2)
    x0 = new.pack_x(wp, ts)
    out["new"] = new.optimize(g3, x0, head, tail, order=False)
    out["count"].append(_launches(ctx))
    old = npa.BatchPlanner(ctx=ctx, sample_dtype="f32x", waves_per_simd=2)
    tr = torch.zeros(B, CAP, 4, dtype=torch.float64, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    ctx.check(ctx.lib.neo_optimize_trace(ctx.h, ctypes.c_void_p(tr.data_ptr()), CAP))
    try:
        out["old"] = old.optimize(g3, x0, head, tail, order=False)
    finally:
        ctx.check(ctx.lib.neo_optimize_trace(ctx.h, None, 0))
    out["count"].append(_launches(ctx))
    out["trace"] = tr.cpu().numpy()
    cmp_ = npa.BatchPlanner(ctx=ctx, sample_dtype="f32x", waves_per_simd=2)
    cmp_.flags |= 4096
    cmp_.optimize(g3, x0, head, tail, order=False)
    out["count"].append(_launches(ctx))
    out["default"] = npa.BatchPlanner(ctx=ctx, sample_dtype="f32x").optimize(g3, x0, head, tail, order=False)
    return out


def test_gather_ahead_loop_is_the_blocked_loop_bit_for_bit(runs):
    for k in KEYS:
        assert np.array_equal(runs["new"][k], runs["old"][k]), (runs["case"], k, int((runs["new"][k] != runs["old"][k]).sum()))
        assert np.array_equal(runs["new"][k], runs["default"][k]), (runs["case"], k)


def test_routing_first_run_fixed_form_reference_and_flag_4096_dynamic(runs):
    c = runs["count"]
    d = [(b[0] - a[0], b[1] - a[1]) for a, b in zip(c, c[1:])]      # (fixed, dynamic) launches of each step
    assert d == [(1, 0), (0, 1), (0, 1)], d


def test_the_reference_run_shows_what_the_case_exercises(runs, dist):
    case, M, ref, tr = runs["case"], runs["M"], runs["old"], runs["trace"]
    head, tail, wp, ts = runs["req"]
    nfev = ref["nfev"]
    assert nfev.min() >= 1 and nfev.max() <= CAP
    totals = [tr[b, :nfev[b], 2] for b in range(B)]
    assert all(np.all(t > 0) for t in totals)
    # rounds of an evaluation: the fewest R with sum ceil(ns / R) <= 64 (balanced_sample_lanes) >= ceil(total / 64)
    if case in ("varied17", "varied21"):
        assert np.all(tr[:, 0, 2] > 2 * 64)                        # three rounds and more at the start
        # sample counts -- and with them the lanes and the rounds -- that change along a run
        assert any(np.unique(t).size > 1 for t in totals)
    elif case == "one_round":
        assert M * 5 <= 64 and np.all(tr[:, 0, 2] == M * 5)        # every piece five samples: one lane each, one round
        assert sum(int((t <= 64).sum()) for t in totals) >= B
    elif case == "two_rounds":
        assert np.all(tr[:, 0, 2] == M * 5) and M * 5 > 64 and M * 3 <= 64     # ceil(5 / 1) lanes do not fit, ceil(5 / 2) do
    elif case == "border":
        pos, mask = samples_of_x0(head, tail, wp, ts, dist)
        lo = np.asarray(synth.DOMAIN_ORIGIN)
        outside = mask & np.any((pos < lo - 0.05) | (pos > lo + N * RES + 0.05), axis=3)
        inside = mask & np.all((pos > lo + 0.05) & (pos < lo + N * RES - 0.05), axis=3)
        # requests whose start trajectory -- the first point the run evaluates -- has samples on both sides of the border
        assert (outside.any(axis=(1, 2)) & inside.any(axis=(1, 2))).sum() >= B // 2
    elif case == "violations":
        assert ref["collision"].any()
