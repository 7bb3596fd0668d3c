"""
The gather-ahead sample loop of the all-fp32 optimiser kernel forms a round's velocity once, with the position its ESDF
addresses come from, and keeps it in LDS until the round is consumed: two alternating halves [it & 1][d][lane] at the
front of the staging buffer (csrc/neo_device.hpp minco_sample, velocity_stash_bytes).  The L-BFGS pairs lie right behind
the staging buffer, and below M = 20 the staging the fold and the exchange table ask for is SMALLER than the stash
(1 536 B at D = 3): the launcher sizes it for the stash as well (csrc/neo_launch_opt.hpp).  A stash that overran it would
corrupt the history silently -- other iterates, not a fault.

Method of tests/test_gpu_gather_ahead.py (its helpers are imported): a 48^3 field in the brick and the yz4 layout, B = 96
requests a case; the plain launch (fixed plan: the stash) against the same launch through a trace buffer
(optimize_dyn_kernel: the blocked loop, velocity in registers), bit for bit: x, both sets of cost terms, nit, nfev,
status, collision flag.  neo_optimize_plan_launches shows which kernel served each launch: no launch may have lost the
fixed plan to the stash.  Each case asserts on the reference run alone (its trace, its flags), on the start point x0 or
on the launcher's arithmetic that it exercises what it claims:

  m12 m16 m17 m19   durations U(0.7, 4.6): the shapes whose staging was smaller than the stash; one FLAT slot (n <= 64)
                    up to M = 16, two from M = 17; four rounds and more at the start, counts that change along a run
  three_rounds      M = 21, seven to nine samples a piece: three lanes a piece, exactly three rounds at the first
                    evaluation -- an odd count: the loop's last round is read from half 0
  four_rounds       M = 21, ten to twelve samples a piece: exactly four rounds -- the last round is read from half 1
  five_rounds       M = 21, eleven to fifteen samples a piece: five rounds, each half written three / two times
  violations21      M = 21, goals inside inflated obstacles and pieces too short for v_max: the stashed velocity feeds
                    sample_accumulate in most rounds

(M = 21 cannot have three rounds with more than nine samples a piece -- 21 pieces get three lanes each at the most --
so eleven to fifteen samples are a case of their own.)
"""
import ctypes

import numpy as np
import pytest

import neo_planner_amd as npa
from neo_planner_amd import synth
from test_gpu_gather_ahead import B, CAP, DT, KEYS, RES, _launches, _move_goal, dist, scene  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = ("m12", "m16", "m17", "m19", "three_rounds", "four_rounds", "five_rounds", "violations21")
ROUNDS = {"three_rounds": (7, 9, 3), "four_rounds": (10, 12, 4), "five_rounds": (11, 15, 5)}     # samples a piece, rounds
STASH = 2 * 3 * 64 * 4          # bytes: two rounds of a 3-D velocity, 64 lanes of floats


def requests(case, dist_):
    vol = dict(D=3, length_range=(10.0, 26.0), z_range=(1.5, 26.0), y_range=(-12.0, 12.0), pitch=0.25)
    if case[0] == "m":
        M = int(case[1:])
        head, tail, wp, ts = synth.replan_requests(140 + M, B, M - 1, **vol)
        ts = np.random.default_rng(1700 + M).uniform(0.7, 4.6, ts.shape)
    elif case in ROUNDS:
        M = 21
        lo, hi, _ = ROUNDS[case]
        head, tail, wp, ts = synth.replan_requests(190 + hi, B, M - 1, **vol)
        rng = np.random.default_rng(1800 + hi)
        # int(T / 0.1) = the drawn count, in fp32 as in fp64: T stays 0.02 s clear of the multiples of delta_t
        ts = (rng.integers(lo, hi + 1, ts.shape) + rng.uniform(0.2, 0.8, ts.shape)) * DT
    elif case == "violations21":
        M = 21
        head, tail, wp, ts = synth.replan_requests(163, B, M - 1, **vol)
        # goals on voxels well inside the inflated obstacles (distance <= 0.1 m against safe_dis = 0.7 m), nearest to the
        # drawn goal; 10 - 26 m in 21 pieces of 0.6 - 1.5 s: the start trajectory is faster than v_max = 1 m/s
        zz, yy, xx = np.nonzero(dist_[1:-1, 1:-1, 1:-1] <= 0.1)
        centres = (np.stack([xx, yy, zz], axis=1) + 1.5) * RES + np.asarray(synth.DOMAIN_ORIGIN)
        near = tail[:, 0, :]
        _move_goal(tail, wp, np.stack([centres[np.argmin(((centres - near[b]) ** 2).sum(axis=1))] for b in range(B)]))
        ts = np.random.default_rng(1863).uniform(0.6, 1.5, ts.shape)
    else:
        raise KeyError(case)
    return head, tail, wp, ts


def rounds_of(ns):
    """rounds of an evaluation with `ns` [M] samples a piece: the fewest R >= ceil(total / 64) with sum ceil(ns / R) <= 64
    (csrc/neo_device.hpp balanced_sample_lanes)"""
    R = max(1, -(-int(ns.sum()) // 64))
    while int((-(-ns // R)).sum()) > 64:
        R += 1
    return R


@pytest.fixture(scope="module", params=CASES)
def runs(request, scene, dist):  # noqa: F811
    """the plain launch (fixed plan: the stash), the same launch with a trace (optimize_dyn_kernel), and the cost terms of
    the start point from eval_kernel (the blocked loop as well)"""
    import torch
    ctx, g3 = scene
    case = request.param
    head, tail, wp, ts = requests(case, dist)
    out = {"case": case, "M": ts.shape[1], "ts": ts, "count": [_launches(ctx)]}
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
    out["costs_x0"] = old.cost_grad(g3, x0, head, tail)["costs"]
    return out


def test_stashed_velocity_gives_the_blocked_loop_bit_for_bit(runs):
    for k in KEYS:
        assert np.array_equal(runs["new"][k], runs["old"][k]), (runs["case"], k, int((runs["new"][k] != runs["old"][k]).sum()))


def test_plain_launch_keeps_the_fixed_plan_reference_is_dynamic(runs):
    c = runs["count"]
    d = [(b[0] - a[0], b[1] - a[1]) for a, b in zip(c, c[1:])]      # (fixed, dynamic) launches of each step
    assert d == [(1, 0), (0, 1)], (runs["case"], d)


def test_the_reference_run_shows_what_the_case_exercises(runs):
    case, M, ref, tr, ts = runs["case"], runs["M"], runs["old"], runs["trace"], runs["ts"]
    nfev = ref["nfev"]
    assert nfev.min() >= 1 and nfev.max() <= CAP
    totals = [tr[b, :nfev[b], 2] for b in range(B)]
    assert all(np.all(t > 0) for t in totals)
    ns = np.floor(ts / DT + 1e-9).astype(np.int64)
    if case[0] == "m":
        # what the fold (80 B a piece) and the exchange table ((M + 1) * 12 + 128 floats) ask of the staging: less than the stash
        assert max(M * 80, ((M + 1) * 12 + 128) * 4, 64 * 8 * (1 if 4 * M - 3 <= 64 else 2)) < STASH
        assert (4 * M - 3 <= 64) == (M <= 16)                      # FLAT slots: one up to M = 16, two from M = 17
        assert np.all(tr[:, 0, 2] > 3 * 64)                        # four rounds and more at the start: both halves, twice each
        assert any(np.unique(t).size > 1 for t in totals)          # counts -- lanes, rounds -- that change along a run
    elif case in ROUNDS:
        lo, hi, R = ROUNDS[case]
        assert ns.min() >= lo and ns.max() <= hi
        assert np.array_equal(tr[:, 0, 2], ns.sum(axis=1))         # the first evaluation saw exactly these samples
        assert all(rounds_of(ns[b]) == R for b in range(B))
    elif case == "violations21":
        assert ref["collision"].any()
        c0 = runs["costs_x0"]                                      # (energy, time, feasibility, collision) at x0
        assert (c0[:, 2] > 0).sum() >= B // 2 and (c0[:, 3] > 0).sum() >= B // 2
        assert np.all(tr[:, 0, 2] > 2 * 64)
