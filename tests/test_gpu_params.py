"""
The kernels away from the default planner parameters and optimiser caps (tests/param_sets.py: sets A, B, C and the
non-default optimiser options).  Every other GPU test runs at the ROS YAML defaults, where 1 / delta_t is 10.0f exactly, a
piece never has more than 50 samples, every fp32 copy of a parameter in DevParams is (nearly) exact and no run ever ends
on maxiter / maxfun.

Per evaluation: cost_grad in the fp64 mode against oracle/minco_np.OraclePlanner (1e-10 / 1e-9, the bars of
test_gpu_parity.test_cost_grad_matches_oracle_on_random_batches), in the fp32 modes against oracle/cpu_native.eval_points
(2e-5 / 4e-5 on the cost, five times that on the gradient: test_cost_grad_trilinear_matches_oracle; the inputs are those for
which the CPU oracle with fp32 sampling itself stays inside 2e-5 / 1e-4 at every point -- measured at most 3.0e-6 / 3.1e-5 --
so no evaluation is exempt), recorded sample counts, the ESDF-lookup kernel alone on ragged durations, the lane-group
kernel against the default one.  Inputs: param_sets.case_inputs; at every case each weighted cost term with a non-zero
weight is positive in at least five of the six trajectories (checked with the oracle when the ranges were chosen).
A 3-D field takes D = 3 only (neo_abi.hip dispatch), so the D = 2 shapes run on the 2-D map.

Optimiser options on the device: capped runs are prefixes of the uncapped run, bit for bit, and end where
csrc/neo_lbfgs.hpp ends them; the same runs on the CPU optimiser (oracle/cpu_native.optimize_batch) with the same options;
maxfun counted over all launches of a budgeted run.  Every optimiser result of this file is checked for
collision == (costs_last[3] * weights[3] > collision_cost_tol).
"""
import ctypes

import numpy as np
import pytest

import param_sets as ps
from helpers import rel_err

pytestmark = pytest.mark.gpu

SETS3 = ["A", "B", "C"]
ROUND = {"f64": 1e-13, "f32": 1e-6, "f32x": 1e-6}      # test_gpu_trace_parity.ROUND: w . costs4_last against the recorded f


@pytest.fixture(scope="module")
def world():
    import neo_planner_amd as npa
    from neo_planner_amd import _lib, synth
    from oracle import cpu_native as cn
    from oracle import minco_np as onp
    ctx = _lib.Context(0)
    occ = synth.occupancy_2d(3)
    m2 = npa.ESDF(ctx)
    m2.occupancy_map_cb(synth.OccupancyGridMsg(occ))
    o2 = onp.GridESDF(occ, synth.RES, 300, 300, (0.0, -15.0))
    assert np.array_equal(m2.esdf_map, o2.esdf_map)
    w = dict(ctx=ctx, dev={"2d": m2}, np={"2d": o2}, cn={"2d": cn.NativeMap.from_grid2d(o2)})
    for store in ("f32", "f16"):
        d = ps.field32(0)
        if store == "f16":
            d = d.astype(np.float16).astype(np.float32)          # the values as stored: fp16 widened
        w["dev"]["3d" + store] = npa.ESDF3D(d, ps.RES3, ps.ORIGIN3, store=store, layout="brick", ctx=ctx)
        w["np"]["3d" + store] = onp.Grid3DESDF(d, ps.RES3, ps.ORIGIN3)
        w["cn"]["3d" + store] = cn.NativeMap.from_field3d(d, ps.RES3, ps.ORIGIN3)
    return w


def _planner(world, name, mode="f64", **kw):
    import neo_planner_amd as npa
    opts = kw.pop("opts", {})
    return npa.BatchPlanner(config=ps.planner_config(name, **opts), ctx=world["ctx"], sample_dtype=mode, **kw)


def _check_flag(res, cfg):
    """the collision flag of an optimiser result is the reference's test (expert_planner.py:235) at the set's values"""
    ok = res["status"] <= 3
    want = res["costs_last"][:, 3] * float(cfg.weights[3]) > float(cfg.collision_cost_tol)
    assert np.array_equal(res["collision"][ok], want[ok])
    assert set(np.unique(res["status"]).tolist()) <= {0, 1, 2, 3, 4, 5}


# ------------------------------------------------------------------------------------------------ cost_grad, fp64 mode
FP64_CASES = [("2d", M, D) for M, D in ((1, 2), (2, 2), (3, 2), (21, 2), (21, 3), (44, 2), (64, 3))] + \
             [("3df32", 21, 3), ("3df32", 64, 3)]


@pytest.mark.parametrize("name", SETS3)
@pytest.mark.parametrize("kind,M,D", FP64_CASES)
def test_cost_grad_fp64_matches_the_oracle_at_the_sets(world, name, kind, M, D):
    from oracle import minco_np as onp
    head, tail, wp, ts = ps.case_inputs(name, kind[:2], M, D)
    cfg = ps.oracle_params(name)
    wts = np.asarray(cfg.weights)
    active = np.zeros(4)
    for stale in (True, False):
        if M == 1 and stale:
            continue                     # the reference itself fails for M = 1 (unbound T at :529)
        bp = _planner(world, name, "f64", stale_T=stale)
        x = bp.pack_x(wp, ts)
        assert np.array_equal(x, ps.pack_x(name, wp, ts))
        out = bp.cost_grad(world["dev"][kind], x, head, tail, want_coeffs=True)
        for b in range(x.shape[0]):
            pl = onp.OraclePlanner(cfg, stale_T=stale)
            pl.read_planning_conditions(world["np"][kind], head[b], tail[b], wp[b], ts[b])
            c = pl.get_cost(x[b]); costs = pl.costs.copy(); g = pl.get_grad(x[b])
            errs = (rel_err(out["coeffs"][b], pl.coeffs), abs(out["cost"][b] - c) / abs(c), rel_err(out["costs"][b], costs),
                    rel_err(out["grad"][b], g))
            print(name, kind, M, D, stale, b, "coeffs %.1e cost %.1e terms %.1e grad %.1e" % errs)
            assert errs[0] < 1e-10 and errs[1] <= 1e-10 and errs[2] < 1e-10 and errs[3] < 1e-9, (name, kind, M, D, stale, b, errs)
            active += (costs * wts > 0) * (0.5 if M > 1 else 1.0)
    assert np.all(active[wts > 0] >= 3), active      # every weighted term at work in at least half of the trajectories


# ------------------------------------------------------------------------------------------------ cost_grad, fp32 modes
@pytest.mark.parametrize("name", SETS3)
@pytest.mark.parametrize("store", ["f32", "f16"])
@pytest.mark.parametrize("M", [1, 3, 16, 21, 41, 64])
def test_cost_grad_fp32_modes_match_the_oracle_at_the_sets(world, name, store, M):
    from oracle import cpu_native as cn
    kind = "3d" + store
    head, tail, wp, ts = ps.case_inputs(name, "3d", M, 3)
    cfg = ps.oracle_params(name)
    x = ps.pack_x(name, wp, ts)
    ref = [cn.eval_points(world["cn"][kind], x[b:b + 1], head[b], tail[b], M, 3, cn.make_params(cfg)) for b in range(len(x))]
    assert all(r["status"][0] == 0 for r in ref)
    for mode, tol in (("f32", 2e-5), ("f32x", 4e-5)):
        out = _planner(world, name, mode).cost_grad(world["dev"][kind], x, head, tail)
        for b, r in enumerate(ref):
            ef, eg = abs(out["cost"][b] - r["f"][0]) / abs(r["f"][0]), rel_err(out["grad"][b], r["grad"][0])
            print(name, store, M, mode, b, "cost %.1e grad %.1e" % (ef, eg))
            assert ef <= tol and eg < 5 * tol, (name, store, M, mode, b, ef, eg)


# ------------------------------------------------------------------------------------------------ traced launches
def _launch(world, bp, dmap, x0, head, tail, cap=0):
    """one optimize_dev launch; cap > 0 records the first `cap` evaluations of every run (trace, xg)"""
    import torch
    ctx = world["ctx"]
    dev = torch.device("cuda", ctx.device)
    B, n = x0.shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = dict(x=torch.empty(B, n, dtype=torch.float64, device=dev), costs=torch.zeros(B, 4, dtype=torch.float64, device=dev),
               costs_last=torch.zeros(B, 4, dtype=torch.float64, device=dev), nit=torch.zeros(B, dtype=torch.int32, device=dev),
               nfev=torch.zeros(B, dtype=torch.int32, device=dev), status=torch.zeros(B, dtype=torch.int32, device=dev))
    if cap:
        out["trace"] = torch.zeros(B, cap, 4, dtype=torch.float64, device=dev)
        out["xg"] = torch.zeros(B, cap, 2, n, dtype=torch.float64, device=dev)
    d_x0, d_h, d_t = t(x0), t(head), t(tail)
    torch.cuda.synchronize(dev)
    bp._sync()
    try:
        if cap:
            ctx.check(ctx.lib.neo_optimize_trace(ctx.h, ctypes.c_void_p(out["trace"].data_ptr()), cap))
            ctx.check(ctx.lib.neo_optimize_trace_xg(ctx.h, ctypes.c_void_p(out["xg"].data_ptr()), cap))
        bp.optimize_dev(dmap, out["x"], d_h, d_t, out["costs"], out["costs_last"], out["nit"], out["nfev"], out["status"], x0=d_x0)
        ctx.synchronize()
    finally:
        ctx.check(ctx.lib.neo_optimize_trace(ctx.h, None, 0))
        ctx.check(ctx.lib.neo_optimize_trace_xg(ctx.h, None, 0))
    r = {k: v.cpu().numpy() for k, v in out.items()}
    r["collision"] = (r["status"] & 0x100) != 0
    r["status"] = r["status"] & 0xff
    _check_flag(r, bp.cfg)
    return r


@pytest.mark.parametrize("name", SETS3)
@pytest.mark.parametrize("mode", ["f64", "f32"])
def test_recorded_sample_counts_are_the_references(world, name, mode):
    """int(T / delta_t) per piece (expert_planner.py:401), summed: what the fp64 and f32 modes record for the first
    evaluation of a run -- with T from the kernel's own tau -> T map, on the 2-D map and the field"""
    s = ps.SETS[name]
    for kind, M, D in (("2d", 3, 2), ("2d", 44, 2), ("3df32", 1, 3), ("3df32", 21, 3), ("3df32", 64, 3)):
        head, tail, wp, ts = ps.case_inputs(name, kind[:2], M, D, seed=1)
        x0 = ps.pack_x(name, wp, ts)
        r = _launch(world, _planner(world, name, mode, opts=dict(maxfun=1)), world["dev"][kind], x0, head, tail, cap=2)
        T = (s["T_max"] - s["T_min"]) / (1.0 + np.exp(-x0[:, D * (M - 1):])) + s["T_min"]
        q = T / s["delta_t"]
        assert np.abs(q - np.round(q)).min() > 1e-9        # no duration on a sample boundary: the count is unambiguous
        assert np.array_equal(r["trace"][:, 0, 2], ps.sample_count(T, name)), (name, mode, kind, M)
        if name == "B":
            assert np.floor(q).max() > 50                  # pieces with more samples than the defaults can give


# ------------------------------------------------------------------------------------------------ sampled_terms alone
def _ragged(rng, name, B, M):
    s = ps.SETS[name]
    dt = s["delta_t"]
    ts = ps.durations(rng, name, (B, M), *ps.DUR[name])
    ts[2:4] = rng.uniform(0.2, 3.5, (2, M)) * dt                       # 0 .. 3 samples a piece
    ts[4] = np.where(rng.random(M) < 0.5, 0.5 * dt, ts[4])             # pieces without samples among ordinary ones
    ts[5] = 1.2 * dt; ts[5, M // 2] = 0.98 * s["T_max"]                # one long piece among one-sample pieces
    ts[6] = 0.5 * (s["T_min"] + s["T_max"])                            # every piece alike
    ts[7] = 0.3 * dt                                                   # a trajectory without any sample
    return ts


@pytest.mark.parametrize("name", SETS3)
@pytest.mark.parametrize("M", [1, 3, 21, 64])
def test_sampled_terms_on_ragged_durations_at_the_sets(world, name, M):
    """the ESDF-lookup kernel alone (add_sampled_cost + add_sampled_grad_CT, :392-466): fp64 against the oracle at 1e-11,
    fp32 sampling against fp64 trajectory by trajectory (the rule of test_gpu_parity.test_sampled_terms_on_ragged_durations),
    the fp32-buffer form carries the fp32 form's bits.  Set B's long piece has floor(0.98 * 3.1 / 0.013) = 233 samples."""
    import zlib
    from oracle import minco_np as onp
    B, D = 8, 3
    rng = np.random.default_rng(zlib.crc32(f"ragged-{name}-{M}".encode()))
    head, tail, wp, ts0 = ps.case_inputs(name, "3d", M, D, B=B, seed=2)
    g3, o3 = world["dev"]["3df32"], world["np"]["3df32"]
    bp64 = _planner(world, name, "f64")
    coeffs = bp64.cost_grad(g3, bp64.pack_x(wp, ts0), head, tail, want_coeffs=True)["coeffs"]
    ts = _ragged(rng, name, B, M)
    ns = np.floor(ts / ps.SETS[name]["delta_t"]).astype(int)
    assert ns[5].max() == int(0.98 * ps.SETS[name]["T_max"] / ps.SETS[name]["delta_t"]) and (ns[7] == 0).all()
    a = bp64.sampled_terms(g3, coeffs, ts)
    cfg = ps.oracle_params(name)
    for b in range(B):
        pl = onp.OraclePlanner(cfg)
        pl.read_planning_conditions(o3, head[b], tail[b], wp[b], ts[b])
        pl.coeffs = coeffs[b]
        pl.reset_cost(); pl.add_sampled_cost()
        pl.reset_grad_CT(); pl.add_sampled_grad_CT()
        for got, want in ((a["costs2"][b], pl.costs[2:]), (a["grad_C"][b], pl.grad_C), (a["grad_T"][b], pl.grad_T)):
            if np.abs(want).max() == 0:
                assert np.all(got == 0), (name, M, b)
            else:
                assert rel_err(got, want) < 1e-11, (name, M, b, rel_err(got, want))
    bp32 = _planner(world, name, "f32")
    f = bp32.sampled_terms(g3, coeffs, ts)
    f2 = bp32.sampled_terms(g3, coeffs, ts)
    for k in ("costs2", "grad_C", "grad_T"):
        assert np.array_equal(f[k], f2[k]) and np.isfinite(f[k]).all(), k
        for t in range(B):
            sc = max(np.abs(a[k][t]).max(), 1e-3 * np.abs(a[k]).max())
            assert np.abs(f[k][t] - a[k][t]).max() <= 1e-3 * sc, (name, M, k, t, ns[t])
    assert np.all(f["costs2"][7] == 0) and np.all(f["grad_C"][7] == 0) and np.all(f["grad_T"][7] == 0)
    for r in (a, f):
        assert np.all(r["grad_C"].reshape(B, M, 6, D)[ns == 0] == 0) and np.all(r["grad_T"][ns == 0] == 0)
    c32 = bp32.sampled_terms(g3, coeffs, ts, io32=True)
    assert c32["grad_C"].dtype == np.float32 and c32["grad_T"].dtype == np.float32
    assert np.array_equal(c32["costs2"], f["costs2"])
    assert np.array_equal(c32["grad_C"].astype(np.float64), f["grad_C"]) and np.array_equal(c32["grad_T"].astype(np.float64), f["grad_T"])
    # (the weighted terms are at work: an ordinary trajectory has a collision partial at every set)
    assert a["costs2"][:2, 1].max() > 0 and np.abs(a["grad_C"][:2]).max() > 0


# ------------------------------------------------------------------------------------------------ the lane-group kernel
def _opt_inputs(name, kind, M, D, B, seed):
    """start points for whole runs: durations in the lower part of the set's range, as the whole-run parity rows take them"""
    import zlib
    rng = np.random.default_rng(zlib.crc32(f"opt-{name}-{kind}-{M}-{D}-{seed}".encode()))
    lo, hi = ps.BOX2 if kind == "2d" else ps.BOX3
    head, tail, wp = ps.random_requests(rng, B, M, D, lo[:D], hi[:D])
    ts = ps.durations(rng, name, (B, M), *ps.RUN_DUR[name])
    return head, tail, wp, ts


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("kind,D", [("2d", 2), ("3df32", 3)])
@pytest.mark.parametrize("M", [3, 8, 16])
def test_lane_group_kernel_at_the_sets(world, name, kind, D, M):
    """NEO_FLAG_LANE_GROUPS against the default kernel (fp32 sampling) on the small problems of
    test_gpu_api_edges.test_lane_group_kernel_small_problems, to its bars: bit-reproducible; runs on the default kernel's
    path end within 1e-2 in x (90 %) and 1e-5 in the final cost (median).
    The compared runs are capped at three iterations.  Whole runs cannot be held to the x bar at set B by any pair of fp32
    evaluations: the CPU optimiser with fp32 sampling (cpu_native, sample_f32) against itself with 1e-7 noise on the
    coefficients ends 9e-2 (2-D, M = 3) and 1.9e-1 (field, M = 3) apart in x (90 %) among the runs with equal counts --
    set B's small time weight leaves flat directions -- while its three-iteration runs agree to 6e-5 in x and 1.5e-6 in the
    cost, 43 to 48 of 48 on the same path; the kernels are asked for the 40 % of
    test_gpu_parity.test_lane_groups_on_the_2d_reference_map_match_the_default_kernel.  The whole runs are held to
    reproducibility, the collision flag and valid statuses; their figures are printed.
    M = 16 has n > 32 variables: not a lane-group shape, the default kernel's bits (neo_abi.hip lane_group_launch)."""
    B = 48
    head, tail, wp, ts = ps.small_requests(name, kind[:2], M, D, B)
    x0 = ps.pack_x(name, wp, ts)
    dmap = world["dev"][kind]
    for opts in ({}, dict(maxiter=3)):
        a = _launch(world, _planner(world, name, "f32", opts=opts), dmap, x0, head, tail)
        g = _planner(world, name, "f32", lane_groups=True, opts=opts)
        b, b2 = _launch(world, g, dmap, x0, head, tail), _launch(world, g, dmap, x0, head, tail)
        for k in ("x", "costs", "costs_last", "nit", "nfev", "status"):
            assert np.array_equal(b[k], b2[k]), (M, k)
        if M == 16:
            for k in ("x", "costs", "costs_last", "nit", "nfev", "status"):
                assert np.array_equal(a[k], b[k]), (M, k)
            continue
        lim = 3 if opts else 1
        same = (a["status"] <= lim) & (b["status"] <= lim) & (a["nit"] == b["nit"]) & (a["nfev"] == b["nfev"]) & \
               (a["status"] == b["status"])
        w = np.asarray(g.cfg.weights)
        fa, fb = (a["costs_last"] * w).sum(axis=1), (b["costs_last"] * w).sum(axis=1)
        dx90 = np.percentile(np.abs(a["x"][same] - b["x"][same]).max(axis=1), 90) if same.any() else np.nan
        dc = np.median(np.abs(fa[same] - fb[same]) / np.abs(fa[same])) if same.any() else np.nan
        print(name, kind, M, opts, "same path", int(same.sum()), "of", B, "x (90 %%) %.1e cost (median) %.1e" % (dx90, dc))
        if opts:
            assert same.mean() >= 0.4, (name, kind, M, same.mean())
            assert np.all(b["nit"][b["status"] == 3] == 3) and (b["status"] == 3).sum() >= B // 2
            assert dx90 < 1e-2 and dc < 1e-5, (name, kind, M, dx90, dc)


# ------------------------------------------------------------------------------------------------ thresholds, neo_params_set
def test_collision_flag_follows_the_sets_tolerance(world):
    """the same run -- set A with its own collision_cost_tol (40) and with set B's (0.5): the tolerance does not enter the
    optimisation, so costs_last is the same bit for bit, and the flag changes for exactly the runs in between"""
    M, D, B = 21, 3, 24
    head, tail, wp, ts = _opt_inputs("A", "3d", M, D, B, 8)
    x0 = ps.pack_x("A", wp, ts)
    # (three iterations: runs that are still near the obstacles, five of them in between on the CPU optimiser)
    bpA = _planner(world, "A", opts=dict(maxiter=3))
    bpB = _planner(world, "A", opts=dict(maxiter=3))
    bpB.cfg.collision_cost_tol = ps.SETS["B"]["collision_cost_tol"]
    rA = bpA.optimize(world["dev"]["3df32"], x0, head, tail)
    rB = bpB.optimize(world["dev"]["3df32"], x0, head, tail)
    _check_flag(rA, bpA.cfg); _check_flag(rB, bpB.cfg)
    for k in ("x", "costs", "costs_last", "nit", "nfev", "status"):
        assert np.array_equal(rA[k], rB[k]), k
    wc = rA["costs_last"][:, 3] * ps.SETS["A"]["weights"][3]
    between = (rA["status"] <= 3) & (wc > 0.5) & (wc <= 40.0)
    print("weighted collision cost of the runs:", np.sort(wc))
    assert between.any()
    assert np.all(rB["collision"][between]) and not np.any(rA["collision"][between])


def test_params_set_refuses_bad_values_and_the_context_stays_usable(world):
    from neo_planner_amd import _lib
    ctx = world["ctx"]
    head, tail, wp, ts = ps.case_inputs("A", "3d", 3, 3)
    bp = _planner(world, "A", "f32")
    x = bp.pack_x(wp, ts)
    before = bp.cost_grad(world["dev"]["3df32"], x, head, tail)
    for bad in (dict(delta_t=0.0), dict(delta_t=-0.07), dict(delta_t=float("nan")), dict(T_max=0.33), dict(T_max=0.2),
                dict(maxls=0)):
        with pytest.raises(_lib.NeoError):
            ctx.set_params(**bad)
        after = bp.cost_grad(world["dev"]["3df32"], x, head, tail)      # (pushes the planner's own parameters again)
        for k in ("cost", "costs", "grad"):
            assert np.array_equal(before[k], after[k]), (bad, k)


# ------------------------------------------------------------------------------------------------ optimiser caps
CAPS = [dict(maxiter=1), dict(maxiter=3), dict(maxfun=1), dict(maxfun=6), dict(maxiter=4, maxfun=5)]
CAP = 128         # recorded evaluations per run (a capped run has at most four iterations; _expected_end checks that this is enough)


def _expected_end(it, nfev, nit, status, opts):
    """where csrc/neo_lbfgs.hpp ends a capped run, from the uncapped run's iteration column `it` (the accepted-iteration
    count at each of its first evaluations): iteration k ends with the last evaluation whose column is k - 1, and the run
    stops at the first such end with k >= maxiter or evaluations > maxfun -- STOP (NEO_TRAJ_MAXITER), tested before
    convergence as SciPy's driver does.  A run that ends on its own before that is unchanged."""
    maxiter, maxfun = opts.get("maxiter", 15000), opts.get("maxfun", 15000)
    for k in range(1, nit + 1):
        n_k = int((it[:min(nfev, len(it))] <= k - 1).sum())
        assert n_k < len(it) or n_k == nfev, "trace too short for this derivation"
        if k >= maxiter or n_k > maxfun:
            return n_k, k, 3
    return nfev, nit, status


@pytest.mark.parametrize("mode", ["f64", "f32x"])
@pytest.mark.parametrize("kind,M,D", [("3df32", 21, 3), ("2d", 3, 2)])
def test_capped_runs_are_prefixes_of_the_uncapped_run(world, mode, kind, M, D):
    name, B = "A", 24
    head, tail, wp, ts = _opt_inputs(name, kind[:2], M, D, B, 4)
    x0 = ps.pack_x(name, wp, ts)
    dmap = world["dev"][kind]
    full = _launch(world, _planner(world, name, mode), dmap, x0, head, tail, cap=CAP)
    w = np.asarray(ps.SETS[name]["weights"])
    n_capped = 0
    for opts in CAPS:
        r = _launch(world, _planner(world, name, mode, opts=opts), dmap, x0, head, tail, cap=CAP)
        for b in range(B):
            want = _expected_end(full["trace"][b, :, 3], int(full["nfev"][b]), int(full["nit"][b]), int(full["status"][b]), opts)
            got = (int(r["nfev"][b]), int(r["nit"][b]), int(r["status"][b]))
            assert got == want, (mode, kind, opts, b, got, want)
            E = min(got[0], CAP)
            assert np.array_equal(r["trace"][b, :E], full["trace"][b, :E]), (mode, kind, opts, b)
            assert np.array_equal(r["xg"][b, :E], full["xg"][b, :E]), (mode, kind, opts, b)
            if got[2] == 3:
                n_capped += 1
                assert E == got[0]
                # the run returns the accepted point of its last iteration -- the last recorded evaluation -- and its terms
                assert np.array_equal(r["x"][b], full["xg"][b, E - 1, 0]), (mode, kind, opts, b)
                f_last = full["trace"][b, E - 1, 0]
                assert abs(float(w @ r["costs_last"][b]) - f_last) <= ROUND[mode] * abs(f_last), (mode, kind, opts, b)
                assert np.array_equal(r["costs"][b], r["costs_last"][b])
    assert n_capped >= 4 * B, n_capped          # the caps were at work


@pytest.mark.parametrize("kind,M,D", [("3df32", 21, 3), ("2d", 3, 2)])
@pytest.mark.parametrize("opts", CAPS + [dict(maxls=2), dict(ftol=1e-2, gtol=1e-1)], ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_runs_with_options_follow_the_cpu_optimiser(world, kind, M, D, opts):
    """fp64 mode against oracle/cpu_native.optimize_batch (the host build of the same control flow on the fp64 oracle) with
    the same options: equal status, nit, nfev and x to 1e-8 for at least 75 % of the trajectories (the share
    test_gpu_parity.test_optimize_batch_matches_cpu_optimizer asks of short runs); the rest is reported.  In the all-fp32
    mode every run ends with a valid status, and looser tolerances do not lengthen a run.
    The start points (seed 4 of _opt_inputs) are those for which the CPU optimiser follows ITSELF best when its coefficients
    are perturbed by +-1 and +-5 ulp (make_params(coeff_eps=...)): at least 20 of 24 with every option set; the uncapped
    M = 21 runs with maxls = 2 take up to 440 evaluations and other seeds give 16 to 19 of 24 in that control."""
    from oracle import cpu_native as cn
    name, B = "A", 24
    head, tail, wp, ts = _opt_inputs(name, kind[:2], M, D, B, 4)
    x0 = ps.pack_x(name, wp, ts)
    dmap = world["dev"][kind]
    bp = _planner(world, name, "f64", opts=opts)
    r = _launch(world, bp, dmap, x0, head, tail)
    cpu = cn.optimize_batch(world["cn"][kind], x0, head, tail, M, D, params=cn.make_params(bp.cfg), threads=16)
    cpu_collision, cpu["status"] = (cpu["status"] & 0x100) != 0, cpu["status"] & 0xff
    same = (r["status"] == cpu["status"]) & (r["nit"] == cpu["nit"]) & (r["nfev"] == cpu["nfev"])
    dx = np.abs(r["x"] - cpu["x"]).max(axis=1) / np.abs(cpu["x"]).max(axis=1)
    same &= dx <= 1e-8
    print(kind, M, opts, "follow the CPU optimiser:", int(same.sum()), "of", B, "; the rest (b, gpu, cpu):",
          [(int(b), (int(r["status"][b]), int(r["nit"][b]), int(r["nfev"][b])), (int(cpu["status"][b]), int(cpu["nit"][b]), int(cpu["nfev"][b])))
           for b in np.flatnonzero(~same)])
    assert same.sum() >= 0.75 * B, (kind, M, opts, int(same.sum()))
    ended = same & (r["status"] <= 3)       # (a run that left the range of exp(-tau) has no cost terms at its last point)
    assert np.array_equal(r["collision"][ended], cpu_collision[ended])
    if "maxiter" in opts or "maxfun" in opts:
        assert (r["status"] == 3).sum() >= B // 2
    x = _launch(world, _planner(world, name, "f32x", opts=opts), dmap, x0, head, tail)
    if "ftol" in opts:
        d = _launch(world, _planner(world, name, "f32x"), dmap, x0, head, tail)
        assert np.all(x["nfev"] <= d["nfev"]), (x["nfev"], d["nfev"])
        assert x["nfev"].sum() < d["nfev"].sum()


def test_lane_group_kernel_with_caps_matches_the_default_kernel(world):
    """the lane-group kernel takes no trace: its capped runs against the default kernel's capped runs (2-D map, M = 3, both
    arithmetics) -- nit, nfev and status, and x to the kernels' fp32 bar, by the figures of
    test_gpu_parity.test_lane_groups_on_the_2d_reference_map_match_the_default_kernel: the same path for 90 % of the runs in
    fp64 and 40 % with fp32 sampling, x there to 1e-7 / 1e-3 relative (90 %)"""
    name, M, D, B = "A", 3, 2, 24
    head, tail, wp, ts = _opt_inputs(name, "2d", M, D, B, 1)
    x0 = ps.pack_x(name, wp, ts)
    for mode, xtol in (("f64", 1e-7), ("f32", 1e-3)):
        for opts in CAPS:
            a = _launch(world, _planner(world, name, mode, opts=opts), world["dev"]["2d"], x0, head, tail)
            g = _launch(world, _planner(world, name, mode, opts=opts, lane_groups=True), world["dev"]["2d"], x0, head, tail)
            same = (a["nit"] == g["nit"]) & (a["nfev"] == g["nfev"]) & (a["status"] == g["status"])
            assert same.mean() >= (0.9 if mode == "f64" else 0.4), (mode, opts, same.mean())
            dx = np.abs(a["x"][same] - g["x"][same]).max(axis=1) / np.abs(a["x"][same]).max(axis=1)
            assert np.quantile(dx, 0.9) <= xtol, (mode, opts, np.quantile(dx, 0.9))
            assert (g["status"] == 3).sum() >= B // 2


@pytest.mark.parametrize("mode", ["f64", "f32x"])
def test_maxfun_counts_over_all_launches_of_a_budgeted_run(world, mode):
    """include/neo_planner.h: maxiter and maxfun "count over all launches of a run" (neo_optimize_batch_budget_dev) -- state
    carried in the resume buffer.  maxfun = 40 with budgets of 3 and 17 evaluations per launch: the unbudgeted capped run,
    bit for bit."""
    name, M, D, B = "A", 21, 3, 48
    head, tail, wp, ts = _opt_inputs(name, "3d", M, D, B, 3)
    x0 = ps.pack_x(name, wp, ts)
    bp = _planner(world, name, mode, opts=dict(maxfun=40))
    ref = bp.optimize(world["dev"]["3df32"], x0, head, tail, order=False)
    _check_flag(ref, bp.cfg)
    assert (ref["status"] == 3).sum() >= B // 2 and ref["nfev"][ref["status"] == 3].min() > 40
    for budget in (3, 17):
        got = bp.optimize_budgeted(world["dev"]["3df32"], x0, head, tail, budget)
        for k in ("x", "costs", "costs_last", "nit", "nfev", "status", "collision"):
            assert np.array_equal(got[k], ref[k]), (mode, budget, k, int((got[k] != ref[k]).sum()))
        assert len(got["launch_sizes"]) == int((-(-ref["nfev"].astype(np.int64) // budget)).max())
