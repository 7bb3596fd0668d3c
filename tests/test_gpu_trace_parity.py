"""
Per-evaluation oracle parity along whole runs, for every optimize_kernel instantiation dispatch_opt reaches.

tests/test_gpu_replay.py holds every evaluation of cfg2's runs (3-D, fp32 yz4 field, M = 21) to the fp64 CPU oracle and
re-derives every optimiser decision on the host.  The other instantiations -- about forty, chosen by mode, map kind,
field element, waves per SIMD, FLAT slots and lane layout (neo_abi.hip dispatch_opt, the neo_disp_opt*.hip units) -- were
held elsewhere to the FIRST evaluation of a run or to end-of-run statistics, which a kernel that drifts from evaluation 5
on passes as long as the chaotic run still ends somewhere plausible.  Most of these kernels carry state from one
evaluation to the next (fp32 L-BFGS pairs beyond n = 128, the all-fp32 kernels' multiplier reuse and lane-assignment
cache, the stale-T adjoint, the per-launch LDS staging), so a fault there shows only after the first evaluation.

Here each row of CASES names the launch_opt<...> instantiation it reaches and runs a small batch with
neo_optimize_trace + neo_optimize_trace_xg.  EVERY point the kernel evaluates is evaluated again by the fp64 CPU oracle
(oracle/cpu_native.eval_points) on the map the kernel reads (the 2-D reference map; a 3-D field as stored, fp16 values
widened) with the run's parameters (make_params(cfg, stale_T)), and value, gradient and sample count must agree to
test_gpu_replay.TOL of the mode.  Decision replay stays with cfg2; the end of every run is checked for consistency instead:
the traced launch is the untraced one bit for bit, costs4_last is the last evaluation, the returned x is a recorded point
and costs4 the oracle's cost terms there, the iteration counter never decreases.

Field layouts: one per element type (brick).  test_gpu_parity.py::test_every_layout_holds_the_same_numbers_and_gives_the_
same_bits makes the four layouts give the same bits as each other, so the layout does not enter the arithmetic checked here.

Boundary states: the 3-D requests have non-zero head and tail velocity and acceleration (the synthetic replan requests
leave three of those rows at zero), so every row of the boundary state enters every evaluation.

Counted exceptions, as in test_gpu_replay.py:
  * the all-fp32 mode forms T in fp32: an evaluation whose q = T / delta_t lies within fp32 rounding of an integer may use
    one sample more or fewer than the oracle -- identified by the recorded sample count, each within 2e-7 * max(q, 50) of a
    boundary (1e-5 at the default parameters, where q <= 50), rare;
  * gradient cell-face events of the fp32 modes: a sample whose fp32 position lies on the other side of a voxel face than
    the oracle's reads the neighbouring cell's gradient (the trilinear interpolant is continuous, its gradient is not);
  * on the 2-D NEAREST map the VALUE jumps at cell faces too (tests/helpers.py reference_jump): an fp32 sample position
    within ~1e-6 m of a face reads the neighbour's distance, up to res = 0.1 m away -- times the collision weight 1e4, and
    the neighbour's (piecewise constant) gradient.  Such an evaluation needs a sample inside the safety band that lands
    within fp32 rounding of a face: per sample ~2 * 1e-6 / 0.1 = 2e-5, at a few hundred samples per evaluation below 1 %
    of the evaluations.  An evaluation beyond the tolerance counts as one only if the oracle, at one of FACE_TRIALS points
    within fp32 rounding of x (relative noise 2^-22), gives the kernel's value and gradient to the tolerance; their share
    is bounded by MAX_FACE_SHARE_2D (the reason at the assertion).  The fp64 mode computes positions as the oracle does and
    is held without exceptions.
"""
import ctypes
import json
import os
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import param_sets as ps
from test_gpu_replay import TOL

pytestmark = pytest.mark.gpu

B, CAP = 10, 3000
MAX_FACE_SHARE_2D = 5e-2
FACE_NOISE, FACE_TRIALS = 2.0 ** -22, 32      # relative perturbations of x at fp32 rounding, per cell-face candidate
# (weighted sum of the cost terms against the recorded value: four non-negative terms, no cancellation -- a few
#  roundings of the mode's arithmetic)
ROUND = {"f64": 1e-13, "f32": 1e-6, "f32x": 1e-6}
FLAG_LANE_PIECE = 512          # flags bit 512: lane = piece even where D * M fits the wavefront (comparison runs)


def _k(D, NS, real, map_, lookup, waves, lg, num):
    return f"optimize_kernel<{D}, {NS}, {real}, {map_}, {lookup}, {waves}, {lg}, {num}, false>"


def k3(NS, real, waves, lg, num="double", elem="float"):
    """3-D field in the brick layout (Lookup3D<Real, element, 3>)"""
    return _k(3, NS, real, "Map3D", f"Lookup3D<{real}, {elem}, 3>", waves, lg, num)


def k2(D, NS, real, waves, lg, num="double"):
    """the 2-D reference map (nearest-cell Lookup2D)"""
    return _k(D, NS, real, "Map2D", f"Lookup2D<{real}>", waves, lg, num)


PD3, PD2, WL = "WaveLanesPD<3>", "WaveLanesPD<2>", "WaveLanes"


def case(name, inst, mode, M, waves=None, flags=0, stale_T=True, map="3d", store="f32", D=3, scenes=1, order=None, cfg=None):
    """cfg: None (the default parameters) or the name of a parameter set of tests/param_sets.py -- the run's parameters and
    the range its start durations are drawn from.
    inst: the optimize_kernel<D, NS, Real, MapT, LookupT, WAVES, LG, Num, BUDGET> that dispatch_opt's choice of
    launch_opt<D, Real, MapT, LookupT, WAVES, Num> launches for this shape (NS = ceil(n / 64), capped at 4; LG =
    WaveLanesPD<D> where D * M <= 64 and flags bit 512 is clear, else WaveLanes)"""
    return pytest.param(dict(name=name, inst=inst, mode=mode, M=M, waves=waves, flags=flags, stale_T=stale_T, map=map,
                             store=store, D=D, scenes=scenes, order=order, cfg=cfg), id=name)


CASES = [
    # ---- 3-D field, fp32 brick: launch_opt_3d_f64 (one wave) / _3d_f64_w2 (flag, NS <= 2)
    case("f64-w1-M3", k3(1, "double", 1, PD3), "f64", 3),
    case("f64-w1-M21", k3(2, "double", 1, PD3), "f64", 21),
    case("f64-w1-M22", k3(2, "double", 1, WL), "f64", 22),
    case("f64-w1-M41", k3(3, "double", 1, WL), "f64", 41),
    case("f64-w1-M64", k3(4, "double", 1, WL), "f64", 64),
    case("f64-w2-M3", k3(1, "double", 2, PD3), "f64", 3, waves=2),
    case("f64-w2-M21", k3(2, "double", 2, PD3), "f64", 21, waves=2),
    case("f64-w2-M32", k3(2, "double", 2, WL), "f64", 32, waves=2),
    case("f64-w1-M21-lane-piece", k3(2, "double", 1, WL), "f64", 21, flags=FLAG_LANE_PIECE),
    case("f64-w1-M21-fresh-T", k3(2, "double", 1, PD3), "f64", 21, stale_T=False),
    # ---- fp32 sampling, fp64 solve: launch_opt_3d_f32 / _3d_w2 (two waves: pairs in fp32 from NS 3, pairs_in_f32)
    case("f32-w1-M3", k3(1, "float", 1, PD3), "f32", 3),
    case("f32-w1-M21", k3(2, "float", 1, PD3), "f32", 21),
    case("f32-w1-M41", k3(3, "float", 1, WL), "f32", 41),
    case("f32-w1-M64", k3(4, "float", 1, WL), "f32", 64),
    case("f32-w2-M21", k3(2, "float", 2, PD3), "f32", 21, waves=2),
    case("f32-w2-M41", k3(3, "float", 2, WL), "f32", 41, waves=2),
    case("f32-w2-M64", k3(4, "float", 2, WL), "f32", 64, waves=2),
    # ---- all-fp32: launch_opt_3d_x (two waves always; M 3 / 16 / 21 / 34 / 41 / 64 bracket the fp32 reduction's
    #      five-level cap and the slot switches)
    case("f32x-M3", k3(1, "float", 2, PD3, "float"), "f32x", 3),
    case("f32x-M16", k3(1, "float", 2, PD3, "float"), "f32x", 16),
    case("f32x-M21", k3(2, "float", 2, PD3, "float"), "f32x", 21),
    case("f32x-M34", k3(3, "float", 2, WL, "float"), "f32x", 34),
    case("f32x-M41", k3(3, "float", 2, WL, "float"), "f32x", 41),
    case("f32x-M64", k3(4, "float", 2, WL, "float"), "f32x", 64),
    # (NEO_FLAG_ONE_WAVE_PER_SIMD: the one-wave all-fp32 kernel is an experiment, tools/probe/x_one_wave.patch, and in no
    #  product source; the product's dispatch keeps the two-waves kernel -- this row pins that the flag changes nothing else)
    case("f32x-M21-one-wave-flag", k3(2, "float", 2, PD3, "float"), "f32x", 21, waves=1),
    # ---- fp16 field (cfg5's store; M = 41 is cfg5's shape)
    case("f16-f64-M21", k3(2, "double", 1, PD3, elem="__half"), "f64", 21, store="f16"),
    case("f16-f64-M41", k3(3, "double", 1, WL, elem="__half"), "f64", 41, store="f16"),
    case("f16-f32-M21", k3(2, "float", 1, PD3, elem="__half"), "f32", 21, store="f16"),
    case("f16-f32-M41", k3(3, "float", 1, WL, elem="__half"), "f32", 41, store="f16"),
    case("f16-f32x-M21", k3(2, "float", 2, PD3, "float", elem="__half"), "f32x", 21, store="f16"),
    case("f16-f32x-M41", k3(3, "float", 2, WL, "float", elem="__half"), "f32x", 41, store="f16"),
    # ---- the 2-D reference map: launch_opt_2d / _2d_w2 (NS <= 2 only: M = 44 goes to one wave with the flag too) / _2d_x
    case("2d-f64-w1-M3", k2(2, 1, "double", 1, PD2), "f64", 3, map="2d", D=2),
    case("2d-f64-w2-M3", k2(2, 1, "double", 2, PD2), "f64", 3, waves=2, map="2d", D=2),
    case("2d-f64-w1-M21", k2(2, 1, "double", 1, PD2), "f64", 21, map="2d", D=2),
    case("2d-f64-w2-M21", k2(2, 1, "double", 2, PD2), "f64", 21, waves=2, map="2d", D=2),
    case("2d-f64-w1-M44", k2(2, 3, "double", 1, WL), "f64", 44, map="2d", D=2),
    case("2d-f64-w2flag-M44", k2(2, 3, "double", 1, WL), "f64", 44, waves=2, map="2d", D=2),
    case("2d-f32-w1-M3", k2(2, 1, "float", 1, PD2), "f32", 3, map="2d", D=2),
    case("2d-f32-w2-M3", k2(2, 1, "float", 2, PD2), "f32", 3, waves=2, map="2d", D=2),
    case("2d-f32-w1-M21", k2(2, 1, "float", 1, PD2), "f32", 21, map="2d", D=2),
    case("2d-f32-w2-M21", k2(2, 1, "float", 2, PD2), "f32", 21, waves=2, map="2d", D=2),
    case("2d-f32-w1-M44", k2(2, 3, "float", 1, WL), "f32", 44, map="2d", D=2),
    case("2d-f32x-M3", k2(2, 1, "float", 2, PD2, "float"), "f32x", 3, map="2d", D=2),
    case("2d-f32x-M21", k2(2, 1, "float", 2, PD2, "float"), "f32x", 21, map="2d", D=2),
    case("2d-f32x-M32", k2(2, 2, "float", 2, PD2, "float"), "f32x", 32, map="2d", D=2),
    # D = 3 on the 2-D map (z is free)
    case("2d-D3-f64-M21", k2(3, 2, "double", 1, PD3), "f64", 21, map="2d", D=3),
    case("2d-D3-f32x-M21", k2(3, 2, "float", 2, PD3, "float"), "f32x", 21, map="2d", D=3),
    # ---- indexing paths: two 3-D maps with per-trajectory slots; a reversed dispatch order
    case("scenes2-f64-M21", k3(2, "double", 1, PD3), "f64", 21, scenes=2),
    case("scenes2-f32x-M21", k3(2, "float", 2, PD3, "float"), "f32x", 21, scenes=2),
    case("reversed-f64-M21", k3(2, "double", 1, PD3), "f64", 21, order="reversed"),
    case("reversed-f32x-M21", k3(2, "float", 2, PD3, "float"), "f32x", 21, order="reversed"),
    # ---- away from the default parameters (tests/param_sets.py): one row per dispatch unit and set.  A: inexact 1 / delta_t,
    #      T_min no multiple of delta_t; B: up to 238 samples per piece (M <= 21); C: T_min = 4 delta_t, a zero weight
    case("A-f64-w1-M21", k3(2, "double", 1, PD3), "f64", 21, cfg="A"),
    case("B-f64-w1-M3", k3(1, "double", 1, PD3), "f64", 3, cfg="B"),
    case("C-f64-w1-M41", k3(3, "double", 1, WL), "f64", 41, cfg="C"),
    case("B-f64-w2-M21", k3(2, "double", 2, PD3), "f64", 21, waves=2, cfg="B"),
    case("B-f32-w1-M21", k3(2, "float", 1, PD3), "f32", 21, cfg="B"),
    case("A-f32-w1-M64", k3(4, "float", 1, WL), "f32", 64, cfg="A"),
    case("A-f32-w2-M41", k3(3, "float", 2, WL), "f32", 41, waves=2, cfg="A"),
    case("B-f32x-M3", k3(1, "float", 2, PD3, "float"), "f32x", 3, cfg="B"),
    case("A-f32x-M21", k3(2, "float", 2, PD3, "float"), "f32x", 21, cfg="A"),
    case("C-f32x-M34", k3(3, "float", 2, WL, "float"), "f32x", 34, cfg="C"),
    case("B-f16-f32x-M21", k3(2, "float", 2, PD3, "float", elem="__half"), "f32x", 21, store="f16", cfg="B"),
    case("A-2d-f64-w1-M21", k2(2, 1, "double", 1, PD2), "f64", 21, map="2d", D=2, cfg="A"),
    case("B-2d-f32-w1-M3", k2(2, 1, "float", 1, PD2), "f32", 3, map="2d", D=2, cfg="B"),
    case("B-2d-f32x-M21", k2(2, 1, "float", 2, PD2, "float"), "f32x", 21, map="2d", D=2, cfg="B"),
]


def _requests(rng, M, D, lo, hi):
    """start and goal at opposite ends of the box, every boundary row non-zero (test_gpu_parity._random_requests)"""
    head = np.zeros((B, 3, D)); tail = np.zeros((B, 3, D))
    head[:, 0] = rng.uniform(lo, lo + 0.2 * (hi - lo), (B, D))
    tail[:, 0] = rng.uniform(lo + 0.7 * (hi - lo), hi, (B, D))
    head[:, 1] = rng.normal(0, 0.4, (B, D)); head[:, 2] = rng.normal(0, 0.3, (B, D))
    tail[:, 1] = rng.normal(0, 0.4, (B, D)); tail[:, 2] = rng.normal(0, 0.3, (B, D))
    k = np.arange(1, M)[None, None, :] / M
    wp = head[:, 0, :, None] + (tail[:, 0] - head[:, 0])[:, :, None] * k + rng.normal(0, 0.5, (B, D, M - 1))
    ts = rng.uniform(0.8, 2.5, (B, M))
    return head, tail, wp, ts


def _field(shift):
    """32^3 field of test_every_boundary_row_reaches_every_optimiser_kernel: a floor ramp and one box (moved by `shift`
    cells in y for the second scene)"""
    n = 32
    dist = np.full((n, n, n), 4.0, np.float32)
    dist[:, :, :6] = np.linspace(0.0, 1.2, 6)[None, None, :]
    dist[10:14, 12 + shift:18 + shift, :] = 0.05
    return dist


RES3, ORIGIN3 = 0.4, (0.0, -6.4, 0.0)


@pytest.fixture(scope="module")
def world():
    from neo_planner_amd import _lib
    ctx = _lib.Context(0)
    return dict(ctx=ctx, maps={}, pool=ThreadPoolExecutor(16))


def _maps(world, kind, store, scenes):
    """(device maps, oracle maps) -- built once per module"""
    import neo_planner_amd as npa
    from neo_planner_amd import _lib, synth
    from oracle import cpu_native as cn
    from oracle import minco_np as onp
    key = (kind, store, scenes)
    if key not in world["maps"]:
        # (a multi-scene call wants every map of its kind in the context to share element type and layout: its own context)
        ctx = world["ctx"] if scenes == 1 else _lib.Context(0)
        if kind == "2d":
            occ = synth.occupancy_2d(3)
            m = npa.ESDF(ctx)
            m.occupancy_map_cb(synth.OccupancyGridMsg(occ))
            o = onp.GridESDF(occ, synth.RES, 300, 300, (0.0, -15.0))
            assert np.array_equal(m.esdf_map, o.esdf_map)
            world["maps"][key] = (ctx, [m], [cn.NativeMap.from_grid2d(o)])
        else:
            dev, ora = [], []
            for s in range(scenes):
                d = _field(8 * s)
                if store == "f16":
                    d = d.astype(np.float16).astype(np.float32)      # the values as stored: fp16 widened
                dev.append(npa.ESDF3D(d, RES3, ORIGIN3, store=store, layout="brick", ctx=ctx))
                ora.append(cn.NativeMap.from_field3d(d, RES3, ORIGIN3))
            world["maps"][key] = (ctx, dev, ora)
    return world["maps"][key]


def _traced_run(world, c):
    import torch
    import neo_planner_amd as npa
    from neo_planner_amd import _lib
    dev = torch.device("cuda", 0)
    M, D, mode = c["M"], c["D"], c["mode"]
    n = D * (M - 1) + M
    ctx, dmaps, omaps = _maps(world, c["map"], c["store"], c["scenes"])
    rng = np.random.default_rng(zlib.crc32(c["name"].encode()))
    if c["map"] == "2d":
        lo, hi = np.array([1.0, -10.0, 0.5])[:D], np.array([26.0, 10.0, 3.0])[:D]
    else:
        lo, hi = np.array([1.0, -5.0, 1.0]), np.array([11.5, 5.0, 10.0])
    head, tail, wp, ts = _requests(rng, M, D, lo, hi)
    config = None
    if c["cfg"] is not None:
        # (the default rows' 0.8 .. 2.5 s are no valid durations at every set: the set's own range, drawn after the rest)
        ts = ps.durations(rng, c["cfg"], (B, M), *ps.RUN_DUR[c["cfg"]])
        config = ps.planner_config(c["cfg"])
    bp = npa.BatchPlanner(config=config, ctx=ctx, sample_dtype=mode, stale_T=c["stale_T"], waves_per_simd=c["waves"])
    bp.flags |= c["flags"]
    bp._sync()
    x0 = bp.pack_x(wp, ts)
    t = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt)
    d_x0, d_h, d_t = t(x0), t(head), t(tail)
    scene = np.arange(B) % c["scenes"]
    d_slots = None
    if c["scenes"] > 1:
        slot = [int(ctx.lib.neo_scene_slot(ctx.h, m.scene_id)) for m in dmaps]
        assert min(slot) >= 0 and len(set(slot)) == len(slot)
        d_slots = t(np.array([slot[s] for s in scene], dtype=np.int32), torch.int32)
    perm = np.arange(B)[::-1].astype(np.int32).copy() if c["order"] == "reversed" else None

    def launch(trace):
        out = dict(x=torch.empty(B, n, dtype=torch.float64, device=dev), costs=torch.zeros(B, 4, dtype=torch.float64, device=dev),
                   last=torch.zeros(B, 4, dtype=torch.float64, device=dev), nit=torch.zeros(B, dtype=torch.int32, device=dev),
                   nfev=torch.zeros(B, dtype=torch.int32, device=dev), status=torch.zeros(B, dtype=torch.int32, device=dev))
        if trace:
            out["trace"] = torch.zeros(B, CAP, 4, dtype=torch.float64, device=dev)
            out["xg"] = torch.zeros(B, CAP, 2, n, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        ctx.check(ctx.lib.neo_optimize_dispatch_order_host(ctx.h, _lib.ptr(perm), 0 if perm is None else B))
        try:
            if trace:
                ctx.check(ctx.lib.neo_optimize_trace(ctx.h, ctypes.c_void_p(out["trace"].data_ptr()), CAP))
                ctx.check(ctx.lib.neo_optimize_trace_xg(ctx.h, ctypes.c_void_p(out["xg"].data_ptr()), CAP))
            bp.optimize_dev(dmaps[0], out["x"], d_h, d_t, out["costs"], out["last"], out["nit"], out["nfev"], out["status"],
                            slots=d_slots, x0=d_x0)
            ctx.synchronize()
        finally:
            ctx.check(ctx.lib.neo_optimize_trace(ctx.h, None, 0))
            ctx.check(ctx.lib.neo_optimize_trace_xg(ctx.h, None, 0))
            ctx.check(ctx.lib.neo_optimize_dispatch_order_host(ctx.h, None, 0))
        return out

    traced, plain = launch(True), launch(False)
    # the traced launch is THE run: the same launch without tracing returns the same bits
    for k in ("x", "nfev", "nit", "status", "costs", "last"):
        assert torch.equal(traced[k], plain[k]), (c["name"], k)
    nfev = traced["nfev"].cpu().numpy()
    E = int(nfev.max())
    assert 1 <= E <= CAP, (c["name"], E)          # every run's evaluations fit the trace
    r = {k: v.cpu().numpy() for k, v in traced.items() if k not in ("trace", "xg")}
    r["trace"] = traced["trace"][:, :E].cpu().numpy()
    r["xg"] = traced["xg"][:, :E].cpu().numpy()
    r.update(head=head, tail=tail, n=n, omaps=[omaps[s] for s in scene], cfg=bp.cfg)
    return r


def _check_run(args):
    """oracle side of one trajectory (ctypes releases the GIL: runs on the pool)"""
    from oracle import cpu_native as cn
    r, b, mode, M, D, params, tol, face = args
    nq = D * (M - 1)
    cfg = r["cfg"]
    E = int(r["nfev"][b])
    st = int(r["status"][b]) & 0xff
    xs, gs = r["xg"][b, :E, 0], r["xg"][b, :E, 1]
    fs, ns_d, it_d = r["trace"][b, :E, 0], r["trace"][b, :E, 2], r["trace"][b, :E, 3]
    # a run that ended on a range error / non-finite value: its last evaluation is where the reference raises
    Ec = E - 1 if st >= 4 else E
    ref = cn.eval_points(r["omaps"][b], xs[:Ec], r["head"][b], r["tail"][b], M, D, params)
    T = (cfg.T_max - cfg.T_min) / (1.0 + np.exp(-xs[:Ec, nq:])) + cfg.T_min
    ns_ref = np.floor(T / cfg.delta_t).sum(axis=1)
    same_ns = ns_ref == ns_d[:Ec]
    ok = ref["status"] == 0
    sel = ok & same_ns & np.isfinite(fs[:Ec])
    out = dict(E=E, Ec=Ec, status=st, n_eval=int(sel.sum()), n_bad=int((~ok).sum()), nonfinite=int((ok & ~np.isfinite(fs[:Ec])).sum()))
    rel_f = np.abs(fs[:Ec][sel] - ref["f"][sel]) / np.abs(ref["f"][sel])
    G = float(np.abs(ref["grad"][ok]).max()) if ok.any() else 1.0
    gmax = np.abs(ref["grad"][sel]).max(axis=1)
    dg = np.abs(gs[:Ec][sel] - ref["grad"][sel]).max(axis=1)
    rel_g = dg / G
    # nearest-map cell-face events (module docstring): an evaluation beyond the tolerance is one when the oracle, at a point
    # within fp32 rounding of x, gives the kernel's value AND gradient to the tolerance -- else it stays in the statistics
    keep = np.ones(len(rel_f), dtype=bool)
    faces = set()
    if face:
        idx = np.flatnonzero(sel)
        rng = np.random.default_rng(b)
        for j in np.flatnonzero((rel_f > tol["f"]) | (rel_g > tol["g"])):
            k = idx[j]
            xp = xs[k][None, :] * (1.0 + FACE_NOISE * rng.standard_normal((FACE_TRIALS, xs.shape[1])))
            pr = cn.eval_points(r["omaps"][b], xp, r["head"][b], r["tail"][b], M, D, params)
            ef = np.abs(fs[k] - pr["f"]) / np.abs(pr["f"])
            eg = np.abs(gs[k][None, :] - pr["grad"]).max(axis=1) / G
            if np.any((pr["status"] == 0) & (ef <= tol["f"]) & (eg <= tol["g"])):
                keep[j] = False
                faces.add(int(k))
    out["face_events"] = len(faces)
    out["rel_f"], out["rel_g"] = rel_f[keep], rel_g[keep]
    out["rel_g_own"] = (dg / np.maximum(gmax, 1e-300))[keep & (gmax >= 1e-2 * G)]
    near = []
    for k in np.flatnonzero(ok & ~same_ns):
        q = T[k] / cfg.delta_t
        e = np.abs(q - np.round(q))
        near.append((float(e.min()), float(q[np.argmin(e)])))
    out["ns_diff"], out["near_edge"] = len(near), near
    out["iter_monotone"] = bool(np.all(np.diff(it_d) >= 0))
    # ---- end of the run
    w = np.asarray(cfg.weights, dtype=np.float64)
    out["last_rel"] = None
    if st <= 3 and np.isfinite(fs[E - 1]):
        out["last_rel"] = float(abs(float(w @ r["last"][b]) - fs[E - 1]) / abs(fs[E - 1]))
    out["x_recorded"] = None
    out["final_rel"] = None
    if st <= 2:
        hit = np.flatnonzero(np.all(xs == r["x"][b][None, :], axis=1))
        out["x_recorded"] = bool(hit.size)
        fin = cn.eval_points(r["omaps"][b], r["x"][b][None, :], r["head"][b], r["tail"][b], M, D, params)
        Tf = (cfg.T_max - cfg.T_min) / (1.0 + np.exp(-r["x"][b][nq:])) + cfg.T_min
        # (compared where the kernel's evaluation at x used the oracle's sample count -- the recorded one)
        if fin["status"][0] == 0 and hit.size and ns_d[hit[0]] == np.floor(Tf / cfg.delta_t).sum() and int(hit[0]) not in faces:
            out["final_rel"] = float(np.abs(w * (r["costs"][b] - fin["costs"][0])).max() / abs(fin["f"][0]))
    return out


@pytest.mark.parametrize("c", CASES)
def test_every_evaluation_of_every_kernel_is_an_oracle_evaluation(world, c):
    from oracle import cpu_native as cn
    r = _traced_run(world, c)
    mode, M, D = c["mode"], c["M"], c["D"]
    tol = TOL[mode]
    params = cn.make_params(r["cfg"], stale_T=c["stale_T"])
    face_2d = c["map"] == "2d" and mode != "f64"
    runs = list(world["pool"].map(_check_run, [(r, b, mode, M, D, params, tol, face_2d) for b in range(B)]))
    cat = lambda k: np.concatenate([o[k] for o in runs])
    rel_f, rel_g, rel_g_own = cat("rel_f"), cat("rel_g"), cat("rel_g_own")
    n_eval = sum(o["n_eval"] for o in runs)
    n_face = sum(o["face_events"] for o in runs)
    ns_diff = sum(o["ns_diff"] for o in runs)
    near_edge = [e for o in runs for e in o["near_edge"]]
    last_rel = [o["last_rel"] for o in runs if o["last_rel"] is not None]
    final_rel = [o["final_rel"] for o in runs if o["final_rel"] is not None]
    q = lambda a: [float(np.quantile(a, p)) for p in (0.5, 0.9, 0.99, 0.999, 1.0)] if len(a) else []
    report = dict(case=c["name"], inst=c["inst"], mode=mode, M=M, D=D, params=c["cfg"] or "default", evaluations=n_eval,
                  nfev=[int(o["E"]) for o in runs], status=[o["status"] for o in runs],
                  value_rel_err_quantiles_50_90_99_999_max=q(rel_f), grad_err_over_run_scale_quantiles=q(rel_g),
                  grad_err_over_own_max_quantiles=q(rel_g_own),
                  value_over_tol=int((rel_f > tol["f"]).sum()), grad_over_tol=int((rel_g > tol["g"]).sum()),
                  grad_over_10tol=int((rel_g > 10 * tol["g"]).sum()),
                  cell_face_events_2d=n_face, evaluations_with_other_sample_count=ns_diff, their_distance_to_a_sample_boundary=near_edge,
                  oracle_range_errors_before_the_end=sum(o["n_bad"] for o in runs),
                  nonfinite_device_values=sum(o["nonfinite"] for o in runs),
                  costs4_last_vs_last_value_max=max(last_rel, default=None), costs4_vs_oracle_at_x_max=max(final_rel, default=None),
                  tolerances=tol)
    print(json.dumps(report))
    dump = os.environ.get("NEO_TRACE_REPORT")
    if dump:
        os.makedirs(dump, exist_ok=True)
        with open(os.path.join(dump, "trace_parity.jsonl"), "a") as f:
            f.write(json.dumps(report) + "\n")
    name = c["name"]
    assert n_eval >= 10 * B, (name, n_eval)
    # ---- every recorded evaluation against the oracle
    assert report["oracle_range_errors_before_the_end"] == 0 and report["nonfinite_device_values"] == 0, report
    # cell faces of the 2-D nearest map in the fp32 modes: each event is the oracle's value at a point within fp32 rounding
    # of x (_check_run), rare -- below 1 % of independent evaluations (module docstring), and a line search that has
    # collapsed onto a face repeats one for up to maxls = 20 evaluations: one such cluster in a case of >= 500 evaluations
    # adds 4 %.  The rest is held to the rules of every other case.
    assert n_face <= MAX_FACE_SHARE_2D * n_eval, (name, n_face, n_eval)
    assert (rel_f <= tol["f"]).all(), (name, report["value_rel_err_quantiles_50_90_99_999_max"])
    assert np.quantile(rel_f, 0.99) <= tol["f99"], (name, report["value_rel_err_quantiles_50_90_99_999_max"])
    assert np.quantile(rel_g, 0.999) <= tol["g"], (name, report["grad_err_over_run_scale_quantiles"])
    if mode == "f64":
        assert (rel_g <= tol["g"]).all(), (name, report["grad_err_over_run_scale_quantiles"])
    else:
        # cell-face events of the trilinear gradient: rare (test_gpu_replay: <= 2e-4 of the evaluations beyond ten times
        # the tolerance)
        assert (rel_g > 10 * tol["g"]).sum() <= 2e-4 * n_eval, (name, report["grad_over_10tol"])
    assert np.quantile(rel_g_own, 0.99) <= tol["g_own"], (name, report["grad_err_over_own_max_quantiles"])
    # sample counts: the oracle's int(T / delta_t) at every evaluation (the all-fp32 mode: counted boundary cases)
    # (the share: test_gpu_replay bounds it at 1e-3 on cfg2's requests; the random boundary states here drive some durations
    #  onto T_min = 5 delta_t, where T / delta_t is an integer at every evaluation of the line search: 1 %)
    # (the boundary test: an fp32 T * (1 / delta_t) carries a RELATIVE error, so the distance of q = T / delta_t to an integer
    #  is held to 2e-7 * max(q, 50) -- 1e-5 for every q the default parameters can give, q <= 50, and in proportion beyond:
    #  set B reaches q = 238)
    assert ns_diff <= 1e-2 * n_eval and all(e <= 2e-7 * max(q_, 50.0) for e, q_ in near_edge), (name, ns_diff, near_edge)
    if mode != "f32x":
        assert ns_diff == 0, (name, ns_diff)
    # ---- end of every run
    assert all(o["iter_monotone"] for o in runs), name
    assert all(v <= ROUND[mode] for v in last_rel), (name, max(last_rel))
    assert all(o["x_recorded"] for o in runs if o["x_recorded"] is not None), (name, "returned x is not a recorded point")
    assert len(final_rel) >= B // 2, (name, len(final_rel))
    assert max(final_rel) <= tol["f"], (name, final_rel)
