#!/usr/bin/env python3
"""Times the goal-route kernels (csrc/neo_track.hpp: neo_fleet_goal_route_dev, neo_fleet_hold_dev,
neo_fleet_track_audit_dev) and flies a fleet that chases moving goals next to the same fleet flying to fixed ones.

  kernels  the three kernels for 4096 missions: HIP events on the context's stream around 20 launches of each after 3
           warm-up launches, repeated 5 times: the median per launch, the smallest and the largest.  Routes of 4 vertices;
           every hold launch appends one replan period (60 rows) to every mission; the track audit takes the 401 samples
           of 2401 flown rows at stride 6.  neo_fleet_audit_batch_dev over the same rows is timed next to it.
  fleet    4096 missions (8 scenes x 512, `draw_missions` starts) in mode `basic`, resident=True, flown twice: tracked for
           `--ticks` ticks along closed routes through three of the scene's drawn goals at 0.5 m/s, and towards their fixed
           goals -- one warm-up flight each, then `--flights` measured ones: the run time, the tick's plan / fleet / host
           split, and what the chase looked like (gaps, failed ticks)

Each part is one process; run them one after the other, every one under its own time limit, e.g.
  timeout -k 10 120 python tools/gpu_track_fleet_time.py kernels --json profiles/track_fleet.json && \\
  timeout -k 10 600 python tools/gpu_track_fleet_time.py fleet --json profiles/track_fleet.json
Prints one line per figure; --json PATH also writes them (both parts into one file)."""
import argparse, ctypes, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "neo-planner_amd"))
import numpy as np, torch
import neo_planner_amd as npa
from neo_planner_amd import synth, _lib
from neo_planner_amd.fleet import draw_missions
from neo_planner_amd.goal_routes import GoalRoutes

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["kernels", "fleet"])
ap.add_argument("--missions", type=int, default=4096)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--scenes", type=int, default=8)
ap.add_argument("--per-scene", type=int, default=512)
ap.add_argument("--ticks", type=int, default=40)
ap.add_argument("--flights", type=int, default=2)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--json", default=None)
a = ap.parse_args()

dev = torch.device("cuda", 0)
ctx = _lib.default_context()
p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None


def dump(obj):
    """both parts write into one file: the part's keys replace what the file held of them"""
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        old = json.load(open(a.json)) if os.path.exists(a.json) else {}
        old.update(obj)
        with open(a.json, "w") as f:
            json.dump(old, f, indent=1)


def spread(v):
    v = sorted(v)
    return dict(median=round(float(np.median(v)), 4), min=round(v[0], 4), max=round(v[-1], 4), n=len(v))


if a.what == "kernels":
    B, K, step, stride, hz = a.missions, 4, 60, 6, 60.0
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    rng = np.random.default_rng(0)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    m = npa.ESDF(ctx=ctx)
    m.occupancy_map_cb(synth.OccupancyGridMsg(synth.occupancy_2d(3)))
    routes = GoalRoutes(np.stack([rng.uniform(1.0, 29.0, B * K), rng.uniform(-14.0, 14.0, B * K)], 1), np.arange(B + 1) * K,
                        rng.uniform(0.2, 1.0, B), rng.integers(0, 2, B))
    d_v, d_rb, d_sp, d_cl = up(routes.vertices), up(routes.route_begin), up(routes.speed), up(routes.closed)
    n_launch = a.repeats * (a.warmup + a.launches)
    cap = max((n_launch + 2) * step, 2401)
    cmd = torch.zeros((B, cap, 3, 2), dtype=torch.float64, device=dev)
    cmd[:, :2401] = up(rng.uniform(-10.0, 25.0, (B, 1, 3, 2))) + 0.01 * torch.randn((B, 2401, 3, 2), dtype=torch.float64, device=dev)
    goal = torch.zeros((B, 2), dtype=torch.float64, device=dev)
    n_flown = torch.full((B,), 2401, dtype=torch.int32, device=dev)
    track = torch.zeros((B, _lib.NEO_TRACK_FIELDS), dtype=torch.float64, device=dev)
    audit = torch.zeros((B, _lib.NEO_AUDIT_FIELDS), dtype=torch.float64, device=dev)
    count, flags = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(2))
    # the hold: launch k finds every mission on row k * step of an array that ends there, and appends one period
    cmd_len = torch.ones(B, dtype=torch.int32, device=dev)
    idx = [torch.full((B,), k * step, dtype=torch.int32, device=dev) for k in range(n_launch)]
    hold_flags = torch.zeros(B, dtype=torch.int32, device=dev)
    nth = [0]
    L, h = ctx.lib, ctx.h
    t_goal = [0.0]

    def k_goal():
        t_goal[0] += 1.0
        ctx.check(L.neo_fleet_goal_route_dev(h, B, None, 0, p(d_v), B * K, p(d_rb), p(d_sp), p(d_cl), t_goal[0], p(goal)))

    def k_hold():
        ctx.check(L.neo_fleet_hold_dev(h, B, None, 0, p(cmd), cap, p(cmd_len), p(idx[nth[0]]), step, p(hold_flags)))
        nth[0] += 1

    k_track = lambda: ctx.check(L.neo_fleet_track_audit_dev(h, B, None, 0, p(cmd), cap, p(n_flown), stride, hz, p(d_v), B * K, p(d_rb),
                                                            p(d_sp), p(d_cl), 1.0, p(track), p(count), p(flags)))
    k_audit = lambda: ctx.check(L.neo_fleet_audit_batch_dev(h, m.scene_id, None, B, None, 0, p(cmd), cap, p(n_flown), stride, hz, None,
                                                            p(audit), p(count), p(flags)))

    def events(fn):
        torch.cuda.synchronize(dev)
        for _ in range(a.warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.launches):
            fn()
        e1.record(stream)
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / a.launches      # microseconds a launch

    res = dict(missions=B, route_vertices=K, step=step, samples=401, launches=a.launches, warmup=a.warmup, repeats=a.repeats)
    for name, fn in (("goal", k_goal), ("track_audit", k_track), ("flight_audit", k_audit), ("hold", k_hold)):
        res[name + "_us"] = spread([events(fn) for _ in range(a.repeats)])
        s = res[name + "_us"]
        print(f"{name}: {s['median']:.2f} us a launch of {B} missions (median of {s['n']} x {a.launches} launches, {s['min']:.2f} - "
              f"{s['max']:.2f})", flush=True)
    assert int(cmd_len.min().item()) == int(cmd_len.max().item()) == (n_launch - 1) * step + step + 1 and not hold_flags.any().item()
    ctx.set_stream(None)
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    dump(dict(kernels=res))
    sys.exit(0)

# ---- fleet
maps = []
for s in range(a.scenes):
    m = npa.ESDF(ctx=ctx)
    m.occupancy_map_cb(synth.OccupancyGridMsg(synth.occupancy_2d(s)))
    maps.append(m)
bp = npa.BatchPlanner(ctx=ctx)
start, goals, sids = draw_missions(maps, a.per_scene, seed=a.seed)
B = len(goals)
# a mission's route: its own drawn goal, then two other drawn goals of its scene, and back (closed), at 0.5 m/s
rng = np.random.default_rng([a.seed, 0x7AC])
other = np.stack([s * a.per_scene + rng.integers(0, a.per_scene, (a.per_scene, 2)) for s in range(a.scenes)]).reshape(B, 2)
routes = GoalRoutes(np.stack([goals, goals[other[:, 0]], goals[other[:, 1]]], 1).reshape(-1, 2), np.arange(B + 1) * 3,
                    np.full(B, 0.5), np.ones(B, np.int32))


def fly(tracked):
    kw = dict(goal_routes=routes) if tracked else {}
    loop = npa.FleetReplanLoop(bp, maps[0], None if tracked else goals, mode="basic", scene_ids=sids, seed=a.seed, resident=True, **kw)
    t0 = time.perf_counter()
    out = loop.run(start, max_replans=a.ticks)
    return loop, out, time.perf_counter() - t0


res = dict(missions=B, scenes=a.scenes, seed=a.seed, flights=a.flights, ticks=a.ticks, fleets={})
for name, tracked in (("tracked", True), ("fixed_goal", False)):
    fly(tracked)                                       # warm-up: first-use allocations and caches
    walls, splits = [], []
    for _ in range(a.flights):
        loop, out, wall = fly(tracked)
        ticks = loop.timings
        walls.append(wall)
        splits.append({k: 1e3 * sum(t.get(k, 0.0) for t in ticks) / len(ticks) for k in ("tick_s", "plan_s", "fleet_s", "host_s")})
    r = dict(ticks=len(ticks), wall_s=spread(walls), per_tick_ms={k: spread([s[k] for s in splits]) for k in splits[0]},
             active_last_tick=int(ticks[-1]["active"]), plan_rounds=int(sum(t["plans"] for t in ticks)),
             plan_requests=int(sum(t["plan_requests"] for t in ticks)), plans_per_mission=round(float(out["replans"].mean()), 3),
             iterations_per_mission=round(float(out["iter_num"].mean()), 2), success_rate=round(float(out["success"].mean()), 4),
             failed_attempts=int(out["failed_attempts"].sum()), abandoned=int(out["abandoned"].sum()),
             metric_fail=int(out["metric_fail"].sum()), cmd_full=int(((out["flags"] & _lib.NEO_FLEET_FLAG_CMD_FULL) != 0).sum()),
             median_weighted_metric=round(float(np.nanmedian(out["weighted"])), 4), audit_ms=round(1e3 * loop.audit_s, 3))
    if tracked:
        r.update(track_audit_ms=round(1e3 * loop.track_audit_s, 3), failed_ticks=int(out["failed_ticks"].sum()),
                 missions_with_a_failed_tick=int((out["failed_ticks"] > 0).sum()),
                 median_gap_mean=round(float(np.nanmedian(out["track_gap_mean"])), 3),
                 median_gap_min=round(float(np.nanmedian(out["track_gap_min"])), 3),
                 median_gap_final=round(float(np.nanmedian(out["track_gap_final"])), 3),
                 median_frac_within=round(float(np.nanmedian(out["track_frac_within"])), 3),
                 caught_up=round(float((out["track_t_first_within"] >= 0).mean()), 4))
    pt = r["per_tick_ms"]
    print(f"{name}: run {r['wall_s']['median']:.3f} s ({r['wall_s']['min']:.3f} - {r['wall_s']['max']:.3f}), {r['ticks']} ticks, a tick "
          f"{pt['tick_s']['median']:.2f} ms (plan {pt['plan_s']['median']:.2f}, fleet {pt['fleet_s']['median']:.2f}, host "
          f"{pt['host_s']['median']:.2f}); {r['plans_per_mission']} plans a mission, {r['plan_requests']} plan requests, "
          f"{r['failed_attempts']} failed attempts, success {100 * r['success_rate']:.1f} %, still active at the last tick "
          f"{r['active_last_tick']}; " + (f"failed ticks {r['failed_ticks']}, median gap mean {r['median_gap_mean']} m, final "
                                          f"{r['median_gap_final']} m, within the radius {r['median_frac_within']} of the samples, "
                                          f"{100 * r['caught_up']:.1f} % caught up once" if tracked else ""), flush=True)
    res["fleets"][name] = r
    dump(res)
