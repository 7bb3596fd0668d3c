#!/usr/bin/env python3
"""Times the fleet's `warmstart` mode (neo_fleet_warm_guess_dev, neo_fleet_warm_carry_dev; FleetReplanLoop
mode="warmstart") and flies fleets on it next to mode `basic`.

  kernels  the two kernels for 4096 missions, M = 3: HIP events on the context's stream around 20 launches of each after
           3 warm-up launches, repeated 5 times: the median per launch, the smallest and the largest
  fleet    4096 missions (8 scenes x 512, goals drawn at 25 - 30 m, as profiles/fleet_basic.json) flown in mode `basic`
           with resident=True and in mode `warmstart` in turn, each with jitter "numpy" and "counter": one warm-up flight,
           then `--flights` measured ones of the same missions (the flights are deterministic: the same flight every
           time, so only the clock varies) -- the median run time with its spread, the tick's plan / fleet / host split,
           iterations and optimiser runs a mission, success, failed attempts, abandoned and the median weighted metric

Each part is one process; run them one after the other, every one under its own time limit, e.g.
  timeout -k 10 120 python tools/gpu_warm_fleet_time.py kernels --json profiles/fleet_warmstart.json && \\
  timeout -k 10 600 python tools/gpu_warm_fleet_time.py fleet --json profiles/fleet_warmstart.json
Prints one line per figure; --json PATH also writes them (both parts into one file)."""
import argparse, ctypes, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "neo-planner_amd"))
import numpy as np, torch
import neo_planner_amd as npa
from neo_planner_amd import synth, _lib
from neo_planner_amd.fleet import draw_missions

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["kernels", "fleet"])
ap.add_argument("--missions", type=int, default=4096)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--scenes", type=int, default=8)
ap.add_argument("--per-scene", type=int, default=512)
ap.add_argument("--max-replans", type=int, default=60)
ap.add_argument("--flights", type=int, default=3)
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
    B, M = a.missions, 3
    count, n = M - 1, 3 * M - 2
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    rng = np.random.default_rng(0)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    bp = npa.BatchPlanner(ctx=ctx)
    bp._sync()
    head = up(rng.uniform(-4, 30, (B, 3, 2)))
    x = up(np.concatenate([rng.uniform(-4, 30, (B, 2 * count)), rng.uniform(-3, 3, (B, M))], 1))
    solved = up((rng.random(B) < 0.9).astype(np.int32))
    status = up(np.where(rng.random(B) < 0.5, 1, 0x101).astype(np.int32))
    attempts = up(rng.integers(1, 6, B).astype(np.int32))
    wl, tc, x0 = (torch.zeros(s, dtype=torch.float64, device=dev) for s in ((B, 2, count), (B, M), (B, n)))
    init_ts = bp._batch_ts_tau(M - 1)[0]
    L, h = ctx.lib, ctx.h
    k_carry = lambda: ctx.check(L.neo_fleet_warm_carry_dev(h, B, None, 0, M, p(x), p(head), p(solved), p(status), p(attempts),
                                                           _lib.ptr(init_ts), p(wl), p(tc)))
    k_guess = lambda: ctx.check(L.neo_fleet_warm_guess_dev(h, B, None, 0, M, p(head), p(wl), p(tc), p(x0)))

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

    res = dict(missions=B, M=M, launches=a.launches, warmup=a.warmup, repeats=a.repeats)
    for name, fn in (("carry", k_carry), ("guess", k_guess)):
        res[name + "_us"] = spread([events(fn) for _ in range(a.repeats)])
        s = res[name + "_us"]
        print(f"{name}: {s['median']:.2f} us a launch of {B} missions (median of {s['n']} x {a.launches} launches, {s['min']:.2f} - "
              f"{s['max']:.2f})", flush=True)
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


def fly(mode, jitter):
    loop = npa.FleetReplanLoop(bp, maps[0], goals, mode=mode, scene_ids=sids, seed=a.seed, resident=True, jitter=jitter)
    t0 = time.perf_counter()
    out = loop.run(start, max_replans=a.max_replans)
    return loop, out, time.perf_counter() - t0


res = dict(missions=B, scenes=a.scenes, seed=a.seed, flights=a.flights, fleets={})
for mode in ("basic", "warmstart"):
    for jitter in ("numpy", "counter"):
        fly(mode, jitter)                                       # warm-up: first-use allocations and caches
        walls, splits = [], []
        for _ in range(a.flights):
            loop, out, wall = fly(mode, jitter)
            ticks = loop.timings
            walls.append(wall)
            splits.append({k: 1e3 * sum(t.get(k, 0.0) for t in ticks) / len(ticks) for k in ("tick_s", "plan_s", "fleet_s", "host_s")})
        ok = out["success"]
        r = dict(mode=mode, jitter=jitter, ticks=len(ticks), wall_s=spread(walls),
                 per_tick_ms={k: spread([s[k] for s in splits]) for k in splits[0]},
                 plan_rounds=int(sum(t["plans"] for t in ticks)), plan_requests=int(sum(t["plan_requests"] for t in ticks)),
                 iterations_per_mission=round(float(out["iter_num"].mean()), 2), opt_runs_per_mission=round(float(out["opt_runs"].mean()), 3),
                 iterations_per_run=round(float(out["iter_num"].sum()) / max(int(out["opt_runs"].sum()), 1), 2),
                 plans_per_mission=round(float(out["replans"].mean()), 3), success_rate=round(float(ok.mean()), 4),
                 failed_attempts=int(out["failed_attempts"].sum()), failed_attempts_per_mission=round(float(out["failed_attempts"].mean()), 3),
                 abandoned=int(out["abandoned"].sum()), metric_fail=int(out["metric_fail"].sum()),
                 median_weighted_metric=round(float(np.nanmedian(out["weighted"])), 4),
                 median_weighted_metric_successful=round(float(np.nanmedian(out["weighted"][ok])), 4) if ok.any() else None,
                 min_clearance_successful=round(float(out["min_clearance"][ok].min()), 4) if ok.any() else None,
                 mean_commands=round(float(out["n_cmd"].mean()), 1))
        pt = r["per_tick_ms"]
        print(f"{mode} / {jitter}: run {r['wall_s']['median']:.3f} s ({r['wall_s']['min']:.3f} - {r['wall_s']['max']:.3f}), {r['ticks']} "
              f"ticks, a tick {pt['tick_s']['median']:.2f} ms (plan {pt['plan_s']['median']:.2f}, fleet {pt['fleet_s']['median']:.2f}, host "
              f"{pt['host_s']['median']:.2f}); {r['iterations_per_mission']} iterations and {r['opt_runs_per_mission']} runs a mission "
              f"({r['iterations_per_run']} a run); {100 * r['success_rate']:.1f} % reach the goal, {r['failed_attempts']} failed attempts, "
              f"{r['abandoned']} abandoned; median weighted metric {r['median_weighted_metric']}", flush=True)
        res["fleets"][f"{mode}_{jitter}"] = r
        dump(res)
