#!/usr/bin/env python3
"""Times the resident geo warm start (neo_geo_guess_dev, neo_geo.hpp; BatchGeoPlanner, FleetReplanLoop(mode="geo", geo=...)).

  search    the search alone: --batch requests with 5 m local targets on a static forest map (scene 0), through
            neo_geo_guess_dev on head / tail (B, 3, 2) -- masked and direct ALTERNATING in one session, HIP events around
            each launch, --reps launches each after --warm warm-up launches of each form -- and, beside them, the dense
            masked entry point (neo_geo_search_batch_dev, what the figure of DESIGN section 5 was taken with).  The three
            give equal key nodes (checked).
  fleet     a fleet in mode geo, 8 scenes x 512 goals at 25 - 30 m: the host form (geo_plan through the host) against
            geo=BatchGeoPlanner, jitter numpy and counter, every configuration flown once as a warm-up and then --laps
            times timed, host and resident alternating; per lap the median and mean tick time and the plan step's share,
            over the laps the median and the spread, and that both forms flew the same flights (every result array)
  onboard   geo on onboard maps (geo=, the direct search) against basic on onboard maps, the experiment of
            tools/gpu_onboard_time.py fleet: tick time, goals reached, unsafe share; the resident basic form beside them;
            --masked adds geo= with the masked search (meant for a smaller fleet: --per-scene 64)

Each step is one process: run them one after the other, every one under its own time limit, e.g.
  timeout -k 10 300 python tools/gpu_geo_fleet_time.py search --json profiles/geo_resident.json && \\
  timeout -k 10 600 python tools/gpu_geo_fleet_time.py fleet --json profiles/geo_resident.json && \\
  timeout -k 10 600 python tools/gpu_geo_fleet_time.py onboard --json profiles/geo_resident.json && \\
  timeout -k 10 600 python tools/gpu_geo_fleet_time.py onboard --per-scene 64 --masked --key onboard_512 --json profiles/geo_resident.json
Prints one line per figure; --json PATH keeps every step's figures under its name in one file."""
import argparse, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "neo-planner_amd"))
import numpy as np, torch
import neo_planner_amd as npa
from neo_planner_amd import synth, _lib
from neo_planner_amd.depth import DepthCamera
from neo_planner_amd.fleet import draw_missions
from neo_planner_amd.geo_resident import BatchGeoPlanner
from neo_planner_amd.onboard import OnboardMapper

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["search", "fleet", "onboard"])
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--scenes", type=int, default=8)
ap.add_argument("--per-scene", type=int, default=512)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--size", default="640x480")
ap.add_argument("--max-replans", type=int, default=60)
ap.add_argument("--laps", type=int, default=3, help="fleet: timed runs of every configuration")
ap.add_argument("--masked", action="store_true", help="onboard: fly geo= with the masked search as well (a mask per map and tick)")
ap.add_argument("--key", default=None, help="the step's name in the --json file (default: the step)")
ap.add_argument("--json", default=None)
a = ap.parse_args()

dev = torch.device("cuda", 0)
ctx = _lib.default_context()


def dump(step, obj):
    if not a.json:
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    doc = {}
    if os.path.exists(a.json):
        with open(a.json) as f:
            doc = json.load(f)
    doc[a.key or step] = obj
    with open(a.json, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def scene_map(s):
    m = npa.ESDF(ctx=ctx)
    m.occupancy_map_cb(synth.OccupancyGridMsg(synth.occupancy_2d(s)))
    return m


def spread(ms):
    return dict(median=round(float(np.median(ms)), 4), min=round(float(min(ms)), 4), max=round(float(max(ms)), 4), all=[round(v, 4) for v in ms])


if a.what == "search":
    stream = torch.cuda.Stream()          # (not the null stream: its handle 0 would hand the context back its own stream)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    m = scene_map(0)
    bp = npa.BatchPlanner(ctx=ctx)
    rng = np.random.default_rng(42)
    B = a.batch
    head, tail = np.zeros((B, 3, 2)), np.zeros((B, 3, 2))
    k = 0
    while k < B:         # tools/gpu_geo_time.py's local requests: free starts, 5 m towards a random goal
        s = np.array([rng.uniform(0.5, 29.5), rng.uniform(-14.5, 14.5)])
        if m.esdf_map[int((s[1] + 15.0) / 0.1), int(s[0] / 0.1)] < 0.6:
            continue
        goal = np.array([rng.uniform(0.0, 30.0), rng.uniform(-15.0, 15.0)])
        if np.linalg.norm(goal - s) < 5.0:
            continue
        head[k, 0], tail[k, 0] = s, s + 5.0 * (goal - s) / np.linalg.norm(goal - s)
        k += 1
    d_head, d_tail = torch.from_numpy(head).to(dev), torch.from_numpy(tail).to(dev)
    st, tg = d_head[:, 0].contiguous(), d_tail[:, 0].contiguous()
    forms = {"masked": BatchGeoPlanner(bp, direct=False), "direct": BatchGeoPlanner(bp, direct=True)}
    kp = torch.zeros((B, 4, 2), dtype=torch.float64, device=dev)
    cost = torch.zeros(B, dtype=torch.float64, device=dev)
    plen, nexp, flags = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3))
    stream.synchronize()
    calls = {name: (lambda g=g: g.warm_start_dev(m, d_head, d_tail)) for name, g in forms.items()}
    calls["dense_masked"] = lambda: bp.geo_init_dev(m, st, tg, kp, plen, cost, nexp, flags)
    for _ in range(a.warm):
        for call in calls.values():
            call()
    ctx.synchronize()
    ms = {name: [] for name in calls}
    for _ in range(a.reps):
        for name, call in calls.items():        # alternating: whatever else the machine does meets every form alike
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    keys = {name: g.key_pts.cpu().numpy() for name, g in forms.items()}
    assert np.array_equal(keys["masked"], keys["direct"]) and np.array_equal(keys["masked"], kp.cpu().numpy())
    assert np.array_equal(forms["masked"].x0.cpu().numpy(), forms["direct"].x0.cpu().numpy())
    n = forms["direct"].expansions.cpu().numpy()
    f = forms["direct"].flags.cpu().numpy()
    res = dict(batch=B, scene=0, warm=a.warm, reps=a.reps, ms={name: spread(v) for name, v in ms.items()},
               expansions={str(q): float(np.percentile(n, q)) for q in (50, 90, 100)},
               no_path=int(((f & _lib.NEO_GEO_FLAG_NO_PATH) != 0).sum()), mask_builds=forms["direct"].mask_builds())
    for name, v in res["ms"].items():
        print(f"{name:>12}: median {v['median']:.2f} ms, min {v['min']:.2f}, max {v['max']:.2f} a launch of {B} requests", flush=True)
    ctx.set_stream(None)
    dump("search", res)
    sys.exit(0)


def tick_figures(loop, out, wall):
    ticks = loop.timings
    tick_ms = [1e3 * t["tick_s"] for t in ticks]
    plan_ms = [1e3 * t["plan_s"] for t in ticks]
    full = [1e3 * t["tick_s"] for t in ticks if t["active"] == loop.B and t["tick"] > 0]      # every mission still planning
    unsafe = (out["audit_flags"] & _lib.NEO_AUDIT_FLAG_UNSAFE) != 0
    return dict(missions=loop.B, wall_s=round(wall, 3), ticks=len(ticks), tick_ms_median=round(float(np.median(tick_ms)), 3),
                tick_ms_mean=round(float(np.mean(tick_ms)), 3), plan_ms_median=round(float(np.median(plan_ms)), 3),
                plan_ms_mean=round(float(np.mean(plan_ms)), 3),
                full_fleet_tick_ms_median=round(float(np.median(full)), 3) if full else None, full_fleet_ticks=len(full),
                success_rate=float(out["success"].mean()), unsafe_share=float(unsafe.mean()),
                metric_fail=int(out["metric_fail"].sum()), abandoned=int(out["abandoned"].sum()),
                plans_per_mission=float(out["replans"].mean()), failed_attempts_per_mission=float(out["failed_attempts"].mean()),
                sense_ms_mean=round(float(np.mean([1e3 * t.get("sense_s", 0.0) for t in ticks])), 3))


maps = [scene_map(s) for s in range(a.scenes)]
start, goals, sids = draw_missions(maps, a.per_scene, seed=0)
B = len(goals)

if a.what == "fleet":
    def fly(resident, jitter):
        bp = npa.BatchPlanner(ctx=ctx)
        loop = npa.FleetReplanLoop(bp, maps[0], goals, mode="geo", scene_ids=sids, seed=0, jitter=jitter,
                                   geo=BatchGeoPlanner(bp) if resident else None)
        t0 = time.perf_counter()
        out = loop.run(start, max_replans=a.max_replans)
        return loop, out, time.perf_counter() - t0

    runs = []
    for jitter in ("numpy", "counter"):
        outs, laps = {}, {False: [], True: []}
        for lap in range(-1, a.laps):         # lap -1: the warm-up
            for resident in (False, True):        # alternating
                loop, out, wall = fly(resident, jitter)
                if lap >= 0:
                    laps[resident].append(tick_figures(loop, out, wall))
                    outs[resident] = out
        for resident in (False, True):
            med = [r["tick_ms_median"] for r in laps[resident]]
            res = dict(form="geo=" if resident else "host", jitter=jitter, laps=a.laps, tick_ms_median_of_laps=round(float(np.median(med)), 3),
                       tick_ms_median_by_lap=med, tick_ms_mean_by_lap=[r["tick_ms_mean"] for r in laps[resident]],
                       plan_ms_median_by_lap=[r["plan_ms_median"] for r in laps[resident]],
                       wall_s_by_lap=[r["wall_s"] for r in laps[resident]], **laps[resident][-1])
            runs.append(res)
            print(f"geo {res['form']:>4} {jitter:>7}: {B} missions, {res['ticks']} ticks; tick median over {a.laps} laps "
                  f"{res['tick_ms_median_of_laps']:.1f} ms (by lap {med}), tick mean by lap {res['tick_ms_mean_by_lap']}, plan step "
                  f"median by lap {res['plan_ms_median_by_lap']}; success {res['success_rate']:.3f}", flush=True)
        same = all(np.array_equal(np.asarray(outs[True][k]), np.asarray(outs[False][k]), equal_nan=True) for k in outs[False])
        print(f"{jitter}: the two forms flew the same flights: {same}", flush=True)
        runs.append(dict(jitter=jitter, same_flights=bool(same)))
    dump("fleet", dict(scenes=a.scenes, per_scene=a.per_scene, max_replans=a.max_replans, runs=runs))
    sys.exit(0)

# ---- onboard: geo (resident, the direct search) against basic, both on the missions' own maps
W, H = (int(v) for v in a.size.split("x"))
cam = DepthCamera(ctx, width=W, height=H)
scenes = [DepthCamera.boxes_of(synth.forest_boxes(s)) for s in range(a.scenes)]
boxes, begin = DepthCamera.pack_scenes(scenes)
scene_index = (np.arange(B) // a.per_scene).astype(np.int32)
mapper = OnboardMapper(ctx, cam, B)
probe = BatchGeoPlanner(npa.BatchPlanner(ctx=ctx))
runs = []
for lap in ("warm-up", "timed"):
    forms = [("basic", dict(mode="basic")), ("basic resident", dict(mode="basic", resident=True)), ("geo=", dict(mode="geo"))]
    if a.masked:
        forms.append(("geo= masked", dict(mode="geo")))
    for name, kw in forms:
        bp = npa.BatchPlanner(ctx=ctx)
        if kw["mode"] == "geo":
            kw = dict(kw, geo=BatchGeoPlanner(bp, direct=False if name == "geo= masked" else None))
        loop = npa.FleetReplanLoop(bp, maps[0], goals, scene_ids=sids, seed=0, onboard=mapper, scenes=(boxes, begin),
                                   scene_index=scene_index, **kw)
        n0 = probe.mask_builds()
        t0 = time.perf_counter()
        out = loop.run(start, max_replans=a.max_replans)
        wall = time.perf_counter() - t0
        if lap == "timed":
            res = dict(form=name, size=a.size, mask_builds=probe.mask_builds() - n0, **tick_figures(loop, out, wall))
            runs.append(res)
            print(f"onboard {name:>14}: {B} missions, {res['ticks']} ticks in {wall:.2f} s; tick median {res['tick_ms_median']:.1f} ms "
                  f"(mean {res['tick_ms_mean']:.1f}; sensing {res['sense_ms_mean']:.1f}, plan step mean {res['plan_ms_mean']:.1f}); "
                  f"success {res['success_rate']:.3f}, unsafe {res['unsafe_share']:.3f}, abandoned {res['abandoned']}, "
                  f"metric_fail {res['metric_fail']}, masks built {res['mask_builds']}", flush=True)
dump("onboard", dict(scenes=a.scenes, per_scene=a.per_scene, max_replans=a.max_replans, runs=runs))
