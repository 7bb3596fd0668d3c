#!/usr/bin/env python3
"""Times the learned warm start on resident arrays and flies fleets on it
(neo_init_motion_dev, neo_init_head_dev, neo_init_guess_dev; BatchNeoPlanner.warm_start_dev; FleetReplanLoop modes
"neo" and "nn").

  kernels  the three kernels for 4096 requests: HIP events on the context's stream around 20 launches of each after 3
           warm-up launches, and of the three in a row; next to the torch head path for the same rows (net.head on the
           same stream, also by events) and warm_start_dev(head_impl="torch") with its waits, by the wall clock
  fleet    512 missions (8 scenes x 64, goals drawn at 25 - 30 m, 160 x 120 camera) recorded in mode `batch` and a
           PlannerNet(120, 160) trained on the rows, as `gpu_record_time.py train` does; then 512 missions of another seed
           flown in mode `basic` with resident=True, `neo` with the trained network, `neo` with an untrained one and `nn`
           with the trained one (each flown once before as a warm-up): iterations an optimiser run, the tick's split,
           the share that reaches the goal and the audit's metric

Each part is one process; run them one after the other, every one under its own time limit, e.g.
  timeout -k 10 300 python tools/gpu_neo_fleet_time.py kernels --json profiles/neo_kernels.json && \\
  timeout -k 10 900 python tools/gpu_neo_fleet_time.py fleet --json profiles/neo_fleet.json
Prints one line per figure; --json PATH also writes them."""
import argparse, ctypes, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "neo-planner_amd"))
import numpy as np, torch
import neo_planner_amd as npa
from neo_planner_amd import synth, _lib, initializer as ini
from neo_planner_amd.depth import DepthCamera
from neo_planner_amd.fleet import draw_missions
from neo_planner_amd.record import DemoRecorder

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["kernels", "fleet"])
ap.add_argument("--requests", type=int, default=4096)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--scenes", type=int, default=8)
ap.add_argument("--per-scene", type=int, default=64)
ap.add_argument("--max-replans", type=int, default=60)
ap.add_argument("--epochs", type=int, default=5)
ap.add_argument("--batch-size", type=int, default=64)
ap.add_argument("--json", default=None)
a = ap.parse_args()

dev = torch.device("cuda", 0)
ctx = _lib.default_context()
p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None


def dump(obj):
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(obj, f, indent=1)


if a.what == "kernels":
    B = a.requests
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    rng = np.random.default_rng(0)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    yaw = rng.uniform(-np.pi, np.pi, B)
    pose = up(np.stack([rng.uniform(0, 30, B), rng.uniform(-15, 15, B), np.full(B, 2.0), np.cos(yaw), np.sin(yaw)], 1))
    vel, head, tail = up(rng.uniform(-2, 2, (B, 2))), up(rng.uniform(-4, 30, (B, 3, 2))), up(rng.uniform(-4, 30, (B, 3, 2)))
    feature = up(rng.normal(0, 1, (B, 24)).astype(np.float32))
    torch.manual_seed(0)
    net = ini.PlannerNet(24, 32).to(dev).eval()
    w = ini.pack_head_weights(net)
    motion = torch.zeros((B, 24), dtype=torch.float32, device=dev)
    out = torch.zeros((B, 9), dtype=torch.float32, device=dev)
    x0 = torch.zeros((B, 7), dtype=torch.float64, device=dev)
    L, h = ctx.lib, ctx.h
    npa.BatchPlanner(ctx=ctx)._sync()
    k_motion = lambda: ctx.check(L.neo_init_motion_dev(h, B, None, 0, p(pose), p(vel), p(head), p(tail), p(motion)))
    k_head = lambda: ctx.check(L.neo_init_head_dev(h, B, None, 0, p(w), w.numel(), p(feature), B, p(motion), p(out)))
    k_guess = lambda: ctx.check(L.neo_init_guess_dev(h, B, None, 0, p(out), p(pose), p(x0)))

    def all_three():
        k_motion(); k_head(); k_guess()

    def torch_head():
        with torch.no_grad():
            out.copy_(net.head(feature, motion))

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
        return e0.elapsed_time(e1) / a.launches

    res = dict(requests=B, launches=a.launches, warmup=a.warmup)
    for name, fn in (("motion", k_motion), ("head", k_head), ("guess", k_guess), ("motion_head_guess", all_three),
                     ("torch_head", torch_head)):
        res[name + "_ms"] = round(events(fn), 4)
        print(f"{name}: {res[name + '_ms']:.4f} ms for {B} requests", flush=True)
    res["head_gflops"] = round(2 * 20448 * B / (res["head_ms"] * 1e-3) / 1e9, 1)
    ctx.set_stream(None)
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    # the whole call as the fleet makes it, by the wall clock: the kernel path queues three launches, the torch path waits
    # for the context's stream, runs net.head on torch's and waits again
    neo = ini.BatchNeoPlanner(npa.BatchPlanner(ctx=ctx), ini.BatchInitializer(net, device=dev), DepthCamera(ctx, width=32, height=24))
    for impl in ("kernel", "torch"):
        for k in range(a.warmup + a.launches):
            if k == a.warmup:
                ctx.synchronize()
                t0 = time.perf_counter()
            neo.warm_start_dev(pose, vel, head, tail, feature, head_impl=impl)
        ctx.synchronize()
        res["warm_start_dev_" + impl + "_wall_ms"] = round(1e3 * (time.perf_counter() - t0) / a.launches, 4)
        print(f"warm_start_dev(head_impl={impl!r}): {res['warm_start_dev_' + impl + '_wall_ms']:.4f} ms a call by the wall clock", flush=True)
    dump(res)
    sys.exit(0)

# ---- fleet: record, train, fly
W, H = 160, 120
cam = DepthCamera(ctx, width=W, height=H)
scenes = [DepthCamera.boxes_of(synth.forest_boxes(s)) for s in range(a.scenes)]
packed = DepthCamera.pack_scenes(scenes)
maps = []
for s in range(a.scenes):
    m = npa.ESDF(ctx=ctx)
    m.occupancy_map_cb(synth.OccupancyGridMsg(synth.occupancy_2d(s)))
    maps.append(m)
bp = npa.BatchPlanner(ctx=ctx)
Bf = a.scenes * a.per_scene


def fly(seed, mode, **kw):
    start, goals, sids = draw_missions(maps, a.per_scene, seed=seed)
    scene_index = (np.arange(len(goals)) // a.per_scene).astype(np.int32)
    if kw.get("record") is not None or kw.get("neo") is not None:
        kw.update(scenes=packed, scene_index=scene_index)
    loop = npa.FleetReplanLoop(bp, maps[0], goals, mode=mode, scene_ids=sids, seed=seed, **kw)
    t0 = time.perf_counter()
    out = loop.run(start, max_replans=a.max_replans)
    return loop, out, time.perf_counter() - t0


rec = DemoRecorder(cam, capacity=Bf * (a.max_replans + 4), M=3, ctx=ctx)
_, flown, _ = fly(0, "batch", record=rec)
inputs, labels = rec.training_tensors(rec.rows())
t0 = time.perf_counter()
torch.manual_seed(42)
net, losses, held_out = npa.train_initializer(inputs, labels, net=ini.PlannerNet(H, W), epochs=a.epochs, batch_size=a.batch_size,
                                              device=dev)
res = dict(missions=Bf, size=f"{W}x{H}", recorded=dict(mode="batch", seed=0, rows=rec.n_rows, dropped=rec.dropped,
                                                         success_rate=float(flown["success"].mean())),
           train=dict(rows=int(inputs.shape[0]), epochs=a.epochs, batch_size=a.batch_size, seconds=round(time.perf_counter() - t0, 1),
                      loss_per_epoch=[round(v, 5) for v in losses], held_out_mse=round(held_out, 5)), test_seed=1, fleets={})
print(f"recorded {rec.n_rows} rows, trained {a.epochs} epochs: held out {held_out:.4f}", flush=True)
del inputs, rec
torch.cuda.empty_cache()
dump(res)

torch.manual_seed(7)
make = lambda the_net: ini.BatchNeoPlanner(bp, ini.BatchInitializer(net=the_net, device=dev, T_min=bp.cfg.T_min, T_max=bp.cfg.T_max), cam)
trained, untrained = make(net), make(ini.PlannerNet(H, W))
for name, mode, kw in (("basic_resident", "basic", dict(resident=True)), ("neo_trained", "neo", dict(neo=trained)),
                       ("neo_untrained", "neo", dict(neo=untrained)), ("nn_trained", "nn", dict(neo=trained))):
    fly(1, mode, **kw)                                       # warm-up: first-use allocations and caches
    loop, out, wall = fly(1, mode, **kw)
    ticks = loop.timings
    per_tick = lambda k: round(1e3 * sum(t.get(k, 0.0) for t in ticks) / len(ticks), 3)
    flew = out["n_flown"] > 0
    r = dict(mode=mode, ticks=len(ticks), wall_s=round(wall, 3), opt_runs=int(out["opt_runs"].sum()), replans=int(out["replans"].sum()),
             failed_attempts=int(out["failed_attempts"].sum()),
             iterations_per_run=round(float(out["iter_num"].sum()) / max(int(out["opt_runs"].sum()), 1), 2),
             tick_ms=per_tick("tick_s"), neo_ms=per_tick("neo_s"), plan_ms=per_tick("plan_s"), fleet_ms=per_tick("fleet_s"),
             host_ms=per_tick("host_s"), plan_rounds_per_tick=round(sum(t["plans"] for t in ticks) / len(ticks), 2),
             success_rate=round(float(out["success"].mean()), 4), abandoned=int(out["abandoned"].sum()),
             metric_fail=int(out["metric_fail"].sum()),
             audit_weighted_mean=round(float(np.nanmean(out["weighted"][flew])), 5) if flew.any() else None,
             audit_path_length_mean=round(float(np.nanmean(out["path_length"][flew])), 3) if flew.any() else None,
             audit_duration_mean=round(float(np.nanmean(out["duration"][flew])), 3) if flew.any() else None)
    print(f"{name}: {r['iterations_per_run']} iterations a run over {r['opt_runs']} runs; a tick {r['tick_ms']} ms (neo {r['neo_ms']}, "
          f"plan {r['plan_ms']}, fleet {r['fleet_ms']}); {100 * r['success_rate']:.1f} % reach the goal; weighted metric "
          f"{r['audit_weighted_mean']}", flush=True)
    res["fleets"][name] = r
    dump(res)
