#!/usr/bin/env python3
"""Times the fleet's record mode and measures what a network trained on its rows is worth
(neo_record_commit_dev; neo_planner_amd.DemoRecorder, train_initializer).

  commit  neo_record_commit_dev (rank + commit) for 4096 missions that all solved at --size 640x480 or 160x120: HIP
          events on the context's stream around 20 launches after 3 warm-up launches, every launch appending to a dataset
          with room for all of them, next to the floor of moving the images (read + write at the 6.29 TB/s copy rate)
  train   512 missions (8 scenes x 64, goals drawn at 25 - 30 m) flown in mode `batch`, as the reference records, with a
          160 x 120 camera: rows, dropped rows and the tick time, next to the same fleet with record=None in the same
          session (flown once before as a warm-up, then timed); a PlannerNet(120, 160) trained on the rows; then, on
          requests recorded from missions of another seed, BatchNeoPlanner.plan with the trained net, with an untrained
          one, and BatchPlanner.plan from the straight line: mean nit_total, first-attempt success, solved share

Each part is one process; run them one after the other, every one under its own time limit, e.g.
  timeout -k 10 300 python tools/gpu_record_time.py commit --json profiles/record_commit.json && \\
  timeout -k 10 900 python tools/gpu_record_time.py train --json profiles/record_train.json
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

COPY_RATE = 6.29e12      # bytes a second of a float4 copy on one MI355X

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["commit", "train"])
ap.add_argument("--sizes", default="640x480,160x120")
ap.add_argument("--missions", type=int, default=4096)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--scenes", type=int, default=8)
ap.add_argument("--per-scene", type=int, default=64)
ap.add_argument("--test-per-scene", type=int, default=16)
ap.add_argument("--max-replans", type=int, default=60)
ap.add_argument("--epochs", type=int, default=5)
ap.add_argument("--batch-size", type=int, default=64)
ap.add_argument("--requests", type=int, default=2048)
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


if a.what == "commit":
    B, M = a.missions, 3
    out = []
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        rng = np.random.default_rng(0)
        rec = DemoRecorder(DepthCamera(ctx, width=W, height=H), capacity=B * (a.launches + a.warmup), M=M, ctx=ctx)
        rec.bind(B)
        rec.staging.copy_(torch.randint(0, 256, (B, H, W), dtype=torch.uint8, device=dev))
        yaw = rng.uniform(-np.pi, np.pi, B)
        up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
        pose = up(np.stack([rng.uniform(0, 30, B), rng.uniform(-15, 15, B), np.full(B, 2.0), np.cos(yaw), np.sin(yaw)], 1))
        x, head, tail = up(rng.uniform(-4, 30, (B, 3 * M - 2))), up(rng.uniform(-4, 30, (B, 3, 2))), up(rng.uniform(-4, 30, (B, 3, 2)))
        solved = torch.ones(B, dtype=torch.int32, device=dev)
        rec.cur_vel.copy_(up(rng.uniform(-2, 2, (B, 2))))
        launch = lambda k: rec.commit(B, None, x, head, tail, solved, pose, None, k, 0)
        torch.cuda.synchronize(dev)
        for k in range(a.warmup):
            launch(k)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for k in range(a.launches):
            launch(a.warmup + k)
        e1.record(stream)
        e1.synchronize()
        ms = e0.elapsed_time(e1) / a.launches
        assert rec.n_rows == rec.capacity and rec.dropped == 0
        moved = 2 * B * H * W
        floor_ms = 1e3 * moved / COPY_RATE
        res = dict(size=size, missions=B, commit_ms=round(ms, 4), us_per_row=round(1e3 * ms / B, 4), image_bytes_moved=moved,
                   tbytes_per_s=round(moved / (ms * 1e-3) / 1e12, 3), floor_ms=round(floor_ms, 4), times_the_floor=round(ms / floor_ms, 2),
                   staging_mbytes=round(B * H * W / 1e6, 1), launches=a.launches, warmup=a.warmup)
        print(f"commit {size}: {B} rows in {ms:.3f} ms ({res['tbytes_per_s']} TB/s of image reads + writes); the floor of moving "
              f"the images is {floor_ms:.3f} ms: {res['times_the_floor']} x", flush=True)
        out.append(res)
        del rec
        torch.cuda.empty_cache()
    ctx.set_stream(None)
    dump(out)
    sys.exit(0)

# ---- train: fly and record, train, and plan from the network's warm start
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


def fly(per_scene, seed, record):
    start, goals, sids = draw_missions(maps, per_scene, seed=seed)
    scene_index = (np.arange(len(goals)) // per_scene).astype(np.int32)
    kw = dict(record=record, scenes=packed, scene_index=scene_index) if record is not None else {}
    loop = npa.FleetReplanLoop(bp, maps[0], goals, mode="batch", scene_ids=sids, seed=seed, **kw)
    t0 = time.perf_counter()
    out = loop.run(start, max_replans=a.max_replans)
    wall = time.perf_counter() - t0
    ticks = loop.timings
    return dict(out=out, sids=sids, scene_index=scene_index, wall_s=wall, ticks=len(ticks),
                tick_ms=1e3 * sum(t["tick_s"] for t in ticks) / len(ticks),
                record_ms=1e3 * sum(t.get("record_s", 0.0) for t in ticks) / len(ticks),
                fleet_ms=1e3 * sum(t["fleet_s"] for t in ticks) / len(ticks))


Bf = a.scenes * a.per_scene
rec = DemoRecorder(cam, capacity=Bf * (a.max_replans + 4), M=3, ctx=ctx)
fly(a.per_scene, 0, None)                                   # warm-up: first-use allocations and caches
plain = fly(a.per_scene, 0, None)
flown = fly(a.per_scene, 0, rec)
for k in plain["out"]:
    assert np.array_equal(np.asarray(plain["out"][k]), np.asarray(flown["out"][k]), equal_nan=True), k
rows = rec.rows()
res = dict(missions=Bf, size=f"{W}x{H}", mode="batch", rows=rec.n_rows, dropped=rec.dropped, ticks=flown["ticks"],
           success_rate=float(flown["out"]["success"].mean()), tick_ms_recorded=round(flown["tick_ms"], 3),
           tick_ms_unrecorded=round(plain["tick_ms"], 3), record_ms_per_tick=round(flown["record_ms"], 3),
           fleet_kernels_ms_per_tick=dict(recorded=round(flown["fleet_ms"], 3), unrecorded=round(plain["fleet_ms"], 3)),
           wall_s=dict(recorded=round(flown["wall_s"], 3), unrecorded=round(plain["wall_s"], 3)))
print(f"recorded fleet: {Bf} missions, {res['rows']} rows ({res['dropped']} dropped) in {res['ticks']} ticks; a tick "
      f"{res['tick_ms_recorded']:.1f} ms recorded ({res['record_ms_per_tick']:.1f} ms of it pose, state and images) against "
      f"{res['tick_ms_unrecorded']:.1f} ms unrecorded; the flights are the same", flush=True)
dump(res)

inputs, labels = rec.training_tensors(rows)
t0 = time.perf_counter()
torch.manual_seed(42)
net, losses, held_out = npa.train_initializer(inputs, labels, net=ini.PlannerNet(H, W), epochs=a.epochs, batch_size=a.batch_size,
                                              device=dev)
train_s = time.perf_counter() - t0
res.update(train=dict(rows=int(inputs.shape[0]), epochs=a.epochs, batch_size=a.batch_size, seconds=round(train_s, 1),
                      loss_per_epoch=[round(v, 5) for v in losses], held_out_mse=round(held_out, 5),
                      label_variance=round(float(labels.var(axis=0).mean()), 5)))
print(f"trained on {inputs.shape[0]} rows, {a.epochs} epochs of batches of {a.batch_size} in {train_s:.0f} s: loss per epoch "
      f"{res['train']['loss_per_epoch']}, held out {held_out:.4f} (mean label variance {res['train']['label_variance']})", flush=True)
dump(res)
del inputs

# requests the recorder never saw: the plans of missions drawn from another seed, rebuilt from their recorded rows
test_rec = DemoRecorder(cam, capacity=a.scenes * a.test_per_scene * (a.max_replans + 4), M=3, ctx=ctx)
test = fly(a.test_per_scene, 1, test_rec)
tr = test_rec.rows()
pick = np.random.default_rng(1).permutation(tr["meta"].shape[0])[:a.requests]
pick.sort()
pose, mo, ids = tr["pose"][pick], tr["motion"][pick], tr["meta"][pick, 0]
c, s = pose[:, 3], pose[:, 4]
world = lambda v: np.stack([c * v[:, 0] - s * v[:, 1], s * v[:, 0] + c * v[:, 1]], 1)      # R v, x and y
cur_vel = world(mo[:, 0:3])
n = len(pick)
head, tail = np.zeros((n, 3, 2)), np.zeros((n, 3, 2))
head[:, 0], head[:, 1] = pose[:, :2] + world(mo[:, 12:15]), cur_vel + world(mo[:, 15:18])
tail[:, 0], tail[:, 1] = pose[:, :2] + world(mo[:, 18:21]), cur_vel + world(mo[:, 21:24])
drone_vel = np.concatenate([cur_vel, np.zeros((n, 1))], 1)
yaw = np.arctan2(s, c)
sids, sidx = test["sids"][ids], test["scene_index"][ids]


def report(name, out):
    first = out["solved"] & (out["attempts"] == 1)
    r = dict(mean_nit_total=round(float(out["nit_total"].mean()), 2), first_attempt_success=round(float(first.mean()), 4),
             solved_share=round(float(out["solved"].mean()), 4),
             mean_nit_total_of_solved=round(float(out["nit_total"][out["solved"]].mean()), 2))
    print(f"{name}: mean nit_total {r['mean_nit_total']}, first attempt {r['first_attempt_success']}, solved {r['solved_share']}", flush=True)
    return r


plans = {}
torch.manual_seed(7)
for name, the_net in (("trained", net), ("untrained", ini.PlannerNet(H, W))):
    neo = ini.BatchNeoPlanner(bp, ini.BatchInitializer(net=the_net, device=dev, T_min=bp.cfg.T_min, T_max=bp.cfg.T_max), cam)
    plans[name] = report(name + " network warm start", neo.plan(maps[0], scenes, pose[:, :3], drone_vel, mo[:, 0:3], yaw, head, tail,
                                                                scene_index=sidx, scene_ids=sids, seed=3))
plans["straight_line"] = report("straight line", bp.plan(maps[0], head, tail, scene_ids=sids, seed=3))
res.update(requests=n, test_missions=a.scenes * a.test_per_scene, test_seed=1, plans=plans)
dump(res)
