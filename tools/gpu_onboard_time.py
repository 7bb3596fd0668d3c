#!/usr/bin/env python3
"""Times onboard mapping (neo_onboard_integrate_batch_dev, neo_esdf_build_2d_batch_dev; neo_planner_amd.OnboardMapper).

  integrate  B = 4096 missions (8 scenes x 512 poses) on 300 x 300 grids at --size 640x480 or 160x120: HIP events on the
             context's stream around --launches launches after 2 warm-up launches, on rendered images; and the NumPy
             model's time for one of the images on the host (tests/onboard_oracle_np.py)
  rebuild    the batched 2-D ESDF build of the 4096 occupancy grids that scan leaves, wall time of the call (it waits for
             its own work), against 4096 neo_esdf_build_2d calls on the same grids, one after the other
  fleet      the 4096-mission experiment (8 scenes x 512 goals drawn at 25 - 30 m) flown on onboard maps: success rate
             and unsafe share against the true maps, wall time per tick and the share of it spent sensing and mapping;
             then the same missions on the global maps

Each step is one process: run them one after the other, every one under its own time limit, e.g.
  timeout -k 10 300 python tools/gpu_onboard_time.py integrate --size 640x480 --json profiles/onboard_integrate_640.json && \\
  timeout -k 10 300 python tools/gpu_onboard_time.py integrate --size 160x120 --json profiles/onboard_integrate_160.json && \\
  timeout -k 10 300 python tools/gpu_onboard_time.py rebuild --json profiles/onboard_rebuild.json && \\
  timeout -k 10 900 python tools/gpu_onboard_time.py fleet --size 160x120 --json profiles/onboard_fleet.json
Prints one line per figure; --json PATH also writes them."""
import argparse, ctypes, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "neo-planner_amd")); sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np, torch
import neo_planner_amd as npa
from neo_planner_amd import synth, _lib
from neo_planner_amd.depth import DepthCamera
from neo_planner_amd.fleet import draw_missions
from neo_planner_amd.onboard import OnboardMapper

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["integrate", "rebuild", "fleet"])
ap.add_argument("--size", default="640x480")
ap.add_argument("--scenes", type=int, default=8)
ap.add_argument("--per-scene", type=int, default=512)
ap.add_argument("--launches", type=int, default=5)
ap.add_argument("--single-calls", type=int, default=4096)
ap.add_argument("--mode", default="basic", choices=["basic", "batch"])
ap.add_argument("--resident", action="store_true")
ap.add_argument("--max-replans", type=int, default=60)
ap.add_argument("--json", default=None)
a = ap.parse_args()

dev = torch.device("cuda", 0)
ctx = _lib.default_context()
W, H = (int(v) for v in a.size.split("x"))
cam = DepthCamera(ctx, width=W, height=H)
B = a.scenes * a.per_scene
p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None


def dump(obj):
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(obj, f, indent=1)


scenes = [DepthCamera.boxes_of(synth.forest_boxes(s)) for s in range(a.scenes)]
boxes, begin = DepthCamera.pack_scenes(scenes)
d_boxes, d_begin = torch.from_numpy(boxes).to(dev), torch.from_numpy(begin).to(dev)


def scan_poses():
    """512 poses a scene: eyes over the forest's near half, looking roughly along +x"""
    rng = np.random.default_rng(0)
    eye = np.stack([rng.uniform(0.5, 20.0, B), rng.uniform(-5.0, 5.0, B), np.full(B, 2.0)], 1)
    yaw = rng.uniform(-0.6, 0.6, B)
    return eye, yaw, (np.arange(B) // a.per_scene).astype(np.int32)


if a.what in ("integrate", "rebuild"):
    eye, yaw, sidx = scan_poses()
    pose = torch.from_numpy(DepthCamera.poses(eye, yaw)).to(dev)
    d_sidx = torch.from_numpy(sidx).to(dev)
    mapper = OnboardMapper(ctx, cam, B)
    depth = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    chunk = 512
    torch.cuda.synchronize(dev)
    for b0 in range(0, B, chunk):
        ctx.check(ctx.lib.neo_depth_render_batch_dev(ctx.h, W, H, cam.focal_px, cam.max_range, p(d_boxes), p(d_begin), a.scenes,
                                                     p(d_sidx[b0:b0 + chunk]), min(chunk, B - b0), p(pose[b0:b0 + chunk]),
                                                     p(depth[b0:b0 + chunk]), None, None))
    ctx.synchronize()
    changed = mapper.integrate(depth, pose).cpu().numpy()
    occupied = (mapper.occupancy == 100).sum().item() / B

if a.what == "integrate":
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    l = mapper.lodds

    def launch():
        ctx.check(ctx.lib.neo_onboard_integrate_batch_dev(
            ctx.h, B, None, 0, p(depth), p(pose), W, H, cam.focal_px, cam.max_range, mapper.width, mapper.height,
            mapper.resolution, p(mapper._origins_dev), mapper.sensor_range, mapper.z_band[0], mapper.z_band[1], l[0], l[1], l[2],
            l[3], p(mapper.logodds), p(mapper.occupancy), p(mapper.changed)))

    torch.cuda.synchronize(dev)
    for _ in range(2):
        launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(a.launches):
        launch()
    e1.record(stream)
    e1.synchronize()
    ms = e0.elapsed_time(e1) / a.launches
    ctx.set_stream(None)
    import depth_oracle_np as don, onboard_oracle_np as oon
    u, v = oon.camera_tables(W, H, cam.focal_px)
    img = depth[0].cpu().numpy()
    t0 = time.perf_counter()
    oon.integrate(oon.empty(mapper.width, mapper.height), img, u, v, np.float32(np.cos(yaw[0])), np.float32(np.sin(yaw[0])), eye[0],
                  mapper.resolution, tuple(mapper.origins[0]))
    host_ms = 1e3 * (time.perf_counter() - t0)
    res = dict(size=a.size, missions=B, integrate_ms=round(ms, 3), us_per_image=round(1e3 * ms / B, 3),
               gbytes_per_s=round(B * H * W * 4 / (ms * 1e-3) / 1e9, 1), oracle_ms_per_image=round(host_ms, 2),
               speedup_per_image=round(host_ms / (ms / B), 0), changed=int(changed.sum()), occupied_cells_per_mission=occupied)
    print(f"integrate {a.size}: {B} images in {ms:.3f} ms ({1e3 * ms / B:.2f} us an image, {res['gbytes_per_s']} GB/s of depth "
          f"read); the NumPy model {host_ms:.1f} ms an image ({res['speedup_per_image']:.0f} x)", flush=True)
    dump(res)
    sys.exit(0)

if a.what == "rebuild":
    occ_host = mapper.occupancy.cpu().numpy()
    ids = mapper.scene_ids
    org = np.ascontiguousarray(mapper.origins)
    times = []
    for _ in range(3):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        ctx.check(ctx.lib.neo_esdf_build_2d_batch_dev(ctx.h, _lib.ptr(ids), B, p(mapper.occupancy), mapper.width, mapper.height,
                                                      mapper.resolution, _lib.ptr(org)))
        times.append(1e3 * (time.perf_counter() - t0))
    batch_ms = min(times)
    single = ctx.new_scene_id()
    n1 = min(a.single_calls, B)
    one = lambda k: ctx.check(ctx.lib.neo_esdf_build_2d(ctx.h, single, _lib.ptr(occ_host[k]), mapper.width, mapper.height,
                                                        mapper.resolution, org[k, 0], org[k, 1], None, None, None))
    one(0)
    t0 = time.perf_counter()
    for k in range(n1):
        one(k)
    single_ms = 1e3 * (time.perf_counter() - t0) * (B / n1)
    res = dict(maps=B, batch_ms=round(batch_ms, 2), batch_ms_all=[round(t, 2) for t in times], us_per_map=round(1e3 * batch_ms / B, 2),
               single_calls_timed=n1, single_calls_ms=round(single_ms, 1), ratio=round(single_ms / batch_ms, 1),
               occupied_cells_per_map=occupied)
    print(f"rebuild: {B} maps of {mapper.width} x {mapper.height} in {batch_ms:.1f} ms ({1e3 * batch_ms / B:.1f} us a map); {B} neo_esdf_build_2d calls "
          f"{single_ms:.0f} ms ({n1} timed): {single_ms / batch_ms:.1f} x", flush=True)
    dump(res)
    sys.exit(0)

# ---- fleet: the 4096-mission experiment on onboard maps
maps = []
for s in range(a.scenes):
    m = npa.ESDF(ctx=ctx)
    m.occupancy_map_cb(synth.OccupancyGridMsg(synth.occupancy_2d(s)))
    maps.append(m)
start, goals, sids = draw_missions(maps, a.per_scene, seed=0)
scene_index = (np.arange(B) // a.per_scene).astype(np.int32)
bp = npa.BatchPlanner(ctx=ctx)
mapper = OnboardMapper(ctx, cam, B)
loop = npa.FleetReplanLoop(bp, maps[0], goals, mode=a.mode, scene_ids=sids, seed=0, resident=a.resident, onboard=mapper,
                           scenes=(boxes, begin), scene_index=scene_index)
ctx.check(ctx.lib.neo_profile_enable(ctx.h, 1))
t0 = time.perf_counter()
out = loop.run(start, max_replans=a.max_replans)
wall = time.perf_counter() - t0
n_opt, opt_ms = ctypes.c_int64(0), ctypes.c_double(0.0)
ctx.check(ctx.lib.neo_profile_read(ctx.h, _lib.NEO_KERNEL_OPTIMIZE, ctypes.byref(n_opt), ctypes.byref(opt_ms)))
ctx.check(ctx.lib.neo_profile_enable(ctx.h, 0))
ticks = loop.timings
keys = ("tick_s", "fleet_s", "plan_s", "host_s", "sense_s", "render_s", "integrate_s", "rebuild_s")
tot = {k: sum(t[k] for t in ticks) for k in keys}
ok = out["success"]
unsafe = (out["audit_flags"] & _lib.NEO_AUDIT_FLAG_UNSAFE) != 0
res = dict(mode=a.mode, resident=bool(a.resident), size=a.size, missions=B, wall_s=round(wall, 3), ticks=len(ticks),
           success_rate=float(ok.mean()), unsafe_share=float(unsafe.mean()), metric_fail=int(out["metric_fail"].sum()),
           abandoned=int(out["abandoned"].sum()), plans_per_mission=float(out["replans"].mean()),
           failed_attempts_per_mission=float(out["failed_attempts"].mean()),
           min_clearance_median=float(np.nanmedian(out["min_clearance"])),
           maps_rebuilt=int(sum(t["rebuilt"] for t in ticks)), missions_sensed=int(sum(t["active"] for t in ticks)),
           optimise_ms_per_tick=round(opt_ms.value / len(ticks), 3),
           per_tick_ms={k: round(1e3 * v / len(ticks), 3) for k, v in tot.items()},
           share={k: round(v / tot["tick_s"], 4) for k, v in tot.items() if k != "tick_s"},
           ticks_detail=[{k: (round(v, 5) if isinstance(v, float) else v) for k, v in t.items()} for t in ticks])
print(f"onboard {a.mode} {a.size}: {B} missions in {wall:.2f} s, {len(ticks)} ticks; success {res['success_rate']:.3f}, unsafe "
      f"{res['unsafe_share']:.3f}, metric_fail {res['metric_fail']}, abandoned {res['abandoned']}, plans a mission "
      f"{res['plans_per_mission']:.2f}", flush=True)
print(f"per tick {res['per_tick_ms']['tick_s']:.1f} ms: sensing and mapping {res['per_tick_ms']['sense_s']:.1f} "
      f"({100 * res['share']['sense_s']:.0f} %: render {res['per_tick_ms']['render_s']:.1f}, integrate "
      f"{res['per_tick_ms']['integrate_s']:.1f}, rebuild {res['per_tick_ms']['rebuild_s']:.1f}), plans "
      f"{res['per_tick_ms']['plan_s']:.1f} (optimiser kernels {res['optimise_ms_per_tick']:.1f}), fleet kernels "
      f"{res['per_tick_ms']['fleet_s']:.1f}, host {res['per_tick_ms']['host_s']:.1f}", flush=True)
# the same missions on the global maps: what the onboard figures stand next to
ref = npa.FleetReplanLoop(bp, maps[0], goals, mode=a.mode, scene_ids=sids, seed=0, resident=a.resident)
g = ref.run(start, max_replans=a.max_replans)
g_unsafe = (g["audit_flags"] & _lib.NEO_AUDIT_FLAG_UNSAFE) != 0
res.update(global_success_rate=float(g["success"].mean()), global_unsafe_share=float(g_unsafe.mean()),
           global_min_clearance_median=float(np.nanmedian(g["min_clearance"])),
           global_tick_ms=round(1e3 * sum(t["tick_s"] for t in ref.timings) / len(ref.timings), 3))
print(f"global maps, the same missions: success {res['global_success_rate']:.3f}, unsafe {res['global_unsafe_share']:.3f}, "
      f"median minimum clearance {res['global_min_clearance_median']:.2f} m (onboard {res['min_clearance_median']:.2f} m), "
      f"{res['global_tick_ms']:.1f} ms a tick", flush=True)
dump(res)
