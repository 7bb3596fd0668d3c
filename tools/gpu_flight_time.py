#!/usr/bin/env python3
"""Times the fleet's flight model (csrc/neo_flight.hpp: neo_fleet_fly_dev, neo_fleet_fly_error_dev;
FleetReplanLoop(flight=FlightModel)).

  kernels  B = 4096 missions on scene 0, on the state a fleet run with the default model left behind (real command
           arrays): fleet_fly_kernel at step = 60 and 300 sub-steps, gusts off and on, next to fleet_advance_kernel, and
           fleet_fly_error_kernel next to fleet_audit_kernel over the same rows.  Every launch is timed on its own, HIP
           events on the context's stream around it, 20 launches after 3 warm-ups; cmd_index and the drones are put back
           before every launch (outside the events), so that each launch flies the same rows.
  fleet    the 4096 missions of profiles/fleet_basic.json (8 scenes x 512 goals drawn at 25 - 30 m, seed 0) flown three
           ways -- no model, the default model, the default model with gust_sigma = 0.3 -- in mode basic and in mode neo
           (the network trained as tools/gpu_neo_fleet_time.py trains it: on the rows a 512-mission record flight of
           another seed left).  Each configuration is flown once as a warm-up and then timed.  Per row: success,
           abandoned, metric failures, the median flight metric, fly_pos_err_rms / max, saturated sub-steps, the tick's
           wall time with its spread over the ticks, and the settle and fly_error launches of the end.

Each step is one process, every one under its own time limit:
  timeout -k 10 300 python tools/gpu_flight_time.py kernels --json profiles/flight_kernels.json && \\
  timeout -k 10 900 python tools/gpu_flight_time.py fleet --json profiles/flight.json
(`fleet` merges the figures of --kernels-json, default profiles/flight_kernels.json, into its file when that exists.)"""
import argparse, ctypes, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "neo-planner_amd"))
import numpy as np, torch
import neo_planner_amd as npa
from neo_planner_amd import synth, _lib, initializer as ini
from neo_planner_amd.depth import DepthCamera
from neo_planner_amd.fleet import draw_missions
from neo_planner_amd.flight_model import FlightModel
from neo_planner_amd.record import DemoRecorder

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["kernels", "fleet"])
ap.add_argument("--scenes", type=int, default=8)
ap.add_argument("--per-scene", type=int, default=512)
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--max-replans", type=int, default=60)
ap.add_argument("--epochs", type=int, default=5)
ap.add_argument("--modes", default="basic,neo")
ap.add_argument("--json", default=None)
ap.add_argument("--kernels-json", default=os.path.join(REPO, "profiles", "flight_kernels.json"))
a = ap.parse_args()

dev = torch.device("cuda", 0)
ctx = _lib.default_context()
p = lambda v: ctypes.c_void_p(v.data_ptr()) if v is not None else None
GUSTS = dict(gust_sigma=0.3, seed=1)


def scene_map(s):
    m = npa.ESDF(ctx=ctx)
    m.occupancy_map_cb(synth.OccupancyGridMsg(synth.occupancy_2d(s)))
    return m


def dump(obj):
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(obj, f, indent=1)
            f.write("\n")


if a.what == "kernels":
    stream = torch.cuda.Stream()          # (not the null stream: its handle 0 would hand the context back its own stream)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    m = scene_map(0)
    B = a.batch
    start, goals, _ = draw_missions([m], B, seed=0)
    loop = npa.FleetReplanLoop(npa.BatchPlanner(ctx=ctx), m, goals, seed=0, flight=FlightModel())
    loop.run(start, max_replans=12)
    d, lib, h, cap = loop._dev, ctx.lib, ctx.h, loop.cap
    n_cmd = d["cmd_len"].cpu().numpy()
    keep = {k: d[k].clone() for k in ("cmd_index", "future_index", "drone", "flown_len", "fly_saturated", "flags", "cur_pos", "head")}
    zero_index = torch.zeros_like(d["cmd_index"])

    def restore():
        for k, v in keep.items():
            d[k].copy_(v)
        d["cmd_index"].copy_(zero_index)      # every launch flies rows 1 .. min(step, cmd_len - 1)

    def fly_call(model, step):
        ms = _lib.NeoFlightModel(*model.derived(loop.cmd_hz))
        return lambda: lib.neo_fleet_fly_dev(h, B, ctypes.byref(ms), None, 0, p(d["cmd"]), cap, p(d["cmd_len"]), p(d["cmd_index"]),
                                             p(d["future_index"]), step, 60, 0, 0, 0.2, p(d["mission_ids"]), p(d["goal"]),
                                             p(d["drone"]), p(d["flown"]), p(d["flown_len"]), p(d["fly_saturated"]), p(d["flags"]),
                                             p(d["cur_pos"]), p(d["head"]))

    calls = {"advance step 60": (lambda: lib.neo_fleet_advance_dev(h, B, None, 0, p(d["cmd"]), cap, p(d["cmd_len"]), p(d["cmd_index"]),
                                                                   p(d["future_index"]), 60, 60, p(d["cur_pos"]), p(d["head"])), 60)}
    for step in (60, 300):
        calls[f"fly step {step}"] = (fly_call(FlightModel(), step), step)
        calls[f"fly step {step} gusts"] = (fly_call(FlightModel(**GUSTS), step), step)
    rows = []

    def timed(name, call, before, **extra):
        ev = []
        for k in range(3 + a.launches):
            before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            ctx.check(call())
            e1.record(stream)
            if k >= 3:
                ev.append((e0, e1))
        stream.synchronize()
        us = np.array([1e3 * e0.elapsed_time(e1) for e0, e1 in ev])
        row = dict(kernel=name, batch=B, us_per_launch=round(float(np.median(us)), 2), us_min=round(float(us.min()), 2),
                   us_max=round(float(us.max()), 2), **extra)
        rows.append(row)
        print(f"{name:>22}: median {row['us_per_launch']:8.1f} us (min {row['us_min']:.1f}, max {row['us_max']:.1f}) per launch of {B} "
              + " ".join(f"{k}={v:.4g}" for k, v in extra.items()), flush=True)

    for name, (call, step) in calls.items():
        timed(name, call, restore, sub_steps_mean=float(np.minimum(step, np.maximum(n_cmd - 1, 0)).mean()))
    # the two reductions over the same rows: every mission's whole array flown out first
    restore()
    d["flown_len"].zero_()
    ctx.check(fly_call(FlightModel(**GUSTS), cap)())
    stream.synchronize()
    d["n_flown"].copy_(d["flown_len"])
    stream.synchronize()
    nothing = lambda: None
    timed("audit", lambda: lib.neo_fleet_audit_batch_dev(h, m.scene_id, None, B, None, 0, p(d["flown"]), cap, p(d["n_flown"]),
                                                         loop.stride, 60.0, None, p(d["audit"]), p(d["count"]), p(d["audit_flags"])),
          nothing, rows_mean=float(n_cmd.mean()))
    timed("fly_error", lambda: lib.neo_fleet_fly_error_dev(h, B, p(d["flown_len"]), None, 0, p(d["flown"]), p(d["cmd"]), cap,
                                                           p(d["cmd_len"]), loop.stride, p(d["fly"]), p(d["fly_count"]), p(d["fly_flags"])),
          nothing, rows_mean=float(n_cmd.mean()), samples_mean=float(d["fly_count"].cpu().numpy().mean()))
    timed("fly_error stride 1", lambda: lib.neo_fleet_fly_error_dev(h, B, p(d["flown_len"]), None, 0, p(d["flown"]), p(d["cmd"]), cap,
                                                                    p(d["cmd_len"]), 1, p(d["fly"]), p(d["fly_count"]), p(d["fly_flags"])),
          nothing, rows_mean=float(n_cmd.mean()))
    ctx.set_stream(None)
    dump(dict(kernels=rows, note="each launch timed on its own (HIP events around it); median over the launches"))
    sys.exit(0)

# ---- fleet: the same 4096 missions, three ways, in the modes asked for
modes = [s for s in a.modes.split(",") if s]
maps = [scene_map(s) for s in range(a.scenes)]
bp = npa.BatchPlanner(ctx=ctx)
res = dict(missions=a.scenes * a.per_scene, scenes=a.scenes, max_replans=a.max_replans, gusts=GUSTS, fleets={})
if os.path.exists(a.kernels_json):
    res["kernels"] = json.load(open(a.kernels_json))["kernels"]
neo = None
if "neo" in modes:      # the network of tools/gpu_neo_fleet_time.py: trained on a 512-mission record flight of seed 1
    W, H = 160, 120
    cam = DepthCamera(ctx, width=W, height=H)
    packed = DepthCamera.pack_scenes([DepthCamera.boxes_of(synth.forest_boxes(s)) for s in range(a.scenes)])
    per = 64
    s1, g1, sid1 = draw_missions(maps, per, seed=1)
    rec = DemoRecorder(cam, capacity=a.scenes * per * (a.max_replans + 4), M=3, ctx=ctx)
    npa.FleetReplanLoop(bp, maps[0], g1, mode="batch", scene_ids=sid1, seed=1, record=rec, scenes=packed,
                        scene_index=(np.arange(len(g1)) // per).astype(np.int32)).run(s1, max_replans=a.max_replans)
    inputs, labels = rec.training_tensors(rec.rows())
    torch.manual_seed(42)
    t0 = time.perf_counter()
    net, losses, held_out = npa.train_initializer(inputs, labels, net=ini.PlannerNet(H, W), epochs=a.epochs, batch_size=64, device=dev)
    res["train"] = dict(rows=int(inputs.shape[0]), epochs=a.epochs, seconds=round(time.perf_counter() - t0, 1), held_out_mse=round(held_out, 5))
    print(f"recorded {rec.n_rows} rows, trained {a.epochs} epochs: held out {held_out:.4f}", flush=True)
    del inputs, rec
    torch.cuda.empty_cache()
    neo = ini.BatchNeoPlanner(bp, ini.BatchInitializer(net=net, device=dev, T_min=bp.cfg.T_min, T_max=bp.cfg.T_max), cam)

start, goals, sids = draw_missions(maps, a.per_scene, seed=0)
scene_index = (np.arange(len(goals)) // a.per_scene).astype(np.int32)
WAYS = (("none", None), ("default", FlightModel()), ("gusts", FlightModel(**GUSTS)))
for mode in modes:
    for way, model in WAYS:
        kw = dict(neo=neo, scenes=packed, scene_index=scene_index) if mode == "neo" else {}
        for timed_run in (False, True):      # flown once as a warm-up (first-use allocations and caches), then timed
            loop = npa.FleetReplanLoop(bp, maps[0], goals, mode=mode, scene_ids=sids, seed=0, flight=model, **kw)
            t0 = time.perf_counter()
            out = loop.run(start, max_replans=a.max_replans)
            wall = time.perf_counter() - t0
        ticks = loop.timings
        tick_ms = np.array([1e3 * t["tick_s"] for t in ticks])
        full = np.array([1e3 * t["tick_s"] for t in ticks if t["active"] == len(goals)])      # the ticks everybody flies in
        ok = out["success"]
        r = dict(mode=mode, flight=way, wall_s=round(wall, 3), ticks=len(ticks), success_rate=round(float(ok.mean()), 5),
                 abandoned=int(out["abandoned"].sum()), metric_fail=int(out["metric_fail"].sum()),
                 cmd_full=int(((out["flags"] & _lib.NEO_FLEET_FLAG_CMD_FULL) != 0).sum()),
                 median_weighted_metric=float(np.nanmedian(out["weighted"])),
                 min_clearance_successful=float(out["min_clearance"][ok].min()) if ok.any() else None,
                 unsafe=int(((out["audit_flags"] & _lib.NEO_AUDIT_FLAG_UNSAFE) != 0).sum()),
                 plans_per_mission=round(float(out["replans"].mean()), 3),
                 failed_attempts_per_mission=round(float(out["failed_attempts"].mean()), 4),
                 iterations_per_run=round(float(out["iter_num"].sum()) / max(int(out["opt_runs"].sum()), 1), 2),
                 tick_ms_mean=round(float(tick_ms.mean()), 3), tick_ms_full_fleet_median=round(float(np.median(full)), 3) if full.size else None,
                 tick_ms_full_fleet_min=round(float(full.min()), 3) if full.size else None,
                 tick_ms_full_fleet_max=round(float(full.max()), 3) if full.size else None,
                 fleet_ms_mean=round(1e3 * float(np.mean([t["fleet_s"] for t in ticks])), 3),
                 plan_ms_mean=round(1e3 * float(np.mean([t["plan_s"] for t in ticks])), 3), audit_ms=round(1e3 * loop.audit_s, 3))
        if model is not None:
            r.update(fly_pos_err_rms_median=float(np.nanmedian(out["fly_pos_err_rms"])), fly_pos_err_rms_max=float(np.nanmax(out["fly_pos_err_rms"])),
                     fly_pos_err_max_median=float(np.nanmedian(out["fly_pos_err_max"])), fly_pos_err_max_max=float(np.nanmax(out["fly_pos_err_max"])),
                     fly_pos_err_final_median=float(np.nanmedian(out["fly_pos_err_final"])),
                     fly_saturated_missions=int((out["fly_saturated"] > 0).sum()), fly_flags_set=int((out["fly_flags"] != 0).sum()),
                     settle_rows_mean=float(np.maximum(out["n_flown"] - out["n_cmd"], 0).mean()),
                     settle_ms=round(1e3 * loop.settle_s, 3), fly_error_ms=round(1e3 * loop.fly_error_s, 3))
        res["fleets"][f"{mode}/{way}"] = r
        print(f"{mode}/{way}: success {r['success_rate']:.4f}, abandoned {r['abandoned']}, metric_fail {r['metric_fail']}, unsafe "
              f"{r['unsafe']}, median metric {r['median_weighted_metric']:.2f}, iterations a run {r['iterations_per_run']}; tick "
              f"{r['tick_ms_mean']:.1f} ms mean, full-fleet ticks median {r['tick_ms_full_fleet_median']} (min "
              f"{r['tick_ms_full_fleet_min']}, max {r['tick_ms_full_fleet_max']})"
              + (f"; fly rms median {r['fly_pos_err_rms_median']:.4f} max-of-max {r['fly_pos_err_max_max']:.4f} m, saturated missions "
                 f"{r['fly_saturated_missions']}, settle rows {r['settle_rows_mean']:.1f}" if model is not None else ""), flush=True)
        dump(res)
