#!/usr/bin/env python3
"""Times the fleet replan loop (neo_fleet_*, neo_fleet.hpp; neo_planner_amd.FleetReplanLoop).

  kernels   the four fleet kernels at B = 4096 missions on scene 0 -- HIP events on the context's stream around 20
            launches after 3 warm-up launches, on the state a fleet run left behind (real command arrays) -- and the
            two kernels of the batch mode (neo_batch.hpp) at 4096 requests x 3 candidates on the same state, and the
            two kernels of the resident plan (neo_plan.hpp: guess with jitter, merge with its compaction launch) at 4096
            requests
  fleet     one whole run of 4096 missions (8 scenes x 512 goals drawn at 25 - 30 m) in mode basic, geo or batch: wall time per
            tick split into fleet kernels (with their small copies) / plan launches / host, missions per second, success
            rate, plans and failed attempts per mission, median weighted metric; --resident plans through
            BatchPlanner.plan_dev on the resident arrays (modes basic and batch; the same flights); --jitter counter draws
            the target jitter and the retry noise from the counter-based streams on the device (other flights)
  jitter    the counter-based jitter (neo_counter_rng.hpp) in one session: plan_jitter_kernel and fleet_jitter_kernel alone
            at 4096 requests, M = 3, D = 2 (HIP events, 20 launches after 3 warm-ups), then whole runs of 4096 missions in
            modes basic and batch, resident off and on, jitter numpy and counter, each flown once as a warm-up and then timed

Each step is one process: run them one after the other, every one under its own time limit, e.g.
  timeout -k 10 300 python tools/gpu_fleet_time.py kernels --json profiles/fleet_kernels.json && \\
  timeout -k 10 600 python tools/gpu_fleet_time.py fleet --mode basic --json profiles/fleet_basic.json && \\
  timeout -k 10 600 python tools/gpu_fleet_time.py fleet --mode geo --json profiles/fleet_geo.json && \\
  timeout -k 10 600 python tools/gpu_fleet_time.py fleet --mode batch --json profiles/fleet_batch.json && \\
  timeout -k 10 600 python tools/gpu_fleet_time.py fleet --mode basic --resident --json profiles/fleet_basic_resident.json && \\
  timeout -k 10 600 python tools/gpu_fleet_time.py jitter --json profiles/fleet_jitter.json
Prints one line per figure; --json PATH also writes them."""
import argparse, ctypes, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "neo-planner_amd"))
import numpy as np, torch
import neo_planner_amd as npa
from neo_planner_amd import synth, _lib
from neo_planner_amd.fleet import draw_missions

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["kernels", "fleet", "jitter"])
ap.add_argument("--mode", default="basic", choices=["basic", "geo", "batch"])
ap.add_argument("--scenes", type=int, default=8)
ap.add_argument("--per-scene", type=int, default=512)
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--max-replans", type=int, default=60)
ap.add_argument("--resident", action="store_true")
ap.add_argument("--jitter", default="numpy", choices=["numpy", "counter"])
ap.add_argument("--json", default=None)
a = ap.parse_args()

dev = torch.device("cuda", 0)
ctx = _lib.default_context()


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


def fly(maps, start, goals, sids, mode, resident, jitter, detail=True):
    """one whole run: the figures of a row"""
    bp = npa.BatchPlanner(ctx=ctx)
    loop = npa.FleetReplanLoop(bp, maps[0], goals, mode=mode, scene_ids=sids, seed=0, resident=resident, jitter=jitter)
    t0 = time.perf_counter()
    out = loop.run(start, max_replans=a.max_replans)
    wall = time.perf_counter() - t0
    B = len(goals)
    ticks = loop.timings
    tot = {k: sum(t[k] for t in ticks) for k in ("tick_s", "fleet_s", "plan_s", "host_s")}
    ok = out["success"]
    res = dict(mode=mode, resident=bool(resident), jitter=jitter, missions=B, scenes=a.scenes, wall_s=round(wall, 3), ticks=len(ticks),
               missions_per_s=round(B / wall, 1), success_rate=float(ok.mean()),
               plans_per_mission=float(out["replans"].mean()), failed_attempts_per_mission=float(out["failed_attempts"].mean()),
               plan_launch_rounds=int(sum(t["plans"] for t in ticks)), plan_requests=int(sum(t["plan_requests"] for t in ticks)),
               abandoned=int(out["abandoned"].sum()), metric_fail=int(out["metric_fail"].sum()),
               cmd_full=int(((out["flags"] & _lib.NEO_FLEET_FLAG_CMD_FULL) != 0).sum()),
               median_weighted_metric=float(np.nanmedian(out["weighted"])),
               median_weighted_metric_successful=float(np.nanmedian(out["weighted"][ok])) if ok.any() else None,
               min_clearance_successful=float(out["min_clearance"][ok].min()) if ok.any() else None,
               mean_commands=float(out["n_cmd"].mean()), max_commands=int(out["n_cmd"].max()),
               iterations_per_run=float(out["iter_num"].sum() / max(int(out["opt_runs"].sum()), 1)),
               audit_ms=round(1e3 * loop.audit_s, 3),
               per_tick_ms={k: round(1e3 * v / len(ticks), 3) for k, v in tot.items()},
               share={k: round(v / tot["tick_s"], 4) for k, v in tot.items() if k != "tick_s"})
    if detail:
        res["ticks_detail"] = [{k: (round(v, 5) if isinstance(v, float) else v) for k, v in t.items()} for t in ticks]
    tag = f"{mode}{' resident' if resident else ''}{' counter' if jitter == 'counter' else ''}"
    print(f"{tag}: {B} missions in {wall:.2f} s ({B / wall:.0f} missions/s), {len(ticks)} ticks; success "
          f"{res['success_rate']:.3f}, plans a mission {res['plans_per_mission']:.2f}, failed attempts a mission "
          f"{res['failed_attempts_per_mission']:.3f}, abandoned {res['abandoned']}, metric_fail {res['metric_fail']}, "
          f"median weighted metric {res['median_weighted_metric']:.2f}", flush=True)
    print(f"{tag}: per tick {res['per_tick_ms']['tick_s']:.1f} ms = fleet kernels and their copies "
          f"{res['per_tick_ms']['fleet_s']:.1f} + plan launches {res['per_tick_ms']['plan_s']:.1f} + host "
          f"{res['per_tick_ms']['host_s']:.1f}; final audit {res['audit_ms']:.2f} ms", flush=True)
    return res


if a.what == "fleet":
    maps = [scene_map(s) for s in range(a.scenes)]
    start, goals, sids = draw_missions(maps, a.per_scene, seed=0)
    dump(fly(maps, start, goals, sids, a.mode, a.resident, a.jitter))
    sys.exit(0)

if a.what == "jitter":
    # the two kernels alone, on the context's own stream, timed with HIP events
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    B, M, D = a.batch, 3, 2
    p = lambda v: ctypes.c_void_p(v.data_ptr()) if v is not None else None
    ids = torch.arange(B, dtype=torch.int32, device=dev) * 3 + 500
    noise = torch.zeros((B, D, M - 1), dtype=torch.float64, device=dev)
    jit = torch.zeros((B, 2), dtype=torch.float64, device=dev)
    lib, h = ctx.lib, ctx.h
    calls = {"plan_jitter": lambda: lib.neo_plan_jitter_dev(h, B, None, 0, M, D, 12345, 1, p(ids), p(noise)),
             "fleet_jitter": lambda: lib.neo_fleet_jitter_dev(h, B, None, 0, 12345, 7, 3, p(ids), p(jit))}
    stream.synchronize()
    rows = []
    for name, call in calls.items():
        for _ in range(3):
            ctx.check(call())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.launches):
            ctx.check(call())
        e1.record(stream)
        e1.synchronize()
        us = 1e3 * e0.elapsed_time(e1) / a.launches
        row = dict(kernel=name, batch=B, values=int(noise.numel() if name == "plan_jitter" else jit.numel()),
                   us_per_launch=round(us, 2))
        if name == "plan_jitter":
            row.update(M=M, D=D)
        rows.append(row)
        print(f"{name:>12}: {us:8.1f} us per launch of {B}", flush=True)
    from neo_planner_amd import counter_rng
    assert np.array_equal(noise.cpu().numpy(), counter_rng.retry_noise(12345, ids.cpu().numpy(), 1, D, M - 1))
    assert np.array_equal(jit.cpu().numpy(), counter_rng.target_jitter(12345, ids.cpu().numpy(), 7, 3))
    ctx.set_stream(None)
    torch.cuda.set_stream(torch.cuda.default_stream())
    # whole runs, one session: every configuration flown once as a warm-up, then timed
    maps = [scene_map(s) for s in range(a.scenes)]
    start, goals, sids = draw_missions(maps, a.per_scene, seed=0)
    runs = []
    for mode in ("basic", "batch"):
        for resident in (False, True):
            for jitter in ("numpy", "counter"):
                warm = fly(maps, start, goals, sids, mode, resident, jitter, detail=False)
                res = fly(maps, start, goals, sids, mode, resident, jitter, detail=False)
                res["warm_up_wall_s"] = warm["wall_s"]
                runs.append(res)
    dump(dict(kernels=rows, runs=runs))
    sys.exit(0)

# ---- kernels: B missions on scene 0, timed on the state a short fleet run leaves (arrays a few plans long)
stream = torch.cuda.Stream()          # (not the null stream: its handle 0 would hand the context back its own stream)
torch.cuda.set_stream(stream)
ctx.set_stream(stream.cuda_stream)
m = scene_map(0)
B = a.batch
start, goals, _ = draw_missions([m], B, seed=0)
bp = npa.BatchPlanner(ctx=ctx)
loop = npa.FleetReplanLoop(bp, m, goals, seed=0)
ctx.check(ctx.lib.neo_profile_enable(ctx.h, 1))      # HIP events around the optimiser launches of the run's plans
out = loop.run(start, max_replans=12)
n_opt, opt_ms = ctypes.c_int64(0), ctypes.c_double(0.0)
ctx.check(ctx.lib.neo_profile_read(ctx.h, _lib.NEO_KERNEL_OPTIMIZE, ctypes.byref(n_opt), ctypes.byref(opt_ms)))
ctx.check(ctx.lib.neo_profile_enable(ctx.h, 0))
opt_ms_tick = opt_ms.value / len(loop.timings)
d = loop._dev
p = lambda v: ctypes.c_void_p(v.data_ptr()) if v is not None else None
plan_ms = [t["plan_s"] * 1e3 for t in loop.timings]
n_cmd = d["cmd_len"].cpu().numpy()
d["n_flown"].copy_(d["cmd_len"])
M = int(bp.cfg.init_wpts_num) + 1
d["solved"].fill_(1)
lib, h = ctx.lib, ctx.h
calls = {
    "target": lambda: lib.neo_fleet_target_batch_dev(h, m.scene_id, None, B, None, 0, p(d["cur_pos"]), p(d["goal"]),
                                                     p(d["jitter"]), 5.0, 1.0, loop.move_vel, p(d["tail"]), p(d["near"]),
                                                     p(d["steps"]), p(d["flags"])),
    # (step 0: the index stays, so that every launch reads the same rows)
    "advance": lambda: lib.neo_fleet_advance_dev(h, B, None, 0, p(d["cmd"]), loop.cap, p(d["cmd_len"]), p(d["cmd_index"]),
                                                 p(d["future_index"]), 0, 60, p(d["cur_pos"]), p(d["head"])),
    "splice": lambda: lib.neo_fleet_splice_dev(h, B, None, 0, M, p(d["x"]), p(d["head"]), p(d["tail"]), p(d["solved"]), 60.0,
                                               0, p(d["cmd"]), loop.cap, p(d["cmd_len"]), p(d["cmd_index"]),
                                               p(d["future_index"]), p(d["flags"])),
    "audit": lambda: lib.neo_fleet_audit_batch_dev(h, m.scene_id, None, B, None, 0, p(d["cmd"]), loop.cap, p(d["n_flown"]),
                                                   loop.stride, 60.0, None, p(d["audit"]), p(d["count"]),
                                                   p(d["audit_flags"])),
}
# the batch mode's kernels on the run's last look-ahead states and targets: 4096 requests x 3 candidates; select on the
# results of one optimiser launch over the 12 288 candidates (not timed here)
bufs = bp.batch_buffers(B, 3, dev)
_, tau = bp._batch_ts_tau(M - 1)
w4 = _lib.as_f64(bp.cfg.weights)
calls["batch_candidates"] = lambda: lib.neo_batch_candidates_dev(h, B, None, 0, M, 2, 3, p(d["head"]), p(d["tail"]), None,
                                                                 _lib.ptr(tau), None, p(bufs["x_k"]), p(bufs["head_k"]),
                                                                 p(bufs["tail_k"]), None)
calls["batch_select"] = lambda: lib.neo_batch_select_dev(
    h, B, None, 0, M, 2, 3, p(bufs["x_k"]), p(bufs["costs_k"]), p(bufs["last_k"]), p(bufs["nit_k"]), p(bufs["nfev_k"]),
    p(bufs["status_k"]), _lib.ptr(w4), p(bufs["chosen"]), p(bufs["candidate_cost"]), p(bufs["solved"]), p(bufs["x"]),
    p(bufs["costs"]), p(bufs["costs_last"]), p(bufs["nit"]), p(bufs["nfev"]), p(bufs["status"]), p(bufs["nit_total"]),
    p(bufs["opt_runs"]), p(bufs["fallback"]), p(bufs["n_fallback"]))
# the resident plan's kernels on the same states: the guess of a re-seeded attempt (with jitter) for 4096 requests, and the
# merge of one optimiser launch's results (not timed here) with its compaction launch
pb = bp.plan_buffers(B, dev)
frac, ptau = bp._plan_frac_tau(M - 1)
pb["noise"].copy_(torch.from_numpy(np.random.default_rng(0).normal(0.0, 0.5, tuple(pb["noise"].shape))))
calls["plan_guess"] = lambda: lib.neo_plan_guess_dev(h, B, None, 0, M, 2, p(d["head"]), p(d["tail"]), None, None, p(pb["noise"]),
                                                     _lib.ptr(frac), _lib.ptr(ptau), p(pb["x_k"]), p(pb["head_k"]),
                                                     p(pb["tail_k"]), None)
calls["plan_merge"] = lambda: lib.neo_plan_merge_dev(
    h, B, None, 0, M, 2, 0, p(pb["x_k"]), p(pb["costs_k"]), p(pb["last_k"]), p(pb["nit_k"]), p(pb["nfev_k"]), p(pb["status_k"]),
    p(pb["x"]), p(pb["costs"]), p(pb["costs_last"]), p(pb["nit"]), p(pb["nfev"]), p(pb["status"]), p(pb["attempts"]),
    p(pb["nit_total"]), p(pb["solved"]), p(pb["todo"][0]), p(pb["counts"][0:]), p(pb["counts"][1:]))
stream.synchronize()
bp.batch_plan_dev(m, d["head"], d["tail"], bufs)
bp.plan_dev(m, d["head"], d["tail"], pb, max_attempts=1, seed=0)       # (leaves one launch's packed results in pb)
ctx.synchronize()
rows = []
for name in ("advance", "target", "splice", "audit", "batch_candidates", "batch_select", "plan_guess", "plan_merge"):
    for _ in range(3):
        ctx.check(calls[name]())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(a.launches):
        ctx.check(calls[name]())
    e1.record(stream)
    e1.synchronize()
    us = 1e3 * e0.elapsed_time(e1) / a.launches
    row = dict(kernel=name, batch=B, us_per_launch=round(us, 2))
    if name == "splice":
        cnt = d["cmd_len"].cpu().numpy() - d["future_index"].cpu().numpy()
        row.update(rows_written_mean=float(cnt.mean()), gbytes_per_s=float(cnt.sum() * 48 / (us * 1e-6) / 1e9))
    if name == "audit":
        cnt = d["count"].cpu().numpy()
        row.update(samples_mean=float(cnt.mean()), lookups_per_s=float(cnt.sum() / (us * 1e-6)), rows_mean=float(n_cmd.mean()))
    if name == "target":
        row.update(lateral_steps_mean=float(d["steps"].cpu().numpy().mean()))
    if name == "batch_candidates":
        row.update(candidates=3 * B)
    if name == "batch_select":       # (select and its compaction launch)
        row.update(candidates=3 * B, fallback=int(bufs["n_fallback"].item()), launches_per_call=2)
    if name == "plan_merge":         # (merge and its compaction launch; the memset of the bad-scene word)
        row.update(failed=int(pb["counts"][0].item()), launches_per_call=2)
    rows.append(row)
    print(f"{name:>8}: {us:8.1f} us per launch of {B} " + " ".join(f"{k}={v:.4g}" for k, v in row.items()
                                                                     if k not in ("kernel", "batch", "us_per_launch")), flush=True)
print(f"plan launches of the same run's ticks (B = {B}, host arrays in and out): median {np.median(plan_ms):.1f} ms, "
      f"min {min(plan_ms):.1f} ms a tick", flush=True)
print(f"optimiser kernels of those plans (HIP events): {opt_ms.value:.1f} ms in {n_opt.value} launches over {len(loop.timings)} "
      f"ticks = {opt_ms_tick:.2f} ms a tick; a tenth of that is {100 * opt_ms_tick:.0f} us", flush=True)
ctx.set_stream(None)
dump(dict(kernels=rows, optimise_ms_per_tick=round(opt_ms_tick, 3), optimise_launches=int(n_opt.value), plan_ms_per_tick=[round(v, 3) for v in plan_ms], plan_ms_median=float(np.median(plan_ms))))
