#!/usr/bin/env python3
"""Times fleet campaigns (neo_fleet_leg_*, neo_legs.hpp; FleetReplanLoop(goal_sequences=...)).

4096 missions (8 scenes x 512) fly flap campaigns of 4 legs across the synthetic maps (x flaps between 2 and 26, y drawn from
the counter stream), mode basic on resident arrays with the counter jitter:

  campaign   one run(): a leg that ends is closed, audited and the next one opened on the device, the mission stays in the
             tick's launch list
  chained    the parent behaviour: the same legs as four run() calls from the host, one FleetReplanLoop per leg over all
             missions, each started from the position and velocity the leg before ended on (read back from the command
             arrays); with --onboard every run() starts from an empty map

and reports for both: wall time, legs per second, ticks, mean active missions a tick, per-tick time, success per leg index.
Then the close and open kernels alone, HIP events around --launches launches at B missions on the state the campaign left.
With --onboard the missions fly on what they have seen (OnboardMapper, a 64 x 48 camera): success rate and audit of the
later legs against the first legs, with the map kept (campaign) and thrown away (chained).

One process a configuration, each under its own time limit, e.g.
  timeout -k 10 600 python tools/gpu_campaign_time.py --json profiles/campaign.json && \\
  timeout -k 10 900 python tools/gpu_campaign_time.py --onboard --per-scene 128 --json profiles/campaign_onboard.json
Prints one line per figure; --json PATH also writes them."""
import argparse, ctypes, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "neo-planner_amd")); sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np, torch
import neo_planner_amd as npa
from neo_planner_amd import synth, _lib
from neo_planner_amd.fleet import draw_missions
from neo_planner_amd.goal_sequences import GoalSequences

ap = argparse.ArgumentParser()
ap.add_argument("--scenes", type=int, default=8)
ap.add_argument("--per-scene", type=int, default=512)
ap.add_argument("--legs", type=int, default=4)
ap.add_argument("--leg-replans", type=int, default=60, help="tick budget of a leg: a chained run() gets it, the campaign legs times it")
ap.add_argument("--leg-timeout", type=float, default=45.0, help="bash/demo_auto_stop.sh's max_target_find_time")
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--onboard", action="store_true")
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--json", default=None)
a = ap.parse_args()

dev = torch.device("cuda", 0)
ctx = _lib.default_context()
X_PAIR = (2.0, 26.0)      # inside the 30 m maps


def scene_map(s):
    m = npa.ESDF(ctx=ctx)
    m.occupancy_map_cb(synth.OccupancyGridMsg(synth.occupancy_2d(s)))
    return m


maps = [scene_map(s) for s in range(a.scenes)]
start, _, sids = draw_missions(maps, a.per_scene, seed=a.seed)
B = len(start)
flap = GoalSequences.flap(B, a.legs, a.seed, x_pair=X_PAIR)
extra = {}
if a.onboard:
    import depth_oracle_np as don
    from neo_planner_amd.depth import DepthCamera
    from neo_planner_amd.onboard import OnboardMapper
    cam = DepthCamera(width=64, height=48)
    mapper = OnboardMapper(ctx, cam, B)
    extra = dict(onboard=mapper, scenes=DepthCamera.pack_scenes([don.boxes_of(synth.forest_boxes(s)) for s in range(a.scenes)]),
                 scene_index=np.repeat(np.arange(a.scenes), a.per_scene).astype(np.int32))
common = dict(mode="basic", resident=True, jitter="counter", scene_ids=sids, seed=a.seed, leg_timeout=None, **extra)


def ticks_of(timings):
    tot = sum(t["tick_s"] for t in timings)
    return dict(ticks=len(timings), mean_active=float(np.mean([t["active"] for t in timings])), tick_ms_mean=round(1e3 * tot / len(timings), 3),
                tick_ms_full=round(1e3 * float(np.mean([t["tick_s"] for t in timings if t["active"] == B] or [np.nan])), 3),
                legs_ms=round(1e3 * sum(t.get("legs_s", 0.0) for t in timings), 3))


def leg_table(success, outcome, clearance, unsafe):
    """per leg index: legs flown, success rate, outcomes, median minimum clearance, share with an unsafe sample"""
    rows = []
    for k in range(a.legs):
        on = outcome[:, k] > 0
        if not on.any():
            continue
        rows.append(dict(leg=k, flown=int(on.sum()), success_rate=round(float(success[on, k].mean()), 4),
                         landed=int((outcome[on, k] == _lib.NEO_LEG_LANDED).sum()), abandoned=int((outcome[on, k] == _lib.NEO_LEG_ABANDONED).sum()),
                         timeout=int((outcome[on, k] == _lib.NEO_LEG_TIMEOUT).sum()), stuck=int((outcome[on, k] == _lib.NEO_LEG_STUCK).sum()),
                         open=int((outcome[on, k] == _lib.NEO_LEG_OPEN).sum()),
                         median_min_clearance=round(float(np.nanmedian(clearance[on, k])), 4), unsafe_rate=round(float(unsafe[on, k].mean()), 4)))
    return rows


def report(tag, res):
    print(f"{tag}: {res['legs_closed']} legs in {res['wall_s']:.2f} s = {res['legs_per_s']:.0f} legs/s; {res['ticks']} ticks, mean active "
          f"{res['mean_active']:.0f} of {B}, {res['tick_ms_mean']:.1f} ms a tick ({res['tick_ms_full']:.1f} ms with all {B} active)", flush=True)
    for r in res["per_leg"]:
        print(f"{tag}: leg {r['leg']}: {r['flown']} flown, success {r['success_rate']:.3f}, landed {r['landed']} abandoned {r['abandoned']} "
              f"timeout {r['timeout']} stuck {r['stuck']} open {r['open']}, median min clearance {r['median_min_clearance']:.2f} m, unsafe "
              f"{r['unsafe_rate']:.3f}", flush=True)


def fly_campaign():
    loop = npa.FleetReplanLoop(npa.BatchPlanner(ctx=ctx), maps[0], None, goal_sequences=flap, **{**common, "leg_timeout": a.leg_timeout})
    t0 = time.perf_counter()
    out = loop.run(start, max_replans=a.legs * (a.leg_replans + 1) - 1)
    wall = time.perf_counter() - t0
    closed = int(((out["leg_outcome"] > 0) & (out["leg_outcome"] != _lib.NEO_LEG_OPEN)).sum())
    res = dict(wall_s=round(wall, 3), legs_closed=closed, legs_per_s=round(closed / wall, 1), **ticks_of(loop.timings),
               per_leg=leg_table(out["leg_success"] == 1, out["leg_outcome"], out["leg_min_clearance"],
                                 (out["leg_audit_flags"] & _lib.NEO_AUDIT_FLAG_UNSAFE) != 0),
               campaign_success_rate=float(out["success"].mean()))
    return loop, out, res


def fly_chained():
    """the legs as run() calls from the host: every leg a fleet of all B missions, started where the leg before ended"""
    pos, vel = start.copy(), np.zeros_like(start)
    success, outcome = np.zeros((B, a.legs), bool), np.zeros((B, a.legs), np.int32)
    clearance, unsafe = np.full((B, a.legs), np.nan), np.zeros((B, a.legs), bool)
    timings, wall = [], 0.0
    for k in range(a.legs):
        loop = npa.FleetReplanLoop(npa.BatchPlanner(ctx=ctx), maps[0], flap.leg_goals(k), **common)
        t0 = time.perf_counter()
        out = loop.run(pos, vel, max_replans=a.leg_replans)
        # where every mission stopped: the last row it flew (a host read of the command arrays' end rows)
        nf = out["n_flown"]
        last = torch.from_numpy(np.maximum(nf - 1, 0).astype(np.int64)).to(dev)
        end = loop._dev["cmd"][torch.arange(B, device=dev), last, :2].cpu().numpy()
        flew = nf > 0
        pos[flew], vel[flew] = end[flew, 0], end[flew, 1]
        wall += time.perf_counter() - t0
        timings += loop.timings
        success[:, k] = out["success"]
        landed = out["n_flown"] == out["n_cmd"]
        outcome[:, k] = np.where(out["abandoned"], _lib.NEO_LEG_ABANDONED, np.where(landed & (nf > 0), _lib.NEO_LEG_LANDED, _lib.NEO_LEG_OPEN))
        clearance[:, k], unsafe[:, k] = out["min_clearance"], (out["audit_flags"] & _lib.NEO_AUDIT_FLAG_UNSAFE) != 0
    closed = int((outcome != _lib.NEO_LEG_OPEN).sum())
    return dict(wall_s=round(wall, 3), legs_closed=closed, legs_per_s=round(closed / wall, 1), **ticks_of(timings),
                per_leg=leg_table(success, outcome, clearance, unsafe), campaign_success_rate=float(success.all(axis=1).mean()))


# a warm-up flight of one leg (allocations, the first launches), then the two ways, timed
npa.FleetReplanLoop(npa.BatchPlanner(ctx=ctx), maps[0], flap.leg_goals(0), **common).run(start, max_replans=3)
loop, out, camp = fly_campaign()
report("campaign", camp)
chain = fly_chained()
report("chained ", chain)
print(f"campaign against chained: {camp['legs_per_s'] / chain['legs_per_s']:.2f} x the legs per second, mean active "
      f"{camp['mean_active']:.0f} against {chain['mean_active']:.0f}", flush=True)

# ---- the two kernels alone, on the state the campaign left, all B missions a launch
stream = torch.cuda.Stream()          # (not the null stream: its handle 0 would hand the context back its own stream)
torch.cuda.set_stream(stream)
ctx.set_stream(stream.cuda_stream)
d = loop._dev
p = lambda v: ctypes.c_void_p(v.data_ptr()) if v is not None else None
codes = torch.from_numpy((np.arange(B) % 4 + 1).astype(np.int32)).to(dev)      # landed, abandoned, timeout, stuck in turn
n_launch = a.launches + 3
legs_at = torch.zeros((n_launch, B), dtype=torch.int32, device=dev)             # every launch logs leg 0 and opens leg 1
log = torch.zeros((B, loop.max_legs, _lib.NEO_LEG_FIELDS), dtype=torch.float64, device=dev)
lib, h = ctx.lib, ctx.h
stream.synchronize()
close = lambda i: lib.neo_fleet_leg_close_dev(h, B, p(codes), None, 0, p(d["cmd"]), loop.cap, p(d["cmd_len"]), p(d["cmd_index"]),
                                              p(d["head"]), p(d["goal"]), p(d["n_flown"]), p(d["leg_end"]), p(d["final_dist"]))
open_ = lambda i: lib.neo_fleet_leg_open_dev(h, B, p(codes), None, 0, ctypes.byref(loop._seq), loop.max_legs, 0.2, p(d["n_flown"]),
                                             p(d["leg_end"]), p(d["final_dist"]), p(d["count"]), p(d["audit_flags"]), p(d["audit"]),
                                             p(legs_at[i]), p(log), p(d["leg_start"]), p(d["goal"]), p(d["cur_pos"]), p(d["head"]),
                                             p(d["cmd_len"]), p(d["cmd_index"]), p(d["future_index"]), p(d["flags"]))
kernels = []
for name, call in (("leg_close", close), ("leg_open", open_)):      # (close first: open empties the command arrays)
    for i in range(3):
        ctx.check(call(i))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for i in range(3, n_launch):
        ctx.check(call(i))
    e1.record(stream)
    e1.synchronize()
    us = 1e3 * e0.elapsed_time(e1) / a.launches
    kernels.append(dict(kernel=name, batch=B, launches=a.launches, us_per_launch=round(us, 2)))
    print(f"{name:>10}: {us:8.1f} us per launch of {B}", flush=True)
assert int(legs_at.min().item()) == 1 == int(legs_at.max().item())
ctx.set_stream(None)
torch.cuda.set_stream(torch.cuda.default_stream())

res = dict(missions=B, scenes=a.scenes, legs=a.legs, x_pair=list(X_PAIR), onboard=bool(a.onboard), leg_timeout_s=a.leg_timeout,
           leg_replans=a.leg_replans, campaign=camp, chained=chain, kernels=kernels,
           legs_per_s_ratio=round(camp["legs_per_s"] / chain["legs_per_s"], 3))
if a.onboard:      # later legs against first legs, with the map kept and thrown away
    later = lambda rows: [r for r in rows if r["leg"] > 0]
    mean = lambda rows, key: float(np.average([r[key] for r in rows], weights=[r["flown"] for r in rows])) if rows else None
    for tag, rows in (("campaign", camp["per_leg"]), ("chained", chain["per_leg"])):
        res[tag + "_later_vs_first"] = dict(first_success=rows[0]["success_rate"], later_success=mean(later(rows), "success_rate"),
                                            first_unsafe=rows[0]["unsafe_rate"], later_unsafe=mean(later(rows), "unsafe_rate"),
                                            first_clearance=rows[0]["median_min_clearance"],
                                            later_clearance=mean(later(rows), "median_min_clearance"))
        print(f"{tag}: first legs success {rows[0]['success_rate']:.3f} unsafe {rows[0]['unsafe_rate']:.3f}; later legs success "
              f"{res[tag + '_later_vs_first']['later_success']:.3f} unsafe {res[tag + '_later_vs_first']['later_unsafe']:.3f}", flush=True)
    mapper.close()
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
