#!/usr/bin/env python3
"""Times the geo warm start (neo_geo_search_batch_dev, neo_geo.hpp) on a 300^2 synthetic scene at 0.1 m: HIP events on
the context's stream around one launch of --batch requests (after one warm-up launch), and the quantiles of the
searches' expansions and path lengths.  One step per run, so that each can have its own time limit:

    --step local   cfg2-style 2-D requests: starts in free space, 5 m local targets (set_local_target)
    --step raw     the synthetic workload's raw goals (synth.replan_requests tails, 10-28 m away; some blocked)
    --step mask    the blocked-mask build alone (a map update, then one request whose start cell is its target cell)
    --step plan    BatchPlanner.plan from straight lines against geo_plan on the same local requests: attempts, solved

Prints one JSON line; --json PATH appends it to a file."""
import argparse, ctypes, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "neo-planner_amd"))
import numpy as np, torch
import neo_planner_amd as npa
from neo_planner_amd import synth, _lib

ap = argparse.ArgumentParser()
ap.add_argument("--step", choices=("local", "raw", "mask", "plan"), required=True)
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--scene", type=int, default=0)
ap.add_argument("--json", default=None)
a = ap.parse_args()

dev = torch.device("cuda", 0)
ctx = _lib.default_context()
stream = torch.cuda.Stream()          # (not the null stream: its handle 0 would hand the context back its own stream)
torch.cuda.set_stream(stream)
ctx.set_stream(stream.cuda_stream)
occ = synth.occupancy_2d(a.scene)
m = npa.ESDF(ctx=ctx)
m.occupancy_map_cb(synth.OccupancyGridMsg(occ))
bp = npa.BatchPlanner(ctx=ctx)
rng = np.random.default_rng(42)


def local_requests(B):
    starts, targets = [], []
    while len(starts) < B:
        s = np.array([rng.uniform(0.5, 29.5), rng.uniform(-14.5, 14.5)])
        if m.esdf_map[int((s[1] + 15.0) / 0.1), int(s[0] / 0.1)] < 0.6:
            continue
        goal = np.array([rng.uniform(0.0, 30.0), rng.uniform(-15.0, 15.0)])
        if np.linalg.norm(goal - s) < 5.0:
            continue
        p = s + 5.0 * (goal - s) / np.linalg.norm(goal - s)
        starts.append(s)
        targets.append(p)
    return np.array(starts), np.array(targets)


def timed(S, T, reps=1):
    B = len(S)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    st, tg = t(S), t(T)
    kp = torch.zeros((B, 4, 2), dtype=torch.float64, device=dev)
    cost = torch.zeros(B, dtype=torch.float64, device=dev)
    plen, nexp, flags = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3))
    bp.geo_init_dev(m, st, tg, kp, plen, cost, nexp, flags)      # warm-up: mask, workspace
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        bp.geo_init_dev(m, st, tg, kp, plen, cost, nexp, flags)
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    f = flags.cpu().numpy()
    q = lambda v: {str(p): float(np.percentile(v, p)) for p in (50, 90, 99, 100)}
    return dict(ms=min(ms), ms_all=ms, expansions=q(nexp.cpu().numpy()), path_len=q(plen.cpu().numpy()),
                no_path=int(((f & _lib.NEO_GEO_FLAG_NO_PATH) != 0).sum()),
                start_outside=int(((f & _lib.NEO_GEO_FLAG_START_OUTSIDE) != 0).sum()),
                slots=int(ctx.lib.neo_scene_slot(ctx.h, m.scene_id) >= 0))


out = dict(step=a.step, batch=a.batch, scene=a.scene)
if a.step == "local":
    S, T = local_requests(a.batch)
    out.update(timed(S, T, reps=3))
elif a.step == "raw":
    head, tail, _, _ = synth.replan_requests(a.scene, a.batch, 2, D=2)
    out.update(timed(head[:, 0], tail[:, 0], reps=1))
elif a.step == "mask":
    S = np.array([[3.0, 1.0]]); T = S.copy()
    timed(S, T)
    ms = []
    for _ in range(3):
        m.occupancy_map_cb(synth.OccupancyGridMsg(occ))          # a map update: the mask is rebuilt on the next call
        torch.cuda.synchronize()
        r = timed(S, T)                                            # (its warm-up call builds the mask)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        m.occupancy_map_cb(synth.OccupancyGridMsg(occ))
        torch.cuda.synchronize()
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        st, tg = t(S), t(T)
        kp = torch.zeros((1, 4, 2), dtype=torch.float64, device=dev)
        cost = torch.zeros(1, dtype=torch.float64, device=dev)
        plen, nexp, flags = (torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(3))
        e0.record(stream)
        bp.geo_init_dev(m, st, tg, kp, plen, cost, nexp, flags)
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    out.update(mask_plus_trivial_request_ms=min(ms), trivial_request_ms=r["ms"])
else:
    B = min(a.batch, 1024)
    S, T = local_requests(B)
    head = np.zeros((B, 3, 2)); head[:, 0] = S
    tail = np.zeros((B, 3, 2)); tail[:, 0] = T
    t0 = time.perf_counter()
    straight = bp.plan(m, head, tail, seed=7)
    t1 = time.perf_counter()
    g = bp.geo_plan(m, head, tail, seed=7)
    t2 = time.perf_counter()
    for name, r, dt in (("straight", straight, t1 - t0), ("geo", g, t2 - t1)):
        out[name] = dict(solved=float(r["solved"].mean()), attempts_mean=float(r["attempts"].mean()),
                         attempts_max=int(r["attempts"].max()), launches=r.get("launch_sizes"),
                         final_cost_median=float(np.median(r["final_cost"][r["solved"]])) if r["solved"].any() else None,
                         nit_median=float(np.median(r["nit"])), wall_s=dt)
line = json.dumps(out)
print(line)
if a.json:
    with open(a.json, "a") as f:
        f.write(line + "\n")
