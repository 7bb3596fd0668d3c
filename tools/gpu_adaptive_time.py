#!/usr/bin/env python3
"""Times adaptive waypoint counts (neo_adaptive_*, BatchPlanner.plan_dev(waypoints="adaptive")).

  kernels  adaptive_count_kernel and adaptive_bucket_kernel at P = 4096 and 65 536 random 2-D requests 10 - 28 m long: HIP
           events on the context's stream around 20 launches of each after 3 warm-up launches
  plan     4096 cfg2-style 2-D requests (synth.replan_requests: L uniform in 10 - 28 m) on a synthetic forest map, planned
           three ways, each called once as a warm-up and then `--calls` times in turn by the wall clock:
             (a) one plan_dev(waypoints="adaptive") call;
             (b) the same requests at what there was before: one plan_dev(waypoints=c, subset=...) call per distinct
                 count, back to back (the counts and the grouping taken from the host, outside the clock);
             (c) every request with 20 waypoints (M = 21).
           Per way: wall time a call, L-BFGS iterations, the share solved, and the mean final cost of the requests all
           three ways solve.

Each part is one process; run them one after the other, every one under its own time limit, e.g.
  timeout -k 10 120 python tools/gpu_adaptive_time.py kernels --json profiles/adaptive_kernels.json && \\
  timeout -k 10 300 python tools/gpu_adaptive_time.py plan --json profiles/adaptive.json
Prints one line per figure; --json PATH also writes them."""
import argparse, ctypes, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "neo-planner_amd"))
import numpy as np, torch
import neo_planner_amd as npa
from neo_planner_amd import synth, _lib

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["kernels", "plan"])
ap.add_argument("--requests", type=int, default=4096)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--scene", type=int, default=1)
ap.add_argument("--mode", default="f64", choices=["f64", "f32", "f32x"])
ap.add_argument("--json", default=None)
a = ap.parse_args()

dev = torch.device("cuda", 0)
ctx = _lib.default_context()
p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
G = _lib.NEO_MAX_PIECES


def dump(obj):
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(obj, f, indent=1)


if a.what == "kernels":
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    L, h = ctx.lib, ctx.h
    res = dict(launches=a.launches, warmup=a.warmup)

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

    for P in (4096, 65536):
        hd, tl, _, _ = synth.replan_requests(a.scene, P, 1, D=2)
        head, tail = up(hd), up(tl)
        counts = torch.zeros(P, dtype=torch.int32, device=dev); clamped = torch.zeros(P, dtype=torch.int32, device=dev)
        order = torch.zeros(P, dtype=torch.int32, device=dev); table = torch.zeros(G + 2, dtype=torch.int32, device=dev)
        k_count = lambda: ctx.check(L.neo_adaptive_count_dev(h, P, None, 0, 2, p(head), p(tail), 2.0, 63, p(counts), p(clamped)))
        k_bucket = lambda: ctx.check(L.neo_adaptive_bucket_dev(h, P, None, 0, p(counts), p(order), p(table), p(table[G + 1:])))
        for name, fn in (("count", k_count), ("bucket", k_bucket)):
            res[f"{name}_ms_{P}"] = round(events(fn), 4)
            print(f"{name}: {res[f'{name}_ms_{P}']:.4f} ms for {P} requests", flush=True)
        groups = np.bincount(counts.cpu().numpy(), minlength=G)
        res[f"groups_{P}"] = {int(c): int(k) for c, k in enumerate(groups) if k}
    ctx.set_stream(None)
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    dump(res)
    sys.exit(0)

# ---- plan: the three ways
B = a.requests
m = npa.ESDF(ctx=ctx)
m.occupancy_map_cb(synth.OccupancyGridMsg(synth.occupancy_2d(a.scene)))
bp = npa.BatchPlanner(ctx=ctx, sample_dtype=a.mode)
hd, tl, _, _ = synth.replan_requests(a.scene, B, 1, D=2)
head, tail = up(hd), up(tl)
counts, clamped = bp.adaptive_counts(hd, tl)
distinct = [int(c) for c in np.unique(counts)]
groups = {c: up(np.flatnonzero(counts == c).astype(np.int32)) for c in distinct}
w = np.asarray(bp.cfg.weights, dtype=np.float64)
SEED = 11
print(f"{B} requests, counts {distinct[0]} .. {distinct[-1]}: {[int((counts == c).sum()) for c in distinct]}", flush=True)

bufs_a = bp.plan_buffers(B, dev, waypoints="adaptive")
bufs_b = {c: bp.plan_buffers(B, dev, waypoints=c) for c in distinct}
bufs_c = bp.plan_buffers(B, dev, waypoints=20)
torch.cuda.synchronize(dev)


def way_a():
    bp.plan_dev(m, head, tail, bufs=bufs_a, waypoints="adaptive", seed=SEED, jitter="counter")
    return [bufs_a]


def way_b():
    for c in distinct:
        bp.plan_dev(m, head, tail, bufs=bufs_b[c], subset=groups[c], waypoints=c, seed=SEED, jitter="counter")
    return [bufs_b[c] for c in distinct]


def way_c():
    bp.plan_dev(m, head, tail, bufs=bufs_c, waypoints=20, seed=SEED, jitter="counter")
    return [bufs_c]


def gathered(used, by_group):
    """solved, nit_total, final cost by request"""
    solved = np.zeros(B, bool); nit = np.zeros(B, np.int64); cost = np.zeros(B)
    for k, d in enumerate(used):
        rows = groups[distinct[k]].cpu().numpy() if by_group else np.arange(B)
        solved[rows] = d["solved"].cpu().numpy()[rows] != 0
        nit[rows] = d["nit_total"].cpu().numpy()[rows]
        cost[rows] = (d["costs"].cpu().numpy()[rows] * w).sum(axis=1)
    return solved, nit, cost


res = dict(requests=B, mode=a.mode, scene=a.scene, calls=a.calls, counts={c: int((counts == c).sum()) for c in distinct}, ways={})
ways = (("a_adaptive", way_a, False), ("b_per_count", way_b, True), ("c_fixed_20", way_c, False))
for _, fn, _ in ways:
    fn()                                                     # warm-up: first-use allocations and caches
walls = {name: [] for name, _, _ in ways}
used = {}
for _ in range(a.calls):                                     # the three ways in turn, so that a drift of the machine meets all of them
    for name, fn, _ in ways:
        ctx.synchronize()
        t0 = time.perf_counter()
        used[name] = fn()                                    # (plan_dev returns after its last wait for the stream)
        walls[name].append(1e3 * (time.perf_counter() - t0))
got = {}
for name, _, by_group in ways:
    solved, nit, cost = got[name] = gathered(used[name], by_group)
    r = dict(wall_ms_median=round(float(np.median(walls[name])), 3), wall_ms_min=round(min(walls[name]), 3),
             wall_ms_max=round(max(walls[name]), 3), lbfgs_iterations=int(nit.sum()), solved_share=round(float(solved.mean()), 4))
    if name == "a_adaptive":
        r.update(launch_sizes=bufs_a["launch_sizes"], host_waits=sum(bufs_a["host_waits"].values()),
                 optimiser_launches=sum(len(v) for v in bufs_a["group_launch_sizes"].values()))
    elif name == "b_per_count":
        r.update(host_waits=sum(len(bufs_b[c]["launch_sizes"]) for c in distinct),
                 optimiser_launches=sum(len(bufs_b[c]["launch_sizes"]) for c in distinct))
    else:
        r.update(launch_sizes=bufs_c["launch_sizes"], host_waits=len(bufs_c["launch_sizes"]), optimiser_launches=len(bufs_c["launch_sizes"]))
    res["ways"][name] = r
    print(f"{name}: {r['wall_ms_median']} ms a call (median of {a.calls}; {r['wall_ms_min']} .. {r['wall_ms_max']}), {r['lbfgs_iterations']} "
          f"L-BFGS iterations, {100 * r['solved_share']:.2f} % solved, {r['optimiser_launches']} optimiser launches, {r['host_waits']} host waits",
          flush=True)
common = got["a_adaptive"][0] & got["b_per_count"][0] & got["c_fixed_20"][0]
res["commonly_solved"] = int(common.sum())
for name in got:
    res["ways"][name]["mean_final_cost_commonly_solved"] = round(float(got[name][2][common].mean()), 6) if common.any() else None
    print(f"{name}: mean final cost of the {int(common.sum())} commonly solved requests {res['ways'][name]['mean_final_cost_commonly_solved']}", flush=True)
res["a_equals_b"] = bool(all(np.array_equal(x, y) for x, y in zip(got["a_adaptive"], got["b_per_count"])))
print(f"(a) and (b) give the same solved flags, iterations and costs: {res['a_equals_b']}", flush=True)
dump(res)
