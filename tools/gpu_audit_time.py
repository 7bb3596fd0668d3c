#!/usr/bin/env python3
"""Times the trajectory-audit kernel (neo_audit_traj_batch_dev, neo_audit.hpp) on the cfg2 shape: 4096 trajectories,
M = 21, D = 3, on the fp32 corner-brick field of a 300^3 forest scene, at 10 Hz and 60 Hz -- HIP events on the context's
stream around 20 launches after 3 warm-up launches, for the optimiser's results and for the raw initial guesses.
Prints one line per case; --json PATH also writes them."""
import argparse, ctypes, json, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "neo-planner_amd"))
import numpy as np, torch
import neo_planner_amd as npa
from neo_planner_amd import synth, _lib

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--json", default=None)
a = ap.parse_args()

dev = torch.device("cuda", 0)
ctx = _lib.default_context()
stream = torch.cuda.Stream()          # (not the null stream: its handle 0 would hand the context back its own stream)
torch.cuda.set_stream(stream)
ctx.set_stream(stream.cuda_stream)
occ = synth.occupancy_3d(0, n=300, res=0.1, canopy=80)
g3 = npa.ESDF3D.from_occupancy(torch.from_numpy(occ).to(dev), 0.1, synth.DOMAIN_ORIGIN, store="f32", layout="brick",
                               ctx=ctx)
bp = npa.BatchPlanner(sample_dtype="f32x", ctx=ctx)
head, tail, wp, ts = synth.replan_requests(0, a.batch, 20, D=3, **synth.VOLUME)
x0 = bp.pack_x(wp, ts)
xo = bp.optimize(g3, x0, head, tail)["x"]
t = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
d_head, d_tail = t(head), t(tail)
B = a.batch
audit = torch.zeros((B, _lib.NEO_AUDIT_FIELDS), dtype=torch.float64, device=dev)
count = torch.zeros(B, dtype=torch.int32, device=dev)
flags = torch.zeros(B, dtype=torch.int32, device=dev)
rows = []
p = lambda v: ctypes.c_void_p(v.data_ptr())
for name, x in (("optimised", xo), ("initial guess", x0)):
    d_x = t(x)
    for hz in (10.0, 60.0):
        for _ in range(3):
            bp.audit_dev(g3, d_x, d_head, d_tail, audit, count, flags, hz=hz)
        # the timed launches go straight to the C entry point (the parameters are already on the context): the events
        # bracket the kernels, not BatchPlanner's per-call parameter push
        args = [ctx.h, g3.scene_id, None, B, 21, 3] + [p(v) for v in (d_x, d_head, d_tail)] + [hz, None] + \
            [p(v) for v in (audit, count, flags)]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.launches):
            ctx.check(ctx.lib.neo_audit_traj_batch_dev(*args))
        e1.record(stream)
        e1.synchronize()
        us = 1e3 * e0.elapsed_time(e1) / a.launches
        cnt = count.cpu().numpy()
        fl = flags.cpu().numpy()
        row = dict(x=name, hz=hz, batch=B, us_per_launch=round(us, 2), samples_mean=float(cnt.mean()),
                   samples_max=int(cnt.max()), lookups_per_s=float(cnt.sum() / (us * 1e-6)),
                   unsafe=int(((fl & _lib.NEO_AUDIT_FLAG_UNSAFE) != 0).sum()),
                   nonfinite=int(((fl & _lib.NEO_AUDIT_FLAG_NONFINITE) != 0).sum()))
        rows.append(row)
        print(f"{name:>13} {hz:4.0f} Hz: {us:8.1f} us per launch of {B} ({row['samples_mean']:.0f} samples mean, "
              f"{row['samples_max']} max; {row['lookups_per_s'] / 1e9:.2f} G lookups/s; unsafe {row['unsafe']}, "
              f"nonfinite {row['nonfinite']})", flush=True)
ctx.set_stream(None)
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(rows, f, indent=1)
