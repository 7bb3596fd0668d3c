#!/usr/bin/env python3
"""Times the batched depth camera (neo_depth_render_batch_dev, neo_depth.hpp) on one MI355X: 4096 requests in forest
scene 0 with its 80 canopy boxes, eye x in [0.5, 20], y in [-4, 4], z = 2, yaw in [-1, 1] -- at 480 x 640 in chunks of
512 images and at 48 x 64 in one launch.  HIP events on the context's stream around 20 launches after 3 warm-up
launches, once with depth_u8 (render pass + normalise pass) and once without (render pass alone; the normalise pass is
the difference).  Box tests per ray after culling come from neo_depth_box_test_counter in a pass of their own.
Prints one line per case; --json PATH also writes them."""
import argparse, ctypes, json, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "neo-planner_amd"))
import numpy as np, torch
from neo_planner_amd import synth, _lib
from neo_planner_amd.depth import DepthCamera

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--scene", type=int, default=0)
ap.add_argument("--json", default=None)
a = ap.parse_args()

HBM_BYTES_PER_S = 6.29e12        # measured float4 copy rate of an MI355X (79 % of the 8 TB/s specification)
TICK_MS = 31.0                   # optimiser kernels of one 4096-mission tick (fleet kernels)

dev = torch.device("cuda", 0)
ctx = _lib.default_context()
stream = torch.cuda.Stream()          # (not the null stream: its handle 0 would hand the context back its own stream)
torch.cuda.set_stream(stream)
ctx.set_stream(stream.cuda_stream)
boxes = DepthCamera.boxes_of(synth.forest_boxes(a.scene), synth.canopy_boxes(a.scene, 80))
rng = np.random.default_rng(42)
B = a.batch
eye = np.stack([rng.uniform(0.5, 20.0, B), rng.uniform(-4.0, 4.0, B), np.full(B, 2.0)], axis=1)
yaw = rng.uniform(-1.0, 1.0, B)
t = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
p = lambda v: ctypes.c_void_p(v.data_ptr()) if v is not None else None
d_boxes, d_begin = t(boxes), t(np.array([0, boxes.shape[0]], dtype=np.int32))
d_pose = t(DepthCamera.poses(eye, yaw))
counter = torch.zeros(1, dtype=torch.int64, device=dev)
rows = []
for (W, H, chunk) in ((640, 480, 512), (64, 48, B)):
    cam = DepthCamera(ctx=ctx, width=W, height=H)
    chunk = min(chunk, B)
    nchunks = (B + chunk - 1) // chunk
    d_m = torch.empty((chunk, H, W), dtype=torch.float32, device=dev)
    d_u8 = torch.empty((chunk, H, W), dtype=torch.uint8, device=dev)
    d_max = torch.empty(chunk, dtype=torch.float32, device=dev)

    def launch(k, with_u8):
        b0 = (k % nchunks) * chunk
        n = min(chunk, B - b0)
        ctx.check(ctx.lib.neo_depth_render_batch_dev(ctx.h, W, H, cam.focal_px, cam.max_range, p(d_boxes), p(d_begin), 1,
                                                     None, n, p(d_pose[b0:b0 + n]), p(d_m), p(d_u8) if with_u8 else None,
                                                     p(d_max)))
        return n

    # box tests per ray after culling: every chunk once, counted
    counter.zero_()
    torch.cuda.synchronize(dev)
    ctx.check(ctx.lib.neo_depth_box_test_counter(ctx.h, p(counter)))
    for k in range(nchunks):
        launch(k, False)
    ctx.synchronize()
    ctx.check(ctx.lib.neo_depth_box_test_counter(ctx.h, None))
    tests_per_ray = float(counter.item()) / (B * H * W)
    ms = {}
    for with_u8 in (True, False):
        for k in range(3):
            launch(k, with_u8)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        images = sum(launch(k, with_u8) for k in range(a.launches))
        e1.record(stream)
        e1.synchronize()
        ms[with_u8] = e0.elapsed_time(e1) / images          # per image
    both, render = ms[True] * B, ms[False] * B              # per batch of B
    floor = B * H * W * 5 / HBM_BYTES_PER_S * 1e3
    row = dict(width=W, height=H, batch=B, chunk=chunk, boxes=int(boxes.shape[0]), box_tests_per_ray=round(tests_per_ray, 2),
               ms_per_batch=round(both, 3), render_ms=round(render, 3), normalise_ms=round(both - render, 3),
               images_per_s=B / (both * 1e-3), rays_per_s=B * H * W / (both * 1e-3), output_floor_ms=round(floor, 3),
               tick_ms=TICK_MS)
    rows.append(row)
    print(f"{B} x {H}x{W} in chunks of {chunk}: {both:8.2f} ms per batch (render {render:.2f} ms, normalise "
          f"{both - render:.2f} ms); {row['images_per_s']:.0f} images/s, {row['rays_per_s'] / 1e9:.2f} G rays/s; "
          f"{tests_per_ray:.2f} box tests per ray of {boxes.shape[0]} boxes; output floor (5 B a pixel at "
          f"{HBM_BYTES_PER_S / 1e12:.2f} TB/s) {floor:.2f} ms; optimiser tick {TICK_MS:.0f} ms", flush=True)
ctx.set_stream(None)
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(rows, f, indent=1)
