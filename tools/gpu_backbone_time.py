#!/usr/bin/env python3
"""Times the HIP image backbone (neo_backbone_features_dev, csrc/neo_backbone.hpp) and flies a fleet on it.

  kernels  for n images of W x H (64 and 512 of 160 x 120, 64 of 640 x 480): every launch of the chain
           (neo_backbone_launch_times: an event behind every launch; the median of --reps calls after --warmup), the whole
           backbone by HIP events around --reps calls on the context's stream, as time and as a fraction of the 157.3
           TFLOP/s fp32 matrix peak (FLOPs counted from the layer shapes, padding taps included); at 512 images the same
           for backbone_chunk 32 .. 512; next to them, in the same process, BatchInitializer.image_features on the torch
           module with CONV_IMPL "gemm" and "miopen" (64 images a pass, torch's stream, by events)
  fleet    the 512 missions of tools/gpu_neo_fleet_time.py fleet (same scenes, seeds, recording and training), flown in
           mode `neo` with the trained network on the torch backbone and on the kernel backbone, and in mode `basic`:
           tick, neo_s and plan_s a tick

  --bf16   kernels: next to the fp32 kernels the bf16 route (neo_backbone_features_bf16_dev, csrc/neo_backbone_bf16.hpp),
           every launch with its share of the 2.5 PF bf16 matrix peak, and MIOpen, without the chunk sweep and the torch
           GEMM route (profiles/backbone_bf16.json); fleet: `basic`, `neo` on "kernel" and `neo` on "kernel_bf16"
           (profiles/backbone_bf16_fleet.json)

Each part is one process; run them one after the other, every one under its own time limit, e.g.
  timeout -k 10 600 python tools/gpu_backbone_time.py kernels --json profiles/backbone.json && \\
  timeout -k 10 900 python tools/gpu_backbone_time.py fleet --json profiles/backbone_fleet.json
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
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--no-miopen", action="store_true")
ap.add_argument("--bf16", action="store_true",
                help="kernels: also the bf16 route (neo_backbone_features_bf16_dev), without the chunk sweep and the torch GEMM "
                     "route; fleet: basic, neo on 'kernel' and neo on 'kernel_bf16'")
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
PEAK_TFLOPS = 157.3
PEAK_BF16_TFLOPS = 2500.0        # dense bf16 matrix peak of the chip


def dump(obj):
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(obj, f, indent=1)


def chain(n, H, W):
    """(name, FLOPs) of the 21 launches for n images of H x W, in launch order"""
    size = lambda s, stride: (s - 1) // stride + 1
    hc, wc = size(H, 2), size(W, 2)
    h, w = size(hc, 2), size(wc, 2)
    out = [("stem 7x7 1->64 + pool", 2 * 49 * 64 * n * hc * wc)]
    cin = 64
    for li, cout in enumerate((64, 128, 256, 512)):
        for blk in range(2):
            s = 2 if (li and blk == 0) else 1
            ho, wo = size(h, s), size(w, s)
            out.append((f"layer{li + 1}.{blk}.conv1 3x3 {cin}->{cout}", 2 * 9 * cin * cout * n * ho * wo))
            if s != 1 or cin != cout:
                out.append((f"layer{li + 1}.{blk}.downsample 1x1 {cin}->{cout}", 2 * cin * cout * n * ho * wo))
            out.append((f"layer{li + 1}.{blk}.conv2 3x3 {cout}->{cout}", 2 * 9 * cout * cout * n * ho * wo))
            h, w, cin = ho, wo, cout
    out.append(("avgpool + fc", n * (512 * h * w + 2 * 512 * 24)))
    return out


if a.what == "kernels":
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    torch.manual_seed(0)
    res = dict(reps=a.reps, warmup=a.warmup, peak_tflops=PEAK_TFLOPS, sizes={})

    def events(fn, reps=a.reps, warmup=a.warmup):
        torch.cuda.synchronize(dev)
        for _ in range(warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    for n, H, W in ((64, 120, 160), (512, 120, 160), (64, 480, 640)):
        key = f"{n}x{W}x{H}"
        net = ini.PlannerNet(H, W).to(dev).eval()
        init = ini.BatchInitializer(net, device=dev)
        blob = init.backbone_weights()
        img = torch.randint(0, 256, (n, H, W), dtype=torch.uint8, device=dev)
        out = torch.zeros((n, 24), dtype=torch.float32, device=dev)
        layers = chain(n, H, W)
        flops = sum(f for _, f in layers)
        r = dict(images=n, width=W, height=H, gflop=round(flops / 1e9, 2))

        def whole(chunk):
            ws = torch.empty(int(ctx.lib.neo_backbone_workspace_bytes(min(chunk, n), H, W)), dtype=torch.uint8, device=dev)
            return events(lambda: ini.backbone_features_kernel(ctx, blob, img, out=out, chunk=chunk, workspace=ws))

        ws = torch.empty(int(ctx.lib.neo_backbone_workspace_bytes(n, H, W)), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        ms = (ctypes.c_float * _lib.NEO_BACKBONE_LAUNCHES)()
        rows = []
        for k in range(a.warmup + a.reps):
            ctx.call("neo_backbone_launch_times", p(blob), blob.numel(), p(img), n, H, W, p(ws), ws.numel(), p(out), ms)
            if k >= a.warmup:
                rows.append(list(ms))
        med = np.median(np.asarray(rows), axis=0)
        r["launches"] = [dict(name=name, ms=round(float(t), 4), tflops=round(f / (t * 1e-3) / 1e12, 2))
                         for (name, f), t in zip(layers, med)]
        r["launches_sum_ms"] = round(float(med.sum()), 3)
        for l in r["launches"]:
            print(f"  {key} {l['name']}: {l['ms']:.4f} ms, {l['tflops']:.1f} TF", flush=True)
        del ws
        if a.bf16:
            packed = init.backbone_weights(precision="bf16")
            ws = torch.empty(int(ctx.lib.neo_backbone_bf16_workspace_bytes(n, H, W)), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)
            rows = []
            for k in range(a.warmup + a.reps):
                ctx.call("neo_backbone_bf16_launch_times", p(packed), packed.numel(), p(img), n, H, W, p(ws), ws.numel(), p(out), ms)
                if k >= a.warmup:
                    rows.append(list(ms))
            med = np.median(np.asarray(rows), axis=0)
            r["bf16_launches"] = [dict(name=name, ms=round(float(t), 4), tflops=round(f / (t * 1e-3) / 1e12, 2),
                                       fraction_of_bf16_peak=round(f / (t * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4))
                                  for (name, f), t in zip(layers, med)]
            r["bf16_launches_sum_ms"] = round(float(med.sum()), 3)
            for l in r["bf16_launches"]:
                print(f"  {key} bf16 {l['name']}: {l['ms']:.4f} ms, {l['tflops']:.1f} TF, "
                      f"{100 * l['fraction_of_bf16_peak']:.1f} % of the bf16 peak", flush=True)
            t = events(lambda: ini.backbone_features_kernel(ctx, packed, img, out=out, chunk=n, workspace=ws, precision="bf16"))
            r["bf16_ms"] = round(t, 3)
            r["bf16_tflops"] = round(flops / (t * 1e-3) / 1e12, 2)
            print(f"{key}: bf16 backbone {t:.3f} ms in one call, {r['bf16_tflops']} TF (launches add up to "
                  f"{r['bf16_launches_sum_ms']} ms)", flush=True)
            del ws, packed
        t = whole(n)
        r["kernel_ms"] = round(t, 3)
        r["kernel_tflops"] = round(flops / (t * 1e-3) / 1e12, 2)
        r["kernel_fraction_of_peak"] = round(r["kernel_tflops"] / PEAK_TFLOPS, 3)
        print(f"{key}: kernel backbone {t:.3f} ms in one call, {r['kernel_tflops']} TF = {100 * r['kernel_fraction_of_peak']:.1f} % of the "
              f"matrix peak (launches add up to {r['launches_sum_ms']} ms)", flush=True)
        if a.bf16:
            print(f"{key}: bf16 route {r['kernel_ms'] / r['bf16_ms']:.2f} x as fast as the fp32 kernels", flush=True)
            res["sizes"][key] = r
            dump(res)
            del net, init, blob, img, out
            torch.cuda.empty_cache()
            continue
        if n > 64:
            r["kernel_ms_by_chunk"] = {}
            for chunk in (32, 64, 128, 256, 512):
                r["kernel_ms_by_chunk"][str(chunk)] = round(whole(chunk), 3)
                print(f"{key}: backbone_chunk {chunk}: {r['kernel_ms_by_chunk'][str(chunk)]} ms", flush=True)
        t = events(lambda: init.image_features(img, chunk=64))
        r["torch_gemm_ms"] = round(t, 3)
        print(f"{key}: torch module, CONV_IMPL 'gemm': {t:.3f} ms ({t / r['kernel_ms']:.2f} x the kernel backbone)", flush=True)
        res["sizes"][key] = r
        dump(res)
        del net, init, blob, img, out
        torch.cuda.empty_cache()
    # MIOpen last (its first call of a shape searches for a kernel): whatever it does, the figures above are written
    for key, r in ([] if a.no_miopen else list(res["sizes"].items())):
        n, H, W = r["images"], r["height"], r["width"]
        init = ini.BatchInitializer(ini.PlannerNet(H, W), device=dev)
        img = torch.randint(0, 256, (n, H, W), dtype=torch.uint8, device=dev)
        ini.CONV_IMPL = "miopen"
        t = events(lambda: init.image_features(img, chunk=64), reps=3, warmup=1)
        ini.CONV_IMPL = "gemm"
        r["torch_miopen_ms"] = round(t, 3)
        print(f"{key}: torch module, CONV_IMPL 'miopen': {t:.3f} ms ({t / r['kernel_ms']:.2f} x the kernel backbone)", flush=True)
        dump(res)
        del init, img
        torch.cuda.empty_cache()
    ctx.set_stream(None)
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    sys.exit(0)

# ---- fleet: record, train, fly (the recipe of gpu_neo_fleet_time.py fleet)
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
torch.manual_seed(42)
net, losses, held_out = npa.train_initializer(inputs, labels, net=ini.PlannerNet(H, W), epochs=a.epochs, batch_size=a.batch_size,
                                              device=dev)
res = dict(missions=Bf, size=f"{W}x{H}", train=dict(rows=int(inputs.shape[0]), epochs=a.epochs, held_out_mse=round(held_out, 5)),
           test_seed=1, fleets={})
print(f"recorded {rec.n_rows} rows, trained {a.epochs} epochs: held out {held_out:.4f}", flush=True)
del inputs, rec
torch.cuda.empty_cache()
make = lambda impl: ini.BatchNeoPlanner(bp, ini.BatchInitializer(net=net, device=dev, T_min=bp.cfg.T_min, T_max=bp.cfg.T_max), cam,
                                        backbone_impl=impl)
second = ("neo_kernel_bf16_backbone", "kernel_bf16") if a.bf16 else ("neo_torch_backbone", "torch")
for name, mode, kw in (("basic_resident", "basic", dict(resident=True)), (second[0], "neo", dict(neo=make(second[1]))),
                       ("neo_kernel_backbone", "neo", dict(neo=make("kernel")))):
    fly(1, mode, **kw)                                       # warm-up: first-use allocations and caches
    flights = []
    for _ in range(2):
        loop, out, wall = fly(1, mode, **kw)
        ticks = loop.timings
        per_tick = lambda k: round(1e3 * sum(t.get(k, 0.0) for t in ticks) / len(ticks), 3)
        flights.append(dict(ticks=len(ticks), wall_s=round(wall, 3), tick_ms=per_tick("tick_s"), neo_ms=per_tick("neo_s"),
                            plan_ms=per_tick("plan_s"), opt_runs=int(out["opt_runs"].sum()),
                            iterations_per_run=round(float(out["iter_num"].sum()) / max(int(out["opt_runs"].sum()), 1), 2),
                            success_rate=round(float(out["success"].mean()), 4)))
    r = dict(mode=mode, backbone_chunk=kw["neo"].backbone_chunk if "neo" in kw else None, flights=flights)
    f = flights[-1]
    print(f"{name}: a tick {f['tick_ms']} ms (neo {f['neo_ms']}, plan {f['plan_ms']}); {f['iterations_per_run']} iterations a run; "
          f"{100 * f['success_rate']:.1f} % reach the goal", flush=True)
    res["fleets"][name] = r
    dump(res)
