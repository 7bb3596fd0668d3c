#!/usr/bin/env python3
"""GPU regression harness: runs a fixed set of calls through two builds of libneo_planner_hip.so and compares the
outputs BIT FOR BIT -- for refactors that must not change any arithmetic (e.g. templating the device code on the
lane-group policy).

    python tools/compare_libs.py tools/probe/old_lib/libneo_ref.so [new.so]      (default new = the in-tree build)
"""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(out):
    sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "neo-planner_amd"))
    import numpy as np
    import neo_planner_amd as npa
    from neo_planner_amd import synth
    res = {}
    occ = synth.occupancy_3d(0, n=160, res=30.0 / 160, canopy=40)
    g3 = npa.ESDF3D.from_occupancy(occ, 30.0 / 160, synth.DOMAIN_ORIGIN)
    g16 = npa.ESDF3D.from_occupancy(occ, 30.0 / 160, synth.DOMAIN_ORIGIN, store="f16")
    m2 = npa.ESDF(); m2.occupancy_map_cb(synth.OccupancyGridMsg(synth.occupancy_2d(3)))
    for tag, M, B, lr in (("M21", 21, 512, (10.0, 28.0)), ("M3", 3, 2048, (4.0, 6.0)), ("M6", 6, 1024, (8.0, 14.0)),
                          ("M41", 41, 128, (14.0, 28.0))):
        h, t, w, ts = synth.replan_requests(5, B, M - 1, D=3, length_range=lr, **synth.VOLUME)
        for dt in ("f32", "f64"):
            bp = npa.BatchPlanner(sample_dtype=dt)
            x0 = bp.pack_x(w, ts)
            e = bp.cost_grad(g3, x0, h, t, want_coeffs=True)
            res[f"{tag}_{dt}_eval_cost"] = e["cost"]; res[f"{tag}_{dt}_eval_grad"] = e["grad"]
            s = bp.sampled_terms(g3, e["coeffs"], ts)
            res[f"{tag}_{dt}_sample_gC"] = s["grad_C"]; res[f"{tag}_{dt}_sample_gT"] = s["grad_T"]
            for wv in (1, 2):
                if dt == "f64" and wv == 2:
                    continue
                o = npa.BatchPlanner(sample_dtype=dt, waves_per_simd=wv).optimize(g3, x0, h, t)
                res[f"{tag}_{dt}_w{wv}_x"] = o["x"]; res[f"{tag}_{dt}_w{wv}_nfev"] = o["nfev"]
        if M <= 8:
            o = npa.BatchPlanner(sample_dtype="f32", lane_groups=True).optimize(g3, bp.pack_x(w, ts), h, t)
            res[f"{tag}_group_x"] = o["x"]; res[f"{tag}_group_nfev"] = o["nfev"]
            o = npa.BatchPlanner(sample_dtype="f32", lane_groups=True).optimize(g16, bp.pack_x(w, ts), h, t)
            res[f"{tag}_group16_x"] = o["x"]
    h, t, w, ts = synth.replan_requests(3, 256, 2, D=2, length_range=(4.0, 6.0))
    for dt in ("f32", "f64"):
        bp = npa.BatchPlanner(sample_dtype=dt)
        o = bp.optimize(m2, bp.pack_x(w, ts), h, t)
        res[f"map2d_{dt}_x"] = o["x"]; res[f"map2d_{dt}_nfev"] = o["nfev"]
    host_forms(res, g3, g16, m2)
    field_kinds(res)
    np.savez(out, **res)


def host_forms(res, g3, g16, m2):
    """every host-pointer entry point of the C ABI, each staged form once below and once above the pinned-mirror
    threshold (B = 1 and B = 4096), multi-scene calls through host scene_ids, optional outputs left out"""
    import numpy as np
    import neo_planner_amd as npa
    from neo_planner_amd import _lib, synth
    ctx, p, g3_default = m2.ctx, _lib.ptr, g3
    m2b = npa.ESDF(); m2b.occupancy_map_cb(synth.OccupancyGridMsg(synth.occupancy_2d(4)))
    h2, t2, w2, ts2 = synth.replan_requests(7, 4096, 2, D=2, length_range=(4.0, 6.0))
    bp = npa.BatchPlanner()
    x2 = bp.pack_x(w2, ts2)
    for B in (1, 4096):
        o = bp.optimize(m2, x2[:B], h2[:B], t2[:B])
        for k in ("x", "costs", "costs_last", "nit", "nfev", "status"):
            res[f"host_opt_B{B}_{k}"] = o[k]
        e = bp.cost_grad(m2, x2[:B], h2[:B], t2[:B], want_coeffs=B == 1)
        for k in ("cost", "costs", "grad", "status") + (("coeffs",) if B == 1 else ()):
            res[f"host_eval_B{B}_{k}"] = e[k]
        K = 40
        state = np.zeros((B, K, 3, 2)); cnt = np.zeros(B, np.int32)
        ctx.check(ctx.lib.neo_eval_traj_batch(ctx.h, B, 3, 2, p(o["x"]), p(h2[:B]), p(t2[:B]), 10.0, K, p(state), p(cnt)))
        res[f"host_traj_B{B}_state"] = state; res[f"host_traj_B{B}_count"] = cnt
    # multi-scene: 2-D ids (optimise, audit, geo), 3-D ids (optimise, audit); the same calls on one scene
    B = 256
    ids2 = np.where(np.arange(B) % 3 == 0, m2b.scene_id, m2.scene_id).astype(np.int32)
    o = bp.optimize(m2, x2[:B], h2[:B], t2[:B], scene_ids=ids2)
    res["host_opt_ids2_x"] = o["x"]; res["host_opt_ids2_status"] = o["status"]
    for tag, a in (("ids2", bp.audit(m2, o["x"], h2[:B], t2[:B], scene_ids=ids2)), ("one2", bp.audit(m2b, o["x"], h2[:B], t2[:B], hz=25.0,
                                                                                                   weights=(1.0, 2.0, 50.0)))):
        for k, v in a.items():
            res[f"host_audit_{tag}_{k}"] = v
    h3, t3, w3, ts3 = synth.replan_requests(9, B, 5, D=3, length_range=(8.0, 14.0), **synth.VOLUME)
    # (a context of its own: a multi-scene call wants every 3-D map of its context in one element type and layout)
    ctx3 = _lib.Context(0)
    g3, g3b = (npa.ESDF3D.from_occupancy(synth.occupancy_3d(k, n=96, res=30.0 / 96, canopy=24), 30.0 / 96, synth.DOMAIN_ORIGIN, ctx=ctx3)
               for k in (0, 1))
    b32 = npa.BatchPlanner(ctx=ctx3, sample_dtype="f32")
    ids3 = np.where(np.arange(B) % 2 == 0, g3b.scene_id, g3.scene_id).astype(np.int32)
    o3 = b32.optimize(g3, b32.pack_x(w3, ts3), h3, t3, scene_ids=ids3)
    res["host_opt_ids3_x"] = o3["x"]; res["host_opt_ids3_nfev"] = o3["nfev"]
    for k, v in b32.audit(g3, o3["x"], h3, t3, scene_ids=ids3).items():
        res[f"host_audit_ids3_{k}"] = v
    e3 = b32.cost_grad(g3, o3["x"], h3, t3, want_coeffs=True)
    s32 = b32.sampled_terms(g3, e3["coeffs"], ts3, io32=True)
    for k, v in s32.items():
        res[f"host_sample_io32_{k}"] = v
    rng = np.random.default_rng(11)
    S = np.column_stack([rng.uniform(0.5, 12.0, 96), rng.uniform(-12.0, 12.0, 96)])
    T = S + rng.uniform(-8.0, 8.0, (96, 2))
    idsg = np.where(np.arange(96) % 2 == 0, m2.scene_id, m2b.scene_id).astype(np.int32)
    for tag, kw in (("one", dict(path_cap=512)), ("nopath", dict()), ("ids", dict(scene_ids=idsg, path_cap=512)),
                    ("capped", dict(max_expansions=200, path_cap=64))):
        g = bp.geo_init(m2, S, T, **kw)
        for k in ("key_pts", "path_len", "path_cost", "expansions", "flags") + (("paths",) if "paths" in g else ()):
            res[f"host_geo_{tag}_{k}"] = g[k]
        if tag in ("one", "ids"):
            plen = np.clip(g["path_len"], 1, 512)
            res[f"host_prune_{tag}"] = bp.geo_prune(m2, np.nan_to_num(g["paths"]), plen, scene_ids=kw.get("scene_ids"))
    pts2 = np.column_stack([rng.uniform(-1.0, 31.0, 5000), rng.uniform(-16.0, 16.0, 5000)])
    res["host_query2_d"], res["host_query2_g"] = m2.query(pts2)
    pts3 = np.column_stack([pts2, rng.uniform(-0.5, 6.0, 5000)])
    for tag, g in (("f32", g3_default), ("f16", g16)):
        res[f"host_query3_{tag}_d"], res[f"host_query3_{tag}_g"] = g.query(pts3)
    d = np.empty(5000)
    ctx.check(ctx.lib.neo_esdf_query(ctx.h, m2.scene_id, 5000, p(np.ascontiguousarray(pts2)), p(d), None))
    res["host_query2_nograd_d"] = d

def field_kinds(res):
    """the dispatch on a 3-D field's layout and element type: every (layout, store) through evaluation, ESDF lookup, audit
    and the optimiser in each arithmetic mode and register allocation; lane groups and budgeted launches where they exist"""
    import numpy as np
    import neo_planner_amd as npa
    from neo_planner_amd import _lib, synth
    occ = synth.occupancy_3d(2, n=96, res=30.0 / 96, canopy=24)
    h, t, w, ts = synth.replan_requests(13, 192, 5, D=3, length_range=(8.0, 14.0), **synth.VOLUME)
    for layout in ("linear", "yz4", "cell8", "brick"):
        for store in ("f32", "f16"):
            ctx = _lib.Context(0)
            g = npa.ESDF3D.from_occupancy(occ, 30.0 / 96, synth.DOMAIN_ORIGIN, store=store, layout=layout, ctx=ctx)
            tag = f"kind_{layout}_{store}"
            for dt in ("f64", "f32", "f32x"):
                bp = npa.BatchPlanner(ctx=ctx, sample_dtype=dt)
                x0 = bp.pack_x(w, ts)
                e = bp.cost_grad(g, x0, h, t, want_coeffs=True)
                res[f"{tag}_{dt}_eval_cost"] = e["cost"]; res[f"{tag}_{dt}_eval_grad"] = e["grad"]
                res[f"{tag}_{dt}_sample_gC"] = bp.sampled_terms(g, e["coeffs"], ts)["grad_C"]
                for wv in (1, 2):
                    o = npa.BatchPlanner(ctx=ctx, sample_dtype=dt, waves_per_simd=wv).optimize(g, x0, h, t)
                    res[f"{tag}_{dt}_w{wv}_x"] = o["x"]; res[f"{tag}_{dt}_w{wv}_nfev"] = o["nfev"]
            res[f"{tag}_audit"] = np.column_stack([np.asarray(v, np.float64) for v in bp.audit(g, o["x"], h, t).values()])
            if layout != "cell8":
                res[f"{tag}_group_x"] = npa.BatchPlanner(ctx=ctx, sample_dtype="f32", lane_groups=True).optimize(g, x0, h, t)["x"]
            if store == "f32" and layout in ("linear", "brick"):
                for dt in ("f64", "f32", "f32x"):
                    o = npa.BatchPlanner(ctx=ctx, sample_dtype=dt).optimize_budgeted(g, x0, h, t, 24)
                    res[f"{tag}_{dt}_budget_x"] = o["x"]; res[f"{tag}_{dt}_budget_nfev"] = o["nfev"]


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2])
    import numpy as np
    libs = [os.path.abspath(sys.argv[1]),
            os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.join(REPO, "neo-planner_amd", "neo_planner_amd", "libneo_planner_hip.so")]
    outs = []
    for i, lib in enumerate(libs):
        out = f"/tmp/neo_cmp_{i}.npz"
        env = dict(os.environ, NEO_PLANNER_LIB=lib)
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", out], env=env)
        outs.append(np.load(out))
    bad = 0
    for k in outs[0].files:
        a, b = outs[0][k], outs[1][k]
        same = a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
        if not same:
            bad += 1
            d = np.abs(a - b).max() / max(np.abs(a).max(), 1e-300) if a.shape == b.shape else float("nan")
            print(f"DIFF {k}: max rel {d:.3e}, {float((a != b).mean()) if a.shape == b.shape else 1.0:.3f} of entries")
    print(f"{len(outs[0].files) - bad} of {len(outs[0].files)} outputs identical bit for bit")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
