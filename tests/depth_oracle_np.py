"""NumPy float32 restatement of the depth camera's arithmetic (include/neo_planner.h, neo_depth_render_batch), vectorised
over one image.  Not a test: tests/test_depth_cpu.py holds it to initializer.raycast_depth, tests/test_gpu_depth.py
holds the kernel to its bits.

Every per-ray operation is one float32 NumPy operation (each product rounded on its own); the pixel coordinates and the
boxes' corners relative to the eye are computed in float64 and rounded once.  max(tn, 0) and the final clip are written
as selections, so that a zero is +0 whatever NumPy's maximum does with (-0, +0)."""
import numpy as np

f32 = np.float32


def boxes_of(pillars, canopy=()):
    """the (lo, hi) rows exactly as initializer.raycast_depth forms them: (n, 6) float64"""
    rows = [(cx - sx / 2, cy - sy / 2, 0.0, cx + sx / 2, cy + sy / 2, sz) for (cx, cy, sx, sy, sz) in pillars]
    rows += [(cx - sx / 2, cy - sy / 2, cz - sz / 2, cx + sx / 2, cy + sy / 2, cz + sz / 2)
             for (cx, cy, cz, sx, sy, sz) in canopy]
    return np.asarray(rows, dtype=np.float64).reshape(-1, 6)


def focal_px(width, hfov_deg):
    return (width / 2) / np.tan(np.radians(hfov_deg) / 2)


def render(boxes, eye, yaw, width, height, hfov_deg=87.0, max_range=20.0):
    """boxes (n, 6) float64 -> dict(depth_m (H, W) float32, depth_max float32, depth_u8 (H, W) uint8)"""
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 6)
    eye = np.asarray(eye, dtype=np.float64)
    f = focal_px(width, hfov_deg)
    u = ((np.arange(width) - (width - 1) / 2.0) / f).astype(f32)[None, :]
    v = ((np.arange(height) - (height - 1) / 2.0) / f).astype(f32)[:, None]
    c, s = f32(np.cos(yaw)), f32(np.sin(yaw))
    mr = f32(max_range)
    zero = f32(0.0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        us = u * s
        dx = np.broadcast_to(c + us, (height, width))
        uc = u * c
        dy = np.broadcast_to(s - uc, (height, width))
        dz = np.broadcast_to(-v, (height, width))
        inv = [f32(1.0) / dx, f32(1.0) / dy, f32(1.0) / dz]
        tg = np.where(dz < 0, f32(-eye[2]) / dz, f32(np.inf)).astype(f32)
        depth = np.where(tg < mr, tg, mr).astype(f32)
        for row in boxes:
            rel_lo = (row[:3] - eye).astype(f32)
            rel_hi = (row[3:] - eye).astype(f32)
            tn = tf = None
            for a in range(3):
                t0 = rel_lo[a] * inv[a]
                t1 = rel_hi[a] * inv[a]
                near, far = np.minimum(t0, t1), np.maximum(t0, t1)          # NaN propagates
                tn = near if tn is None else np.maximum(tn, near)
                tf = far if tf is None else np.minimum(tf, far)
            enter = np.where(tn > 0, tn, zero)                              # max(tn, 0); a NaN tn gives 0 ...
            hit = (tf >= enter) & ~np.isnan(tn) & ~np.isnan(tf)             # ... and is a miss
            depth = np.where(hit & (enter < depth), enter, depth)
        depth = np.where(depth > 0, depth, zero)
        depth = np.where(depth < mr, depth, mr).astype(f32)
    dmax = f32(depth.max())
    q = depth / max(dmax, f32(1e-9))
    u8 = (q * f32(255.0)).astype(np.uint8)
    assert q.dtype == f32 and depth.dtype == f32
    return dict(depth_m=depth, depth_max=dmax, depth_u8=u8)
