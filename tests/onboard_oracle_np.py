"""NumPy restatement of the onboard mapping model (include/neo_planner.h, neo_onboard_integrate_batch): one depth image
into one mission's 2-D log-odds grid, octomap's scan insertion projected to 2-D.  Not a test: tests/test_onboard_cpu.py
holds it to the scenes' true footprints, tests/test_gpu_onboard.py holds the kernel to its bits.

The ray directions are the depth camera's own float32 values (tests/depth_oracle_np.py) widened to float64; everything
after that is one float64 NumPy operation per model operation (no product and sum in one expression that a compiler
could fuse -- NumPy fuses none), integers from there on."""
import math

import numpy as np

f32 = np.float32
UNKNOWN = -128                      # the log-odds byte of a cell never updated
LOGODDS = (17, -8, -40, 70)         # hit, miss, lo, hi in units of 0.05: octomap's 0.7 / 0.4 / 0.12 / 0.97


def camera_tables(width, height, focal_px):
    """the renderer's float32 pixel tables u (W,), v (H,)"""
    u = ((np.arange(width) - (width - 1) / 2.0) / focal_px).astype(f32)
    v = ((np.arange(height) - (height - 1) / 2.0) / focal_px).astype(f32)
    return u, v


def directions(u, v, c, s):
    """dx (W,), dy (W,), dz (H,) float64: the renderer's float32 direction components, each product and sum rounded on
    its own in float32, then widened"""
    c, s = f32(c), f32(s)
    us = u * s
    dx = c + us
    uc = u * c
    dy = s - uc
    assert dx.dtype == f32 and dy.dtype == f32
    return dx.astype(np.float64), dy.astype(np.float64), (-v).astype(np.float64)


def n_samples(sensor_range, res):
    return int(math.ceil(sensor_range / (res / 2)))


def window_half(u, sensor_range, res):
    """cells from the eye's cell to the edge of the window a scan can touch: a point lies d along the axis and d u across
    it, so at most sensor_range sqrt(1 + u_max^2) from the eye (1e-6 of slack for the float32 directions), plus one cell
    for the eye's place in its own cell.  The window is (2 half + 1)^2 cells."""
    umax = float(max(abs(float(u[0])), abs(float(u[-1]))))
    ext = sensor_range * math.sqrt(1.0 + umax * umax) * (1.0 + 1e-6)
    return int(math.ceil(ext / res)) + 1


def cells_of(px, py, res, origin, grid_w, grid_h):
    """flat cell index (row * grid_w + column) of each point, -1 outside the grid (or NaN)"""
    fx = (px - origin[0]) / res
    fy = (py - origin[1]) / res
    ok = (fx >= 0) & (fy >= 0) & (fx < grid_w) & (fy < grid_h)
    ix = np.where(ok, fx, 0.0).astype(np.int64)
    iy = np.where(ok, fy, 0.0).astype(np.int64)
    return np.where(ok, iy * grid_w + ix, -1)


def scan_marks(depth_m, u, v, c, s, eye, grid_w, grid_h, res, origin, sensor_range=6.0, z_band=(1.8, 10.0)):
    """the marks of one scan: (hit, passed) boolean arrays over the grid_h * grid_w cells, unions over the pixels"""
    H, W = depth_m.shape
    ex, ey, ez = (float(e) for e in eye)
    z_lo, z_hi = float(z_band[0]), float(z_band[1])
    dx, dy, dz = directions(u, v, c, s)
    ncell = grid_w * grid_h
    hit = np.zeros(ncell, dtype=bool)
    passed = np.zeros(ncell, dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        d = depth_m.astype(np.float64)
        valid = ~np.isnan(d)
        # ---- hits
        zt = d * dz[:, None]
        z = ez + zt
        is_hit = valid & (d < sensor_range) & (z_lo <= z) & (z <= z_hi)
        tx = d * dx[None, :]
        ty = d * dy[None, :]
        hc = cells_of(ex + tx, ey + ty, res, origin, grid_w, grid_h)
        hc = hc[is_hit & (hc >= 0)]
        hit[hc] = True
        # ---- free space: the cells depend on (column, sample), the band on (row, sample)
        N = n_samples(sensor_range, res)
        half = res / 2
        t = np.arange(N) * half
        sx = t[None, :] * dx[:, None]
        sy = t[None, :] * dy[:, None]
        cell_jn = cells_of(ex + sx, ey + sy, res, origin, grid_w, grid_h)          # (W, N)
        szt = t[None, :] * dz[:, None]
        sz = ez + szt
        band_in = (z_lo <= sz) & (sz <= z_hi)                                      # (H, N)
        m = np.where(d < sensor_range, d, sensor_range)
        count = np.searchsorted(t, m, side="left")                                 # samples with t_n < min(d, range)
        count = np.where(valid, count, 0)                                          # (H, W)
        mark_jn = np.zeros((W, N), dtype=bool)
        rows = max(1, (1 << 22) // max(1, W * N))
        ns = np.arange(N)
        for i0 in range(0, H, rows):
            k = count[i0:i0 + rows]                                                # (h, W)
            p = (ns[None, None, :] < k[:, :, None]) & band_in[i0:i0 + rows, None, :]
            mark_jn |= p.any(axis=0)
        pc = cell_jn[mark_jn & (cell_jn >= 0)]
        passed[pc] = True
    return hit, passed


def apply_marks(logodds, hit, passed, lodds=LOGODDS):
    """the per-cell update.  logodds (grid_h, grid_w) int8 -> (logodds, occupancy, changed)"""
    l_hit, l_miss, l_lo, l_hi = (int(x) for x in lodds)
    shape = logodds.shape
    L = logodds.reshape(-1).astype(np.int64)
    was_occ = (L != UNKNOWN) & (L >= 0)
    L0 = np.where(L == UNKNOWN, 0, L)
    only_passed = passed & ~hit
    new = np.where(hit, np.minimum(L0 + l_hit, l_hi), np.where(only_passed, np.maximum(L0 + l_miss, l_lo), L))
    occ = np.where(new == UNKNOWN, -1, np.where(new >= 0, 100, 0)).astype(np.int8)
    changed = int(np.any((occ == 100) != was_occ))
    return new.astype(np.int8).reshape(shape), occ.reshape(shape), changed


def integrate(logodds, depth_m, u, v, c, s, eye, res, origin, sensor_range=6.0, z_band=(1.8, 10.0), lodds=LOGODDS):
    """one scan into one grid: (logodds, occupancy, changed, hit, passed)"""
    grid_h, grid_w = logodds.shape
    hit, passed = scan_marks(depth_m, u, v, c, s, eye, grid_w, grid_h, res, origin, sensor_range, z_band)
    new, occ, changed = apply_marks(logodds, hit, passed, lodds)
    return new, occ, changed, hit.reshape(grid_h, grid_w), passed.reshape(grid_h, grid_w)


def empty(grid_w, grid_h):
    return np.full((grid_h, grid_w), UNKNOWN, dtype=np.int8)


def heading(step, fallback):
    """the fleet's heading rule (neo_fleet_pose_dev): the unit vector of `step`, of `fallback` where step has no length,
    (1, 0) where neither has -- sqrt and division only, every operation rounded on its own"""
    for d in (step, fallback):
        dx, dy = float(d[0]), float(d[1])
        xx = dx * dx
        yy = dy * dy
        n = math.sqrt(xx + yy)
        if n > 0.0 and math.isfinite(n):
            return dx / n, dy / n
    return 1.0, 0.0


def yaw_of(c, s):
    """a yaw whose float32 cosine and sine are exactly float32(c) and float32(s): what tests/depth_oracle_np.render needs
    to draw the image of a pose given by its heading (arctan2, then a few neighbouring doubles if a rounding differs)"""
    want = (f32(c), f32(s))
    yaw = float(np.arctan2(s, c))
    cand = [yaw]
    up = down = yaw
    for _ in range(8):
        up, down = np.nextafter(up, np.inf), np.nextafter(down, -np.inf)
        cand += [float(up), float(down)]
    for y in cand:
        if (f32(np.cos(y)), f32(np.sin(y))) == want:
            return y
    raise ValueError("no yaw reproduces the heading's float32 cosine and sine")
