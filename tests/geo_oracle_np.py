"""CPU restatement of the reference's geo warm start (traj_planner/astar_planner.py, geo_planner.py:37-101), written from
the algorithm: an A* over the expanded grid whose open set is a heapq keyed (f, seq) -- seq the counter of a node's first
insertion -- with lazy deletion, and the pruning of the path to four key nodes.  Every value is computed with the
reference's fp64 operations in the reference's order, so results are equal, not close.  Used by tests/test_geo_cpu.py
(pinned to the reference's fixtures) and tests/test_gpu_geo.py (random requests)."""
import heapq
import math

import numpy as np

SAFE_DIS = 0.5      # esdf.py: has_collision
SEG_DIS = 0.4       # geo_planner.py:55
EXPAND = 10.0       # astar_planner.py:37
MOVES = [(1, 0, 1), (0, 1, 1), (-1, 0, 1), (0, -1, 1), (-1, -1, math.sqrt(2)), (-1, 1, math.sqrt(2)),
         (1, -1, math.sqrt(2)), (1, 1, math.sqrt(2))]
NO_PATH, START_OUTSIDE, CAPPED = 1, 2, 4


class Map:
    """the 2-D ESDF (H, W) at `res` with origin (ox, oy): esdf.py's nearest-cell get_edt_dis"""

    def __init__(self, esdf, res, origin):
        self.esdf = np.asarray(esdf, dtype=np.float64)
        self.H, self.W = self.esdf.shape
        self.res = float(res)
        self.ox, self.oy = float(origin[0]), float(origin[1])

    def dist(self, x, y):
        r = int((y - self.oy) / self.res)
        c = int((x - self.ox) / self.res)
        if r < 0 or r >= self.H or c < 0 or c >= self.W:
            return 10000
        return float(self.esdf[r, c])


class Grid:
    """the expanded grid of astar_planner.py:36-42 and its blocked cells"""

    def __init__(self, m):
        self.m = m
        self.We = m.W + int(EXPAND / m.res)
        self.He = m.H + int(EXPAND / m.res)
        self.oxe = m.ox - EXPAND / 2
        self.oye = m.oy - EXPAND / 2
        # the position of every cell (two roundings, as calc_real_pos), then the map's nearest-cell lookup
        px = self.oxe + np.arange(self.We) * m.res
        py = self.oye + np.arange(self.He) * m.res
        col = np.trunc((px - m.ox) / m.res)
        row = np.trunc((py - m.oy) / m.res)
        cin = (col >= 0) & (col < m.W)
        rin = (row >= 0) & (row < m.H)
        d = np.full((self.He, self.We), 10000.0)
        ri, ci = np.flatnonzero(rin), np.flatnonzero(cin)
        d[np.ix_(ri, ci)] = m.esdf[np.ix_(row[ri].astype(int), col[ci].astype(int))]
        self.blocked = d < SAFE_DIS          # [y, x]

    def pos(self, ix, iy):
        return [self.oxe + ix * self.m.res, self.oye + iy * self.m.res]

    def index(self, x, y):
        return int((x - self.oxe) / self.m.res), int((y - self.oye) / self.m.res)


def astar(g, start, target, max_expansions=0):
    """-> (path as a list of [x, y], cost, expansions, flags)"""
    sx, sy = g.index(start[0], start[1])
    tx, ty = g.index(target[0], target[1])
    one = ([g.pos(tx, ty)], 0.0)
    We, He = g.We, g.He
    if (sx, sy) == (tx, ty):
        return one + (0, 0)
    skey = sx + sy * We
    if skey < 0 or skey >= We * He:
        return one + (0, START_OUTSIDE)
    if not (0 <= tx < We and 0 <= ty < He) or g.blocked[ty, tx]:
        return one + (0, NO_PATH)
    cost = {skey: 0.0}
    parent = {skey: None}
    xy = {skey: (sx, sy)}
    closed = set()
    heap = [(math.hypot(sx - tx, sy - ty), 0, skey)]
    first_seq = {skey: 0}
    seq = 1
    nexp = 0
    while True:
        while heap and heap[0][2] in closed:
            heapq.heappop(heap)
        if not heap:
            return one + (nexp, NO_PATH)
        _, _, key = heap[0]
        cx, cy = xy[key]
        if (cx, cy) == (tx, ty):
            break
        if max_expansions and nexp >= max_expansions:
            return one + (nexp, CAPPED)
        heapq.heappop(heap)
        closed.add(key)
        nexp += 1
        gc = cost[key]
        for dx, dy, mc in MOVES:
            nx, ny = cx + dx, cy + dy
            nk = nx + ny * We
            if nk in closed or not (0 <= nx < We and 0 <= ny < He) or g.blocked[ny, nx]:
                continue
            ng = gc + mc
            if nk not in cost:                  # first insertion: a new seq
                first_seq[nk] = seq
                seq += 1
                xy[nk] = (nx, ny)
            elif not cost[nk] > ng:             # open (closed ones were skipped): keep unless the cost decreases
                continue
            cost[nk] = ng
            parent[nk] = key
            heapq.heappush(heap, (ng + math.hypot(nx - tx, ny - ty), first_seq[nk], nk))
    path = [g.pos(tx, ty)]
    p = parent[key]
    while p is not None:
        path.append(g.pos(*xy[p]))
        p = parent[p]
    return path[::-1], cost[key], nexp, 0


def seg_feasible(m, p0, p1):
    x0, y0 = p0
    x1, y1 = p1
    n = math.ceil(max(abs(x1 - x0), abs(y1 - y0)) / 0.1) + 1
    xs = np.linspace(x0, x1, n)
    ys = np.linspace(y0, y1, n)
    return all(m.dist(xs[i], ys[i]) >= SEG_DIS for i in range(n))


def prune(m, path):
    """the four key nodes of `path` (geo_planner.py:61-101)"""
    n = len(path)
    keys = [0]
    head, tail = 0, 1
    while tail < n:
        while tail - head == 1 or seg_feasible(m, path[head], path[tail]):
            tail += 1
            if tail == n:
                break
        keys.append(tail - 1)
        head = tail - 1
    if len(keys) == 2:
        sel = [int(v) for v in np.linspace(keys[0], keys[1], 4)]
    elif len(keys) == 3:
        if keys[1] - keys[0] > keys[2] - keys[1]:
            sel = [keys[0], (keys[0] + keys[1]) // 2, keys[1], keys[2]]
        else:
            sel = [keys[0], keys[1], (keys[1] + keys[2]) // 2, keys[2]]
    elif len(keys) == 4:
        sel = keys
    else:
        aL, aR = 1 / 3 * keys[-1], 2 / 3 * keys[-1]
        left = min(keys, key=lambda k: abs(k - aL))
        right = min(keys, key=lambda k: abs(k - aR))
        sel = [keys[0], left, right, keys[-1]]
    return [list(path[i]) for i in sel], len(keys)
