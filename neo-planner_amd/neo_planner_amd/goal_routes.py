"""
Goal routes: goals that keep moving (ros_node/tracker_planner_node.py with tracker_manager_node.py -- the global target is
whatever the last message said, :160-162, :313-316).  A mission's goal moves along a polyline at constant speed.

This is the NumPy model of the route part of csrc/neo_track.hpp: the same operations in the same order, every one rounded
on its own, so `GoalRoutes.at` and neo_fleet_goal_route agree bit for bit.

  seg_k = sqrt(dx * dx + dy * dy)        a closed route has the closing segment back to vertex 0
  cum_0 = 0, cum_{k+1} = cum_k + seg_k   summed in order
  s = speed * t                          closed: fmod(s, total); open: s clamped to total
  k                                      the largest index with cum_k <= s, at most the last segment
  point = v_k + ((s - cum_k) / seg_k) * (v_{k+1} - v_k),   v_k exactly where seg_k == 0 or total == 0
"""
import numpy as np

from . import _lib

ROUTE_MAX = _lib.NEO_FLEET_ROUTE_MAX


class GoalRoutes:
    """B routes as a ragged table, laid out as DepthCamera.pack_scenes lays out boxes: vertices (NV, 2), route_begin
    (B + 1,) ascending from 0 (route b is vertices[route_begin[b]:route_begin[b + 1]], 2 to 256 points), speed (B,) in
    metres a second (>= 0), closed (B,) (None: all open).  `at(t)` is where every goal is at time t; `cum[b]` the running
    segment sums of route b."""

    def __init__(self, vertices, route_begin, speed, closed=None):
        v = _lib.as_f64(vertices)
        if v.ndim != 2 or v.shape[1] != 2:
            raise ValueError("GoalRoutes: vertices must be (NV, 2)")
        rb = np.asarray(route_begin)
        if rb.ndim != 1 or rb.shape[0] < 1 or not np.issubdtype(rb.dtype, np.integer):
            raise ValueError("GoalRoutes: route_begin must be (B + 1,) integers")
        rb = rb.astype(np.int64)
        if rb[0] != 0 or np.any(np.diff(rb) < 0) or rb[-1] != v.shape[0]:
            raise ValueError("GoalRoutes: route_begin must ascend from 0 to the number of vertices")
        B = rb.shape[0] - 1
        n = np.diff(rb)
        if np.any(n < 2):
            raise ValueError("GoalRoutes: a route needs at least 2 vertices")
        if np.any(n > ROUTE_MAX):
            raise ValueError("GoalRoutes: a route has at most %d vertices" % ROUTE_MAX)
        sp = _lib.as_f64(speed).reshape(-1)
        if sp.shape[0] != B:
            raise ValueError("GoalRoutes: one speed per route")
        if not np.all(np.isfinite(v)) or not np.all(np.isfinite(sp)):
            raise ValueError("GoalRoutes: vertices and speeds must be finite")
        if np.any(sp < 0.0):
            raise ValueError("GoalRoutes: a speed must be >= 0")
        cl = np.zeros(B, np.int32) if closed is None else (np.asarray(closed).reshape(-1) != 0).astype(np.int32)
        if cl.shape[0] != B:
            raise ValueError("GoalRoutes: one closed flag per route")
        self.vertices, self.route_begin, self.speed, self.closed = v, rb.astype(np.int32), sp, cl
        self.B = B
        self.seg, self.cum = [], []
        for b in range(B):
            seg, cum = _seg_cum(v[rb[b]:rb[b + 1]], bool(cl[b]))
            self.seg.append(seg)
            self.cum.append(cum)

    @classmethod
    def from_lists(cls, routes, speed, closed=None):
        """routes: a list of (K_b, 2) point lists"""
        routes = [_lib.as_f64(r).reshape(-1, 2) for r in routes]
        begin = np.concatenate([[0], np.cumsum([len(r) for r in routes])]).astype(np.int32)
        return cls(np.concatenate(routes) if routes else np.zeros((0, 2)), begin, speed, closed)

    def route(self, b):
        """the (K, 2) vertices of route b"""
        return self.vertices[self.route_begin[b]:self.route_begin[b + 1]]

    def take(self, idx):
        """the routes `idx`, in that order, as a GoalRoutes of their own (a mission flown alone)"""
        idx = np.asarray(idx).reshape(-1)
        return GoalRoutes.from_lists([self.route(int(b)) for b in idx], self.speed[idx], self.closed[idx])

    def at(self, t):
        """(B, 2): every route's point at time t (a scalar, or (B,) one time per route)"""
        tt = np.broadcast_to(np.asarray(t, dtype=np.float64), (self.B,))
        out = np.empty((self.B, 2))
        with np.errstate(invalid="ignore", divide="ignore"):
            for b in range(self.B):
                out[b] = _point(self.route(b), self.seg[b], self.cum[b], bool(self.closed[b]), self.speed[b], tt[b])
        return out


def _seg_cum(v, closed):
    nxt = np.roll(v, -1, axis=0) if closed else v[1:]
    cur = v if closed else v[:-1]
    dx, dy = nxt[:, 0] - cur[:, 0], nxt[:, 1] - cur[:, 1]
    seg = np.sqrt(dx * dx + dy * dy)
    cum = np.zeros(seg.shape[0] + 1)
    c = np.float64(0.0)
    for k in range(seg.shape[0]):      # the sequential running sum (np.cumsum's order is the same; this one says so)
        c = c + seg[k]
        cum[k + 1] = c
    return seg, cum


def _point(v, seg, cum, closed, speed, t):
    nseg = seg.shape[0]
    total = cum[nseg]
    s = np.float64(speed) * np.float64(t)
    if closed:
        s = np.fmod(s, total)                      # (a route without length: NaN, which finds segment 0)
    elif s > total:
        s = total
    k = int(np.count_nonzero(cum[1:nseg] <= s))    # the largest k with cum_k <= s, at most the last segment
    if seg[k] == 0.0 or total == 0.0:
        return v[k].copy()
    k1 = k + 1 if k + 1 < v.shape[0] else 0
    f = (s - cum[k]) / seg[k]
    return v[k] + f * (v[k1] - v[k])
