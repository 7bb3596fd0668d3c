"""What the goal-route tests share (test_track_cpu.py, test_gpu_track.py): the route set, the times asked of it, the three
routes of the oracle flight on scene 3, and the NumPy restatement of the track audit."""
import math

import numpy as np

from neo_planner_amd import _lib
from neo_planner_amd.goal_routes import GoalRoutes

# the oracle flight: scene 3 (synth.occupancy_2d(3), origin (0, -15)), start (0, 0), speed 0.5 m/s, 30 ticks
FLIGHT_ROUTES = [([[24.4, 7.6], [19.9, 9.8], [8.8, 8.9]], True),
                 ([[21.1, 10.9], [15.6, 8.6], [7.2, 9.2]], False),
                 ([[14.3, -7.1], [22.6, -8.0], [24.3, -8.5]], False)]     # the goal reaches its end; the drone replans from on top of it
FLIGHT_SPEED, FLIGHT_TICKS = 0.5, 30


def flight_routes():
    return GoalRoutes.from_lists([r for r, _ in FLIGHT_ROUTES], [FLIGHT_SPEED] * 3, [c for _, c in FLIGHT_ROUTES])


def route_set():
    """K in {2, 3, 17, 256}, each open and closed; a route with a zero-length segment in the middle, one that ends in one, one
    with all vertices equal (open and closed), one with speed 0"""
    rng = np.random.default_rng(812)
    routes, speed, closed = [], [], []
    for K in (2, 3, 17, 256):
        pts = np.stack([rng.uniform(0.0, 30.0, K), rng.uniform(-15.0, 15.0, K)], 1)
        for cl in (0, 1):
            routes.append(pts)
            speed.append(float(rng.uniform(0.2, 3.0)))
            closed.append(cl)
    z = np.array([[1.0, 2.0], [4.0, 6.0], [4.0, 6.0], [9.0, -3.5], [9.0, -3.5]])     # 3-4-5 first: s can sit on a vertex exactly
    for cl in (0, 1):
        routes.append(z)
        speed.append(0.5)
        closed.append(cl)
    same = np.tile([[3.25, -1.5]], (4, 1))
    for cl in (0, 1):
        routes.append(same)
        speed.append(1.0)
        closed.append(cl)
    routes.append(np.array([[2.0, 2.0], [5.0, 6.0], [5.0, 0.0]]))
    speed.append(0.0)
    closed.append(1)
    routes.append(np.array([[0.0, 0.0], [3.0, 4.0], [3.0, 16.0]]))     # lengths 5 and 12, speed 1: integer times sit on vertices
    speed.append(1.0)
    closed.append(1)
    return GoalRoutes.from_lists(routes, speed, closed)


def route_times(routes, b):
    """times for route b: 0, s exactly on every cum (where speed divides it exactly, and otherwise as close as a quotient
    gets), s past the end, several laps, and random ones"""
    rng = np.random.default_rng(1000 + b)
    sp, cum = routes.speed[b], routes.cum[b]
    total = cum[-1]
    ts = [0.0, 1.0, 5.0, 17.0, 30.0, 1.0 / 60.0, 1801.0 / 60.0]
    if sp > 0.0:
        pick = cum if len(cum) <= 20 else cum[rng.integers(0, len(cum), 20)]
        ts += [float(c / sp) for c in pick]
        ts += [float(total / sp) * k for k in (1.0, 1.5, 3.0, 7.25, 100.0)]
        ts += [float(np.nextafter(total / sp, np.inf)), float(np.nextafter(total / sp, 0.0))]
        ts += list(rng.uniform(0.0, 4.0 * total / sp + 1.0, 20))
    else:
        ts += [3.0, 1e6]
    return np.array(ts)


def track_restated(rows, n_flown, stride, hz, route_of_one, radius):
    """the track audit over rows 0, stride, ... < n_flown: gaps from GoalRoutes.at, the mean by math.fsum"""
    idx = np.arange(0, n_flown, stride)
    if len(idx) == 0:
        return dict(count=0, flags=0)
    t = idx / hz
    if not np.isfinite(rows[idx]).all():
        return dict(count=0, flags=_lib.NEO_AUDIT_FLAG_NONFINITE)
    goal = np.stack([route_of_one.at(float(tt))[0] for tt in t])
    d = rows[idx, 0] - goal
    gap = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    within = np.flatnonzero(gap <= radius)
    return dict(count=len(idx), flags=0, gap_mean=math.fsum(gap) / len(idx), gap_max=gap.max(), t_gap_max=t[int(np.argmax(gap))],
                gap_min=gap.min(), t_gap_min=t[int(np.argmin(gap))], gap_final=gap[-1],
                t_first_within=t[within[0]] if len(within) else -1.0, frac_within=len(within) / len(idx), gaps=gap)
