"""NumPy model of the fleet's `warmstart` mode (csrc/neo_fleet.hpp: fleet_warm_guess_kernel, fleet_warm_carry_kernel;
ros_node/traj_planner_node.py:570-571, :597-611): what a mission carries from one plan to the next, and the first guess
made of it.  fp64, every operation rounded on its own; the waypoint arithmetic is one add or one subtraction, so the
kernels give these bits.  The logarithm and the exponential are math.log and math.exp, as in map_T2tau and map_tau2T, so
the model gives the oracle planner's bits; where math.exp raises, exp is inf (a duration of T_min), as on the device.

Per mission: wpts_local (2, count), the last solved plan's waypoints minus the position that plan started from;
ts_carry (M,), M = count + 1, the durations the planner last held.  A plan's x is [x_0 .. x_{count-1}, y_0 ..
y_{count-1}, tau_0 .. tau_{M-1}]."""
import math

import numpy as np

NEO_TRAJ_MAXITER, NEO_TRAJ_NUMERIC_RANGE = 3, 4


def launched(B, subset):
    """the missions a launch works on: all B, or the subset's entries inside 0 .. B - 1"""
    if subset is None:
        return list(range(B))
    return [int(b) for b in subset if 0 <= int(b) < B]


def tau_of(t, T_min, T_max):
    """map_T2tau of one duration; NaN where the reference's raises (t - T_min not > 0: a division by zero or a negative
    argument; an argument of 0: math.log's domain error) and for a NaN duration"""
    dt = t - T_min
    if not dt > 0.0:
        return math.nan
    arg = (T_max - T_min) / dt - 1.0
    if not arg > 0.0:
        return math.nan
    return -math.log(arg)


def durations_of(tau, T_min, T_max):
    """map_tau2T of an array of tau, with the reference's math.exp; where that raises (-tau beyond 709.78) exp is inf and
    the duration T_min"""
    def one(v):
        try:
            e = math.exp(-v)
        except OverflowError:
            e = math.inf
        return (T_max - T_min) / (1.0 + e) + T_min
    return np.array([one(float(v)) for v in np.asarray(tau, dtype=np.float64).reshape(-1)])


def guess(head, wpts_local, ts_carry, T_min, T_max, subset=None, x0=None):
    """x0 (B, n) of the launched missions from head (B, 3, 2), wpts_local (B, 2, count) and ts_carry (B, M); the rows of
    the others stay what `x0` holds (zeros without)"""
    B, M = ts_carry.shape
    count = M - 1
    out = np.zeros((B, 3 * count + 1)) if x0 is None else np.array(x0, dtype=np.float64)
    for b in launched(B, subset):
        for d in range(2):
            out[b, d * count:(d + 1) * count] = wpts_local[b, d] + head[b, 0, d]
        out[b, 2 * count:] = [tau_of(float(t), T_min, T_max) for t in ts_carry[b]]
    return out


def carry(x, head, solved, status, attempts, init_ts, wpts_local, ts_carry, T_min, T_max, subset=None):
    """(wpts_local, ts_carry) after a plan call: copies, updated for the launched missions"""
    B, M = ts_carry.shape
    count = M - 1
    wl, tc = np.array(wpts_local, dtype=np.float64), np.array(ts_carry, dtype=np.float64)
    for b in launched(B, subset):
        ok = solved[b] != 0
        if ok:      # :570-571
            for d in range(2):
                wl[b, d] = x[b, d * count:(d + 1) * count] - head[b, 0, d]
        if ok or (int(status[b]) & 0xff) <= NEO_TRAJ_MAXITER:      # the attempt ran to an answer: planner.ts is its durations
            tc[b] = durations_of(x[b, 2 * count:], T_min, T_max)
        elif attempts[b] > 1:      # it raised: the durations it started from, a re-seeded attempt's
            tc[b] = init_ts
    return wl, tc
