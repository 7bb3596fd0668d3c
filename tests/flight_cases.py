"""What test_flight_cpu.py and test_gpu_flight.py share: the flight models, random fleets of missions on short command
arrays with every kind of cmd_len and cmd_index, launches of the NumPy model (flight_model.fly_launch) on copies of a
fleet's state, and the tracking-error record written as a plain loop."""
import math

import numpy as np

from neo_planner_amd import _lib
from neo_planner_amd import flight_model as fm

CAP = 40
HZ = 60.0
CANARY = float(np.array([0x7ff8dead00000000], dtype=np.uint64).view(np.float64)[0])

# the defaults; an a_max every sub-step runs into; gusts at every sub-step and at every sixth
MODELS = {
    "default": fm.FlightModel(),
    "saturating": fm.FlightModel(a_max=0.5),
    "gust1": fm.FlightModel(gust_sigma=0.3, gust_every=1, seed=77),
    "gust6": fm.FlightModel(gust_sigma=0.3, gust_every=6, seed=2 ** 40 + 5),
}


def fleet(B, seed, cap=CAP, rows=None):
    """B missions: cmd (B, cap, 3, 2) smooth rows with a little noise, cmd_len / cmd_index of every kind in the first
    missions (0 commands, 1, cap, more than cap, an index below 0, on the last row, past the array) and random ones after
    them, drones near their rows, goals, mission ids.  rows: the arrays' row count (cap + 1 leaves a row nothing may write)"""
    rng = np.random.default_rng([seed, B])
    rows = cap if rows is None else rows
    t = np.arange(cap) / HZ
    p0, v0 = rng.uniform(-5.0, 5.0, (B, 1, 2)), rng.uniform(-1.0, 1.0, (B, 1, 2))
    acc = rng.uniform(-0.5, 0.5, (B, 1, 2))
    cmd = np.zeros((B, cap, 3, 2))
    cmd[:, :, 0] = p0 + v0 * t[None, :, None] + 0.5 * acc * (t ** 2)[None, :, None] + rng.normal(0.0, 0.01, (B, cap, 2))
    cmd[:, :, 1] = v0 + acc * t[None, :, None] + rng.normal(0.0, 0.02, (B, cap, 2))
    cmd[:, :, 2] = acc + rng.normal(0.0, 0.05, (B, cap, 2))
    cmd_len = rng.integers(2, cap + 1, B).astype(np.int32)
    cmd_index = np.array([rng.integers(0, n) for n in cmd_len], dtype=np.int32)
    special = [(0, 0), (1, 0), (cap, 0), (cap + 5, 3), (20, -2), (20, 19), (20, 30), (cap, cap - 1)]
    for b, (n, k) in enumerate(special[:B] if B >= 5 else []):
        cmd_len[b], cmd_index[b] = n, k
    if B < 5:
        cmd_len[0], cmd_index[0] = cap, 0
    drone = np.zeros((B, 8))
    at = np.clip(cmd_index, 0, cap - 1)
    drone[:, :2] = cmd[np.arange(B), at, 0] + rng.normal(0.0, 0.05, (B, 2))
    drone[:, 2:4] = cmd[np.arange(B), at, 1] + rng.normal(0.0, 0.05, (B, 2))
    drone[:, 4:6] = rng.normal(0.0, 0.1, (B, 2))
    drone[:, 6:8] = rng.normal(0.0, 0.1, (B, 2))
    flown_len = np.where(cmd_len > 0, np.clip(cmd_index, 0, None) + 1, 0).astype(np.int32)
    flown_len[rng.random(B) < 0.3] = 0      # nothing of these flown yet: the launch writes their first row
    return dict(B=B, cap=cap, cmd=cmd, cmd_len=cmd_len, cmd_index=cmd_index, future_index=np.full(B, -7, np.int32),
                goal=cmd[np.arange(B), np.clip(cmd_len - 1, 0, cap - 1), 0] + rng.normal(0.0, 0.3, (B, 2)), drone=drone,
                flown=np.full((B, rows, 3, 2), CANARY), flown_len=flown_len, saturated=rng.integers(0, 3, B).astype(np.int32),
                flags=np.zeros(B, np.int32), cur_pos=np.full((B, 2), CANARY), head=np.full((B, 3, 2), CANARY),
                mission_ids=(np.arange(B) * 7 + 3).astype(np.int32))


STATE = ("cmd_index", "future_index", "drone", "flown", "flown_len", "saturated", "flags", "cur_pos", "head")


def copy_of(fl):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in fl.items()}


def model_launch(fl, d, step, ahead=5, first=0, settle=0, reach=0.2, subset=None):
    """flight_model.fly_launch on the fleet `fl`, in place"""
    fm.fly_launch(d, fl["cmd"], fl["cmd_len"], fl["cmd_index"], fl["future_index"], step, ahead, first, settle, reach, fl["goal"],
                  fl["drone"], fl["flown"], fl["flown_len"], fl["saturated"], fl["flags"], fl["cur_pos"], fl["head"],
                  mission_ids=fl["mission_ids"], subset=subset)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float64:
        return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    return np.array_equal(a, b)


def differing(fl_a, fl_b):
    """the state arrays in which two fleets differ in any bit"""
    return [k for k in STATE if not same_bits(fl_a[k], fl_b[k])]


def error_restated(flown, commands, stride):
    """the tracking-error record as a plain loop over the samples, sums by math.fsum"""
    fl, cm = np.asarray(flown).reshape(-1, 6), np.asarray(commands).reshape(-1, 6)
    n = len(fl)
    nan = dict(count=0, flags=0)
    if n < 1 or len(cm) < 1:
        return nan
    pe, ve, at = [], [], []
    for r in range(0, n, stride):
        c = cm[min(r, len(cm) - 1)]
        if not (np.all(np.isfinite(fl[r, :4])) and np.all(np.isfinite(c[:4]))):
            return dict(count=0, flags=_lib.NEO_AUDIT_FLAG_NONFINITE)
        pe.append(math.sqrt((fl[r, 0] - c[0]) * (fl[r, 0] - c[0]) + (fl[r, 1] - c[1]) * (fl[r, 1] - c[1])))
        ve.append(math.sqrt((fl[r, 2] - c[2]) * (fl[r, 2] - c[2]) + (fl[r, 3] - c[3]) * (fl[r, 3] - c[3])))
        at.append(r)
    c = cm[min(n - 1, len(cm) - 1)]
    k = int(np.argmax(pe))
    return dict(count=len(pe), flags=0, pos_err_rms=math.sqrt(math.fsum(e * e for e in pe) / len(pe)), pos_err_max=max(pe),
                pos_err_max_at=float(at[k]), vel_err_rms=math.sqrt(math.fsum(e * e for e in ve) / len(ve)), vel_err_max=max(ve),
                pos_err_final=math.sqrt((fl[n - 1, 0] - c[0]) ** 2 + (fl[n - 1, 1] - c[1]) ** 2))
