"""
Fleet campaigns, the host side (FleetReplanLoop(goal_sequences=...); the kernels are csrc/neo_legs.hpp's): the refusals of
the campaign arguments, the per-leg bookkeeping of a run, the end of a tick -- which legs end, and how -- with the one
upload and the three launches that close, audit and open them, and the result dict made of the resident leg log.

The functions take the loop as their first argument: fleet.py keeps the tick, this module what a tick does about legs.
"""
import ctypes
import time

import numpy as np

from . import _lib
from .goal_sequences import GoalSequences

WHO = "FleetReplanLoop"


def check_arguments(goal_sequences, leg_timeout, max_legs, goals, goal_routes, mode):
    """the refusals of FleetReplanLoop's campaign arguments; returns (goals, leg_timeout, max_legs) in shape"""
    if goal_sequences is None:
        if leg_timeout is not None or max_legs is not None:
            raise ValueError(WHO + ": leg_timeout and max_legs need goal_sequences")
        return goals, None, None
    if not isinstance(goal_sequences, GoalSequences):
        raise ValueError(WHO + ": goal_sequences must be a GoalSequences")
    if goal_routes is not None:
        raise ValueError(WHO + ": goal_sequences and goal_routes exclude each other (a route never lands: its leg would never end)")
    if mode == "warmstart":
        raise ValueError(WHO + ": goal_sequences need a mode other than 'warmstart' (a leg's first plan is a basic plan, and "
                         "which plan is a mission's first is taken from the tick today, not kept per mission)")
    if mode == "geo":
        raise ValueError(WHO + ": goal_sequences need a mode other than 'geo' (as goal routes: not built)")
    if goals is not None and _lib.as_f64(goals).reshape(-1, 2).shape[0] != goal_sequences.B:
        raise ValueError(WHO + ": one goal sequence per mission")
    if leg_timeout is not None:
        leg_timeout = float(leg_timeout)
        if not (np.isfinite(leg_timeout) and leg_timeout > 0.0):
            raise ValueError(WHO + ": leg_timeout must be finite and > 0 (None: no limit)")
    if max_legs is None:
        max_legs = int(goal_sequences.count.max()) if goal_sequences.B else 1
    elif isinstance(max_legs, bool) or int(max_legs) != max_legs or not 1 <= int(max_legs) <= _lib.NEO_FLEET_LEGS_MAX:
        raise ValueError(WHO + ": max_legs must be an integer in 1 .. %d" % _lib.NEO_FLEET_LEGS_MAX)
    return goal_sequences.first(), leg_timeout, int(max_legs)      # where the goals start


def check_ids(goal_sequences, mission_ids):
    """a flap's counter streams are keyed by mission id: the sequences' ids must be the loop's"""
    if goal_sequences is not None and goal_sequences.kind == _lib.NEO_LEGS_FLAP and \
            not np.array_equal(goal_sequences.mission_ids, mission_ids):
        raise ValueError(WHO + ": a flap campaign's mission ids must be the loop's mission_ids")


def alloc(loop, f, i):
    """the resident goal lists, the leg counters and log, and what close hands to open (f, i: the loop's makers of zeroed
    fp64 / int32 tensors).  The table goes up as GoalSequences' constructor checked it -- every mission 1 .. 64 goals --
    which neo_fleet_leg_open_dev, holding device pointers, cannot check again (a list that is not one has no next goal)."""
    import torch
    q, d, dev, B = loop.sequences, loop._dev, loop._device, loop.B
    d.update(seq_goals=torch.from_numpy(q.goals).to(dev) if q.goals.shape[0] else f(1, 2),      # (a flap has no table: still a pointer)
             seq_begin=torch.from_numpy(q.seq_begin).to(dev),
             seq_ids=None if q.mission_ids is None else torch.from_numpy(q.mission_ids).to(dev),
             leg=i(B), leg_start=f(B, 2), leg_end=f(B, 2, 2), final_dist=f(B),
             leg_log=torch.full((B, loop.max_legs, _lib.NEO_LEG_FIELDS), float("nan"), dtype=torch.float64, device=dev))
    loop._seq = q.struct(loop._p, d["seq_goals"], d["seq_begin"], d["seq_ids"])
    loop._leg_io = None


class LegTally:
    """a campaign's host bookkeeping: which leg every mission is on, how many ticks that leg has had, who is through, and
    the per-leg counters (B, max_legs) -- the numbers of the reference's planning_metrics.txt line (:292-308)"""

    def __init__(self, B, max_legs, counts):
        self.at = np.zeros(B, np.int64)            # the leg being flown
        self.ticks_now = np.zeros(B, np.int64)     # j: that leg's ticks so far, 0 at its first plan
        self.done = np.zeros(B, bool)
        self.counts = np.minimum(counts, max_legs).astype(np.int64)      # legs a mission can fly
        self.replans, self.failed, self.opt_runs, self.ticks = (np.zeros((B, max_legs), np.int32) for _ in range(4))
        self.iter_num = np.zeros((B, max_legs), np.int64)
        self.first_tick = np.full((B, max_legs), -1, np.int32)

    def begin_tick(self, active, tick):
        opened = active[self.ticks_now[active] == 0]
        self.first_tick[opened, self.at[opened]] = tick

    def count_round(self, pending, ok, nit_total, attempts):
        """one target round's plans of the missions `pending`, booked on the legs they are flying"""
        at = self.at[pending]
        self.iter_num[pending, at] += nit_total
        self.opt_runs[pending, at] += attempts
        self.replans[pending[ok], at[ok]] += 1
        self.failed[pending[~ok], at[~ok]] += 1


def end_of_tick(loop, t, legs, active, stuck, step):
    """which of the active missions' legs end with this tick, and how; those close, are audited and open their next leg on
    the context's stream.  Returns the missions of the next tick: everyone whose campaign goes on."""
    j = legs.ticks_now[active]
    late = np.zeros(active.size, bool) if loop.leg_timeout is None else (j + 1) * step / loop.cmd_hz > loop.leg_timeout
    code = np.where(t.landed[active], _lib.NEO_LEG_LANDED,
                    np.where(t.abandoned[active], _lib.NEO_LEG_ABANDONED,
                             np.where(stuck[active], _lib.NEO_LEG_STUCK, np.where(late, _lib.NEO_LEG_TIMEOUT, 0))))
    legs.ticks[active, legs.at[active]] += 1
    legs.ticks_now[active] += 1
    closing = active[code != 0]
    if closing.size:
        close(loop, closing, code[code != 0])
        legs.at[closing] += 1
        legs.ticks_now[closing] = 0
        t.landed[closing] = t.abandoned[closing] = False      # (facts of a leg)
        legs.done[closing] = legs.at[closing] >= legs.counts[closing]
    return active[~legs.done[active]]


def close(loop, closing, codes):
    """one upload of (outcome by mission, subset), then close, audit (on the true map, as _finish) and open for the missions
    `closing`.  No read and no _ctx_done: what the three write is next read by launches on the same stream, or behind a
    later _ctx_done."""
    import torch
    B, d, p = loop.B, loop._dev, loop._p
    io = np.zeros(B + closing.size, np.int32)
    io[closing] = codes
    io[B:] = closing
    # (kept until the next close: the context reads it on its own stream, and torch must not hand the memory out before)
    loop._leg_io = io = torch.from_numpy(io).to(loop._device)
    loop._torch_done()
    rows = (B, p(io), p(io, B), int(closing.size))      # B, outcome, subset, n_subset
    loop._call("neo_fleet_leg_close_dev", *rows, *loop._cmd(), *loop._ptrs("head", "goal", "n_flown", "leg_end", "final_dist"))
    loop._call("neo_fleet_audit_batch_dev", loop.map.scene_id, p(d["slots"]), B, *rows[2:], p(d["cmd"]), loop.cap, p(d["n_flown"]),
               loop.stride, float(loop.cmd_hz), None if loop.metric_weights is None else _lib.ptr(loop.metric_weights),
               *loop._ptrs("audit", "count", "audit_flags"))
    loop._call("neo_fleet_leg_open_dev", *rows, ctypes.byref(loop._seq), loop.max_legs, float(loop.target_reach_threshold),
               *loop._ptrs("n_flown", "leg_end", "final_dist", "count", "audit_flags", "audit", "leg", "leg_log",
                                  "leg_start", "goal", "cur_pos", "head", "cmd_len", "cmd_index", "future_index", "flags"))


def finish(loop, tally, legs):
    """the legs still open are logged NEO_LEG_OPEN (one last close / audit / open over them, which opens nothing); then the
    log comes to the host, once, and the result dict is made of it and of the host's tallies.  A leg that was opened at the
    end of the last tick and never got a plan is one of them: it is logged with n_flown 0, final_dist inf, leg_ticks 0 and
    leg_first_tick -1, n_legs counts it, and the "last leg" keys describe it -- as the device does, where its empty command
    array (n_cmd 0) has taken the place of the one before."""
    d = loop._dev
    t0 = time.perf_counter()
    still = np.flatnonzero(~legs.done)
    if still.size:
        close(loop, still, np.full(still.size, _lib.NEO_LEG_OPEN, np.int32))
    loop._ctx_done()
    loop.audit_s = time.perf_counter() - t0
    B, L = loop.B, loop.max_legs
    log = d["leg_log"].cpu().numpy()
    n_legs = d["leg"].cpu().numpy()
    F = {name: k for k, name in enumerate(_lib.LEG_FIELDS)}
    flown = np.arange(L)[None, :] < n_legs[:, None]
    last = log[np.arange(B), np.maximum(n_legs - 1, 0)]      # (every mission has flown tick 0: n_legs >= 1)
    whole = lambda col: np.where(np.isnan(col), -1.0, col).astype(np.int32)
    out = {name: last[:, F[name]] for name in _lib.AUDIT_FIELDS}
    audit_flags = whole(last[:, F["audit_flags"]])
    metric_fail = (audit_flags & (_lib.NEO_AUDIT_FLAG_METRIC_FAIL | _lib.NEO_AUDIT_FLAG_NONFINITE)) != 0
    leg_ok = (log[:, :, F["success"]] == 1.0) | ~flown
    success = (n_legs >= loop.sequences.count) & leg_ok.all(axis=1)
    out.update(success=success, replans=tally.replans, failed_attempts=tally.failed, iter_num=tally.iter_num,
               opt_runs=tally.opt_runs, n_cmd=d["cmd_len"].cpu().numpy(), n_flown=whole(last[:, F["n_flown"]]),
               final_dist=last[:, F["final_dist"]], flags=whole(last[:, F["flags"]]), audit_flags=audit_flags,
               count=whole(last[:, F["count"]]), abandoned=last[:, F["outcome"]] == _lib.NEO_LEG_ABANDONED,
               metric_fail=metric_fail, n_legs=n_legs)
    for name, k in F.items():
        out["leg_" + name] = whole(log[:, :, k]) if name in _lib.LEG_INT_FIELDS else log[:, :, k]
    for name, a in (("replans", legs.replans), ("failed_attempts", legs.failed), ("iter_num", legs.iter_num),
                    ("opt_runs", legs.opt_runs), ("ticks", legs.ticks), ("first_tick", legs.first_tick)):
        out["leg_" + name] = np.where(flown, a, -1).astype(a.dtype)
    return loop._with_poses(out)
