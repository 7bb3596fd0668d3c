"""
The fleet's flight model, the host side (FleetReplanLoop(flight=FlightModel); the kernels are csrc/neo_flight.hpp's, the
model and its definition flight_model.py): the refusals of the constructor, the resident arrays, the fly launch that stands
where neo_fleet_advance_dev stood, and what the end of a run adds -- the landed missions flown out and settled, the
tracking-error record, the fly_* keys of the result.  `loop` is the FleetReplanLoop; everything here follows its stream
rule (fleet.py's module docstring): torch work, _torch_done, the context's launches, _ctx_done, reads.
"""
import ctypes
import time

import numpy as np

from . import _lib, counter_rng
from .flight_model import FlightModel


def check_arguments(flight, settle_seconds, goal_sequences, cmd_hz):
    """the constructor's refusals, before anything touches the device; returns (flight, settle_seconds, the
    neo_flight_model of a flight at cmd_hz or None)"""
    if flight is None:
        return None, float(settle_seconds), None
    if not isinstance(flight, FlightModel):
        raise ValueError("FleetReplanLoop: flight must be a FlightModel")
    if goal_sequences is not None:
        raise ValueError("FleetReplanLoop: flight does not work with goal_sequences (campaigns re-open legs from command "
                         "rows; carrying a drone state across legs is not built)")
    if not (np.isfinite(float(settle_seconds)) and float(settle_seconds) >= 0.0):
        raise ValueError("FleetReplanLoop: settle_seconds must be finite and >= 0")
    # the derived constants, computed once: the kernels and the model hold the same doubles
    return flight, float(settle_seconds), _lib.NeoFlightModel(*flight.derived(cmd_hz))


def check_ids(flight, mission_ids):
    """the gust streams are keyed by mission id, whatever the jitter"""
    if flight is not None:
        counter_rng.check_ids(mission_ids, "FleetReplanLoop")


def alloc(loop, f, i):
    """the drones, what they flew, and the tracking-error record (f, i: the loop's zero-filled fp64 / int32 tensors)"""
    B = loop.B
    loop._dev.update(drone=f(B, 8), flown=f(B, loop.cap, 3, 2), flown_len=i(B), fly_saturated=i(B),
                     fly=f(B, _lib.NEO_FLY_FIELDS), fly_count=i(B), fly_flags=i(B))


def start(loop, head):
    """tick 0: the drones start where the missions do, thrust and gust at rest"""
    loop._up("drone", np.concatenate([head[:, 0], head[:, 1], np.zeros((loop.B, 4))], axis=1))


def fly(loop, sub, step, ahead, first, settle=0):
    """one neo_fleet_fly_dev launch for the missions `sub`: the advance's index arithmetic and look-ahead state, `step`
    sub-steps of the model, cur_pos where the drone is"""
    B, subset, n = loop._rows(sub)
    loop._call("neo_fleet_fly_dev", B, ctypes.byref(loop._fly_model), subset, n, *loop._cmd(), loop._p(loop._dev["future_index"]),
               step, ahead, first, settle, float(loop.target_reach_threshold),
               *loop._ptrs("mission_ids", "goal", "drone", "flown", "flown_len", "fly_saturated", "flags", "cur_pos", "head"))


def settle(loop, landed, took):
    """the end of a run: the landed missions fly their arrays out and hold the last command until they are within reach, at
    most settle_seconds; the others stopped on the row they were on.  Returns n_flown (host) and the flown rows; the resident
    n_flown is what the audits take."""
    d = loop._dev
    t0 = time.perf_counter()
    sub = loop._subset(np.flatnonzero(landed)) if landed.any() else None
    loop._torch_done()
    if sub is not None:
        fly(loop, sub, loop.cap, int(loop.planning_time_ahead * loop.cmd_hz), 0, int(round(loop.settle_seconds * loop.cmd_hz)))
        loop._ctx_done()
    loop.settle_s = took["settle_s"] = time.perf_counter() - t0
    n_flown = d["flown_len"].cpu().numpy()
    d["n_flown"].copy_(d["flown_len"])
    loop._torch_done()
    return n_flown, d["flown"]


def error(loop, took):
    """the reference's save_tracking_err table (:310-331), reduced per mission by neo_fleet_fly_error_dev"""
    d, p = loop._dev, loop._p
    t0 = time.perf_counter()
    loop._call("neo_fleet_fly_error_dev", loop.B, p(d["flown_len"]), None, 0, p(d["flown"]), p(d["cmd"]), loop.cap,
               p(d["cmd_len"]), loop.stride, *loop._ptrs("fly", "fly_count", "fly_flags"))
    loop._ctx_done()
    loop.fly_error_s = took["fly_error_s"] = time.perf_counter() - t0


def results(loop, out):
    d = loop._dev
    rec = d["fly"].cpu().numpy()
    out.update({"fly_" + name: rec[:, k] for k, name in enumerate(_lib.FLY_FIELDS)})
    out.update(fly_count=d["fly_count"].cpu().numpy(), fly_flags=d["fly_flags"].cpu().numpy(),
               fly_saturated=d["fly_saturated"].cpu().numpy())


def flown_rows(loop, i):
    """with a flight model: the flown rows of mission i (flown_len, 3, 2) copied to the host"""
    n = int(loop._dev["flown_len"][i].item())
    return loop._dev["flown"][i, :n].cpu().numpy()
