"""
The fleet's resident geo plans, the host side (FleetReplanLoop(mode="geo", geo=BatchGeoPlanner(bp)); the search is
csrc/neo_geo.hpp's, the planner geo_resident.py): the refusals of the constructor, the resident first guess, and the plan
step that stands where the host form's `_plan_geo` stands.  `loop` is the FleetReplanLoop; everything here follows its
stream rule (fleet.py's module docstring): torch work, _torch_done, the context's launches, _ctx_done, reads.

Without geo= the loop is what it was: mode "geo" plans through the host (`_plan_geo`), and refuses resident=True and
onboard maps in the words it always used.  With it the pending missions' A* searches, the prune and the pack run as ONE
launch on the resident look-ahead states and targets (neo_geo_guess_dev, over the round's launch list and the missions'
map slots), and plan_dev takes the guess as attempt 0's start: the host form's flights, bit for bit, with head, tail, the
key nodes and x staying on the device.  With onboard= as well the targets, the search and the optimiser all read the
missions' own maps through onboard.slots, and the search takes its direct form -- the maps change every tick, and a
blocked mask per mission and tick would cost an allocation, a wait and a launch each.
"""
from .geo_resident import BatchGeoPlanner


def check_arguments(geo, mode, batch_planner):
    """the constructor's refusals, before anything touches the device; returns geo"""
    if geo is None:
        return None
    if not isinstance(geo, BatchGeoPlanner):
        raise ValueError("FleetReplanLoop: geo must be a BatchGeoPlanner")
    if mode != "geo":
        raise ValueError("FleetReplanLoop: geo= needs mode 'geo' (the other modes have their own plan steps)")
    if geo.bp is not batch_planner:
        raise ValueError("FleetReplanLoop: geo's planner must be the loop's batch_planner")
    if int(batch_planner.cfg.init_wpts_num) != 2:
        raise ValueError("FleetReplanLoop: the geo plan has M = 3 pieces: geo= needs init_wpts_num = 2")
    return geo


def alloc(loop, f):
    """the resident first guess (f: the loop's zero-filled fp64 tensors)"""
    loop._dev.update(x0=f(loop.B, 7))


def plan_step(loop, sub, pending, tick, r):
    """mode "geo" with geo=: the geo guess of the pending missions on the resident head, tail and map slots
    (BatchGeoPlanner.warm_start_dev, one launch on the context's stream), then plan_dev from it"""
    d = loop._dev
    x0 = loop.geo.warm_start_dev(loop.plan_map, d["head"], d["tail"], slots=d["plan_slots"], subset=sub, x0=d["x0"])
    return loop._plan_resident(sub, pending, tick, r, x0=x0)
