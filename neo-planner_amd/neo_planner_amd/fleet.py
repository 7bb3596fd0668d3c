"""
Fleet replan loop: B closed-loop missions in lock step (ros_node/traj_planner_node.py:390-578, `ReplanLoop` for a fleet).

Every tick is one round of batched launches over the missions still planning:

  advance   perfect tracking for one replan period + get_drone_state_ahead (:527-537)   neo_fleet_advance_dev
  target    set_local_target (:450-488)                                                  neo_fleet_target_batch_dev
  plan      BatchPlanner.plan / geo_plan on the active missions (warm_start_plan / geo_traj_plan), or, in mode
            "batch", batch_plan_dev on the RESIDENT look-ahead states and targets (batch_plan: three lateral candidates)
  splice    the new commands into the old array at the look-ahead index (:574-578)       neo_fleet_splice_dev

and the missions whose plan failed go round again with a jittered target, up to the reference's 11 targets a tick
(:429-445).  At the end neo_fleet_audit_batch_dev takes the reference's flight metric (:333-363) over what was flown.
The command arrays (cmd_hz rows a second and mission) stay in HBM from the first plan to the audit; the small vectors
(look-ahead state, target, x, statuses) pass through the host, as BatchPlanner.plan takes host arrays.  Mode "batch"
is the exception: candidates, the optimiser launch over missions x 3, the choice and the splice work on the resident
arrays; per target round only `near`, `solved`, the two counters and the list of the missions without a feasible
candidate come to the host, and only those missions take the host `plan` (their rows of x / solved are uploaded).
With resident=True the plans are BatchPlanner.plan_dev's, bit for bit the same: mode "basic" plans on the resident
look-ahead states and targets and fetches `solved` and the two counters of the pending missions only; mode "batch" sends
its list of missions without a feasible candidate through plan_dev as well.

With onboard=OnboardMapper the missions fly on what they have seen: before the targets of every tick (tick 0 included)
the active missions sense from where they are -- the eye at (cur_pos, des_pos_z), heading along the last step of the
command array (neo_fleet_pose_dev), mapper.update renders, integrates and rebuilds -- and the targets and the plans use
each mission's onboard scene.  The final audit is taken on the true maps: the flight metric is measured against the
world, not the belief.

With record=DemoRecorder the fleet keeps what its expert did (the reference's `selected_planner:=record`,
traj_planner/record_planner.py): once a tick, after the advance and before the targets, the active missions' poses
(neo_fleet_pose_dev), their velocities now (neo_record_state_dev) and their depth images go into the recorder's
per-mission buffers, and every target round, just before the splice, one neo_record_commit_dev appends a row for each
mission whose plan solved.  The flights are the same with and without it, and no host read is added: the rows and
their counters stay on the device until the recorder is asked.

Modes "neo" and "nn" fly on the learned warm start (the reference's `selected_planner:=neo` and `:=nn`,
traj_planner/neo_planner.py, nn_planner.py) with neo=BatchNeoPlanner: once a tick, before the targets, the active
missions' poses, their velocities now (neo_record_state_dev into the loop's own buffer) and the backbone's features of
what their cameras see go into resident arrays; every target round BatchNeoPlanner.warm_start_dev turns the pending
missions' pose, velocity, look-ahead state, target and features into the resident first guess (three launches on the
context's stream, csrc/neo_init.hpp).  "neo" hands it to plan_dev as attempt 0's start; "nn" splices it as it is, without
an optimiser launch.  Both imply resident plans and work with onboard and record.

Mode "warmstart" starts every replan from the previous plan (the reference's `selected_planner:=warmstart`, :493,
:570-571, :597-611).  A mission's first plan, re-targeted repeats included, is a basic plan.  From then on every mission
carries two resident rows: the last SOLVED plan's waypoints relative to the position that plan started from, and the
durations the planner last held.  Before a plan call neo_fleet_warm_guess_dev moves the waypoints to the new look-ahead
position and maps the durations to tau -- the first guess plan_dev takes as attempt 0's start; after every plan call, in
front of the splice, neo_fleet_warm_carry_dev keeps what the round's missions carry on (csrc/neo_fleet.hpp).  A carried
duration the reference's map_T2tau raises for (one saturated to T_min or T_max) gives a NaN tau: that attempt ends at its
first evaluation, uncounted, and plan_dev re-seeds from the straight line, as warm_start_plan does when it catches the
exception.  Resident plans always; works with onboard, record and both jitter settings; no host read is added.

With goal_routes=GoalRoutes the missions chase goals that keep moving (ros_node/tracker_planner_node.py with
tracker_manager_node.py): every mission's goal moves along its polyline at constant speed (goal_routes.py is the model of
csrc/neo_track.hpp, bit for bit).  Tick k is at time (k * step) / cmd_hz, step = round(replan_period * cmd_hz).  Per tick
neo_fleet_hold_dev runs in front of the advance -- a mission whose commands end before the coming period is over holds
its last one, so row i of its array is its command at time i / cmd_hz, always -- and neo_fleet_goal_route_dev writes the
active missions' resident goals before sensing and the targets, tick 0 included.  Closer than longitu_step_dis the local
target is the goal itself with zero velocity (:319-321) and planning goes on: `near` lands nobody.  A tick whose 11
targets all fail counts in failed_ticks and the mission flies on along its old commands (:265-279); only CMD_FULL and
SPLICE_FAILED end a mission, and the run lasts max_replans ticks.  At the end the flight metric takes the tracker node's
weights (1, 1, 1) (:175) and neo_fleet_track_audit_dev measures the gap between the flown rows and the goal at their times.
The hooks are the same for every mode but "geo" (the tracker node has no geo planner), resident or not, with onboard,
record and both jitters.  Without goal_routes no launch, host read or allocation is added.

With goal_sequences=GoalSequences every mission flies a CAMPAIGN, goal after goal (ros_node/manager_node.py:153-193 sends
the next goal as soon as one is reached or given up; goal_sequences.py is the model of csrc/neo_legs.hpp's goal lists, bit
for bit).  Each goal is a leg.  At the end of a tick the host knows which missions' legs ended -- landed, abandoned, stuck
(CMD_FULL / SPLICE_FAILED) or past leg_timeout (the reference's max_target_find_time) -- and uploads (subset, outcome) for
them once; then, on the context's stream, neo_fleet_leg_close_dev fixes what the leg was, neo_fleet_audit_batch_dev takes
its flight metric on the TRUE map, and neo_fleet_leg_open_dev writes the leg's row of the resident log and opens the next
leg: the sequence's next goal, cur_pos and head from where the leg ended (position and velocity: first_plan plans from
drone_state, :491-504), the command array empty.  No device read is added and the mission never leaves the tick's launch
list: its next plan is the next tick's, with that global tick number in the jitter keys, so the batch stays full and a
mission still flies the same alone and in any fleet.  The kernels of a tick need nothing new for a freshly opened leg: the
advance leaves a mission without commands untouched, the splice with first = 0 starts at future_index = 0, the pose looks
from cur_pos towards the goal.  With onboard the mapper is reset at run()'s start and never at a leg's: the second goal is
flown on the first one's map, as the reference's octomap persists from goal to goal.  Without goal_sequences no launch,
host read or allocation is added.

A mission's flight does not depend on which other missions share the fleet: the kernels work per mission, the target
jitter of mission i at tick t and target r comes from SeedSequence(seed, i, t, r), and BatchPlanner.plan draws the
retries of mission i from SeedSequence(plan_seed(t, r), i, attempt) (its `stream_ids`).  With jitter="counter" both come
from the counter-based streams of counter_rng.py / csrc/neo_counter_rng.hpp instead -- a value is a pure function of
(seed, mission id, tick, target) or (plan_seed, mission id, attempt) -- drawn on the device: neo_fleet_jitter_dev in front
of the target kernel, neo_plan_jitter_dev inside plan_dev.  The property is the same, the flights are other flights.

With flight=FlightModel (flight_model.py, the model of csrc/neo_flight.hpp, bit for bit) the missions no longer sit on
their command rows: every mission has a resident drone state (position, velocity, lagged thrust, gust), and from tick 1
on neo_fleet_fly_dev stands where neo_fleet_advance_dev stood (behind neo_fleet_hold_dev when goals move) -- the same
index arithmetic, the same look-ahead state FROM THE COMMAND ARRAY (:527-537), but cur_pos is where the drone is after
`step` sub-steps of tracking with lag, saturation, drag and gusts, and every sub-step leaves a row of the resident `flown`
array.  What the reference reads from odometry reads the flown rows here: the targets and the camera's eye (cur_pos), the
recorder's and the network's velocity now, the end audit, the tracking audit and final_dist; the camera's heading stays
the command's (:685-687).  At the end one more fly launch flies the landed missions out and holds their last command for
at most settle_seconds, up to the reach test; n_flown is the number of flown rows, and neo_fleet_fly_error_dev reduces the
reference's save_tracking_err table (:310-331) to fly_<field> (_lib.FLY_FIELDS), fly_count, fly_flags and fly_saturated.
The gust of sub-step t is keyed by (model seed, mission id, t): a mission flies the same alone and in any fleet, however
the ticks cut its flight.  Every mode and option works but goal_sequences (campaigns re-open legs from command rows;
carrying a drone state across legs is left out).  Without flight no launch, host read or allocation is added.

With geo=BatchGeoPlanner (mode "geo" only; fleet_geo.py) the geo plans run on the resident arrays: every target round
the pending missions' A* searches, the prune and the pack of the first guess are ONE launch (neo_geo_guess_dev) over the
round's launch list, on the look-ahead states, the targets and the missions' map slots where they lie, and plan_dev takes
the guess as attempt 0's start -- the host form's flights bit for bit.  It may be combined with onboard=: targets, search
and optimiser then read the missions' own maps, and the search takes its direct form, which needs no blocked mask.
Without geo= nothing changes: mode "geo" plans through the host, and resident=True and onboard= are refused for it as
they always were; no launch, wait or allocation is added.

Two streams, one rule.  torch works on its own stream, the context launches on another, and nothing orders the two but
the host.  Every stage of the loop therefore goes: torch work (uploads, gathers, scatters), then `_torch_done`, then the
context's launches, then `_ctx_done`, then torch or host reads of what they wrote.  A launch may only read a tensor torch
wrote before the last `_torch_done`; torch and the host may only read what the context wrote before the last `_ctx_done`.
(Launches whose results only later launches read need no `_ctx_done` of their own: the context's stream orders them.)
The planners' and cameras' own methods (plan_dev, render_dev, OnboardMapper.update ...) follow the same rule inside.
"""
import time

import numpy as np

from . import _lib, counter_rng
from .goal_routes import GoalRoutes
from . import fleet_legs, fleet_flight, fleet_geo

MAX_TARGETS = 11        # :429-445: seed 0 .. 10 are planned, the mission is abandoned after the plan of target 10 fails


def target_jitter(seed, mission_ids, tick, target):
    """(len(mission_ids), 2) N(0, 1) draws of set_local_target's re-targeting (:469): zeros for the first target of a tick,
    mission i's own stream SeedSequence(seed, i, tick, target) for the others"""
    ids = np.asarray(mission_ids).reshape(-1)
    if target == 0:
        return np.zeros((ids.shape[0], 2))
    return np.stack([np.random.default_rng([int(seed), int(i), int(tick), int(target)]).normal(0.0, 1.0, 2) for i in ids]) \
        if ids.shape[0] else np.zeros((0, 2))


def target_jitter_counter(seed, mission_ids, tick, target):
    """`target_jitter` from the counter-based streams (counter_rng.py): mission i's two unit normals of (seed, i, tick,
    target), zeros for target 0 -- the rows neo_fleet_jitter_dev writes, bit for bit"""
    return counter_rng.target_jitter(seed, mission_ids, tick, target)


def plan_seed(seed, tick, target):
    """the seed BatchPlanner.plan gets for the plans of (tick, target): its retries then draw from
    SeedSequence(plan_seed, mission id, attempt)"""
    return int(np.random.SeedSequence([int(seed), int(tick), int(target)]).generate_state(1, np.uint64)[0] >> np.uint64(2))


def _check_arguments(batch_planner, goals, mode, seed, scene_ids, mission_ids, resident, onboard, scenes, scene_index,
                     record, neo, jitter, goal_routes, track_radius, metric_weights, geo=None):
    """FleetReplanLoop's refusals, in the order its callers meet them; returns the arguments it had to bring into shape
    on the way, by name"""
    counter = counter_rng.check_jitter(jitter, "FleetReplanLoop")
    if mode not in ("basic", "geo", "batch", "neo", "nn", "warmstart"):
        raise ValueError("FleetReplanLoop: mode must be 'basic', 'geo', 'batch', 'neo', 'nn' or 'warmstart'")
    if goal_routes is not None:
        if not isinstance(goal_routes, GoalRoutes):
            raise ValueError("FleetReplanLoop: goal_routes must be a GoalRoutes")
        if mode == "geo":
            raise ValueError("FleetReplanLoop: goal routes need a mode other than 'geo' (the tracker node has no geo planner)")
        if goals is not None and _lib.as_f64(goals).reshape(-1, 2).shape[0] != goal_routes.B:
            raise ValueError("FleetReplanLoop: one goal route per mission")
        goals = goal_routes.at(0.0)      # where the goals start
    elif goals is None:
        raise ValueError("FleetReplanLoop: goals may be None only with goal_routes")
    track_radius = float(track_radius)
    if not (np.isfinite(track_radius) and track_radius >= 0.0):
        raise ValueError("FleetReplanLoop: track_radius must be finite and >= 0")
    if metric_weights is None:      # the audit's default for a fixed goal, the tracker node's (1, 1, 1) (:175) with routes
        metric_weights = None if goal_routes is None else np.ones(3)
    else:
        metric_weights = _lib.as_f64(metric_weights).reshape(-1)
        if metric_weights.shape[0] != 3 or not np.all(np.isfinite(metric_weights)):
            raise ValueError("FleetReplanLoop: metric_weights must be three finite numbers")
    learned = mode in ("neo", "nn")
    if learned:
        if neo is None:
            raise ValueError("FleetReplanLoop: modes 'neo' and 'nn' need neo=BatchNeoPlanner")
        if neo.bp is not batch_planner:
            raise ValueError("FleetReplanLoop: neo's planner must be the loop's batch_planner")
        if int(batch_planner.cfg.init_wpts_num) != 2:
            raise ValueError("FleetReplanLoop: the network plans M = 3 pieces: modes 'neo' and 'nn' need init_wpts_num = 2")
        net, cam = neo.init.net, neo.camera
        if (cam.height, cam.width) != (net.img_height, net.img_width):
            raise ValueError("FleetReplanLoop: neo's camera renders %d x %d, its network takes %d x %d"
                             % (cam.height, cam.width, net.img_height, net.img_width))
        if scenes is None:
            raise ValueError("FleetReplanLoop: modes 'neo' and 'nn' need scenes=(boxes, box_begin), what the cameras see")
    # the network's guess and the carried plan live on the device: resident plans always
    resident = bool(resident) or learned or mode == "warmstart"
    if resident and mode == "geo" and geo is None:
        raise ValueError("FleetReplanLoop: resident=True needs mode 'basic' or 'batch' (geo_plan has no resident form)")
    if onboard is not None and mode == "geo" and geo is None:
        raise ValueError("FleetReplanLoop: onboard maps need mode 'basic' or 'batch' (geo on onboard maps is not built)")
    if (onboard is not None or record is not None) and scenes is None:
        raise ValueError("FleetReplanLoop: onboard and record need scenes=(boxes, box_begin), what the cameras see")
    goals = _lib.as_f64(goals).reshape(-1, 2)
    B = goals.shape[0]
    seed = int(seed)
    scene_index = None if scene_index is None else np.ascontiguousarray(scene_index, dtype=np.int32).reshape(-1)
    scene_ids = None if scene_ids is None else np.ascontiguousarray(scene_ids, dtype=np.int32).reshape(-1)
    mission_ids = np.arange(B) if mission_ids is None else np.asarray(mission_ids).reshape(-1)
    if mission_ids.shape[0] != B or (scene_ids is not None and scene_ids.shape[0] != B):
        raise ValueError("FleetReplanLoop: one mission id and one scene id per goal")
    if counter:
        counter_rng.check_seed(seed, "FleetReplanLoop")
        counter_rng.check_ids(mission_ids, "FleetReplanLoop")
    if onboard is not None and onboard.B != B:
        raise ValueError("FleetReplanLoop: the onboard mapper must have one entry per goal")
    if (onboard is not None or record is not None or learned) and scene_index is not None and scene_index.shape[0] != B:
        raise ValueError("FleetReplanLoop: scene_index must have one entry per goal")
    if record is not None and record.M != int(batch_planner.cfg.init_wpts_num) + 1:
        raise ValueError("FleetReplanLoop: the recorder's M must be the planner's init_wpts_num + 1")
    if record is not None and record.ctx is not batch_planner.ctx:
        raise ValueError("FleetReplanLoop: the recorder and the planner must share one context")
    return dict(counter=counter, goals=goals, track_radius=track_radius, metric_weights=metric_weights, resident=resident or geo is not None,
                seed=seed, scene_index=scene_index, scene_ids=scene_ids, mission_ids=mission_ids)


class _Timed:
    """`with _Timed(tm, key):` adds the wall time of the block to tm[key]"""
    __slots__ = ("tm", "key", "t0")

    def __init__(self, tm, key):
        self.tm, self.key = tm, key

    def __enter__(self):
        self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        self.tm[self.key] = self.tm.get(self.key, 0.0) + time.perf_counter() - self.t0


class _Tally:
    """the per-mission host counters of one run"""

    def __init__(self, B, tracked):
        self.replans, self.failed, self.opt_runs = (np.zeros(B, np.int32) for _ in range(3))
        self.iter_num = np.zeros(B, np.int64)
        self.abandoned = np.zeros(B, bool)
        self.landed = np.zeros(B, bool)      # near the goal and that plan spliced (:421-427)
        self.failed_ticks = np.zeros(B, np.int32) if tracked else None


class FleetReplanLoop:
    """`ReplanLoop` for B missions at once.  goals (B, 2); `map` one 2-D ESDF for all missions, or any of the maps plus
    scene_ids (B,) of per-mission scene ids (as BatchPlanner.optimize).  mode "basic" (BatchPlanner.plan), "geo"
    (geo_plan: the A* warm start), "batch" (batch_plan: the cheapest feasible of three lateral candidates, on the
    device), "neo" / "nn" or "warmstart" (below).  mission_ids (B,): the ids the random streams are keyed by
    (None: 0 .. B - 1) -- a mission flown alone with its id flies as it does in the fleet.  max_cmd_seconds sizes the resident command arrays
    (cap = max_cmd_seconds * cmd_hz rows a mission); a mission whose array fills up ends as not reached.
    resident=True (modes "basic" and "batch"): the plans run through BatchPlanner.plan_dev on the resident arrays --
    the same flights; head, tail and x no longer pass through the host.
    onboard: an OnboardMapper for the same B missions -- targets and plans then use each mission's onboard scene, `map` /
    scene_ids only the final audit; scenes = (boxes (NB, 6), box_begin (S + 1,)) as DepthCamera.pack_scenes returns them
    and scene_index (B,) (None: scene 0) say what each mission's camera sees; des_pos_z is the eye's height.  run() starts
    from onboard.reset(): every flight begins knowing nothing, whatever the mapper saw before.
    record_poses adds `poses` (ticks, B, 5) and `sensed` (ticks, B) to the result.
    record: a DemoRecorder (record.py) -- every spliced plan becomes a row of its dataset, in the order (tick, target
    round, ascending mission); works with every mode, resident or not, with or without onboard, and needs scenes /
    scene_index as onboard does (the recorder's camera looks at the same scenes).  run() appends to what the recorder
    holds: recorder.reset() starts over.  With onboard set as well the images are rendered twice a tick, once by the
    mapper (float32 metres) and once for the recorder (uint8), from the same poses.
    mode "neo" / "nn" with neo: a BatchNeoPlanner built on this batch_planner (init_wpts_num = 2) -- plan_dev from the
    network's guess, or the guess flown as it is; scenes / scene_index as for onboard; resident plans always.  The
    network's camera renders its own images (a third render with onboard and record set).  `x` is a host copy of the
    resident plan array.
    mode "warmstart": every replan starts from the mission's previous plan -- its waypoints carried along relative to the
    planning start state, the durations the planner last held (BatchPlanner.warm_guess_dev / warm_carry_dev around
    plan_dev); the first plan is a basic plan; resident plans always; with onboard, record and either jitter.
    jitter "numpy" (one NumPy generator per mission and draw, on the host) or "counter" (every mode, resident or not): the
    target jitter of a round is drawn by neo_fleet_jitter_dev on the context's stream in front of the target kernel, and
    every plan call gets jitter="counter"; mission ids in 0 .. 2^31 - 1 and a seed in 0 .. 2^64 - 1.
    goal_routes: a GoalRoutes (goal_routes.py) of B routes -- the goals move, `goals` may be None (the goals are the
    routes at t = 0) and mode "geo" is refused.  run() then flies max_replans ticks without landing anybody; its result
    gains the eight track_* fields (gap_mean, gap_max, t_gap_max, gap_min, t_gap_min, gap_final, t_first_within,
    frac_within: within track_radius metres of the goal), track_count, track_flags, failed_ticks and goal_final;
    final_dist is the distance to goal_final, n_flown = cmd_index + 1 and success = nothing went wrong (flags == 0, no
    metric failure).  metric_weights (3,): the flight metric's weights; None: the audit's default (1, 1, 100) for fixed
    goals, the tracker node's (1, 1, 1) with routes.
    goal_sequences: a GoalSequences (goal_sequences.py) of B goal lists -- every mission flies its goals one after the
    other, `goals` may be None (the goals start as every mission's goal 0).  A leg ends LANDED, ABANDONED, STUCK or, with
    leg_timeout (seconds; None: no limit), TIMEOUT: a leg whose own tick count j, from 0 at its first plan, has
    (j + 1) * step / cmd_hz > leg_timeout closes at the end of that tick (the reference's max_target_find_time; its node
    reports such a leg failed but forgets end_mission -- here it ends like an aborted one and the next goal follows).
    max_legs (None: the longest list) caps the legs a mission flies and sizes the log.  max_replans is the run's tick
    budget, as with routes; legs still open when it runs out are logged NEO_LEG_OPEN (a leg opened at the end of the last
    tick, never planned, among them: n_flown 0, final_dist inf, and the "last leg" keys describe it).  Refused: goal_routes (a route
    never lands), mode "warmstart" ("the first plan is basic" is a per-mission fact that _plan_warm takes from
    tick > 0 today) and mode "geo" (as for routes).  Everything else works unchanged: basic and batch, resident or not,
    "neo" / "nn", onboard (reset once, at run()'s start), record, both jitters; a flap's mission ids must be the
    loop's.  The result keeps every key: replans, failed_attempts, iter_num and opt_runs are totals over the legs; n_cmd,
    n_flown, final_dist, flags, abandoned, metric_fail, count, audit_flags and the audit fields describe the last leg
    flown; success = every goal of the sequence was flown and every leg succeeded.  New: n_legs (B,), leg_<field>
    (B, max_legs) for every field of the log (_lib.LEG_FIELDS) and the host tallies leg_replans, leg_failed_attempts,
    leg_iter_num, leg_opt_runs, leg_ticks, leg_first_tick; NaN / -1 beyond n_legs.
    flight: a FlightModel (flight_model.py) -- the missions track their commands with lag and gusts instead of sitting on
    them (module docstring); settle_seconds: how long a landed mission may hold its last command until it is within
    target_reach_threshold of the goal.  The result gains fly_<field> for _lib.FLY_FIELDS, fly_count, fly_flags and
    fly_saturated; n_flown counts flown rows (a landed mission's settle rows included) and flown_rows(i) returns them.
    Refused with goal_sequences.
    geo: a BatchGeoPlanner (geo_resident.py) built on this batch_planner, mode "geo" only, init_wpts_num = 2 -- the geo
    plans run on the resident arrays (module docstring), the same flights as the host form's; resident plans always; may
    be combined with onboard (the direct search on the missions' own maps), record, flight and either jitter.  Without
    it mode "geo" still refuses resident=True and onboard, in the same words."""

    def __init__(self, batch_planner, map, goals, mode="basic", cmd_hz=60, replan_period=1.0, planning_time_ahead=1.0,
                 longitu_step_dis=5.0, lateral_step_length=1.0, target_reach_threshold=0.2, max_cmd_seconds=120, seed=0,
                 scene_ids=None, mission_ids=None, metric_eva_interval=0.1, resident=False, onboard=None, scenes=None,
                 scene_index=None, des_pos_z=2.0, record_poses=False, record=None, neo=None, jitter="numpy",
                 goal_routes=None, track_radius=1.0, metric_weights=None, goal_sequences=None, leg_timeout=None, max_legs=None,
                 flight=None, settle_seconds=2.0, geo=None):
        self.flight, self.settle_seconds, self._fly_model = fleet_flight.check_arguments(flight, settle_seconds, goal_sequences, cmd_hz)
        self.geo = fleet_geo.check_arguments(geo, mode, batch_planner)
        goals, self.leg_timeout, self.max_legs = fleet_legs.check_arguments(goal_sequences, leg_timeout, max_legs, goals, goal_routes, mode)
        a = _check_arguments(batch_planner, goals, mode, seed, scene_ids, mission_ids, resident, onboard, scenes, scene_index,
                             record, neo, jitter, goal_routes, track_radius, metric_weights, self.geo)
        self.counter, self.jitter, self.seed = a["counter"], jitter, a["seed"]
        self.routes, self.track_radius, self.metric_weights = goal_routes, a["track_radius"], a["metric_weights"]
        self.bp, self.map, self.mode, self.resident = batch_planner, map, mode, a["resident"]
        self.onboard, self.scenes, self.des_pos_z, self.record_poses = onboard, scenes, float(des_pos_z), bool(record_poses)
        self.record = record
        self.neo = neo if mode in ("neo", "nn") else None
        self.goals, self.scene_index, self.scene_ids, self.mission_ids = a["goals"], a["scene_index"], a["scene_ids"], a["mission_ids"]
        self.B = self.goals.shape[0]
        self.sequences = goal_sequences
        fleet_legs.check_ids(goal_sequences, self.mission_ids)
        self.cmd_hz = cmd_hz
        fleet_flight.check_ids(flight, self.mission_ids)
        self.replan_period, self.planning_time_ahead = replan_period, planning_time_ahead
        self.longitu_step_dis, self.lateral_step_length = float(longitu_step_dis), float(lateral_step_length)
        self.target_reach_threshold = target_reach_threshold
        self.move_vel = 0.8 * float(batch_planner.cfg.v_max)                      # :87
        self.cap = int(round(max_cmd_seconds * cmd_hz))
        self.stride = int(round(cmd_hz * metric_eva_interval))                    # rows between two metric samples (:119)
        # what targets and plans see: the missions' onboard scenes, or the given map(s)
        self.plan_map = map if onboard is None else onboard
        self.plan_scene_ids = self.scene_ids if onboard is None else onboard.scene_ids
        # The mode's plan step (self, sub, pending, tick, r) -> (ok, nit_total, attempts): the resident x and solved are ready
        # for the splice when it returns.  (The class's functions, not bound methods: the loop holds the command arrays, and
        # a reference to itself would leave their release to the cycle collector.)
        cls = type(self)
        self._plan_step = {"basic": cls._plan_resident if self.resident else cls._plan_host, "geo": cls._plan_geo if self.geo is None else fleet_geo.plan_step,
                           "batch": cls._plan_batch, "neo": cls._plan_neo, "nn": cls._plan_nn, "warmstart": cls._plan_warm}[mode]
        self._fallback = cls._fallback_resident if self.resident else cls._fallback_host      # mode "batch"
        # who looks through the cameras once a tick, in this order: (its timing key, its function)
        self._viewers = [(key, see) for key, who, see in (("sense_s", onboard, cls._see_onboard), ("neo_s", self.neo, cls._see_neo),
                                                          ("record_s", record, cls._see_record)) if who is not None]
        self.timings = []
        self._dev = None
        self._batch = None      # mode "batch": BatchPlanner.batch_buffers, made at the first plan
        self._plan = None       # resident=True: BatchPlanner.plan_buffers, made at the first plan
        self.uncounted_candidates = np.zeros(self.B, np.int64)   # mode "batch": per mission, candidate runs left out of opt_runs

    # ------------------------------------------------------------ device calls
    def _subset(self, idx):
        import torch
        return torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(self._device)

    def _up(self, name, host):
        """mission-indexed host array -> its resident device tensor"""
        import torch
        self._dev[name].copy_(torch.from_numpy(np.ascontiguousarray(host)))

    # ---- the stream rule (module docstring): torch work, _torch_done, the context's launches, _ctx_done, torch / host reads
    def _torch_done(self):
        """what torch has queued is in place: the context, on its own stream, may launch on it"""
        import torch
        torch.cuda.synchronize(self._device)

    def _ctx_done(self):
        """what the context has launched is in place: torch and the host may read it"""
        self.bp.ctx.synchronize()

    def _call(self, name, *args):
        """the library's entry point `name` on the loop's context (Context.call)"""
        self.bp.ctx.call(name, *args)

    # the argument groups the fleet entry points share
    def _rows(self, sub):
        """the missions a launch works on: B, subset, count (None: all B)"""
        return self.B, self._p(sub), 0 if sub is None else int(sub.numel())

    def _cmd(self):
        """the resident command arrays: cmd, cap, cmd_len, cmd_index"""
        return (self._p(self._dev["cmd"]), self.cap) + self._ptrs("cmd_len", "cmd_index")

    def _flown(self):
        """the rows that say where the drone WAS: the flown rows with a flight model, the command rows without one --
        same argument group as _cmd(), for whoever reads the actual state"""
        return self._cmd() if self.flight is None else (self._p(self._dev["flown"]), self.cap) + self._ptrs("cmd_len", "cmd_index")

    def _route_table(self):
        return (self._p(self._dev["vertices"]), int(self._dev["vertices"].shape[0])) + self._ptrs("route_begin", "speed", "closed")

    def _ptrs(self, *names):
        """the device pointers of the named resident tensors"""
        return tuple(self._p(self._dev[k]) for k in names)

    # ---- the camera stage: one pose launch a tick, then whoever looks through the cameras
    def _camera_stage(self, sub, active, tm):
        """the active missions' poses from where they are (the eye at (cur_pos, des_pos_z), heading along the last step of
        the command array), once, then the viewers in their order: the onboard mapper, the network's features, the
        recorder's images.  The pose launch is charged to the first viewer.  `view` is the gather of the active missions'
        pose / scene_index rows the network and the recorder share: made once, after a _ctx_done behind the pose launch."""
        view = None
        for k, (key, see) in enumerate(self._viewers):
            with _Timed(tm, key):
                if k == 0:
                    self._torch_done()
                    self._call("neo_fleet_pose_dev", *self._rows(sub), *self._cmd(), *self._ptrs("cur_pos", "goal"),
                               self.des_pos_z, self._p(self._dev["pose"]))
                view = see(self, sub, active, tm, view)
        if self.record_poses and self.onboard is not None:
            self._poses.append(self._dev["pose"].cpu().numpy())
            sensed = np.zeros(self.B, bool)
            sensed[active] = True
            self._sensed.append(sensed)

    def _see_onboard(self, sub, active, tm, view):
        """mapper.update on what the active missions' cameras see: render, integrate, rebuild"""
        d = self._dev
        self._ctx_done()
        rebuilt = self.onboard.update(d["boxes"], d["box_begin"], d["pose"], d["scene_index"], subset=active)
        tm["rebuilt"] = int(len(rebuilt))
        tm.update({k: self.onboard.last[k] for k in ("render_s", "integrate_s", "rebuild_s")})
        return view

    def _see_neo(self, sub, active, tm, view):
        """modes "neo" and "nn": the velocities now and the features of what the cameras see into the loop's resident
        cur_vel and feature arrays (the scatter is torch's: every target round starts with a _torch_done)"""
        d = self._dev
        return self._see_images(sub, active, view, d["cur_vel"], self.neo.features_dev, d["feature"])

    def _see_record(self, sub, active, tm, view):
        """record: the velocities now and the depth images into the recorder's per-mission buffers"""
        rec = self.record
        render = lambda *a: rec.camera.render_dev(*a, chunk=rec.chunk, want_m=False)["depth_u8"]
        return self._see_images(sub, active, view, rec.cur_vel, render, rec.staging)

    def _see_images(self, sub, active, view, cur_vel, render, into):
        """one image consumer: the active missions' velocities now into its `cur_vel`, then render(boxes, box_begin, pose
        rows, scene_index rows) of the active missions scattered into its per-mission buffer `into`"""
        d = self._dev
        self._call("neo_record_state_dev", *self._rows(sub), *self._flown(), self._p(d["head"]), self._p(cur_vel))
        self._ctx_done()
        if view is None:
            whole = active.size == self.B
            idx64 = None if whole else sub.long()
            take = lambda t: t if (t is None or whole) else t.index_select(0, idx64).contiguous()
            view = idx64, take(d["pose"]), take(d["scene_index"])
        idx64, pose_k, sidx_k = view
        out = render(d["boxes"], d["box_begin"], pose_k, sidx_k)
        if idx64 is None:
            into.copy_(out)
        else:
            into.index_copy_(0, idx64, out)
        return view


    def _alloc(self, n):
        import torch
        c = self.bp.ctx
        self._device = dev = torch.device("cuda", c.device)
        self._p = _lib.dev_ptr
        B = self.B
        f = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
        i = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        self._dev = dict(cmd=f(B, self.cap, 3, 2), cmd_len=i(B), cmd_index=i(B), future_index=i(B), flags=i(B),
                         cur_pos=f(B, 2), goal=f(B, 2), jitter=f(B, 2), head=f(B, 3, 2), tail=f(B, 3, 2), near=i(B),
                         steps=i(B), x=f(B, n), solved=i(B), n_flown=i(B), audit=f(B, _lib.NEO_AUDIT_FIELDS), count=i(B),
                         audit_flags=i(B), slots=None, plan_slots=None)
        if self.scene_ids is not None:
            slot_of = {int(s): int(c.lib.neo_scene_slot(c.h, int(s))) for s in np.unique(self.scene_ids)}
            if min(slot_of.values()) < 0:
                raise _lib.NeoError("FleetReplanLoop: a scene id without a map")
            self._dev["slots"] = self._subset(np.array([slot_of[int(s)] for s in self.scene_ids]))
        self._dev["plan_slots"] = self._dev["slots"]
        if self.onboard is not None:
            self.onboard.reset()      # all unknown, and the slots as the map table numbers them now
            self._dev.update(plan_slots=self.onboard.slots)
        if self.mode == "warmstart":      # what a mission carries from one plan to the next, and the guess made of it
            M = (n + 2) // 3
            self._dev.update(wpts_local=f(B, 2, M - 1), ts_carry=f(B, M), x0=f(B, n))
        if self.neo is not None:      # the network's inputs that are not the plan's own: velocity now, image features
            self._dev.update(cur_vel=f(B, 2), feature=torch.zeros((B, 24), dtype=torch.float32, device=dev))
        if self.mode == "neo":      # the network's guess, attempt 0's start
            self._dev.update(x0=f(B, n))
        if self.geo is not None:      # the geo guess, attempt 0's start
            fleet_geo.alloc(self, f)
        if self.onboard is not None or self.record is not None or self.neo is not None:      # what the cameras see, and where from
            boxes, box_begin = self.scenes
            self._dev.update(pose=f(B, 5),
                             boxes=torch.from_numpy(np.ascontiguousarray(boxes, dtype=np.float64).reshape(-1, 6)).to(dev),
                             box_begin=torch.from_numpy(np.ascontiguousarray(box_begin, dtype=np.int32)).to(dev),
                             scene_index=None if self.scene_index is None else torch.from_numpy(self.scene_index).to(dev))
            if self._dev["boxes"].shape[0] == 0:      # (a scene list without any box still hands over a valid pointer)
                self._dev["boxes"] = f(1, 6)
        if self.record is not None:
            self.record.bind(B)
            self.record.T_min, self.record.T_max = float(self.bp.cfg.T_min), float(self.bp.cfg.T_max)   # what rows() maps tau with
        if self.flight is not None:      # the drones, what they flew, and the tracking-error record
            fleet_flight.alloc(self, f, i)
        if self.record is not None or self.counter or self.flight is not None:
            self._dev["mission_ids"] = self._subset(self.mission_ids)
        if self.routes is not None:      # the route table, and what the track audit writes
            r = self.routes
            self._dev.update(vertices=torch.from_numpy(r.vertices).to(dev), route_begin=torch.from_numpy(r.route_begin).to(dev),
                             speed=torch.from_numpy(r.speed).to(dev), closed=torch.from_numpy(r.closed).to(dev),
                             track=f(B, _lib.NEO_TRACK_FIELDS), track_count=i(B), track_flags=i(B))
        if self.sequences is not None:      # the goal lists, the log, and what close hands to open
            fleet_legs.alloc(self, f, i)
        self._poses, self._sensed = [], []
        self._host_head = self._host_x = None      # the host plan step's copies, made at its first plan
        self._up("goal", self.goals)

    def _plan_bufs(self):
        if self._plan is None:
            self._plan = self.bp.plan_buffers(self.B, self._device, D=2)
            self._torch_done()
        return self._plan

    # ---- the plan steps, one per mode: (sub, pending, tick, r) -> (ok over pending, nit_total, attempts) as the host
    # planner's dict has them; `pending` ascending, `sub` the same on the device; the resident x and solved are written
    def _plan_dev(self, sub, tick, r, **kw):
        """BatchPlanner.plan_dev for the missions `sub` on the resident head / tail, into the resident x and solved"""
        d = self._dev
        return self.bp.plan_dev(self.plan_map, d["head"], d["tail"], bufs=self._plan_bufs(), slots=d["plan_slots"], subset=sub,
                                x=d["x"], solved=d["solved"], seed=plan_seed(self.seed, tick, r), jitter=self.jitter,
                                stream_ids=d["mission_ids"] if self.counter else self.mission_ids, **kw)

    def _plan_resident(self, sub, pending, tick, r, x0=None):
        """resident=True, mode "basic": plan_dev; the other resident modes hand it their guess `x0` as attempt 0's start"""
        bufs = self._plan_dev(sub, tick, r, x0=x0)
        idx = sub.long()
        return (self._dev["solved"][idx].cpu().numpy() != 0, bufs["nit_total"][idx].cpu().numpy(),
                bufs["attempts"][idx].cpu().numpy())

    def _plan_host(self, sub, pending, tick, r, planner=None):
        """resident=False, mode "basic", and mode "geo": BatchPlanner.plan / geo_plan on host arrays -- head and tail come
        down (head once a tick: only the advance moves it), x and solved go up whole, from the host's copy of x"""
        d = self._dev
        if r == 0:
            self._host_head = d["head"].cpu().numpy()
        if self._host_x is None:
            self._host_x = np.zeros(tuple(d["x"].shape))
        out = (planner or self.bp.plan)(self.plan_map, self._host_head[pending], d["tail"].cpu().numpy()[pending],
                                        scene_ids=None if self.plan_scene_ids is None else self.plan_scene_ids[pending],
                                        seed=plan_seed(self.seed, tick, r), stream_ids=self.mission_ids[pending],
                                        **({"jitter": "counter"} if self.counter else {}))
        self._host_x[pending] = out["x"]
        solved = np.zeros(self.B, np.int32)
        solved[pending[out["solved"]]] = 1
        self._up("x", self._host_x)
        self._up("solved", solved)
        return out["solved"], out["nit_total"], out["attempts"]

    def _plan_geo(self, sub, pending, tick, r):
        return self._plan_host(sub, pending, tick, r, planner=self.bp.geo_plan)

    def _plan_neo(self, sub, pending, tick, r):
        """mode "neo": the network's guess for the pending missions on the resident pose, velocity, head, tail and
        features (BatchNeoPlanner.warm_start_dev, on the context's stream), then plan_dev from it"""
        d = self._dev
        x0 = self.neo.warm_start_dev(d["pose"], d["cur_vel"], d["head"], d["tail"], d["feature"], subset=sub, x0=d["x0"])
        return self._plan_resident(sub, pending, tick, r, x0=x0)

    def _plan_warm(self, sub, pending, tick, r):
        """mode "warmstart": the first plan of a mission (tick 0, and its re-targeted repeats) is a basic plan; every
        later one starts from what the mission carries -- neo_fleet_warm_guess_dev writes the resident x0 on the context's
        stream, plan_dev takes it as attempt 0's start.  Then neo_fleet_warm_carry_dev, on the same stream, keeps what the
        round's missions carry on of the plan call just made; status and attempts are plan_dev's."""
        d, pb = self._dev, self._plan_bufs()
        x0 = self.bp.warm_guess_dev(d["head"], d["wpts_local"], d["ts_carry"], d["x0"], subset=sub) if tick > 0 else None
        res = self._plan_resident(sub, pending, tick, r, x0=x0)
        self.bp.warm_carry_dev(d["x"], d["head"], d["solved"], pb["status"], pb["attempts"], d["wpts_local"], d["ts_carry"],
                               subset=sub)
        return res

    def _plan_nn(self, sub, pending, tick, r):
        """mode "nn" (the reference's selected_planner:=nn): the network's guess straight into the resident x, solved = 1
        for the round's missions, no optimiser launch"""
        d = self._dev
        self.neo.warm_start_dev(d["pose"], d["cur_vel"], d["head"], d["tail"], d["feature"], subset=sub, x0=d["x"])
        d["solved"].index_fill_(0, sub.long(), 1)      # (torch's stream: the loop waits for it before the splice)
        return np.ones(pending.size, bool), np.zeros(pending.size, np.int64), np.zeros(pending.size, np.int32)

    def _plan_batch(self, sub, pending, tick, r):
        """mode "batch": one target round's plans for the missions `pending` (ascending; `sub` the same on the device) on the
        resident head / tail -- select writes the resident x and solved -- then the host `plan` for the missions without
        a feasible candidate.  Returns (ok over pending, nit_total, attempts) as the host planners' dicts have them."""
        bp, d = self.bp, self._dev
        if self._batch is None:
            self._batch = bp.batch_buffers(self.B, 3, self._device)
            self._torch_done()
        bufs = bp.batch_plan_dev(self.plan_map, d["head"], d["tail"], self._batch, slots=d["plan_slots"], subset=sub, x=d["x"],
                                 solved=d["solved"])
        fb = bp.batch_fallback(bufs)
        nit = bufs["nit_total"].cpu().numpy()[pending].astype(np.int64)
        runs = bufs["opt_runs"].cpu().numpy()[pending].copy()
        self.uncounted_candidates[pending] += 3 - runs      # candidate runs that overflowed: the reference counts none of them
        if fb.size:
            at = np.searchsorted(pending, fb)
            nit_fb, runs_fb = self._fallback(self, fb, bufs["fallback"][:fb.size], tick, r)
            nit[at] += nit_fb
            runs[at] += runs_fb
        ok = d["solved"].cpu().numpy()[pending] != 0
        return ok, nit, runs

    def _fallback_resident(self, fb, fb_dev, tick, r):
        """the missions `fb` (`fb_dev` the same on the device) through plan_dev: candidate 0 (linspace's bits, with pack_x's
        tau) straight into plan_dev's packed rows.  Returns their nit_total and attempts."""
        bp, d, p, pb = self.bp, self._dev, self._p, self._plan_bufs()
        count = int(bp.cfg.init_wpts_num)
        self._call("neo_batch_candidates_dev", *self._rows(fb_dev), count + 1, 2, 1, *self._ptrs("head", "tail", "plan_slots"),
                   _lib.ptr(bp._plan_frac_tau(count)[1]), None, p(pb["x_k"]), p(pb["head_k"]), p(pb["tail_k"]),
                   p(pb["slots_k"]) if d["plan_slots"] is not None else None)
        self._plan_dev(fb_dev, tick, r, _guessed=True)
        idx = fb_dev.long()
        return pb["nit_total"][idx].cpu().numpy(), pb["attempts"][idx].cpu().numpy()

    def _fallback_host(self, fb, fb_dev, tick, r):
        """the missions `fb` through the host `plan` from candidate 0; their rows of x / solved are uploaded (torch's
        stream: the loop waits for it before the splice).  Returns their nit_total and attempts."""
        import torch
        bp, d = self.bp, self._dev
        idx = torch.from_numpy(fb).to(self._device)
        head, tail = d["head"][idx].cpu().numpy(), d["tail"][idx].cpu().numpy()
        res = bp.plan(self.plan_map, head, tail, int_wpts=bp.batch_init_guess(head, tail, K=1)[0][:, 0],
                      ts=np.tile(bp._batch_ts_tau(int(bp.cfg.init_wpts_num))[0], (fb.size, 1)),
                      scene_ids=None if self.plan_scene_ids is None else self.plan_scene_ids[fb],
                      seed=plan_seed(self.seed, tick, r), stream_ids=self.mission_ids[fb], jitter=self.jitter)
        d["x"][idx] = torch.from_numpy(np.ascontiguousarray(res["x"])).to(self._device)
        d["solved"][idx] = torch.from_numpy(res["solved"].astype(np.int32)).to(self._device)
        return res["nit_total"], res["attempts"]

    # ------------------------------------------------------------ the loop
    def run(self, start_pos, start_vel=None, max_replans=60):
        """fly every mission from start_pos (B, 2) (start_vel (B, 2), None: at rest) towards its goal: the first plan and up to
        `max_replans` replans, one replan period apart.  Returns a dict of (B,) arrays: success (the reference's
        reached_target: the flight ended within target_reach_threshold of the goal, was not abandoned and is no
        METRIC_FAIL), replans (plans that were spliced), failed_attempts, iter_num, opt_runs, n_cmd (rows of the command
        array), n_flown, final_dist, flags (NEO_FLEET_FLAG_*), audit_flags (NEO_AUDIT_FLAG_*), count and the ten audit
        fields by name.  With goal_routes: the first plan and `max_replans` ticks of chasing (class docstring)."""
        B, bp = self.B, self.bp
        count = int(bp.cfg.init_wpts_num)
        M, n = count + 1, 2 * count + count + 1
        bp._sync()
        self._alloc(n)
        d, p = self._dev, self._p
        head = np.zeros((B, 3, 2))
        head[:, 0] = _lib.as_f64(start_pos).reshape(B, 2)
        if start_vel is not None:
            head[:, 1] = _lib.as_f64(start_vel).reshape(B, 2)
        tracked = self.routes is not None
        t = _Tally(B, tracked)
        legs = None if self.sequences is None else fleet_legs.LegTally(B, self.max_legs, self.sequences.count)
        active = np.arange(B)
        self.timings = []
        self.uncounted_candidates[:] = 0
        step = int(round(self.replan_period * self.cmd_hz))
        ahead = int(self.planning_time_ahead * self.cmd_hz)                        # :531
        for tick in range(max_replans + 1):
            if active.size == 0:
                break
            tm = dict(tick=tick, active=int(active.size), fleet_s=0.0, plan_s=0.0, plans=0, plan_requests=0)
            t_tick = time.perf_counter()
            # hold / advance, then where the goals are now: before sensing and the targets, tick 0 included.  (No _ctx_done
            # behind them: the next to read what they write are launches on the same stream, the camera stage's or a target's.)
            with _Timed(tm, "fleet_s"):
                sub_a = self._subset(active)      # the tick's missions, uploaded once
                if tick == 0:
                    self._up("cur_pos", head[:, 0])
                    self._up("head", head)
                    if legs is not None:
                        self._up("leg_start", head[:, 0])
                    if self.flight is not None:
                        fleet_flight.start(self, head)
                if tick > 0 or tracked:
                    self._torch_done()
                if tick > 0:
                    if tracked:      # a mission whose commands end before the coming period is over holds its last one
                        self._call("neo_fleet_hold_dev", *self._rows(sub_a), *self._cmd(), step, p(d["flags"]))
                    if self.flight is None:
                        self._call("neo_fleet_advance_dev", *self._rows(sub_a), *self._cmd(), p(d["future_index"]), step, ahead,
                                   *self._ptrs("cur_pos", "head"))
                    else:
                        fleet_flight.fly(self, sub_a, step, ahead, int(tick == 1))
                if tracked:
                    self._call("neo_fleet_goal_route_dev", *self._rows(sub_a), *self._route_table(),
                               float((tick * step) / self.cmd_hz), p(d["goal"]))
            self._camera_stage(sub_a, active, tm)
            if legs is not None:
                legs.begin_tick(active, tick)
            pending, sub = active, sub_a
            for r in range(MAX_TARGETS):
                with _Timed(tm, "fleet_s"):      # jitter and target
                    if r > 0:
                        sub = self._subset(pending)      # the round's missions, uploaded once
                    if not self.counter:
                        jit = np.zeros((B, 2))
                        jit[pending] = target_jitter(self.seed, self.mission_ids[pending], tick, r)
                        self._up("jitter", jit)
                    self._torch_done()
                    if self.counter:
                        self._call("neo_fleet_jitter_dev", *self._rows(sub), self.seed, tick, r, *self._ptrs("mission_ids", "jitter"))
                    self._call("neo_fleet_target_batch_dev", self.plan_map.scene_id, p(d["plan_slots"]), *self._rows(sub),
                               *self._ptrs("cur_pos", "goal", "jitter"), self.longitu_step_dis, self.lateral_step_length,
                               self.move_vel, *self._ptrs("tail", "near", "steps", "flags"))
                    self._ctx_done()
                    near = d["near"].cpu().numpy() != 0
                with _Timed(tm, "plan_s"):
                    ok, nit_total, attempts = self._plan_step(self, sub, pending, tick, r)
                tm["plans"] += 1
                tm["plan_requests"] += int(pending.size)
                t.iter_num[pending] += nit_total
                t.opt_runs[pending] += attempts
                if legs is not None:
                    legs.count_round(pending, ok, nit_total, attempts)
                with _Timed(tm, "fleet_s"):      # record commit and splice
                    self._torch_done()
                    if self.record is not None:      # the round's rows, from the plans about to be spliced
                        self.record.commit(B, sub, d["x"], d["head"], d["tail"], d["solved"], d["pose"], d["mission_ids"], tick, r)
                    self._call("neo_fleet_splice_dev", *self._rows(sub), M, *self._ptrs("x", "head", "tail", "solved"),
                               float(self.cmd_hz), int(tick == 0), *self._cmd(), *self._ptrs("future_index", "flags"))
                    self._ctx_done()
                t.replans[pending[ok]] += 1
                t.failed[pending[~ok]] += 1
                if not tracked:      # (a tracked mission never lands: planning goes on, :319-321)
                    t.landed[pending[ok]] = near[pending[ok]]
                pending = pending[~ok]
                if pending.size == 0:
                    break
            if tracked:      # all targets of the tick failed: the mission flies on along its old commands (:265-279)
                t.failed_ticks[pending] += 1
            else:
                t.abandoned[pending] = True
            flags = d["flags"].cpu().numpy()
            stuck = (flags & (_lib.NEO_FLEET_FLAG_CMD_FULL | _lib.NEO_FLEET_FLAG_SPLICE_FAILED)) != 0
            if legs is None:
                active = active[~(t.abandoned | t.landed | stuck)[active]]
            else:
                with _Timed(tm, "legs_s"):
                    active = fleet_legs.end_of_tick(self, t, legs, active, stuck, step)
            tm["tick_s"] = time.perf_counter() - t_tick
            tm["host_s"] = tm["tick_s"] - tm["fleet_s"] - tm["plan_s"] - tm.get("sense_s", 0.0) - tm.get("record_s", 0.0) - \
                tm.get("neo_s", 0.0) - tm.get("legs_s", 0.0)
            self.timings.append(tm)
        if legs is not None:
            return fleet_legs.finish(self, t, legs)
        return self._finish(t)

    def _finish(self, tally):
        """the audits on the true maps over what was flown, and the result dict"""
        import torch
        d, p = self._dev, self._p
        abandoned, landed = tally.abandoned, tally.landed
        tracked = self.routes is not None
        cmd_len = d["cmd_len"].cpu().numpy()
        cmd_index = d["cmd_index"].cpu().numpy()
        # a mission that landed flies its array to the end; the others stopped at the row they were on (a tracked mission
        # is always on a row of its array: n_flown = cmd_index + 1, whatever it held on the way)
        took = {}
        if self.flight is None:
            n_flown = np.where(landed, cmd_len, np.minimum(cmd_index + 1, cmd_len)).astype(np.int32)
            self._up("n_flown", n_flown)
            self._torch_done()
            rows = d["cmd"]
        else:      # the landed missions fly their arrays out and settle; the others stopped on the row they were on
            n_flown, rows = fleet_flight.settle(self, landed, took)
        flown = p(rows), self.cap, p(d["n_flown"]), self.stride, float(self.cmd_hz)
        with _Timed(took, "audit_s"):
            self._call("neo_fleet_audit_batch_dev", self.map.scene_id, p(d["slots"]), *self._rows(None), *flown,
                       None if self.metric_weights is None else _lib.ptr(self.metric_weights),
                       *self._ptrs("audit", "count", "audit_flags"))
            self._ctx_done()
        if tracked:
            with _Timed(took, "track_audit_s"):
                self._call("neo_fleet_track_audit_dev", *self._rows(None), *flown, *self._route_table(), self.track_radius,
                           *self._ptrs("track", "track_count", "track_flags"))
                self._ctx_done()
            self.track_audit_s = took["track_audit_s"]
        self.audit_s = took["audit_s"]
        if self.flight is not None:
            fleet_flight.error(self, took)
        goals = d["goal"].cpu().numpy() if tracked else self.goals      # tracked: where the goals were at the last tick
        last = torch.from_numpy(np.maximum(n_flown - 1, 0).astype(np.int64)).to(self._device)
        end = rows[torch.arange(self.B, device=self._device), last, 0].cpu().numpy()
        final_dist = np.where(n_flown > 0, np.linalg.norm(end - goals, axis=1), np.inf)
        flags = d["flags"].cpu().numpy() | np.where(abandoned, _lib.NEO_FLEET_FLAG_ABANDONED, 0).astype(np.int32)
        audit = d["audit"].cpu().numpy()
        audit_flags = d["audit_flags"].cpu().numpy()
        metric_fail = (audit_flags & (_lib.NEO_AUDIT_FLAG_METRIC_FAIL | _lib.NEO_AUDIT_FLAG_NONFINITE)) != 0
        out = {name: audit[:, k] for k, name in enumerate(_lib.AUDIT_FIELDS)}
        if tracked:      # a chase has no arrival: it succeeds when nothing went wrong on the way
            success = (flags == 0) & ~metric_fail
        else:
            success = (final_dist < self.target_reach_threshold) & ~abandoned & ~metric_fail & (flags == 0)
        out.update(success=success,
                   replans=tally.replans, failed_attempts=tally.failed, iter_num=tally.iter_num, opt_runs=tally.opt_runs, n_cmd=cmd_len,
                   n_flown=n_flown, final_dist=final_dist, flags=flags, audit_flags=audit_flags,
                   count=d["count"].cpu().numpy(), abandoned=abandoned, metric_fail=metric_fail)
        if tracked:
            track = d["track"].cpu().numpy()
            out.update({"track_" + name: track[:, k] for k, name in enumerate(_lib.TRACK_FIELDS)})
            out.update(track_count=d["track_count"].cpu().numpy(), track_flags=d["track_flags"].cpu().numpy(),
                       failed_ticks=tally.failed_ticks, goal_final=goals)
        if self.flight is not None:
            fleet_flight.results(self, out)
        return self._with_poses(out)

    def _with_poses(self, out):
        if self.record_poses and self.onboard is not None:
            out.update(poses=np.stack(self._poses) if self._poses else np.zeros((0, self.B, 5)),
                       sensed=np.stack(self._sensed) if self._sensed else np.zeros((0, self.B), bool))
        return out

    @property
    def x(self):
        """a host copy of the resident (B, n) plan array: every mission's last plan (read-only: writing it changes nothing)"""
        if self._dev is None:
            raise _lib.NeoError("FleetReplanLoop.x: no flight yet")
        x = self._dev["x"].cpu().numpy()
        x.flags.writeable = False
        return x

    def commands(self, i):
        """the command array of mission i (n_cmd, 3, 2) copied to the host"""
        n = int(self._dev["cmd_len"][i].item())
        return self._dev["cmd"][i, :n].cpu().numpy()


    flown_rows = fleet_flight.flown_rows      # with a flight model: the flown rows of mission i (flown_len, 3, 2), on the host


def draw_missions(maps, per_map, seed=0, dist_range=(25.0, 30.0), safe_dis=0.7):
    """`per_map` missions on each of the 2-D maps (ESDF objects with their host arrays): a start near the middle of the
    map's low-x edge and goals `dist_range` metres from it, inside the map, start and goal cells at least `safe_dis` from
    the nearest obstacle.  Returns start (B, 2), goals (B, 2), scene_ids (B,) -- the experiment of the reference's
    bash scripts (one start, goals tens of metres away) for a fleet."""
    rng = np.random.default_rng([int(seed), 0xF1EE7])
    starts, goals, sids = [], [], []
    for m in maps:
        res, ox, oy = float(m.map_resolution), float(m.map_origin.x), float(m.map_origin.y)
        H, W = m.esdf_map.shape

        def clear(p):
            row, col = ((p[:, 1] - oy) / res).astype(int), ((p[:, 0] - ox) / res).astype(int)
            inside = (p[:, 0] >= ox) & (p[:, 1] >= oy) & (row < H) & (col < W)
            return inside & (m.esdf_map[np.clip(row, 0, H - 1), np.clip(col, 0, W - 1)] >= safe_dis)

        cand = np.stack([np.full(41, ox + 0.5), oy + 0.5 * H * res + 0.25 * ((np.arange(41) + 1) // 2) * (-1.0) ** np.arange(41)], 1)
        ok = np.flatnonzero(clear(cand))
        if ok.size == 0:
            raise ValueError("draw_missions: no free start on a map")
        start = cand[ok[0]]
        got = np.zeros((0, 2))
        while got.shape[0] < per_map:
            r = rng.uniform(dist_range[0], dist_range[1], 4 * per_map)
            th = rng.uniform(-0.5 * np.pi, 0.5 * np.pi, 4 * per_map)
            g = start + r[:, None] * np.stack([np.cos(th), np.sin(th)], 1)
            got = np.concatenate([got, g[clear(g)]])
        starts.append(np.broadcast_to(start, (per_map, 2)))
        goals.append(got[:per_map])
        sids.append(np.full(per_map, m.scene_id, np.int32))
    return np.concatenate(starts), np.concatenate(goals), np.concatenate(sids)
