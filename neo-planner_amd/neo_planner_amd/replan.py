"""
ROS-free replan loop: the orchestration that sits directly above the optimiser in
ros_node/traj_planner_node.py, with perfect tracking in place of PX4/Gazebo -- or, with flight=FlightModel
(flight_model.py), a drone that tracks its commands with lag and gusts: set_local_target and the returned path then read
the drone's actual state, as the reference reads its odometry (:452, :183, :333-363), and only the planning start state
still comes from the command array (:527-537).

  set_local_target          traj_planner_node.py:450-488   5 m ahead toward the goal, lateral steps out
                                                           of obstacles, target speed 0.8 v_max
  get_drone_state_ahead     :527-537                       state `planning_time_ahead` s ahead on the
                                                           current command array
  try_local_planning/replan :421-448, :539-578             <= 11 re-targeted attempts, splice the new
                                                           command array at the look-ahead index
  first_plan                :490-525
  mode "warmstart"          :493, :570-571, :597-611       the first plan is basic; every replan is
                                                           warm_start_plan from the previous plan's waypoints,
                                                           carried along relative to the planning start state,
                                                           and the durations the planner last held

`TrackerLoop` is the same orchestration as ros_node/tracker_planner_node.py runs it: a goal that keeps moving along a
route (goal_routes.GoalRoutes), no landing, failed ticks flown through, the last command held.

Works with any planner object that has the reference's interface (`plan`, `batch_plan`,
`get_full_state_cmd`, `int_wpts`, `ts`, `iter_num`): neo_planner_amd.MinJerkPlanner on the GPU, or the
CPU oracle in tests.  This is BASELINE.json configs[0] (one trajectory at a time, goal (30, 0)).
"""
import contextlib
import io

import numpy as np

from . import flight_model


class _State:
    def __init__(self, pos, vel):
        self.global_pos = np.asarray(pos, dtype=np.float64)
        self.global_vel = np.asarray(vel, dtype=np.float64)


class ReplanLoop:
    def __init__(self, planner, map, goal=(30.0, 0.0), v_max=1.0, des_pos_z=2.0, cmd_hz=60,
                 replan_period=1.0, planning_time_ahead=1.0, longitu_step_dis=5.0, lateral_step_length=1.0,
                 target_reach_threshold=0.2, mode="basic", quiet=True, flight=None, settle_seconds=2.0, mission_id=0):
        self.planner, self.map = planner, map
        self.global_target = np.asarray(goal, dtype=np.float64)
        self.move_vel = 0.8 * v_max                               # :87
        self.des_pos_z, self.cmd_hz = des_pos_z, cmd_hz
        self.replan_period, self.planning_time_ahead = replan_period, planning_time_ahead
        self.longitu_step_dis, self.lateral_step_length = longitu_step_dis, lateral_step_length
        self.target_reach_threshold = target_reach_threshold
        self.mode, self.quiet = mode, quiet
        self.near_global_target = False
        self.des_state_index = 0
        self.n_plans = self.n_failed_attempts = 0
        self.wpts_local = None      # mode "warmstart": the last plan's waypoints relative to where it started (count, 2)
        # flight: a flight_model.FlightModel, or None for perfect tracking; mission_id keys its gust stream
        self.flight, self.settle_seconds, self.mission_id = flight, settle_seconds, mission_id

    # ---- :450-488
    def set_local_target(self, current_pos, seed=0):
        self.target_state = np.zeros((2, 2))
        goal = self.global_target
        if np.linalg.norm(goal - current_pos) < self.longitu_step_dis:
            self.target_state[0] = goal
            self.near_global_target = True
            return
        ahead = (goal - current_pos) / np.linalg.norm(goal - current_pos)
        side = np.array([[ahead[1], -ahead[0]], [-ahead[1], ahead[0]]])
        which, shift = 0, self.lateral_step_length
        if seed > 1e-3:
            p = current_pos + self.longitu_step_dis * ahead + np.random.normal(0, 1, 2)
        else:
            p = current_pos + self.longitu_step_dis * ahead
        while self.map.has_collision(p):
            p = p + shift * side[which]
            which = 1 - which
            shift += self.lateral_step_length
        to_goal = (goal - p) / np.linalg.norm(goal - p)
        self.target_state = np.array([p, self.move_vel * to_goal])

    def _call_planner(self, start):
        start_2d = np.array([start.global_pos[:2], start.global_vel[:2]])
        sink = io.StringIO() if self.quiet else None
        with (contextlib.redirect_stdout(sink) if sink else contextlib.nullcontext()):
            if self.mode == "batch":
                self.planner.batch_plan(self.map, start_2d, self.target_state)
            elif self.mode == "geo":      # :548-549: A* warm start from the look-ahead state (a GeoPlanner)
                self.planner.geo_traj_plan(self.map, start, self.target_state)
            elif self.mode == "warmstart" and self.wpts_local is not None:      # :597-611: from the previous plan
                self.planner.warm_start_plan(self.map, start_2d, self.target_state,
                                             (self.wpts_local + start.global_pos[:2]).T, self.planner.ts)
            else:      # (warmstart: the first plan, and its re-targeted repeats, are basic plans, :493)
                self.planner.plan(self.map, start_2d, self.target_state)
        if self.mode == "warmstart":      # :570-571, only reached without an exception
            self.wpts_local = self.planner.int_wpts.T - start.global_pos[:2]
        self.n_plans += 1

    def _plan_with_retargeting(self, start_fn, current_pos):
        """:399-448: up to 11 targets (the first deterministic, the rest randomly shifted)"""
        seed = 0
        self.set_local_target(current_pos, seed)
        while True:
            try:
                self._call_planner(start_fn())
                return True
            except Exception:
                self.n_failed_attempts += 1
                seed += 1
                self.set_local_target(current_pos, seed)
                if seed > 10:
                    return False

    # ---- :527-537
    def get_drone_state_ahead(self):
        self.future_index = min(int(self.planning_time_ahead * self.cmd_hz) + self.des_state_index,
                                self.des_state_array.shape[0] - 1)
        return _State(np.append(self.des_state_array[self.future_index, 0, :], self.des_pos_z),
                      np.append(self.des_state_array[self.future_index, 1, :], 0.0))

    def run(self, start_pos=(0.0, 0.0), start_vel=(0.0, 0.0), max_replans=60):
        """fly to the goal; returns a dict of what the reference's metrics file records (:288-308).  With a flight model
        `path` is the flown positions (the whole array flown out, a landed mission's settle rows behind it), `commands` the
        command array, fly_* the tracking-error record, its sample count and flags and the saturation count, `landed`
        whether the plan near the goal was made and n_flown_planned the rows flown when planning stopped"""
        if self.flight is not None:
            return self._run_flown(start_pos, start_vel, max_replans)
        drone = _State(np.append(np.asarray(start_pos, float), self.des_pos_z), np.append(np.asarray(start_vel, float), 0.0))
        if not self._plan_with_retargeting(lambda: drone, drone.global_pos[:2]):      # first_plan :490-525
            return dict(success=False, replans=self.n_plans, path=np.zeros((0, 2)))
        self.des_state_array = self.planner.get_full_state_cmd(self.cmd_hz)
        self.des_state_index = 0
        step = int(round(self.replan_period * self.cmd_hz))
        ok = True
        for _ in range(max_replans):
            if self.near_global_target:
                break
            # perfect tracking: one replan period later the drone is `step` commands further
            self.des_state_index = min(self.des_state_index + step, self.des_state_array.shape[0] - 1)
            cur = self.des_state_array[self.des_state_index, 0, :]
            ok = self._plan_with_retargeting(self.get_drone_state_ahead, cur)
            if not ok:
                break
            new = self.planner.get_full_state_cmd(self.cmd_hz)
            self.des_state_array = np.concatenate((self.des_state_array[:self.future_index], new), axis=0)   # :577
        path = self.des_state_array[:, 0, :]
        reached = ok and np.linalg.norm(path[-1] - self.global_target) < self.target_reach_threshold
        dists = np.array([self.map.get_edt_dis(p) for p in path[::6]])
        return dict(success=bool(reached), replans=self.n_plans, failed_attempts=self.n_failed_attempts,
                    iter_num=self.planner.iter_num, opt_runs=self.planner.opt_running_times, path=path,
                    min_clearance=float(dists.min()), duration=path.shape[0] / self.cmd_hz,
                    max_speed=float(np.linalg.norm(self.des_state_array[:, 1, :], axis=1).max()))


    def _run_flown(self, start_pos, start_vel, max_replans):
        """`run` with a drone that lags: the same orchestration, the drone's position read from the flight"""
        drone = _State(np.append(np.asarray(start_pos, float), self.des_pos_z), np.append(np.asarray(start_vel, float), 0.0))
        if not self._plan_with_retargeting(lambda: drone, drone.global_pos[:2]):      # first_plan :490-525
            return dict(success=False, replans=self.n_plans, path=np.zeros((0, 2)))
        self.des_state_array = self.planner.get_full_state_cmd(self.cmd_hz)
        self.des_state_index = 0
        fl = flight_model.Flight(self.flight, self.cmd_hz, start_pos, start_vel, self.mission_id)
        step = int(round(self.replan_period * self.cmd_hz))
        ok = True
        for _ in range(max_replans):
            if self.near_global_target:
                break
            self.des_state_index = min(self.des_state_index + step, self.des_state_array.shape[0] - 1)
            fl.advance(self.des_state_array, self.des_state_index)
            ok = self._plan_with_retargeting(self.get_drone_state_ahead, fl.pos)      # :452: where the drone IS
            if not ok:
                break
            new = self.planner.get_full_state_cmd(self.cmd_hz)
            self.des_state_array = np.concatenate((self.des_state_array[:self.future_index], new), axis=0)   # :577
        planned = fl.n      # rows flown when planning stopped
        landed = bool(ok and self.near_global_target)
        fl.advance(self.des_state_array, self.des_state_array.shape[0] - 1)
        if landed:
            fl.settle(self.des_state_array, self.global_target, int(round(self.settle_seconds * self.cmd_hz)),
                      self.target_reach_threshold)
        out = fl.result(self.des_state_array, int(round(self.cmd_hz * 0.1)))
        path = out["flown"][:, 0, :]
        reached = ok and np.linalg.norm(path[-1] - self.global_target) < self.target_reach_threshold
        dists = np.array([self.map.get_edt_dis(p) for p in path[::6]])
        out.update(success=bool(reached), replans=self.n_plans, failed_attempts=self.n_failed_attempts,
                   iter_num=self.planner.iter_num, opt_runs=self.planner.opt_running_times, path=path,
                   commands=self.des_state_array, landed=landed, n_flown_planned=planned, min_clearance=float(dists.min()), duration=path.shape[0] / self.cmd_hz,
                   max_speed=float(np.linalg.norm(out["flown"][:, 1, :], axis=1).max()))
        return out


class TrackerLoop(ReplanLoop):
    """The loop of ros_node/tracker_planner_node.py (with tracker_manager_node.py) on any planner with the reference's
    interface: the goal keeps moving, and the mission chases it.

      global target        whatever the last message said when set_local_target runs (:160-162, :313-316): here the
                           mission's goal route (goal_routes.GoalRoutes) at the tick's time
      set_local_target     closer than longitu_step_dis the local target is the goal itself with zero velocity
                           (:319-321) -- and planning goes on: there is no near_global_target
      try_local_planning   a tick whose 11 targets all fail just returns (:265-279): the mission flies on along its old
                           commands, nothing is abandoned
      tracking             a drone that runs out of commands holds the last one (get_drone_state_ahead re-reads that
                           row, :387-391): the array is padded with copies of it, so row i is the command at i / cmd_hz

    Tick k is at time (k * step) / cmd_hz, step = round(replan_period * cmd_hz) commands."""

    def set_local_target(self, current_pos, seed=0):
        super().set_local_target(current_pos, seed)
        self.near_global_target = False      # (:319-321 return without a flag)

    def run_tracking(self, routes_of_one, ticks, start_pos=(0.0, 0.0), start_vel=(0.0, 0.0)):
        """the first plan at tick 0 and one replan at each of the `ticks` ticks after it, chasing the one route of
        `routes_of_one`.  Returns a dict: replans (plans made), failed_attempts, failed_ticks, iter_num, opt_runs,
        commands (n_cmd, 3, 2), n_flown (= ticks * step + 1 once there are commands), path (the flown positions) and
        goals (ticks + 1, 2), where the goal was at every tick."""
        if routes_of_one.B != 1:
            raise ValueError("TrackerLoop.run_tracking: one route")
        step = int(round(self.replan_period * self.cmd_hz))
        drone = _State(np.append(np.asarray(start_pos, float), self.des_pos_z), np.append(np.asarray(start_vel, float), 0.0))
        self.des_state_array = np.zeros((0, 3, 2))
        self.des_state_index = 0
        failed_ticks = 0
        goals = np.zeros((ticks + 1, 2))
        fl = None if self.flight is None else flight_model.Flight(self.flight, self.cmd_hz, start_pos, start_vel, self.mission_id)
        for k in range(ticks + 1):
            self.global_target = goals[k] = routes_of_one.at((k * step) / self.cmd_hz)[0]
            have = self.des_state_array.shape[0]
            if k > 0 and have >= 1:
                need = self.des_state_index + step + 1
                if have < need:      # out of commands before the period is over: hold the last one
                    self.des_state_array = np.concatenate((self.des_state_array, np.repeat(self.des_state_array[-1:], need - have, axis=0)))
                self.des_state_index += step
                if fl is not None:
                    fl.advance(self.des_state_array, self.des_state_index)
            if self.des_state_array.shape[0] >= 1:
                cur, start_fn = self.des_state_array[self.des_state_index, 0, :], self.get_drone_state_ahead
                if fl is not None:
                    cur = fl.pos
            else:      # nothing planned yet: the first plan, from where the drone stands
                cur, start_fn, self.future_index = drone.global_pos[:2], (lambda: drone), 0
            if not self._plan_with_retargeting(start_fn, cur):
                failed_ticks += 1
                continue
            new = self.planner.get_full_state_cmd(self.cmd_hz)
            self.des_state_array = np.concatenate((self.des_state_array[:self.future_index], new), axis=0)   # :430
        n_flown = min(self.des_state_index + 1, self.des_state_array.shape[0])
        if fl is not None:      # the flown rows stand in for the command rows; the commands stay next to them
            out = fl.result(self.des_state_array, int(round(self.cmd_hz * 0.1)))
            out.update(replans=self.n_plans, failed_attempts=self.n_failed_attempts, failed_ticks=failed_ticks,
                       iter_num=self.planner.iter_num, opt_runs=self.planner.opt_running_times, commands=self.des_state_array,
                       n_flown=n_flown, path=out["flown"][:n_flown, 0, :], goals=goals)
            return out
        return dict(replans=self.n_plans, failed_attempts=self.n_failed_attempts, failed_ticks=failed_ticks,
                    iter_num=self.planner.iter_num, opt_runs=self.planner.opt_running_times,
                    commands=self.des_state_array, n_flown=n_flown, path=self.des_state_array[:n_flown, 0, :], goals=goals)
