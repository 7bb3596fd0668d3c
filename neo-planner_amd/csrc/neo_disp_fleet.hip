// neo_disp_fleet.hip -- the fleet kernels (neo_fleet.hpp; goal routes: neo_track.hpp; campaigns: neo_legs.hpp; the flight model: neo_flight.hpp): local targets, tracking and look-ahead, the splice of a new
// plan into the resident command array and the flight metric of what was flown (ros_node/traj_planner_node.py:333-363,
// :450-488, :527-537, :574-578) for B missions.  2-D reference map, D = 2: one instantiation each.
#include "neo_host.hpp"
#include "neo_fleet.hpp"
#include "neo_track.hpp"
#include "neo_legs.hpp"
#include "neo_flight.hpp"

namespace neo {

static dim3 lanes_grid(int n) { return dim3((n + kFleetThreads - 1) / kFleetThreads); }

int fleet_target(neo_ctx *c, const LaunchList &l, const MapRef &m, const FleetTargetArgs &a) {
  hipLaunchKernelGGL(fleet_target_kernel, lanes_grid(l.n), dim3(kFleetThreads), 0, c->stream, l,
                     static_cast<const Map2D *>(m.table), m.slots, m.nmaps, a.cur_pos, a.goal, a.jitter, a.longitu,
                     a.lateral, a.move_vel, a.tail, a.near_goal, a.lateral_steps, a.flags);
  return NEO_OK;
}

int fleet_jitter(neo_ctx *c, const LaunchList &l, uint64_t seed, int tick, int target, const int *mission_ids,
                 double *jitter) {
  hipLaunchKernelGGL(fleet_jitter_kernel, lanes_grid(l.n), dim3(kFleetThreads), 0, c->stream, l, (unsigned long long)seed,
                     tick, target, mission_ids, jitter);
  return NEO_OK;
}

int fleet_advance(neo_ctx *c, const LaunchList &l, const FleetCmd &m, int step, int ahead, double *cur_pos, double *head) {
  hipLaunchKernelGGL(fleet_advance_kernel, lanes_grid(l.n), dim3(kFleetThreads), 0, c->stream, l, m.cmd, m.cap, m.cmd_len,
                     m.cmd_index, m.future_index, step, ahead, cur_pos, head);
  return NEO_OK;
}

int fleet_pose(neo_ctx *c, const LaunchList &l, const FleetCmd &m, const double *cur_pos, const double *goal, double eye_z,
               double *pose) {
  hipLaunchKernelGGL(fleet_pose_kernel, lanes_grid(l.n), dim3(kFleetThreads), 0, c->stream, l, m.cmd, m.cap, m.cmd_len,
                     m.cmd_index, cur_pos, goal, eye_z, pose);
  return NEO_OK;
}

int fleet_warm_guess(neo_ctx *c, const LaunchList &l, int M, const double *head, const double *wpts_local,
                     const double *ts_carry, double *x0) {
  hipLaunchKernelGGL(fleet_warm_guess_kernel, lanes_grid(l.n), dim3(kFleetThreads), 0, c->stream, l, M, c->params.T_min,
                     c->params.T_max, head, wpts_local, ts_carry, x0);
  return NEO_OK;
}

int fleet_warm_carry(neo_ctx *c, const LaunchList &l, const FleetWarmCarryArgs &a) {
  WarmInitTs ts{};
  for (int k = 0; k < a.M; ++k) ts.v[k] = a.init_ts[k];
  hipLaunchKernelGGL(fleet_warm_carry_kernel, lanes_grid(l.n), dim3(kFleetThreads), 0, c->stream, l, a.M, c->params.T_min,
                     c->params.T_max, a.x, a.head, a.solved, a.status, a.attempts, ts, a.wpts_local, a.ts_carry);
  return NEO_OK;
}

int fleet_splice(neo_ctx *c, const LaunchList &l, const FleetCmd &m, const FleetSpliceArgs &a) {
  hipLaunchKernelGGL(fleet_splice_kernel, dim3(l.n), dim3(kWave), 0, c->stream, l, a.M, c->dev, a.x, a.head, a.tail,
                     a.solved, a.hz, a.first, m.cmd, m.cap, m.cmd_len, m.cmd_index, m.future_index, a.flags);
  return NEO_OK;
}

int fleet_audit(neo_ctx *c, const LaunchList &l, const MapRef &m, const FleetAuditArgs &a) {
  hipLaunchKernelGGL(fleet_audit_kernel, dim3(l.n), dim3(kWave), 0, c->stream, l, c->dev,
                     static_cast<const Map2D *>(m.table), m.slots, m.nmaps, a.cmd, a.cap, a.n_flown, a.stride, a.hz, a.w[0],
                     a.w[1], a.w[2], a.audit, a.count, a.flags);
  return NEO_OK;
}

int fleet_goal(neo_ctx *c, const LaunchList &l, const FleetRoutes &r, double t, double *goal) {
  hipLaunchKernelGGL(fleet_goal_kernel, lanes_grid(l.n), dim3(kFleetThreads), 0, c->stream, l, r.vertices, r.n_vertices,
                     r.route_begin, r.speed, r.closed, t, goal);
  return NEO_OK;
}

int fleet_hold(neo_ctx *c, const LaunchList &l, const FleetCmd &m, int step, int *flags) {
  hipLaunchKernelGGL(fleet_hold_kernel, dim3(l.n), dim3(kWave), 0, c->stream, l, m.cmd, m.cap, m.cmd_len, m.cmd_index, step,
                     flags);
  return NEO_OK;
}

int fleet_track_audit(neo_ctx *c, const LaunchList &l, const FleetRoutes &r, const FleetTrackArgs &a) {
  hipLaunchKernelGGL(fleet_track_audit_kernel, dim3(l.n), dim3(kWave), 0, c->stream, l, a.cmd, a.cap, a.n_flown, a.stride,
                     a.hz, r.vertices, r.n_vertices, r.route_begin, r.speed, r.closed, a.radius, a.track, a.count, a.flags);
  return NEO_OK;
}

int fleet_fly(neo_ctx *c, const LaunchList &l, const neo_flight_model &model, const FleetCmd &m, const FleetFlyArgs &a) {
  const FlightParams fp = {model.h, model.kp, model.kv, model.a_max, model.alpha, model.drag, model.rho, model.scale,
                           model.gust_every, (unsigned long long)model.seed};
  const FlightLaunch fl = {m.cap, a.step, a.ahead, a.first, a.settle, a.reach};
  hipLaunchKernelGGL(fleet_fly_kernel, lanes_grid(l.n), dim3(kFleetThreads), 0, c->stream, l, fp, fl, m.cmd, m.cmd_len,
                     m.cmd_index, m.future_index, a.mission_ids, a.goal, a.drone, a.flown, a.flown_len, a.saturated, a.flags,
                     a.cur_pos, a.head);
  return NEO_OK;
}

int fleet_fly_error(neo_ctx *c, const LaunchList &l, const FleetFlyErrorArgs &a) {
  hipLaunchKernelGGL(fleet_fly_error_kernel, dim3(l.n), dim3(kWave), 0, c->stream, l, a.flown, a.cmd, a.cap, a.flown_len,
                     a.cmd_len, a.stride, a.fly, a.count, a.flags);
  return NEO_OK;
}

static LegSequences leg_sequences(const neo_leg_sequences &s) {
  return {s.kind, s.legs, s.goals, s.n_goals, s.seq_begin, (unsigned long long)s.seed, s.mission_ids,
          {s.x_pair[0], s.x_pair[1]}, s.y_scale, s.y_shift};
}

int fleet_leg_close(neo_ctx *c, const LaunchList &l, const FleetLegCloseArgs &a) {
  hipLaunchKernelGGL(fleet_leg_close_kernel, lanes_grid(l.n), dim3(kFleetThreads), 0, c->stream, l, a.outcome, a.cmd, a.cap,
                     a.cmd_len, a.cmd_index, a.head, a.goal, a.n_flown, a.leg_end, a.final_dist);
  return NEO_OK;
}

int fleet_leg_open(neo_ctx *c, const LaunchList &l, const neo_leg_sequences &seq, const FleetLegOpenArgs &a) {
  hipLaunchKernelGGL(fleet_leg_open_kernel, lanes_grid(l.n), dim3(kFleetThreads), 0, c->stream, l, leg_sequences(seq), a);
  return NEO_OK;
}

int fleet_leg_goal(neo_ctx *c, const neo_leg_sequences &seq, int B, int n, const int *mission, const int *leg_of,
                   double *goal, int *exists) {
  hipLaunchKernelGGL(fleet_leg_goal_kernel, lanes_grid(n), dim3(kFleetThreads), 0, c->stream, leg_sequences(seq), B, n,
                     mission, leg_of, goal, exists);
  return NEO_OK;
}

}  // namespace neo
