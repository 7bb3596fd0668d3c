// neo_fleet.hpp -- the glue of a fleet of closed-loop missions (include/neo_planner.h, neo_fleet_*): what
// ros_node/traj_planner_node.py does per mission between two plans, for B missions whose command arrays stay in HBM.
//
//   fleet_target_kernel    set_local_target       (:450-488)   one lane per mission
//   fleet_jitter_kernel    the re-targeting's N(0, 1) draws (:469) on the device (neo_counter_rng.hpp)   one lane per mission
//   fleet_advance_kernel   perfect tracking + get_drone_state_ahead (:527-537)   one lane per mission
//   fleet_pose_kernel      the camera pose a mission senses from (:685-687)          one lane per mission
//   fleet_warm_guess_kernel  the previous plan as the next one's first guess (:597-611)   one lane per mission
//   fleet_warm_carry_kernel  what a mission keeps of a plan for that (:570-571)           one lane per mission
//   fleet_splice_kernel    the splice of replan   (:574-578, first_plan :515-519)   one wavefront per mission
//   fleet_audit_kernel     get_weighted_metric    (:333-363) over the flown rows   one wavefront per mission
// and, in neo_flight.hpp (which includes this file), the drone that is not on its command row:
//   fleet_fly_kernel       the advance with a flight model: lag, saturation, drag, gusts   one lane per mission
//   fleet_fly_error_kernel save_tracking_err (:310-331) reduced per mission             one wavefront per mission
//
// Included by neo_disp_fleet.hip only; the solve of the splice is the piece table's (neo_pieces.hpp, through neo_audit.hpp):
// nothing of the optimiser is included.  2-D reference map, D = 2, fp64.  No floating-point atomics, fixed summation
// order: a mission's results depend on neither the batch, the subset nor the launch.  All arrays are indexed by mission;
// workgroup / lane i works on the mission at position i of the launch list (neo_launch_list.hpp).  A mission is owned
// by one lane (target, advance) or one wavefront (splice, audit) of a launch, so its flags word is updated with a plain
// read-modify-write.
#pragma once
#include "neo_audit.hpp"
#include "neo_counter_rng.hpp"
#include "neo_launch_list.hpp"

namespace neo {

constexpr int kFleetThreads = 256;  // target / advance: missions per workgroup
constexpr int kFleetD = 2;
constexpr int kFleetRow = 3 * kFleetD;  // doubles of a command row: position, velocity, acceleration
// most lateral steps the target walk is ever given, whatever the map and the step (see fleet_walk_bound)
constexpr int kFleetWalkMax = 1 << 20;

// Bound of set_local_target's lateral walk (the reference's `while self.map.has_collision(...)` has none).  After k
// steps the candidate sits at p_0 + (-1)^(k+1) ceil(k / 2) s along the first lateral direction (steps of s, 2 s, 3 s, ...
// with alternating sign), s = lateral_step_length.  has_collision is only true INSIDE the map (outside the lookup
// answers 10000), so a walk that is still going has p_0 and p_k inside: ceil(k / 2) s = |p_k - p_0| <= L, the map's
// diagonal extent, i.e. k <= 2 L / s.  The candidate after floor(2 L / s) + 1 steps is therefore outside or free, and
// ceil(2 L / s) + 2 steps are never all taken; NEO_FLEET_FLAG_TARGET_CAPPED marks the walk that did (rounding of the
// bound itself at worst), or that ran into kFleetWalkMax with a tiny s.
__device__ __forceinline__ int fleet_walk_bound(const Map2D &m, double s) {
  const double ex = (double)m.W * m.res, ey = (double)m.H * m.res;
  const double k = ceil(2.0 * sqrt(ex * ex + ey * ey) / s) + 2.0;
  return k < (double)kFleetWalkMax ? (int)k : kFleetWalkMax;  // (a NaN bound compares false: the hard cap)
}

__global__ __launch_bounds__(kFleetThreads) void fleet_target_kernel(
    LaunchList list, const Map2D *__restrict__ maps, const int *__restrict__ scene_slot, int nmaps,
    const double *__restrict__ cur_pos, const double *__restrict__ goal, const double *__restrict__ jitter,
    double longitu, double lateral, double move_vel, double *__restrict__ tail, int *__restrict__ near_goal,
    int *__restrict__ lateral_steps, int *__restrict__ flags) {
#pragma clang fp contract(off)  // every operation rounded on its own, as the reference's NumPy expressions are
  const int b = list.request(blockIdx.x * kFleetThreads + threadIdx.x);
  if (b < 0) return;
  double *tl = tail + (size_t)b * kFleetRow;
  tl[4] = tl[5] = 0.0;  // the target's acceleration row
  const int slot = scene_slot ? scene_slot[b] : 0;
  if (slot < 0 || slot >= nmaps) {
    tl[0] = tl[1] = tl[2] = tl[3] = __builtin_nan("");
    near_goal[b] = 0;
    lateral_steps[b] = 0;
    flags[b] |= NEO_FLEET_FLAG_BAD_SCENE;
    return;
  }
  const Map2D map = maps[slot];
  const double cx = cur_pos[(size_t)b * 2], cy = cur_pos[(size_t)b * 2 + 1];
  const double gx = goal[(size_t)b * 2], gy = goal[(size_t)b * 2 + 1];
  const double dx = gx - cx, dy = gy - cy;
  const double dist = sqrt(dx * dx + dy * dy);
  if (dist < longitu) {  // :456-459
    tl[0] = gx;
    tl[1] = gy;
    tl[2] = tl[3] = 0.0;
    near_goal[b] = 1;
    lateral_steps[b] = 0;
    return;
  }
  const double ax = dx / dist, ay = dy / dist;  // :461
  // lateral_dir = [[ay, -ax], [-ay, ax]] (:462-463)
  double p[2] = {cx + longitu * ax + jitter[(size_t)b * 2], cy + longitu * ay + jitter[(size_t)b * 2 + 1]};  // :469-472
  const Lookup2D<double> lk(map);
  const int bound = fleet_walk_bound(map, lateral);
  int steps = 0, capped = 0;
  double shift = lateral, sign = 1.0;
  for (;;) {  // :474-477
    double g[2];
    bool inside;
    const double d = lk.fetch<2>(p, g, inside);
    if (!(d < 0.5)) break;  // has_collision (map_server/esdf.py:50-51)
    if (steps >= bound) {
      capped = 1;
      break;
    }
    p[0] = p[0] + shift * (sign * ay);
    p[1] = p[1] + shift * (-(sign * ax));
    sign = -sign;
    shift = shift + lateral;
    ++steps;
  }
  const double tx = gx - p[0], ty = gy - p[1];
  const double tn = sqrt(tx * tx + ty * ty);  // 0 for a target on the goal: 0 / 0 = NaN, as in the reference (:480)
  tl[0] = p[0];
  tl[1] = p[1];
  tl[2] = move_vel * (tx / tn);
  tl[3] = move_vel * (ty / tn);
  near_goal[b] = 0;
  lateral_steps[b] = steps;
  if (capped) flags[b] |= NEO_FLEET_FLAG_TARGET_CAPPED;
}

// jitter[b][0 .. 1] = values 0 and 1 (one block) of the stream (seed, mission_ids[b], tick, target, domain 2):
// fleet.target_jitter_counter's rows, bit for bit; zeros, without drawing, for the first target of a tick.
// `mission_ids` is mission-indexed, or NULL: the mission's index.
__global__ __launch_bounds__(kFleetThreads) void fleet_jitter_kernel(LaunchList list, unsigned long long seed, int tick,
                                                                     int target, const int *__restrict__ mission_ids,
                                                                     double *__restrict__ jitter) {
  const int b = list.request(blockIdx.x * kFleetThreads + threadIdx.x);
  if (b < 0) return;
  double z0 = 0.0, z1 = 0.0;
  if (target != 0) {
    const uint32_t id = (uint32_t)(mission_ids ? mission_ids[b] : b);
    const Philox4 o = counter_stream_block(seed, id, (uint32_t)tick, (uint32_t)target, kRngDomainTarget, 0u);
    z0 = counter_block_normal(o, 0);
    z1 = counter_block_normal(o, 1);
  }
  jitter[(size_t)b * 2] = z0;
  jitter[(size_t)b * 2 + 1] = z1;
}

// The camera pose a mission senses from (onboard maps): the eye is where the mission is, at height eye_z; the heading is
// the unit vector of the last step of its command array, row cmd_index minus the row before it -- :685-687 without the
// arctan2 round trip -- or, where there is no such step or it has no length, of the way to the goal; (1, 0) on the goal.
// Squares, one sum, sqrt and divisions, each rounded on its own: NumPy reproduces the bits.
__device__ __forceinline__ bool fleet_unit(double dx, double dy, double &c, double &s) {
#pragma clang fp contract(off)
  const double xx = dx * dx, yy = dy * dy;
  const double n = sqrt(xx + yy);
  if (!(n > 0.0 && n < __builtin_inf())) return false;
  c = dx / n;
  s = dy / n;
  return true;
}

__global__ __launch_bounds__(kFleetThreads) void fleet_pose_kernel(
    LaunchList list, const double *__restrict__ cmd, int cap, const int *__restrict__ cmd_len,
    const int *__restrict__ cmd_index, const double *__restrict__ cur_pos,
    const double *__restrict__ goal, double eye_z, double *__restrict__ pose) {
#pragma clang fp contract(off)
  const int b = list.request(blockIdx.x * kFleetThreads + threadIdx.x);
  if (b < 0) return;
  const double px = cur_pos[(size_t)b * 2], py = cur_pos[(size_t)b * 2 + 1];
  int len = cmd_len[b];
  len = len > cap ? cap : len;
  const int k = cmd_index[b];
  double c = 1.0, s = 0.0;
  bool have = false;
  if (k >= 1 && k < len) {
    const double *r1 = cmd + ((size_t)b * cap + k) * kFleetRow, *r0 = r1 - kFleetRow;
    have = fleet_unit(r1[0] - r0[0], r1[1] - r0[1], c, s);
  }
  if (!have) have = fleet_unit(goal[(size_t)b * 2] - px, goal[(size_t)b * 2 + 1] - py, c, s);
  if (!have) c = 1.0, s = 0.0;
  double *o = pose + (size_t)b * 5;
  o[0] = px;
  o[1] = py;
  o[2] = eye_z;
  o[3] = c;
  o[4] = s;
}

__global__ __launch_bounds__(kFleetThreads) void fleet_advance_kernel(
    LaunchList list, const double *__restrict__ cmd, int cap, const int *__restrict__ cmd_len,
    int *__restrict__ cmd_index, int *__restrict__ future_index, int step, int ahead, double *__restrict__ cur_pos,
    double *__restrict__ head) {
  const int b = list.request(blockIdx.x * kFleetThreads + threadIdx.x);
  if (b < 0) return;
  int len = cmd_len[b];
  len = len > cap ? cap : len;
  if (len < 1) return;  // nothing planned yet: nothing to fly along
  const int last = len - 1;
  // (sums of non-negative ints below 2^30 each, checked by the caller's wrapper: no overflow)
  int idx = cmd_index[b];
  idx = idx < 0 ? 0 : idx;
  idx = idx > last - step ? last : idx + step;  // min(idx + step, len - 1)
  const int fut = idx > last - ahead ? last : idx + ahead;  // :531-532
  cmd_index[b] = idx;
  future_index[b] = fut;
  const double *row = cmd + ((size_t)b * cap + idx) * kFleetRow;
  cur_pos[(size_t)b * 2] = row[0];
  cur_pos[(size_t)b * 2 + 1] = row[1];
  const double *fr = cmd + ((size_t)b * cap + fut) * kFleetRow;
  double *hd = head + (size_t)b * kFleetRow;
  hd[0] = fr[0];
  hd[1] = fr[1];
  hd[2] = fr[2];
  hd[3] = fr[3];
  hd[4] = hd[5] = 0.0;  // the reference hands plan() a 2 x 2 state (:534-535)
}

// ---- mode "warmstart": what a mission carries from one plan to the next (:570-571, :597-611).  Per mission
// wpts_local[2][M - 1], the last solved plan's waypoints minus the position that plan started from, and ts_carry[M], the
// durations the planner last held.  A mission's x row is [x_0 .. x_{M-2}, y_0 .. y_{M-2}, tau_0 .. tau_{M-1}].
// Differences, sums and quotients only, each rounded on its own: no product meets a sum, so nothing here can contract.
struct WarmInitTs {  // the re-seeded attempts' start durations init_T * [1.5, 1, ..., 1, 1.5], handed over by value
  double v[NEO_MAX_PIECES];
};

// x0[b] = the carried plan seen from head[b]'s position, and map_T2tau (:468-475) of the carried durations.  Where the
// reference's map_T2tau raises (t - T_min not > 0, the log's argument not > 0) or the duration is NaN, tau is NaN: the
// optimiser ends that attempt NEO_TRAJ_NONFINITE at its first evaluation and the plan chain re-seeds it.
__global__ __launch_bounds__(kFleetThreads) void fleet_warm_guess_kernel(
    LaunchList list, int M, double T_min, double T_max, const double *__restrict__ head,
    const double *__restrict__ wpts_local, const double *__restrict__ ts_carry, double *__restrict__ x0) {
#pragma clang fp contract(off)
  const int b = list.request(blockIdx.x * kFleetThreads + threadIdx.x);
  if (b < 0) return;
  const int count = M - 1;
  const double *hd = head + (size_t)b * kFleetRow;
  const double *wl = wpts_local + (size_t)b * kFleetD * count;
  const double *tc = ts_carry + (size_t)b * M;
  double *x = x0 + (size_t)b * (kFleetD * count + M);
  const double px = hd[0], py = hd[1];
  for (int k = 0; k < count; ++k) {
    x[k] = wl[k] + px;
    x[count + k] = wl[count + k] + py;
  }
  const double span = T_max - T_min;
  double *tau = x + kFleetD * count;
  for (int k = 0; k < M; ++k) {
    const double dt = tc[k] - T_min;
    const double arg = span / dt - 1.0;
    tau[k] = (dt > 0.0 && arg > 0.0) ? -log(arg) : __builtin_nan("");  // (a NaN duration compares false)
  }
}

// After a target round's plan call.  Solved: both carries from the plan x[b].  Not solved: the waypoints stay (the
// reference raises before :570); the durations are map_tau2T (:477-483) of the last attempt's answer when it ran to one
// ((status & 0xff) <= NEO_TRAJ_MAXITER: the collision was too large), and that attempt's START durations when it
// raised instead -- init_ts for a re-seeded attempt (attempts > 1), what they were for the first.
__global__ __launch_bounds__(kFleetThreads) void fleet_warm_carry_kernel(
    LaunchList list, int M, double T_min, double T_max, const double *__restrict__ x, const double *__restrict__ head,
    const int *__restrict__ solved, const int *__restrict__ status, const int *__restrict__ attempts, WarmInitTs init_ts,
    double *__restrict__ wpts_local, double *__restrict__ ts_carry) {
#pragma clang fp contract(off)
  const int b = list.request(blockIdx.x * kFleetThreads + threadIdx.x);
  if (b < 0) return;
  const int count = M - 1;
  const double *xr = x + (size_t)b * (kFleetD * count + M);
  double *tc = ts_carry + (size_t)b * M;
  const bool ok = solved[b] != 0;
  if (ok) {
    const double *hd = head + (size_t)b * kFleetRow;
    double *wl = wpts_local + (size_t)b * kFleetD * count;
    const double px = hd[0], py = hd[1];
    for (int k = 0; k < count; ++k) {
      wl[k] = xr[k] - px;
      wl[count + k] = xr[count + k] - py;
    }
  }
  if (ok || (status[b] & 0xff) <= NEO_TRAJ_MAXITER) {
    const double span = T_max - T_min;
    const double *tau = xr + kFleetD * count;
    for (int k = 0; k < M; ++k) tc[k] = span / (1.0 + exp(-tau[k])) + T_min;
  } else if (attempts[b] > 1) {
    for (int k = 0; k < M; ++k) tc[k] = init_ts.v[k];
  }
}

// The solve and the rows are the piece table's (neo_pieces.hpp), as traj_state_kernel's: the same bits as its rows.
__global__ __launch_bounds__(kWave) void fleet_splice_kernel(
    LaunchList list, int M, DevParams prm, const double *__restrict__ x,
    const double *__restrict__ head, const double *__restrict__ tail, const int *__restrict__ solved, double hz, int first,
    double *__restrict__ cmd, int cap, int *__restrict__ cmd_len, int *__restrict__ cmd_index,
    int *__restrict__ future_index, int *__restrict__ flags) {
  constexpr int D = kFleetD;
  NEO_PIECE_LDS(D, lds);
  const int b = list.request(blockIdx.x);  // wave-uniform
  if (b < 0) return;
  if (solved && !solved[b]) return;
  const int lane = lane_id();
  // no trajectory to splice (exp(-tau) overflow, or below a duration that is not finite): the array stays as it is
  auto refuse = [&]() {
    if (lane == 0) flags[b] |= NEO_FLEET_FLAG_SPLICE_FAILED;
  };
  PieceTable<D> pt(lds, M);
  if (pt.solve(b, prm, x, head, tail) != 0) return refuse();
  const double step = 1.0 / hz;
  int cnt;
  if (!pt.sample_count(step, cnt)) return refuse();
  int at = first ? 0 : future_index[b];
  at = at < 0 ? 0 : (at > cap ? cap : at);
  const int room = cap - at;
  const int wr = cnt < room ? cnt : room;  // rows beyond the buffer are dropped
  double *out0 = cmd + ((size_t)b * cap + at) * kFleetRow;
  for (int k = lane; k < wr; k += kWave) {
    const double tt = pt.time_of(k, step);
    const int pc = pt.seek(0, tt);
    double pos[D], vel[D], acc[D];
    pt.state(pc, tt, pos, vel, acc);
    double *out = out0 + (size_t)k * kFleetRow;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      out[0 * D + d] = pos[d];
      out[1 * D + d] = vel[d];
      out[2 * D + d] = acc[d];
    }
  }
  if (lane == 0) {
    cmd_len[b] = at + wr;
    if (first) cmd_index[b] = future_index[b] = 0;
    if (cnt > room) flags[b] |= NEO_FLEET_FLAG_CMD_FULL;
  }
}

// audit_kernel's accumulation (neo_audit.hpp AuditAcc) over GIVEN rows: sample j is row j * stride of the mission's
// command array, j < count = ceil(n_flown / stride).  Per round a lane loads the rows of its kAuditU samples, then has
// their kAuditU map gathers in flight before the first is consumed.
__global__ __launch_bounds__(kWave) void fleet_audit_kernel(
    LaunchList list, DevParams prm, const Map2D *__restrict__ maps,
    const int *__restrict__ scene_slot, int nmaps, const double *__restrict__ cmd, int cap,
    const int *__restrict__ n_flown, int stride, double hz, double w0, double w1, double w2, double *__restrict__ audit,
    int *__restrict__ count, int *__restrict__ flags) {
#pragma clang fp contract(off)  // the metric's own arithmetic rounds every operation as the reference's NumPy does
  constexpr int D = kFleetD;
  const int b = list.request(blockIdx.x);  // wave-uniform
  if (b < 0) return;
  const int lane = lane_id();
  const int slot = scene_slot ? scene_slot[b] : 0;
  if (slot < 0 || slot >= nmaps) return audit_reject(b, audit, count, flags);
  const Map2D map = maps[slot];
  int nf = n_flown[b];
  nf = nf < 0 ? 0 : (nf > cap ? cap : nf);
  const int cnt = (nf + stride - 1) / stride;  // len(range(0, nf, stride)); (cnt - 1) * stride < cap: row indices fit
  const double *rows = cmd + (size_t)b * cap * kFleetRow;

  const Lookup2D<double> lk(map);
  const double vmax2 = prm.v_max * prm.v_max, safe = prm.safe_dis;
  AuditAcc<D> acc;
  for (int base = 0; base < cnt; base += kAuditU * kWave) {
    double st[kAuditU][kFleetRow];
    bool on[kAuditU];
#pragma unroll
    for (int u = 0; u < kAuditU; ++u) {
      const int k = base + u * kWave + lane;
      on[u] = k < cnt;
      const double *r = rows + (size_t)(on[u] ? k : 0) * stride * kFleetRow;  // idle slots read row 0 (cap >= 1)
#pragma unroll
      for (int q = 0; q < kFleetRow; ++q) st[u][q] = r[q];
    }
    Lookup2D<double>::Addr ad[kAuditU];
    Lookup2D<double>::Raw rw[kAuditU];
#pragma unroll
    for (int u = 0; u < kAuditU; ++u) {
      const double pos[D] = {st[u][0], st[u][1]};
      ad[u] = lk.prepare<D>(pos, on[u]);
    }
#pragma unroll
    for (int u = 0; u < kAuditU; ++u) rw[u] = lk.load(ad[u]);
#pragma unroll
    for (int u = 0; u < kAuditU; ++u) {
      const double pos[D] = {st[u][0], st[u][1]}, vel[D] = {st[u][2], st[u][3]}, ac[D] = {st[u][4], st[u][5]};
      double prev[D], gdrop[D];
      acc.neighbour(pos, prev);
      const double dk = lk.finish<D>(ad[u], rw[u], gdrop);
      if (on[u]) {
        acc.kinematics(pos, vel, ac, vmax2);
        acc.clearance(base + u * kWave + lane, pos, prev, dk, ad[u].inside, safe);
      }
    }
  }
  acc.finish(b, cnt, (double)nf / hz, [&](int k) { return (double)(k * stride) / hz; },  // the time of command row k * stride
             w0, w1, w2, prm.coll_tol, audit, count, flags);
}

}  // namespace neo
