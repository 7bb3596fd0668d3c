// neo_legs.hpp -- fleet campaigns: a mission flies goal after goal (ros_node/manager_node.py:153-193 sends the next goal
// as soon as one is reached or given up; every goal starts with execute_mission -> init_mission -> try_first_plan from the
// drone's state at that moment, traj_planner_node.py:187-245, :400-419, :490-525, and ends with one line of metrics,
// report_metrics :271-308).  Each goal is a LEG.
//
// The first part is the goal model, plain C++ as well as HIP (it includes neo_counter_rng.hpp and nothing else; the
// harness tests/host_harness/legs_host.cpp compiles it with the host compiler).  B missions' goal lists, of two kinds:
//
//   table   goals[n_goals][2] and seq_begin[B + 1], laid out as the route table is: mission b's goals are
//           goals[seq_begin[b] .. seq_begin[b + 1]), 1 to kLegsMax of them
//   flap    the reference's set_random_goal (`random` mission mode, how it gathers its training data): `legs` goals a
//           mission, goal k = (x_pair[k & 1], y_scale * (u - y_shift)), u the 52-bit uniform of neo_counter_rng.hpp
//           from domain 3 with the counter (mission id, k, 0, 3 << 24), value 0.  (The reference draws from NumPy's
//           unseeded global stream; a counter stream makes a campaign reproducible and independent of the fleet.)
//
// neo_planner_amd/goal_sequences.py is the NumPy model of this part: the same operations in the same order, every one
// rounded on its own (contraction is off in every function here).  Header and model agree bit for bit.
//
// The second part (HIP only) holds the kernels, launched from neo_disp_fleet.hip, one lane per mission:
//
//   fleet_leg_close_kernel   what a leg was: n_flown, where it ended, how far from its goal
//   fleet_leg_open_kernel    the leg's row of the log, then the next leg's goal and start state
//   fleet_leg_goal_kernel    the goal model alone, for (mission, leg) pairs
//
// Between close and open the caller runs neo_fleet_audit_batch_dev on the same subset with close's n_flown: a leg's rows
// start at row 0 of the mission's command array.  All arrays are indexed by mission, fp64; a mission's results depend on
// neither the batch, the subset nor the launch.
//
// The kernels of neo_fleet.hpp already do the right thing on a freshly opened leg (cmd_len = cmd_index = future_index
// = 0), and tests/test_gpu_legs.py holds them to it:
//   fleet_advance_kernel   leaves a mission with cmd_len < 1 untouched: the opened head and cur_pos survive the advance
//                          of the next tick;
//   fleet_splice_kernel    with first = 0 splices at future_index = 0 and leaves cmd_index = 0 as it is;
//   fleet_pose_kernel      looks from cur_pos towards the goal when cmd_index < 1.
#pragma once
#include "neo_counter_rng.hpp"

#if defined(__HIPCC__)
#define NEO_LEG_HD __host__ __device__ __forceinline__
#else
#define NEO_LEG_HD inline
#endif

namespace neo {

constexpr int kLegsMax = 64;           // NEO_FLEET_LEGS_MAX: goals of a mission
constexpr uint32_t kRngDomainLegs = 3;  // the flap campaign's y: a = leg, b = 0, value 0

// neo_leg_sequences (include/neo_planner.h) as the kernels take it, by value
struct LegSequences {
  int kind;                     // 0 table, 1 flap
  int legs;                     // flap: goals a mission
  const double *goals;          // table: [n_goals][2]
  int n_goals;
  const int *seq_begin;         // table: [B + 1]
  unsigned long long seed;      // flap
  const int *mission_ids;       // flap: [B], or NULL: the mission's index
  double x_pair[2], y_scale, y_shift;
};

// the uniform a flap goal is made of, and the goal
NEO_LEG_HD double leg_flap_uniform(uint64_t seed, uint32_t id, uint32_t k) {
  const Philox4 o = counter_stream_block(seed, id, k, 0u, kRngDomainLegs, 0u);
  return counter_uniform(o.w[0], o.w[1]);
}

NEO_LEG_HD void leg_flap_goal(uint64_t seed, uint32_t id, uint32_t k, double x_even, double x_odd, double y_scale,
                              double y_shift, double *out) {
  NEO_RNG_NO_CONTRACT
  const double u = leg_flap_uniform(seed, id, k);
  const double d = u - y_shift;
  out[0] = (k & 1u) ? x_odd : x_even;
  out[1] = y_scale * d;
}

// goals of mission b in the table, or 0 for a list that is not one (fewer than 1 or more than kLegsMax goals, or goals
// outside the table)
NEO_LEG_HD int leg_table_count(const int *seq_begin, int n_goals, int b, int &begin) {
  begin = seq_begin[b];
  const int end = seq_begin[b + 1];
  const long long n = (long long)end - (long long)begin;
  if (begin < 0 || end > n_goals || n < 1 || n > kLegsMax) return 0;
  return (int)n;
}

NEO_LEG_HD int leg_count(const LegSequences &s, int b) {
  if (s.kind == 0) {
    int begin;
    return leg_table_count(s.seq_begin, s.n_goals, b, begin);
  }
  return s.legs < 1 ? 0 : (s.legs > kLegsMax ? kLegsMax : s.legs);
}

// goal k of mission b into out[2]; false (out untouched) where the mission has no goal k
NEO_LEG_HD bool leg_goal(const LegSequences &s, int b, int k, double *out) {
  if (k < 0 || k >= leg_count(s, b)) return false;
  if (s.kind == 0) {
    const double *g = s.goals + ((size_t)s.seq_begin[b] + (size_t)k) * 2;
    out[0] = g[0];
    out[1] = g[1];
  } else {
    const uint32_t id = (uint32_t)(s.mission_ids ? s.mission_ids[b] : b);
    leg_flap_goal(s.seed, id, (uint32_t)k, s.x_pair[0], s.x_pair[1], s.y_scale, s.y_shift, out);
  }
  return true;
}

}  // namespace neo

#if defined(__HIPCC__)
// ------------------------------------------------------------------ the kernels
#include "neo_fleet.hpp"

namespace neo {

// (FleetLegCloseArgs, FleetLegOpenArgs: neo_host.hpp, which the unit includes first)

// What a leg was, from outcome[b] (NEO_LEG_*):
//   n_flown[b]      cmd_len for LANDED (the drone flies its array to the end), else min(cmd_index + 1, cmd_len) (it
//                   stopped on the row it was on), clamped to 0 .. cap: FleetReplanLoop._finish's rule
//   leg_end[b][2][2]  position and velocity of row n_flown - 1; head[b][0 .. 1] for a leg that never got a plan
//   final_dist[b]   sqrt(dx * dx + dy * dy) to goal[b], each operation rounded on its own (np.linalg.norm's bits); inf
//                   for n_flown == 0
__global__ __launch_bounds__(kFleetThreads) void fleet_leg_close_kernel(
    LaunchList list, const int *__restrict__ outcome, const double *__restrict__ cmd, int cap,
    const int *__restrict__ cmd_len, const int *__restrict__ cmd_index, const double *__restrict__ head,
    const double *__restrict__ goal, int *__restrict__ n_flown, double *__restrict__ leg_end,
    double *__restrict__ final_dist) {
#pragma clang fp contract(off)
  const int b = list.request(blockIdx.x * kFleetThreads + threadIdx.x);
  if (b < 0) return;
  int len = cmd_len[b];
  len = len < 0 ? 0 : (len > cap ? cap : len);
  int nf = len;
  if (outcome[b] != NEO_LEG_LANDED) {
    const long long on = (long long)cmd_index[b] + 1;
    nf = on < (long long)len ? (int)(on < 0 ? 0 : on) : len;
  }
  const double *src = nf > 0 ? cmd + ((size_t)b * cap + (size_t)(nf - 1)) * kFleetRow : head + (size_t)b * kFleetRow;
  const double ex = src[0], ey = src[1];
  double *e = leg_end + (size_t)b * 4;
  e[0] = ex;
  e[1] = ey;
  e[2] = src[2];
  e[3] = src[3];
  double dist = __builtin_inf();
  if (nf > 0) {
    const double dx = ex - goal[(size_t)b * 2], dy = ey - goal[(size_t)b * 2 + 1];
    const double xx = dx * dx, yy = dy * dy;
    dist = sqrt(xx + yy);
  }
  n_flown[b] = nf;
  final_dist[b] = dist;
}

// With k = leg[b] in 0 .. max_legs - 1 (any other k: the mission is skipped, its rows stay): row k of the log, leg[b] =
// k + 1, and, unless the outcome is NEO_LEG_OPEN, the next leg where the mission has a goal k + 1 and k + 1 < max_legs:
// that goal into goal[b], cur_pos[b] and leg_start[b] = the end position, head[b] = [end position, end velocity, 0],
// cmd_len = cmd_index = future_index = 0, flags[b] = 0 -- first_plan plans from drone_state, position and velocity
// (:491-504), and init_mission zeroes des_state_index.  Otherwise nothing more changes: the last leg's command array
// stays.  The integers of a row are stored as doubles (exact).
// A leg's start is kept in leg_start and not taken from head[b][0]: once a leg has flown a tick, head is its look-ahead
// state.  The caller writes leg 0's start; the kernel every later one.
__global__ __launch_bounds__(kFleetThreads) void fleet_leg_open_kernel(LaunchList list, LegSequences seq, FleetLegOpenArgs a) {
  const int b = list.request(blockIdx.x * kFleetThreads + threadIdx.x);
  if (b < 0) return;
  const int k = a.leg[b];
  if (k < 0 || k >= a.max_legs) return;
  const int oc = a.outcome[b];
  const int fl = a.flags[b] | (oc == NEO_LEG_ABANDONED ? NEO_FLEET_FLAG_ABANDONED : 0);
  const int afl = a.audit_flags[b];
  const double fd = a.final_dist[b];
  const double *e = a.leg_end + (size_t)b * 4;
  double *row = a.leg_log + ((size_t)b * a.max_legs + (size_t)k) * NEO_LEG_FIELDS;
  row[NEO_LEG_GOAL_X] = a.goal[(size_t)b * 2];
  row[NEO_LEG_GOAL_Y] = a.goal[(size_t)b * 2 + 1];
  row[NEO_LEG_START_X] = a.leg_start[(size_t)b * 2];
  row[NEO_LEG_START_Y] = a.leg_start[(size_t)b * 2 + 1];
  row[NEO_LEG_OUTCOME] = (double)oc;
  row[NEO_LEG_N_FLOWN] = (double)a.n_flown[b];
  row[NEO_LEG_FINAL_DIST] = fd;
  row[NEO_LEG_FLAGS] = (double)fl;
  row[NEO_LEG_COUNT] = (double)a.count[b];
  row[NEO_LEG_AUDIT_FLAGS] = (double)afl;
#pragma unroll
  for (int q = 0; q < NEO_AUDIT_FIELDS; ++q) row[NEO_LEG_AUDIT + q] = a.audit[(size_t)b * NEO_AUDIT_FIELDS + q];
  // _finish's rule: landed, within the threshold, no metric failure, no flag
  const bool ok = oc == NEO_LEG_LANDED && fd < a.threshold &&
                  !(afl & (NEO_AUDIT_FLAG_METRIC_FAIL | NEO_AUDIT_FLAG_NONFINITE)) && fl == 0;
  row[NEO_LEG_SUCCESS] = ok ? 1.0 : 0.0;
  a.leg[b] = k + 1;
  double g[2];
  if (oc == NEO_LEG_OPEN || k + 1 >= a.max_legs || !leg_goal(seq, b, k + 1, g)) return;
  a.goal[(size_t)b * 2] = g[0];
  a.goal[(size_t)b * 2 + 1] = g[1];
  a.cur_pos[(size_t)b * 2] = a.leg_start[(size_t)b * 2] = e[0];
  a.cur_pos[(size_t)b * 2 + 1] = a.leg_start[(size_t)b * 2 + 1] = e[1];
  double *hd = a.head + (size_t)b * kFleetRow;
  hd[0] = e[0];
  hd[1] = e[1];
  hd[2] = e[2];
  hd[3] = e[3];
  hd[4] = hd[5] = 0.0;
  a.cmd_len[b] = a.cmd_index[b] = a.future_index[b] = 0;
  a.flags[b] = 0;
}

// pair p: goal leg_of[p] of mission mission[p] into goal[p], exists[p] = 1; NaN and 0 where there is none or the
// mission is outside 0 .. B - 1
__global__ __launch_bounds__(kFleetThreads) void fleet_leg_goal_kernel(LegSequences seq, int B, int n,
                                                                       const int *__restrict__ mission,
                                                                       const int *__restrict__ leg_of,
                                                                       double *__restrict__ goal, int *__restrict__ exists) {
  const int p = blockIdx.x * kFleetThreads + threadIdx.x;
  if (p >= n) return;
  const int b = mission[p];
  double g[2] = {__builtin_nan(""), __builtin_nan("")};
  const bool have = b >= 0 && b < B && leg_goal(seq, b, leg_of[p], g);
  goal[(size_t)p * 2] = g[0];
  goal[(size_t)p * 2 + 1] = g[1];
  exists[p] = have ? 1 : 0;
}

}  // namespace neo
#endif  // __HIPCC__
