// neo_flight.hpp -- the fleet's flight model: a drone that tracks its commands with lag and gusts, in place of PX4 /
// Gazebo.  The reference reads the drone's odometry, not the command, for set_local_target
// (ros_node/traj_planner_node.py:452), the reach test (:183), the camera pose, the flight metric (:333-363) and
// save_tracking_err (:310-331); only the planning start state comes from the command array (:527-537).
//
// The first part is the model, plain C++ as well as HIP (it includes neo_counter_rng.hpp and nothing else of the
// project; the harness tests/host_harness/flight_host.cpp compiles it with the host compiler):
//
//   flight_out_row     the flown row of a state: (p, v, a + g - drag * v)
//   flight_substep     one sub-step of one mission against one command row
//   flight_fly         what one launch does for one mission: the index arithmetic of fleet_advance_kernel, the sub-steps
//                      of the period, the settle rows of a landed mission
//
// neo_planner_amd/flight_model.py is the NumPy model and the definition (the reference has no drone model): the same
// operations in the same order, every one rounded on its own (contraction is off in every function here; a host
// compiler that is not clang takes -ffp-contract=off on its command line).  fp64, only + - * / and sqrt; h, alpha, rho
// and scale are computed once on the host and handed over, so both sides hold the same doubles.  Header and model agree
// bit for bit.
//
// The second part (HIP only) holds the kernels, launched from neo_disp_fleet.hip:
//
//   fleet_fly_kernel         fleet_advance_kernel with the model in place of perfect tracking      one lane per mission
//   fleet_fly_error_kernel   save_tracking_err's table reduced: flown rows against command rows     one wavefront per mission
#pragma once
#include <math.h>
#include <stddef.h>

#include "neo_counter_rng.hpp"

#if defined(__HIPCC__)
#define NEO_FLY_HD __host__ __device__ __forceinline__
#else
#define NEO_FLY_HD inline
#endif
#if defined(__clang__)
#define NEO_FLY_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define NEO_FLY_NO_CONTRACT
#endif

namespace neo {

constexpr uint32_t kRngDomainGust = 4;  // a = sub-step / gust_every, b = 0 (domain 3: the flap goals of neo_legs.hpp)
constexpr int kFlyRow = 6;              // doubles of a command row and of a flown row
constexpr int kFlyState = 8;            // doubles of drone[b]: p, v, a, g
constexpr int kFlyFlagCmdFull = 2;      // NEO_FLEET_FLAG_CMD_FULL

struct FlightParams {  // neo_flight_model, field for field
  double h, kp, kv, a_max, alpha, drag, rho, scale;
  int gust_every;
  unsigned long long seed;
};

NEO_FLY_HD void flight_out_row(const FlightParams &m, const double *s, double *out) {
  NEO_FLY_NO_CONTRACT
  const double dx = m.drag * s[2], dy = m.drag * s[3];
  out[0] = s[0];
  out[1] = s[1];
  out[2] = s[2];
  out[3] = s[3];
  out[4] = (s[4] + s[6]) - dx;
  out[5] = (s[5] + s[7]) - dy;
}

// sub-step t of mission `id`, from time (t - 1) / cmd_hz to t / cmd_hz, against the command the drone holds during that
// period, r = cmd[min(t - 1, cmd_len - 1)] = (p_d, v_d, a_d); s[8] is updated.  Returns 1 where the command saturated.
NEO_FLY_HD int flight_substep(const FlightParams &m, uint32_t id, int t, const double *r, double *s) {
  NEO_FLY_NO_CONTRACT
  const double ex = r[0] - s[0], ey = r[1] - s[1], fx = r[2] - s[2], fy = r[3] - s[3];
  const double kpx = m.kp * ex, kpy = m.kp * ey, kvx = m.kv * fx, kvy = m.kv * fy;
  double ux = (r[4] + kpx) + kvx, uy = (r[5] + kpy) + kvy;
  const double xx = ux * ux, yy = uy * uy;
  const double n = sqrt(xx + yy);
  int sat = 0;
  if (n > m.a_max) {
    const double f = m.a_max / n;
    ux = ux * f;
    uy = uy * f;
    sat = 1;
  }
  const double lx = m.alpha * (ux - s[4]), ly = m.alpha * (uy - s[5]);
  s[4] = s[4] + lx;
  s[5] = s[5] + ly;
  if (m.scale != 0.0 && t % m.gust_every == 0) {
    const Philox4 o = counter_stream_block(m.seed, id, (uint32_t)(t / m.gust_every), 0u, kRngDomainGust, 0u);
    const double z0 = m.scale * counter_block_normal(o, 0), z1 = m.scale * counter_block_normal(o, 1);
    const double g0 = m.rho * s[6], g1 = m.rho * s[7];
    s[6] = g0 + z0;
    s[7] = g1 + z1;
  }
  const double dx = m.drag * s[2], dy = m.drag * s[3];
  const double ax = (s[4] + s[6]) - dx, ay = (s[5] + s[7]) - dy;
  const double hx = m.h * ax, hy = m.h * ay;
  s[2] = s[2] + hx;
  s[3] = s[3] + hy;
  const double qx = m.h * s[2], qy = m.h * s[3];
  s[0] = s[0] + qx;
  s[1] = s[1] + qy;
  return sat;
}

struct FlightLaunch {  // what a launch hands every mission
  int cap, step, ahead, first, settle;
  double reach;
};

// what a mission's words are after a launch (flight_fly writes the rows, the caller these)
struct FlightWords {
  int idx, fut, flown_len, saturated, cmd_full;
};

constexpr int kFlyChunk = 4;  // sub-steps whose command rows are handed over together

// One launch for one mission with len = min(cmd_len, cap) >= 1 commands: `first` (or a mission nothing of which has been
// flown yet) writes flown row cmd_index from the state as it stands; the sub-steps cmd_index + 1 .. min(cmd_index + step,
// last) follow; with settle > 0, on the array's last row, the last command (`hold`, 6 doubles) is held for at most
// `settle` more sub-steps, up to the first with the drone within `reach` of the goal, and never at or past row cap
// (kFlyFlagCmdFull).  `rows.next(base)` is called with base = cmd_index, then + kFlyChunk, ...; after it rows.cur[u] is
// command row min(base + u, last), the row sub-step base + u + 1 works against: the kernel's come from its rows in flight,
// the host's from memory.
template <class Rows>
NEO_FLY_HD FlightWords flight_fly(const FlightParams &m, const FlightLaunch &l, uint32_t id, int len, int cmd_index,
                                  int flown_len, const double *goal, const double *hold, double *s, double *flown,
                                  Rows &rows) {
  NEO_FLY_NO_CONTRACT
  const int last = len - 1;
  // (sums of non-negative ints below 2^30 each, checked by the caller's wrapper: no overflow)
  const int idx0 = cmd_index < 0 ? 0 : cmd_index;
  const int idx = idx0 > last - l.step ? last : idx0 + l.step;  // min(idx0 + step, len - 1)
  const int fut = idx > last - l.ahead ? last : idx + l.ahead;  // :531-532
  FlightWords w = {idx, fut, idx + 1, 0, 0};
  if ((l.first || flown_len < 1) && idx0 < l.cap) flight_out_row(m, s, flown + (size_t)idx0 * kFlyRow);
  // (a cmd_index beyond the array flies nothing: the start is taken from idx, so no sum can overflow)
  for (int base = (idx0 < idx ? idx0 : idx) + 1; base <= idx; base += kFlyChunk) {
    rows.next(base - 1);
#pragma unroll
    for (int u = 0; u < kFlyChunk; ++u) {
      const int t = base + u;
      if (t <= idx) {
        w.saturated += flight_substep(m, id, t, rows.cur[u], s);
        flight_out_row(m, s, flown + (size_t)t * kFlyRow);
      }
    }
  }
  if (l.settle > 0 && idx == last) {
    double r[kFlyRow];
    for (int q = 0; q < kFlyRow; ++q) r[q] = hold[q];
    for (int k = 0; k < l.settle; ++k) {
      const double dx = s[0] - goal[0], dy = s[1] - goal[1];
      const double xx = dx * dx, yy = dy * dy;
      if (sqrt(xx + yy) < l.reach) break;
      if (w.flown_len >= l.cap) {
        w.cmd_full = 1;
        break;
      }
      w.saturated += flight_substep(m, id, w.flown_len, r, s);
      flight_out_row(m, s, flown + (size_t)w.flown_len * kFlyRow);
      ++w.flown_len;
    }
  }
  return w;
}

// the rows of a mission from memory, chunk by chunk (the host's Rows; the kernel keeps a chunk ahead in flight)
struct FlightRowsMem {
  const double *rows;
  int last;
  double cur[kFlyChunk][kFlyRow];
  NEO_FLY_HD void next(int base) {
    for (int u = 0; u < kFlyChunk; ++u) {
      const int t = base + u < last ? base + u : last;
      for (int q = 0; q < kFlyRow; ++q) cur[u][q] = rows[(size_t)t * kFlyRow + q];
    }
  }
};

}  // namespace neo

#if defined(__HIPCC__)
// ------------------------------------------------------------------ the kernels
#include "neo_fleet.hpp"

namespace neo {

constexpr int kFlyU = 4;  // fly_error: samples per lane and round, 256 a round, as the flight audit
static_assert(kFlyFlagCmdFull == NEO_FLEET_FLAG_CMD_FULL && kFlyRow == kFleetRow, "the model's copies of the fleet's constants");

// The state chain of a sub-step is serial; the command rows do not depend on it.  A lane therefore has the rows of the
// NEXT kFlyChunk sub-steps in flight while it computes the current kFlyChunk (rows past the array's last are the last's:
// loaded, not used), so the chain waits for HBM once a launch and not once a sub-step.  Every index into cur / nxt is a
// compile-time one: both stay in registers.  Lanes of a wavefront sit at different t: the gust branch diverges, which
// is accepted.
struct FlightRowsAhead {
  const double *rows;  // the mission's command array
  int last;
  bool started;
  double cur[kFlyChunk][kFlyRow], nxt[kFlyChunk][kFlyRow];
  __device__ __forceinline__ void load(double (&into)[kFlyChunk][kFlyRow], int from) const {
#pragma unroll
    for (int u = 0; u < kFlyChunk; ++u) {
      const int t = from + u < last ? from + u : last;
      const double *r = rows + (size_t)t * kFlyRow;
#pragma unroll
      for (int q = 0; q < kFlyRow; ++q) into[u][q] = r[q];
    }
  }
  __device__ __forceinline__ void next(int base) {
    if (!started) {
      load(cur, base);
      started = true;
    } else {
#pragma unroll
      for (int u = 0; u < kFlyChunk; ++u)
#pragma unroll
        for (int q = 0; q < kFlyRow; ++q) cur[u][q] = nxt[u][q];
    }
    load(nxt, base + kFlyChunk);
  }
};

__global__ __launch_bounds__(kFleetThreads) void fleet_fly_kernel(
    LaunchList list, FlightParams model, FlightLaunch launch, const double *__restrict__ cmd,
    const int *__restrict__ cmd_len, int *__restrict__ cmd_index, int *__restrict__ future_index,
    const int *__restrict__ mission_ids, const double *__restrict__ goal, double *__restrict__ drone,
    double *__restrict__ flown, int *__restrict__ flown_len, int *__restrict__ saturated, int *__restrict__ flags,
    double *__restrict__ cur_pos, double *__restrict__ head) {
  const int b = list.request(blockIdx.x * kFleetThreads + threadIdx.x);
  if (b < 0) return;
  const int cap = launch.cap;
  int len = cmd_len[b];
  len = len > cap ? cap : len;
  if (len < 1) return;  // nothing planned yet: nothing to fly along
  const int last = len - 1;
  const double *rows = cmd + (size_t)b * cap * kFlyRow;
  double s[kFlyState];
#pragma unroll
  for (int q = 0; q < kFlyState; ++q) s[q] = drone[(size_t)b * kFlyState + q];
  const double gl[2] = {goal[(size_t)b * 2], goal[(size_t)b * 2 + 1]};
  const int idx_in = cmd_index[b];
  FlightRowsAhead at;
  at.rows = rows;
  at.last = last;
  at.started = false;
  const uint32_t id = (uint32_t)(mission_ids ? mission_ids[b] : b);
  const FlightWords w = flight_fly(model, launch, id, len, idx_in, flown_len[b], gl, rows + (size_t)last * kFlyRow, s,
                                   flown + (size_t)b * cap * kFlyRow, at);
#pragma unroll
  for (int q = 0; q < kFlyState; ++q) drone[(size_t)b * kFlyState + q] = s[q];
  cmd_index[b] = w.idx;
  future_index[b] = w.fut;
  flown_len[b] = w.flown_len;
  if (w.saturated) saturated[b] += w.saturated;
  if (w.cmd_full) flags[b] |= kFlyFlagCmdFull;
  cur_pos[(size_t)b * 2] = s[0];
  cur_pos[(size_t)b * 2 + 1] = s[1];
  const double *fr = rows + (size_t)w.fut * kFlyRow;
  double *hd = head + (size_t)b * kFlyRow;
  hd[0] = fr[0];
  hd[1] = fr[1];
  hd[2] = fr[2];
  hd[3] = fr[3];
  hd[4] = hd[5] = 0.0;  // the reference hands plan() a 2 x 2 state (:534-535)
}

// Sample j is flown row j * stride < flown_len[b] (clamped to 0 .. cap) against command row min(j * stride, len - 1), len
// = min(cmd_len[b], cap): e_j = sqrt(dx * dx + dy * dy) of the positions, the same of the velocities.  Every lane
// accumulates its own samples j = lane, lane + 64, ... in time order; the fixed-order reductions of neo_wave.hpp /
// neo_audit.hpp combine the lanes.  The largest position error goes through wave_min_first as its negative (exact): ties
// to the first sample.  pos_err_final is e at flown row flown_len - 1, whatever the stride.
__global__ __launch_bounds__(kWave) void fleet_fly_error_kernel(
    LaunchList list, const double *__restrict__ flown, const double *__restrict__ cmd, int cap,
    const int *__restrict__ flown_len, const int *__restrict__ cmd_len, int stride, double *__restrict__ fly,
    int *__restrict__ count, int *__restrict__ flags) {
#pragma clang fp contract(off)
  const int b = list.request(blockIdx.x);  // wave-uniform
  if (b < 0) return;
  const int lane = lane_id();
  double *rec = fly + (size_t)b * NEO_FLY_FIELDS;
  auto blank = [&](int fl) {
    if (lane < NEO_FLY_FIELDS) rec[lane] = __builtin_nan("");
    if (lane == 0) {
      count[b] = 0;
      flags[b] = fl;
    }
  };
  int nf = flown_len[b];
  nf = nf < 0 ? 0 : (nf > cap ? cap : nf);
  int len = cmd_len[b];
  len = len > cap ? cap : len;
  const int cnt = nf > 0 ? (nf - 1) / stride + 1 : 0;  // len(range(0, nf, stride)); (cnt - 1) * stride < cap
  if (cnt == 0 || len < 1) return blank(0);
  const double *fr = flown + (size_t)b * cap * kFlyRow, *cr = cmd + (size_t)b * cap * kFlyRow;

  double psum = 0.0, vsum = 0.0, pmax = -__builtin_inf(), vmax = 0.0;
  int kmax = INT_MAX, bad = 0;
  for (int base = 0; base < cnt; base += kFlyU * kWave) {
    double fs[kFlyU][4], cs[kFlyU][4];  // position and velocity: the accelerations are not compared
    bool on[kFlyU];
#pragma unroll
    for (int u = 0; u < kFlyU; ++u) {
      const int k = base + u * kWave + lane;
      on[u] = k < cnt;
      const int row = (on[u] ? k : 0) * stride;  // idle slots read row 0 (cap >= 1)
      const double *f = fr + (size_t)row * kFlyRow, *c = cr + (size_t)(row < len ? row : len - 1) * kFlyRow;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        fs[u][q] = f[q];
        cs[u][q] = c[q];
      }
    }
#pragma unroll
    for (int u = 0; u < kFlyU; ++u) {
      const int k = base + u * kWave + lane;
      if (on[u]) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (!__builtin_isfinite(fs[u][q]) || !__builtin_isfinite(cs[u][q])) bad = 1;
        const double dx = fs[u][0] - cs[u][0], dy = fs[u][1] - cs[u][1], du = fs[u][2] - cs[u][2], dv = fs[u][3] - cs[u][3];
        const double xx = dx * dx, yy = dy * dy, uu = du * du, vv = dv * dv;
        const double p2 = xx + yy, v2 = uu + vv;
        const double pe = sqrt(p2), ve = sqrt(v2);
        psum = psum + p2;
        vsum = vsum + v2;
        if (pe > pmax) {
          pmax = pe;
          kmax = k;
        }
        vmax = ve > vmax ? ve : vmax;
      }
    }
  }
  double pfin = 0.0;
  {  // (every lane the same two rows: one broadcast load each)
    const int row = nf - 1;
    const double *f = fr + (size_t)row * kFlyRow, *c = cr + (size_t)(row < len ? row : len - 1) * kFlyRow;
    const double dx = f[0] - c[0], dy = f[1] - c[1];
    const double xx = dx * dx, yy = dy * dy;
    pfin = sqrt(xx + yy);
  }
  double s_p, s_v, s_u0, s_u1;
  wave_sum4(psum, vsum, 0.0, 0.0, s_p, s_v, s_u0, s_u1);
  const double vmx = wave_max_nonneg(vmax);
  double npmax = -pmax;
  wave_min_first(npmax, kmax);
  const double r_p = sqrt(s_p / (double)cnt), r_v = sqrt(s_v / (double)cnt);
  if (!__builtin_isfinite(r_p) || !__builtin_isfinite(r_v) || !__builtin_isfinite(pfin)) bad = 1;
  if (wave_max_nonneg(bad)) return blank(NEO_AUDIT_FLAG_NONFINITE);
  if (lane == 0) {
    rec[NEO_FLY_POS_ERR_RMS] = r_p;
    rec[NEO_FLY_POS_ERR_MAX] = -npmax;
    rec[NEO_FLY_POS_ERR_MAX_AT] = (double)(kmax * stride);
    rec[NEO_FLY_VEL_ERR_RMS] = r_v;
    rec[NEO_FLY_VEL_ERR_MAX] = vmx;
    rec[NEO_FLY_POS_ERR_FINAL] = pfin;
    count[b] = cnt;
    flags[b] = 0;
  }
}

}  // namespace neo
#endif  // __HIPCC__
