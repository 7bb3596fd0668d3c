// neo_track.hpp -- fleet goal routes: missions that chase a goal which keeps moving (ros_node/tracker_planner_node.py
// with tracker_manager_node.py: the global target is whatever the last message said, :160-162, :313-316).
//
// The first part is the route model, plain C++ as well as HIP (it includes <math.h> and nothing else; the harness
// tests/host_harness/track_host.cpp compiles it with the host compiler): a mission's goal moves along a polyline at
// constant speed.
//
//   route_seg_len      seg_k = sqrt(dx * dx + dy * dy); a closed route has the closing segment back to vertex 0
//   route_cum          cum_0 = 0, cum_{k+1} = cum_k + seg_k, summed in order
//   route_arc          s = speed * t; closed: fmod(s, total); open: s clamped to total
//   route_find         the largest k with cum_k <= s, at most the last segment, by bisection on cum
//   route_point        the point at time t, walking the segments (no cum array: one lane, one route)
//   route_point_cum    the same point from a cum array (the same k, the same bits)
//
// neo_planner_amd/goal_routes.py is the NumPy model of this part: the same operations in the same order, every one
// rounded on its own (contraction is off in every function here; a host compiler that is not clang takes
// -ffp-contract=off on its command line).  Header and model agree bit for bit; fmod is exact, the fp64 division and
// square root are the correctly rounded ones, on the host and on gfx950.
//
// The second part (HIP only) holds the kernels, launched from neo_disp_fleet.hip:
//
//   fleet_goal_kernel          goal[b] = route_point_b(t)                                    one lane per mission
//   fleet_hold_kernel          a drone that runs out of commands holds the last one (:387-391)   one wavefront per mission
//   fleet_track_audit_kernel   the gap between the flown rows and the moving goal            one wavefront per mission
//
// All arrays are indexed by mission, fp64, no floating-point atomics, fixed summation order: a mission's results depend
// on neither the batch, the subset nor the launch.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define NEO_TRK_HD __host__ __device__ __forceinline__
#else
#define NEO_TRK_HD inline
#endif
#if defined(__clang__)
#define NEO_TRK_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define NEO_TRK_NO_CONTRACT
#endif

namespace neo {

constexpr int kRouteMax = 256;  // NEO_FLEET_ROUTE_MAX: vertices of a route

// v: the route's n vertices, x y pairs.  Segment k runs from vertex k to vertex k + 1 (vertex 0 after the last one).
NEO_TRK_HD int route_segments(int n, int closed) { return closed ? n : n - 1; }

NEO_TRK_HD double route_seg_len(const double *v, int n, int k) {
  NEO_TRK_NO_CONTRACT
  const int k1 = k + 1 < n ? k + 1 : 0;
  const double dx = v[2 * k1] - v[2 * k], dy = v[2 * k1 + 1] - v[2 * k + 1];
  const double xx = dx * dx, yy = dy * dy;
  return sqrt(xx + yy);
}

// cum[0 .. segments]
NEO_TRK_HD void route_cum(const double *v, int n, int closed, double *cum) {
  NEO_TRK_NO_CONTRACT
  const int nseg = route_segments(n, closed);
  double c = 0.0;
  cum[0] = 0.0;
  for (int k = 0; k < nseg; ++k) {
    c = c + route_seg_len(v, n, k);
    cum[k + 1] = c;
  }
}

NEO_TRK_HD double route_arc(double speed, double t, double total, int closed) {
  NEO_TRK_NO_CONTRACT
  const double s = speed * t;
  if (closed) return fmod(s, total);  // (a route without length: NaN, which finds segment 0)
  return s > total ? total : s;
}

// cum is non-decreasing and cum_0 = 0; an s that compares false with everything (NaN) finds 0
NEO_TRK_HD int route_find(const double *cum, int nseg, double s) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (cum[mid] <= s)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// v_k + ((s - cum_k) / seg_k) * (v_{k+1} - v_k); v_k exactly on a segment or a route without length
NEO_TRK_HD void route_interp(const double *v, int n, int k, double s, double cum_k, double total, double *out) {
  NEO_TRK_NO_CONTRACT
  const int k1 = k + 1 < n ? k + 1 : 0;
  const double seg = route_seg_len(v, n, k);
  if (seg == 0.0 || total == 0.0) {
    out[0] = v[2 * k];
    out[1] = v[2 * k + 1];
    return;
  }
  const double f = (s - cum_k) / seg;
  const double ex = v[2 * k1] - v[2 * k], ey = v[2 * k1 + 1] - v[2 * k + 1];
  const double px = f * ex, py = f * ey;
  out[0] = v[2 * k] + px;
  out[1] = v[2 * k + 1] + py;
}

NEO_TRK_HD void route_point_cum(const double *v, const double *cum, int n, int closed, double speed, double t, double *out) {
  const int nseg = route_segments(n, closed);
  const double total = cum[nseg];
  const double s = route_arc(speed, t, total, closed);
  const int k = route_find(cum, nseg, s);
  route_interp(v, n, k, s, cum[k], total, out);
}

// the same without an array: the running sum once for the total, once more up to the segment.  The sums are
// non-decreasing, so the first cum_{j+1} that is not <= s ends the search: the k of route_find.
NEO_TRK_HD void route_point(const double *v, int n, int closed, double speed, double t, double *out) {
  NEO_TRK_NO_CONTRACT
  const int nseg = route_segments(n, closed);
  double total = 0.0;
  for (int k = 0; k < nseg; ++k) total = total + route_seg_len(v, n, k);
  const double s = route_arc(speed, t, total, closed);
  int k = 0;
  double ck = 0.0, c = 0.0;
  for (int j = 0; j + 1 < nseg; ++j) {
    c = c + route_seg_len(v, n, j);
    if (!(c <= s)) break;
    k = j + 1;
    ck = c;
  }
  route_interp(v, n, k, s, ck, total, out);
}

}  // namespace neo

#if defined(__HIPCC__)
// ------------------------------------------------------------------ the kernels
#include "neo_fleet.hpp"

namespace neo {

constexpr int kTrackU = 4;  // samples per lane and round: 256 a round, as the flight audit

// mission b's vertices in the table: their number, or 0 for a route that is not one (fewer than 2 or more than kRouteMax
// vertices, or vertices outside the table)
__device__ __forceinline__ int route_of(const int *__restrict__ route_begin, int n_vertices, int b, int &begin) {
  begin = route_begin[b];
  const int end = route_begin[b + 1];
  const long long n = (long long)end - (long long)begin;
  if (begin < 0 || end > n_vertices || n < 2 || n > kRouteMax) return 0;
  return (int)n;
}

__global__ __launch_bounds__(kFleetThreads) void fleet_goal_kernel(
    LaunchList list, const double *__restrict__ vertices, int n_vertices, const int *__restrict__ route_begin,
    const double *__restrict__ speed, const int *__restrict__ closed, double t, double *__restrict__ goal) {
  const int b = list.request(blockIdx.x * kFleetThreads + threadIdx.x);
  if (b < 0) return;
  int begin;
  const int n = route_of(route_begin, n_vertices, b, begin);
  double o[2] = {__builtin_nan(""), __builtin_nan("")};
  if (n) route_point(vertices + (size_t)begin * 2, n, closed ? closed[b] != 0 : 0, speed[b], t, o);
  goal[(size_t)b * 2] = o[0];
  goal[(size_t)b * 2 + 1] = o[1];
}

// need = cmd_index + step + 1 rows are flown by the end of the coming replan period.  A command array that ends before
// that gets copies of its last row -- position, velocity and acceleration as they are: the reference re-reads that row
// (:387-391) -- up to min(need, cap) rows.  The lanes stride over the rows, three 16-byte stores a row.
__global__ __launch_bounds__(kWave) void fleet_hold_kernel(LaunchList list, double *__restrict__ cmd, int cap,
                                                            int *__restrict__ cmd_len, const int *__restrict__ cmd_index,
                                                            int step, int *__restrict__ flags) {
  const int b = list.request(blockIdx.x);  // wave-uniform
  if (b < 0) return;
  const int lane = lane_id();
  int len = cmd_len[b];
  len = len > cap ? cap : len;
  if (len < 1) return;  // nothing planned yet: nothing to hold
  int idx = cmd_index[b];
  idx = idx < 0 ? 0 : idx;
  const long long need = (long long)idx + (long long)step + 1;
  if ((long long)len >= need) return;
  const int upto = need < (long long)cap ? (int)need : cap;
  double2 *rows = reinterpret_cast<double2 *>(cmd + (size_t)b * cap * kFleetRow);
  const double2 *src = rows + (size_t)(len - 1) * 3;
  const double2 s0 = src[0], s1 = src[1], s2 = src[2];
  for (int r = len + lane; r < upto; r += kWave) {
    double2 *dst = rows + (size_t)r * 3;
    dst[0] = s0;
    dst[1] = s1;
    dst[2] = s2;
  }
  if (lane == 0) {
    cmd_len[b] = upto;
    if (need > (long long)cap) flags[b] |= NEO_FLEET_FLAG_CMD_FULL;
  }
}

// The route's vertices and cum in LDS (cum summed by lane 0, in order), then sample j = row j * stride of the mission's
// command array, j * stride < n_flown, at t_j = (j * stride) / hz: gap_j = sqrt of the squared distance between the row's
// position and route_point_cum(t_j).  Every lane accumulates its own samples j = lane, lane + 64, ... in time order; the
// fixed-order reductions of neo_wave.hpp / neo_audit.hpp combine the lanes.  The largest gap goes through
// wave_min_first as its negative (exact), so both extrema give ties to the first sample.
__global__ __launch_bounds__(kWave) void fleet_track_audit_kernel(
    LaunchList list, const double *__restrict__ cmd, int cap, const int *__restrict__ n_flown, int stride, double hz,
    const double *__restrict__ vertices, int n_vertices, const int *__restrict__ route_begin,
    const double *__restrict__ speed, const int *__restrict__ closed, double radius, double *__restrict__ track,
    int *__restrict__ count, int *__restrict__ flags) {
#pragma clang fp contract(off)
  __shared__ double vs[2 * kRouteMax];
  __shared__ double cum[kRouteMax + 1];
  const int b = list.request(blockIdx.x);  // wave-uniform
  if (b < 0) return;
  const int lane = lane_id();
  double *rec = track + (size_t)b * NEO_TRACK_FIELDS;
  auto blank = [&](int fl) {
    if (lane < NEO_TRACK_FIELDS) rec[lane] = __builtin_nan("");
    if (lane == 0) {
      count[b] = 0;
      flags[b] = fl;
    }
  };
  int begin;
  const int n = route_of(route_begin, n_vertices, b, begin);
  if (!n) return blank(NEO_AUDIT_FLAG_NONFINITE);
  int nf = n_flown[b];
  nf = nf < 0 ? 0 : (nf > cap ? cap : nf);
  const int cnt = nf > 0 ? (nf - 1) / stride + 1 : 0;  // len(range(0, nf, stride)); (cnt - 1) * stride < cap
  if (cnt == 0) return blank(0);
  for (int i = lane; i < 2 * n; i += kWave) vs[i] = vertices[(size_t)begin * 2 + i];
  __syncthreads();
  const int cl = closed ? closed[b] != 0 : 0;
  if (lane == 0) route_cum(vs, n, cl, cum);
  __syncthreads();
  const double spd = speed[b];
  const double *rows = cmd + (size_t)b * cap * kFleetRow;

  double gsum = 0.0, gmax = -__builtin_inf(), gmin = __builtin_inf(), glast = 0.0;
  int kmax = INT_MAX, kmin = INT_MAX, kfirst = -1, nin = 0, bad = 0;
  for (int base = 0; base < cnt; base += kTrackU * kWave) {
    double st[kTrackU][kFleetRow];
    bool on[kTrackU];
#pragma unroll
    for (int u = 0; u < kTrackU; ++u) {
      const int k = base + u * kWave + lane;
      on[u] = k < cnt;
      const double *r = rows + (size_t)(on[u] ? k : 0) * stride * kFleetRow;  // idle slots read row 0 (cap >= 1)
#pragma unroll
      for (int q = 0; q < kFleetRow; ++q) st[u][q] = r[q];
    }
#pragma unroll
    for (int u = 0; u < kTrackU; ++u) {
      const int k = base + u * kWave + lane;
      if (on[u]) {
#pragma unroll
        for (int q = 0; q < kFleetRow; ++q)
          if (!__builtin_isfinite(st[u][q])) bad = 1;
        const double tj = (double)(k * stride) / hz;
        double g[2];
        route_point_cum(vs, cum, n, cl, spd, tj, g);
        const double dx = st[u][0] - g[0], dy = st[u][1] - g[1];
        const double xx = dx * dx, yy = dy * dy;
        const double gap = sqrt(xx + yy);
        if (!__builtin_isfinite(gap)) bad = 1;
        gsum = gsum + gap;
        if (gap > gmax) {
          gmax = gap;
          kmax = k;
        }
        if (gap < gmin) {
          gmin = gap;
          kmin = k;
        }
        if (gap <= radius) {
          ++nin;
          if (kfirst < 0) kfirst = k;
        }
        if (k == cnt - 1) glast = gap;
      }
    }
  }
  if (wave_max_nonneg(bad)) return blank(NEO_AUDIT_FLAG_NONFINITE);
  const double s_gap = wave_sum(gsum);
  double ngmax = -gmax;
  wave_min_first(ngmax, kmax);
  wave_min_first(gmin, kmin);
  const int fkey = wave_max_nonneg(kfirst >= 0 ? INT_MAX - kfirst : 0);  // largest key = earliest sample within
  const int n_in = wave_sum(nin);
  glast = rdlane(glast, (cnt - 1) & (kWave - 1));
  if (lane == 0) {
    auto t_of = [&](int k) { return (double)(k * stride) / hz; };  // the time of command row k * stride
    rec[NEO_TRACK_GAP_MEAN] = s_gap / (double)cnt;
    rec[NEO_TRACK_GAP_MAX] = -ngmax;
    rec[NEO_TRACK_T_GAP_MAX] = t_of(kmax);
    rec[NEO_TRACK_GAP_MIN] = gmin;
    rec[NEO_TRACK_T_GAP_MIN] = t_of(kmin);
    rec[NEO_TRACK_GAP_FINAL] = glast;
    rec[NEO_TRACK_T_FIRST_WITHIN] = fkey > 0 ? t_of(INT_MAX - fkey) : -1.0;
    rec[NEO_TRACK_FRAC_WITHIN] = (double)n_in / (double)cnt;
    count[b] = cnt;
    flags[b] = 0;
  }
}

}  // namespace neo
#endif  // __HIPCC__
