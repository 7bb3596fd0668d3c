// neo_audit.hpp -- audit_kernel: the reference's flight metric (ros_node/traj_planner_node.py:333-363,
// get_weighted_metric) for a batch of planned trajectories under perfect tracking (include/neo_planner.h,
// neo_audit_traj_batch), and the accumulation of that metric (AuditAcc), which fleet_audit_kernel (neo_fleet.hpp) runs
// over flown rows.  Included by neo_disp_audit.hip and, through neo_fleet.hpp, by neo_disp_fleet.hip; nothing of the
// optimiser is included here.
//
// One wavefront per trajectory, as traj_state_kernel: the piece table (neo_pieces.hpp: the fp64 solve, the coefficients
// and the sequential prefix sums of the durations in LDS), then the lanes stride over the samples -- kAuditU samples a
// lane per round, whose map gathers are all in flight before the first is consumed (the lookups' prepare / load / finish
// split).  Every lane accumulates its own samples k = lane, lane + 64, ... in increasing order; at the end fixed-order DPP
// reductions combine the lanes (wave_sum4 for the three sums, wave_max_nonneg for the maxima and flags, wave_min_first
// below for the minimum and its sample).  The association order depends on neither kAuditU nor the grid: same bits.
#pragma once
#include <climits>
#include "neo_pieces.hpp"

namespace neo {

constexpr int kAuditU = 4;  // samples per lane and round: 256 a round, 4 gathers in flight per lane

// (value, index) minimum over the wavefront, ties to the smaller index; the result is returned wave-uniform.  The same
// scan as wave_max_nonneg (row_shr 1, 2, 4, 8, then the two row broadcasts, read at lane 63), but every DPP move keeps
// the lane's OWN value where it has no source (dpp_keep): neutral for a minimum, whatever the values are.
// (The six steps are written out: as wave_scan over a (value, index) pair the compiler turns the tie test into other
//  branches and selects.)
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ void min_first_step(double &v, int &k) {
  const double ov = dpp_keep<CTRL, ROW_MASK>(v);
  const int ok = dpp_keep<CTRL, ROW_MASK>(k);
  const bool take = ov < v || (ov == v && ok < k);
  v = take ? ov : v;
  k = take ? ok : k;
}
__device__ __forceinline__ void wave_min_first(double &v, int &k) {
  min_first_step<0x111>(v, k);
  min_first_step<0x112>(v, k);
  min_first_step<0x114>(v, k);
  min_first_step<0x118>(v, k);
  min_first_step<0x142, 0xa>(v, k);
  min_first_step<0x143, 0xc>(v, k);
  v = rdlane(v, kWave - 1);
  k = rdlane(k, kWave - 1);
}

// |u|^2 summed over the axes in order, every product and sum rounded on its own (as NumPy's (u ** 2).sum() rounds)
template <int D>
__device__ __forceinline__ double audit_norm2(const double (&u)[D]) {
#pragma clang fp contract(off)
  double s = u[0] * u[0];
#pragma unroll
  for (int d = 1; d < D; ++d) s += u[d] * u[d];
  return s;
}

// no usable trajectory (a slot outside the table, a failed solve, a state that is not finite): NaN record, no samples
__device__ __forceinline__ void audit_reject(int b, double *__restrict__ audit, int *__restrict__ count,
                                             int *__restrict__ flags) {
  const int lane = lane_id();
  if (lane < NEO_AUDIT_FIELDS) audit[(size_t)b * NEO_AUDIT_FIELDS + lane] = __builtin_nan("");
  if (lane == 0) {
    count[b] = 0;
    flags[b] = NEO_AUDIT_FLAG_NONFINITE;
  }
}

// The metric's accumulation over the samples of one trajectory, for audit_kernel below and fleet_audit_kernel
// (neo_fleet.hpp).  A lane feeds its samples k = lane, lane + 64, ... in increasing order: kinematics() with a sample's
// row, clearance() with its map distance and the position neighbour() fetched; the accumulators of the two are
// independent, so which is fed first within a round does not matter.  finish() combines the lanes and writes the
// record.  Every step rounds each operation on its own, as the reference's NumPy does (the pragma is lexical: each
// carries it).
template <int D>
struct AuditAcc {
  double path = 0.0, feas = 0.0, coll = 0.0, speed_max = 0.0, acc_max = 0.0, dmin = __builtin_inf();
  int kmin = INT_MAX, kunsafe = -1, outside = 0, bad = 0;
  double carry[D];  // position of the sample before this sub-round's lane 0 (lane 63 of the one before)

  __device__ __forceinline__ AuditAcc() {
#pragma unroll
    for (int d = 0; d < D; ++d) carry[d] = 0.0;
  }

  // the row of one of the lane's own samples
  __device__ __forceinline__ void kinematics(const double (&pos)[D], const double (&vel)[D], const double (&acc)[D],
                                             double vmax2) {
#pragma clang fp contract(off)
    const double v2 = audit_norm2<D>(vel), a2 = audit_norm2<D>(acc);
#pragma unroll
    for (int d = 0; d < D; ++d)
      if (!__builtin_isfinite(pos[d]) || !__builtin_isfinite(vel[d]) || !__builtin_isfinite(acc[d])) bad = 1;
    const double speed = sqrt(v2), accn = sqrt(a2);
    speed_max = speed > speed_max ? speed : speed_max;
    acc_max = accn > acc_max ? accn : acc_max;
    const double vv = v2 - vmax2;  // :346-348
    if (vv > 0.0) feas += vv * vv * vv;
  }

  // position of the sample before the lane's in this sub-round (the path increment needs it): called by ALL lanes,
  // whether their sample exists or not
  __device__ __forceinline__ void neighbour(const double (&pos)[D], double (&prev)[D]) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      prev[d] = from_prev(pos[d], carry[d]);
      carry[d] = rdlane(pos[d], kWave - 1);
    }
  }

  // sample k, one of the lane's own: prev from neighbour(), dk its map distance, inside: the lookup was inside the map
  __device__ __forceinline__ void clearance(int k, const double (&pos)[D], const double (&prev)[D], double dk, bool inside,
                                            double safe) {
#pragma clang fp contract(off)
    if (k >= 1) {  // :341-343
      double dp[D];
#pragma unroll
      for (int d = 0; d < D; ++d) dp[d] = pos[d] - prev[d];
      path += sqrt(audit_norm2<D>(dp));
    }
    const double vd = safe - dk;  // :351-355
    const bool unsafe = vd > 0.0;  // (selects, not a branch of its own inside the caller's `on` region)
    coll = unsafe ? coll + vd * vd * vd : coll;
    kunsafe = unsafe && kunsafe < 0 ? k : kunsafe;
    if (dk < dmin) {
      dmin = dk;
      kmin = k;
    }
    if (!inside) outside = 1;
  }

  // the lanes combined in fixed order, the record and the flags of request b.  t_of(k): the time of sample k
  template <class TimeOf>
  __device__ __forceinline__ void finish(int b, int cnt, double duration, TimeOf t_of, double w0, double w1, double w2,
                                         double coll_tol, double *__restrict__ audit, int *__restrict__ count,
                                         int *__restrict__ flags) {
#pragma clang fp contract(off)
    if (wave_max_nonneg(bad)) return audit_reject(b, audit, count, flags);
    double s_path, s_feas, s_coll, s_unused;
    wave_sum4(path, feas, coll, 0.0, s_path, s_feas, s_coll, s_unused);
    const double vmx = wave_max_nonneg(speed_max), amx = wave_max_nonneg(acc_max);
    wave_min_first(dmin, kmin);
    const int ukey = wave_max_nonneg(kunsafe >= 0 ? INT_MAX - kunsafe : 0);  // largest key = earliest unsafe sample
    const int outs = wave_max_nonneg(outside);
    if (lane_id() == 0) {
      double *rec = audit + (size_t)b * NEO_AUDIT_FIELDS;
      const double weighted = w0 * s_path + w1 * s_feas + w2 * s_coll;  // np.dot(raw_cost, metric_weights) (:357)
      rec[NEO_AUDIT_PATH_LENGTH] = s_path;
      rec[NEO_AUDIT_FEASIBILITY] = s_feas;
      rec[NEO_AUDIT_COLLISION] = s_coll;
      rec[NEO_AUDIT_WEIGHTED] = weighted;
      rec[NEO_AUDIT_MIN_CLEARANCE] = dmin;
      rec[NEO_AUDIT_T_MIN_CLEARANCE] = cnt > 0 ? t_of(kmin) : -1.0;
      rec[NEO_AUDIT_MAX_SPEED] = vmx;
      rec[NEO_AUDIT_MAX_ACC] = amx;
      rec[NEO_AUDIT_T_FIRST_UNSAFE] = ukey > 0 ? t_of(INT_MAX - ukey) : -1.0;
      rec[NEO_AUDIT_DURATION] = duration;
      count[b] = cnt;
      flags[b] = (ukey > 0 ? NEO_AUDIT_FLAG_UNSAFE : 0) | (weighted > 10.0 * coll_tol ? NEO_AUDIT_FLAG_METRIC_FAIL : 0) |
                 (outs ? NEO_AUDIT_FLAG_OUTSIDE_MAP : 0);
    }
  }
};

// MapT / LookupT: Map2D with Lookup2D<double>, or Map3D with Lookup3D<double, E, LAYOUT> -- neo_esdf_query's arithmetic
// (its LAYOUT 9 reads the layout at run time; a fixed LAYOUT runs the same load path and keeps the gathers in flight)
template <int D, class MapT, class LookupT>
__global__ __launch_bounds__(kWave) void audit_kernel(int B, int M, DevParams prm, const MapT *__restrict__ maps,
                                                       const int *__restrict__ scene_slot, int nmaps,
                                                       const double *__restrict__ x, const double *__restrict__ head,
                                                       const double *__restrict__ tail, double hz, double w0, double w1,
                                                       double w2, double *__restrict__ audit, int *__restrict__ count,
                                                       int *__restrict__ flags) {
#pragma clang fp contract(off)  // the metric's own arithmetic rounds every operation as the reference's NumPy does
  NEO_PIECE_LDS(D, lds);
  const int b = blockIdx.x;
  if (b >= B) return;
  const int lane = lane_id();
  const int slot = scene_slot ? scene_slot[b] : 0;
  if (slot < 0 || slot >= nmaps) return audit_reject(b, audit, count, flags);
  const MapT map = maps[slot];

  PieceTable<D> pt(lds, M);
  if (pt.solve(b, prm, x, head, tail) != 0) return audit_reject(b, audit, count, flags);
  const double step = 1.0 / hz;
  int cnt;
  if (!pt.sample_count(step, cnt)) return audit_reject(b, audit, count, flags);

  LookupT lk(map);
  const double vmax2 = prm.v_max * prm.v_max, safe = prm.safe_dis;
  AuditAcc<D> acc;
  int pc = 0;  // the lane's piece: its samples only move forward in time, so the search continues where it stopped
  for (int base = 0; base < cnt; base += kAuditU * kWave) {
    double pos[kAuditU][D];
    bool on[kAuditU];
    typename LookupT::Addr ad[kAuditU];
#pragma unroll
    for (int u = 0; u < kAuditU; ++u) {
      const int k = base + u * kWave + lane;
      on[u] = k < cnt;
      const double tt = pt.time_of(k, step);
      pc = pt.seek(pc, tt);
      double vel[D], ac[D];
      pt.state(pc, tt, pos[u], vel, ac);
      ad[u] = lk.template prepare<D>(pos[u], on[u]);
      if (on[u]) acc.kinematics(pos[u], vel, ac, vmax2);
    }
    typename LookupT::Raw rw[kAuditU];
#pragma unroll
    for (int u = 0; u < kAuditU; ++u) rw[u] = lk.load(ad[u]);
#pragma unroll
    for (int u = 0; u < kAuditU; ++u) {
      double prev[D], gdrop[D];
      acc.neighbour(pos[u], prev);
      const double dk = lk.template finish<D>(ad[u], rw[u], gdrop);
      if (on[u]) acc.clearance(base + u * kWave + lane, pos[u], prev, dk, ad[u].inside, safe);
    }
  }
  acc.finish(b, cnt, pt.total, [&](int k) { return pt.time_of(k, step); }, w0, w1, w2, prm.coll_tol, audit, count, flags);
}

}  // namespace neo
