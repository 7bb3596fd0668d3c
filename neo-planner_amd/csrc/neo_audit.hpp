// neo_audit.hpp -- audit_kernel: the reference's flight metric (ros_node/traj_planner_node.py:333-363,
// get_weighted_metric) for a batch of planned trajectories under perfect tracking (include/neo_planner.h,
// neo_audit_traj_batch).  Included by neo_disp_audit.hip only.
//
// One wavefront per trajectory, as traj_state_kernel: the fp64 solve (minco_forward), the coefficients and the
// sequential prefix sums of the durations in LDS, then the lanes stride over the samples -- kAuditU samples a lane per
// round, whose map gathers are all in flight before the first is consumed (the lookups' prepare / load / finish split).
// Every lane accumulates its own samples k = lane, lane + 64, ... in increasing order; at the end fixed-order DPP
// reductions combine the lanes (wave_sum4 for the three sums, wave_max_nonneg for the maxima and flags, wave_min_first
// below for the minimum and its sample).  The association order depends on neither kAuditU nor the grid: same bits.
#pragma once
#include <climits>
#include "neo_kernels.hpp"

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

// position, velocity and acceleration of piece pc at local time T: the expressions of traj_state_kernel (neo_abi.hip),
// written out again rather than shared, so that traj_state_kernel's code stays exactly as it is.  Compiled with the
// units' -ffp-contract=on (no pragma here): the same fused multiply-adds, the same bits as its rows.
template <int D>
__device__ __forceinline__ void audit_sample_state(const double *cs, int pc, double T, double (&p)[D], double (&v)[D],
                                                   double (&a)[D]) {
  const double T2 = T * T, T3 = T2 * T, T4 = T2 * T2, T5 = T4 * T;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const double c0 = cs[(pc * 6 + 0) * D + d], c1 = cs[(pc * 6 + 1) * D + d], c2 = cs[(pc * 6 + 2) * D + d];
    const double c3 = cs[(pc * 6 + 3) * D + d], c4 = cs[(pc * 6 + 4) * D + d], c5 = cs[(pc * 6 + 5) * D + d];
    p[d] = c0 + c1 * T + c2 * T2 + c3 * T3 + c4 * T4 + c5 * T5;
    v[d] = c1 + 2.0 * c2 * T + 3.0 * c3 * T2 + 4.0 * c4 * T3 + 5.0 * c5 * T4;
    a[d] = 2.0 * c2 + 6.0 * c3 * T + 12.0 * c4 * T2 + 20.0 * c5 * T3;
  }
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
  __shared__ double xs[kSlots * kWave];
  __shared__ double cs[kWave * 6 * D];
  __shared__ double tcum[kWave + 1];
  const int b = blockIdx.x;
  if (b >= B) return;
  const int lane = lane_id();
  double *rec = audit + (size_t)b * NEO_AUDIT_FIELDS;
  // no usable trajectory (a slot outside the table, a failed solve, a state that is not finite): NaN record, no samples
  auto reject = [&]() {
    if (lane < NEO_AUDIT_FIELDS) rec[lane] = __builtin_nan("");
    if (lane == 0) {
      count[b] = 0;
      flags[b] = NEO_AUDIT_FLAG_NONFINITE;
    }
  };
  const int slot = scene_slot ? scene_slot[b] : 0;
  if (slot < 0 || slot >= nmaps) return reject();
  const MapT map = maps[slot];

  // the solve and the piece table: traj_state_kernel's
  struct NoMap {};
  struct NoLookup {
    __device__ explicit NoLookup(const NoMap &) {}
  };
  DevParams p = prm;
  NoMap nm;
  DevBackend<D, kSlots, double, NoMap, NoLookup> be(p, nm);
  be.xs = xs;
  be.hist = nullptr;
  be.m = NEO_LBFGS_M;
  be.coeff_out = nullptr;
  load_boundary(be.t, head + (size_t)b * 3 * D, tail + (size_t)b * 3 * D, M);
  const int n = be.t.n;
  typename DevBackend<D, kSlots, double, NoMap, NoLookup>::Vec xv;
#pragma unroll
  for (int k = 0; k < kSlots; ++k) xv.v[k] = (k * kWave + lane < n) ? x[(size_t)b * n + k * kWave + lane] : 0.0;
  be.scatter_x(xv);
  double e, ts;
  if (minco_forward<D>(be.t, p, e, ts) != 0) return reject();
  if (lane < M) {
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
      for (int d = 0; d < D; ++d) cs[(lane * 6 + k) * D + d] = be.t.c[k][d];
  }
  // sequential prefix sums like Python's sum(ts[:k]) (traj_utils.py:98-101)
  if (lane == 0) tcum[0] = 0.0;
  for (int pce = 0; pce < M; ++pce) {
    const double Tp = rdlane(be.t.T, pce);
    if (lane == 0) tcum[pce + 1] = tcum[pce] + Tp;
  }
  __syncthreads();
  const double total = tcum[M];
  const double step = 1.0 / hz;
  const double cnt_d = ceil(total / step);  // len(np.arange(0, total, 1/hz))
  if (!(cnt_d >= 0.0 && cnt_d <= (double)(1 << 30))) return reject();  // a duration that is not finite
  const int cnt = (int)cnt_d;

  LookupT lk(map);
  const double vmax2 = prm.v_max * prm.v_max, safe = prm.safe_dis;
  double path = 0.0, feas = 0.0, coll = 0.0, speed_max = 0.0, acc_max = 0.0, dmin = __builtin_inf();
  int kmin = INT_MAX, kunsafe = -1, outside = 0, bad = 0;
  double carry[D];  // position of the sample before this sub-round's lane 0 (lane 63 of the one before)
#pragma unroll
  for (int d = 0; d < D; ++d) carry[d] = 0.0;
  int pc = 0;  // the lane's piece: its samples only move forward in time, so the search continues where it stopped
  for (int base = 0; base < cnt; base += kAuditU * kWave) {
    double pos[kAuditU][D];
    bool on[kAuditU];
    typename LookupT::Addr ad[kAuditU];
#pragma unroll
    for (int u = 0; u < kAuditU; ++u) {
      const int k = base + u * kWave + lane;
      on[u] = k < cnt;
      double tt = (double)k * step;
      if (tt > total) tt = total;
      while (pc < M - 1 && tcum[pc + 1] < tt) ++pc;
      double vel[D], acc[D];
      audit_sample_state<D>(cs, pc, tt - tcum[pc], pos[u], vel, acc);
      ad[u] = lk.template prepare<D>(pos[u], on[u]);
      if (on[u]) {
        const double v2 = audit_norm2<D>(vel), a2 = audit_norm2<D>(acc);
#pragma unroll
        for (int d = 0; d < D; ++d)
          if (!__builtin_isfinite(pos[u][d]) || !__builtin_isfinite(vel[d]) || !__builtin_isfinite(acc[d])) bad = 1;
        const double speed = sqrt(v2), accn = sqrt(a2);
        speed_max = speed > speed_max ? speed : speed_max;
        acc_max = accn > acc_max ? accn : acc_max;
        const double vv = v2 - vmax2;  // :346-348
        if (vv > 0.0) feas += vv * vv * vv;
      }
    }
    typename LookupT::Raw rw[kAuditU];
#pragma unroll
    for (int u = 0; u < kAuditU; ++u) rw[u] = lk.load(ad[u]);
#pragma unroll
    for (int u = 0; u < kAuditU; ++u) {
      const int k = base + u * kWave + lane;
      double prev[D];
#pragma unroll
      for (int d = 0; d < D; ++d) {
        prev[d] = from_prev(pos[u][d], carry[d]);
        carry[d] = rdlane(pos[u][d], kWave - 1);
      }
      double gdrop[D];
      const double dk = lk.template finish<D>(ad[u], rw[u], gdrop);
      if (on[u]) {
        if (k >= 1) {  // :341-343
          double dp[D];
#pragma unroll
          for (int d = 0; d < D; ++d) dp[d] = pos[u][d] - prev[d];
          path += sqrt(audit_norm2<D>(dp));
        }
        const double vd = safe - dk;  // :351-355
        if (vd > 0.0) {
          coll += vd * vd * vd;
          if (kunsafe < 0) kunsafe = k;
        }
        if (dk < dmin) {
          dmin = dk;
          kmin = k;
        }
        if (!ad[u].inside) outside = 1;
      }
    }
  }
  if (wave_max_nonneg(bad)) return reject();
  double s_path, s_feas, s_coll, s_unused;
  wave_sum4(path, feas, coll, 0.0, s_path, s_feas, s_coll, s_unused);
  const double vmx = wave_max_nonneg(speed_max), amx = wave_max_nonneg(acc_max);
  wave_min_first(dmin, kmin);
  const int ukey = wave_max_nonneg(kunsafe >= 0 ? INT_MAX - kunsafe : 0);  // largest key = earliest unsafe sample
  const int outs = wave_max_nonneg(outside);
  if (lane == 0) {
    auto t_of = [&](int k) {
      const double tt = (double)k * step;
      return tt > total ? total : tt;
    };
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
    rec[NEO_AUDIT_DURATION] = total;
    count[b] = cnt;
    flags[b] = (ukey > 0 ? NEO_AUDIT_FLAG_UNSAFE : 0) | (weighted > 10.0 * prm.coll_tol ? NEO_AUDIT_FLAG_METRIC_FAIL : 0) |
               (outs ? NEO_AUDIT_FLAG_OUTSIDE_MAP : 0);
  }
}

}  // namespace neo
