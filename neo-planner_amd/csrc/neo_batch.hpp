// neo_batch.hpp -- the reference's `batch` planner mode (traj_planner/expert_planner.py:103-168) for P requests on
// RESIDENT arrays (include/neo_planner.h, neo_batch_*): K laterally shifted initial guesses per request packed for one
// optimiser launch of P * K trajectories, and the choice of the cheapest feasible one afterwards.
//
//   batch_candidates_kernel   batch_generate_init_variables (:103-140)          one lane per candidate row
//   batch_select_kernel       the feasibility test, the cost and np.argmin (:160-165, plan_once :233-237)
//                                                                                one wavefront per request
//   batch_compact_kernel      the requests without a feasible candidate as a compacted list   one workgroup
//
// Included by neo_disp_batch.hip only.  D = 2, fp64.  Request-indexed arrays (head, tail, slots and everything select
// writes) are indexed by request b; packed arrays by row p * K + k, p the request's position in the launch list
// (neo_launch_list.hpp).  No atomics: the order of the compacted list follows from the positions alone.
#pragma once
#include "neo_wave.hpp"
#include "neo_launch_list.hpp"

namespace neo {

constexpr int kBatchThreads = 256;   // candidates: rows per workgroup
constexpr int kBatchD = 2;
constexpr int kBatchMaxK = 8;        // candidates a request (include/neo_planner.h NEO_BATCH_MAX_CANDIDATES)
constexpr int kCompactThreads = 1024;

// small host arrays handed over by value: the shared tau (map_T2tau of the durations, computed once on the host), the
// signed lateral offsets and the cost weights
struct BatchTau {
  double v[NEO_MAX_PIECES];
};
struct BatchOffsets {
  double v[kBatchMaxK];
};
struct BatchWeights {
  double v[4];
};

// The waypoints are NumPy's, operation by operation (every one rounded on its own):
//   stride = (target - start) / (count + 1)
//   np.linspace(start + stride, target, count, endpoint=False): first = start + stride, delta = target - first,
//     step = delta / count, row j = j * step + first -- or, when step == 0 in ANY dimension (linspace's denormal branch,
//     taken for the whole array), row j = (j / count) * delta + first;
//   forward = (target - start) / np.linalg.norm(target - start).  The norm of a 2-vector is sqrt(x.dot(x)), and the dot
//     product is BLAS ddot: OpenBLAS accumulates dot += x[i] * y[i] with a fused multiply-add on every x86-64 kernel
//     with FMA3, so the sum of squares is fma(dy, dy, round(dx * dx)).  (Checked on the CPU against np.linalg.norm for
//     20 000 random vectors: equal in all of them; the two separately rounded squares differ in 8 %.)
//   lateral_dir = [[fy, -fx], [-fy, fx]]; candidate k adds off[k] * lateral_dir[0] -- the reference's
//     0.6 * lateral_dir[(k - 1) % 2] is off = +0.6, -0.6, +0.6, ...: lateral_dir[1] is the exact negative of
//     lateral_dir[0].  An offset of exactly 0 adds nothing (candidate 0 stays finite where start == target makes the
//     direction 0 / 0 = NaN, as in the reference).
__global__ __launch_bounds__(kBatchThreads) void batch_candidates_kernel(
    LaunchList list, int M, int K, const double *__restrict__ head, const double *__restrict__ tail,
    const int *__restrict__ slots, BatchTau tau, BatchOffsets off, double *__restrict__ x0, double *__restrict__ head_k,
    double *__restrict__ tail_k, int *__restrict__ slots_k) {
#pragma clang fp contract(off)
  constexpr int D = kBatchD;
  const int row = blockIdx.x * kBatchThreads + threadIdx.x;
  const int p = row / K, k = row - p * K;
  const int b = list.request(p);  // (a row beyond the last position's gives p >= list.n)
  if (b < 0) return;
  const int count = M - 1, n = D * count + M;
  const double *hd = head + (size_t)b * 3 * D, *tl = tail + (size_t)b * 3 * D;
  pack_boundary<D>(head, tail, slots, b, head_k, tail_k, slots_k, (size_t)row);
  double first[D], delta[D], step[D], lat[D];
  const double dx = tl[0] - hd[0], dy = tl[1] - hd[1];
  const double dd[D] = {dx, dy};
  bool any_zero = false;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const double stride = dd[d] / (double)(count + 1);
    first[d] = hd[d] + stride;
    delta[d] = tl[d] - first[d];
    step[d] = delta[d] / (double)count;
    any_zero = any_zero || step[d] == 0.0;
  }
  const double xx = dx * dx;
  const double norm = sqrt(__builtin_fma(dy, dy, xx));
  const double fx = dx / norm, fy = dy / norm;
  lat[0] = fy;
  lat[1] = -fx;
  const double o = off.v[k];
  double *xr = x0 + (size_t)row * n;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const double shift = o * lat[d];
    for (int j = 0; j < count; ++j) {
      double y;
      if (any_zero) {
        const double f = (double)j / (double)count;
        y = f * delta[d];
      } else {
        y = (double)j * step[d];
      }
      y = y + first[d];
      if (o != 0.0) y = y + shift;
      xr[d * count + j] = y;
    }
  }
  for (int i = 0; i < M; ++i) xr[D * count + i] = tau.v[i];
}

// Candidate k of a request is FEASIBLE when its run ended with an answer the reference keeps: (status & 0xff) <=
// NEO_TRAJ_MAXITER and neither NEO_TRAJ_FLAG_COLLISION nor NEO_TRAJ_BAD_SCENE -- the complement of `failed` in
// BatchPlanner.plan.  Its cost is (costs4_last * w).sum(), +inf when it is not feasible.  NumPy sums four contiguous
// doubles from left to right, ((p0 + p1) + p2) + p3 with p_i = c_i * w_i rounded first (its pairwise summation adds
// fewer than eight elements in one plain loop; checked on the CPU against (c * w).sum() and (c * w).sum(axis=1) for
// 200 000 random rows: equal in all of them, the pairwise order (p0 + p1) + (p2 + p3) differs in 22 %).
// chosen = np.argmin(cost), the first index of the minimum; -1 when the minimum is +inf (no feasible candidate) or NaN
// (np.min(cost) < np.inf is false then, and the reference falls back).
// `pending[p]` gets the request's index when chosen is -1, -1 otherwise: batch_compact_kernel packs it afterwards.
__global__ __launch_bounds__(kWave) void batch_select_kernel(
    LaunchList list, int n, int K, RunRowsIn packed, BatchWeights w, int *__restrict__ chosen,
    double *__restrict__ cand_cost, int *__restrict__ solved, RunRows out, int *__restrict__ nit_total,
    int *__restrict__ opt_runs, int *__restrict__ pending) {
#pragma clang fp contract(off)
  const int p = blockIdx.x;
  const int lane = lane_id();
  const int b = list.request(p);  // wave-uniform
  if (b < 0) {
    if (lane == 0 && p < list.size()) pending[p] = -1;
    return;
  }
  // every lane walks the K <= 8 candidates: the same loads and the same result in all of them
  double best = __builtin_inf();
  int pick = -1, runs = 0, its = 0;
  bool nan = false;
  for (int k = 0; k < K; ++k) {
    const size_t row = (size_t)p * K + k;
    const int st = packed.status[row];
    const int code = st & 0xff;
    const bool feasible = code <= NEO_TRAJ_MAXITER && !(st & NEO_TRAJ_FLAG_COLLISION);  // (BAD_SCENE is > MAXITER)
    double cost = __builtin_inf();
    if (feasible) {
      const double *c = packed.costs4_last + row * 4;
      const double p0 = c[0] * w.v[0], p1 = c[1] * w.v[1], p2 = c[2] * w.v[2], p3 = c[3] * w.v[3];
      const double s01 = p0 + p1;
      const double s012 = s01 + p2;
      cost = s012 + p3;
    }
    if (lane == 0) cand_cost[(size_t)b * K + k] = cost;
    if (cost != cost) nan = true;
    if (cost < best) {
      best = cost;
      pick = k;
    }
    if (code < NEO_TRAJ_NUMERIC_RANGE) {  // an overflowed run raises before the reference counts it
      its += packed.nit[row];
      ++runs;
    }
  }
  if (nan) pick = -1;
  if (lane == 0) {
    chosen[b] = pick;
    solved[b] = pick >= 0;
    nit_total[b] = its;
    opt_runs[b] = runs;
    pending[p] = pick >= 0 ? -1 : b;
  }
  if (pick < 0) return;  // x[b] and the other results of the request stay untouched
  scatter_run_row(lane, n, n, packed, (size_t)p * K + pick, out, b);
}

// pending[P] (a request index, or -1) -> its entries >= 0 packed to the front in the order of their positions, and
// their number.  ONE workgroup walks the array in chunks of kCompactThreads: compact_in_place (neo_launch_list.hpp).
// With an ascending subset (or none) the list is ascending.
__global__ __launch_bounds__(kCompactThreads) void batch_compact_kernel(int P, int *__restrict__ pending,
                                                                        int *__restrict__ n_pending) {
  const int kept = compact_in_place<kCompactThreads>(pending, P);
  if (threadIdx.x == 0) *n_pending = kept;
}

}  // namespace neo
