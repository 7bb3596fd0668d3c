// neo_plan.hpp -- BatchPlanner.plan's retry chain (warm_start_plan, traj_planner/expert_planner.py:186-203, for a
// batch) on RESIDENT arrays (include/neo_planner.h, neo_plan_*): what surrounds the optimiser launch of one attempt.
//
//   plan_guess_kernel   generate_init_variables (:82-101): the straight-line guess, with the re-seeded attempts' jitter
//                       added when the host hands it over, packed for one optimiser launch      one lane per request
//   plan_jitter_kernel  the re-seeded attempts' jitter drawn on the device (neo_counter_rng.hpp): the packed noise that
//                       plan_guess_kernel adds, from the request's own stream                     one lane per value
//   plan_merge_kernel   plan's bookkeeping over the launch's results: scatter to the request-indexed arrays, attempts,
//                       nit_total, failed / solved, the bad-scene word                     one wavefront per request
//   (batch_compact_kernel, neo_batch.hpp, then packs the failed requests: the next attempt's launch list)
// The merge serves the fixed chain and, group by group, the chain over mixed waypoint counts (neo_adaptive_merge_dev):
// the one difference is the row length of the request-indexed x.
//
// Included by neo_disp_plan.hip only.  fp64, D = 2 or 3.  Request-indexed arrays are indexed by request b; packed
// arrays by the request's position p in the launch list (neo_launch_list.hpp).  No atomics, no scratch.
#pragma once
#include "neo_counter_rng.hpp"
#include "neo_wave.hpp"
#include "neo_launch_list.hpp"

namespace neo {

constexpr int kPlanThreads = 256;  // guess: requests per workgroup

// small host arrays handed over by value: the fractions f[k] = (k + 1) / M of the M - 1 waypoints along the line and
// the shared tau (map_T2tau of init_T * [1.5, 1, ..., 1, 1.5]), both computed once on the host by NumPy
struct PlanFrac {
  double v[NEO_MAX_PIECES];
};
struct PlanTau {
  double v[NEO_MAX_PIECES];
};

// The waypoints are BatchPlanner.init_guess's, operation by operation (every one rounded on its own, nothing fused):
//   wp = start + (target - start) * f[k]        and, for a re-seeded attempt, wp = wp + noise
// `x_init` (request-indexed [B][n]) replaces all of that: the row is the caller's own start point, copied.
// `noise` is packed [P][D][M - 1]: the host draws it for the launch list in position order.
template <int D>
__global__ __launch_bounds__(kPlanThreads) void plan_guess_kernel(
    LaunchList list, int M, const double *__restrict__ head, const double *__restrict__ tail,
    const int *__restrict__ slots, const double *__restrict__ x_init, const double *__restrict__ noise, PlanFrac f,
    PlanTau tau, double *__restrict__ x0, double *__restrict__ head_k, double *__restrict__ tail_k,
    int *__restrict__ slots_k) {
#pragma clang fp contract(off)
  const int p = blockIdx.x * kPlanThreads + threadIdx.x;
  const int b = list.request(p);
  if (b < 0) return;
  const int count = M - 1, n = D * count + M;
  const double *hd = head + (size_t)b * 3 * D, *tl = tail + (size_t)b * 3 * D;
  pack_boundary<D>(head, tail, slots, b, head_k, tail_k, slots_k, (size_t)p);
  double *xr = x0 + (size_t)p * n;
  if (x_init) {
    const double *xi = x_init + (size_t)b * n;
    for (int i = 0; i < n; ++i) xr[i] = xi[i];
    return;
  }
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const double start = hd[d];
    const double span = tl[d] - start;
    for (int k = 0; k < count; ++k) {
      const double along = span * f.v[k];
      double y = start + along;
      if (noise) y = y + noise[((size_t)p * D + d) * count + k];
      xr[d * count + k] = y;
    }
  }
  for (int i = 0; i < M; ++i) xr[D * count + i] = tau.v[i];
}

// noise[p][d][k] = 0.5 * value d * count + k of the stream (seed, stream_ids[b], attempt, 0, domain 1), b the request at
// position p: BatchPlanner.retry_noise_counter's array for the launch list, bit for bit (the reference's N(0, 0.5), :94).
// `stream_ids` is request-indexed, or NULL: the request's index.  One lane per value; `per` = D * (M - 1) values a
// request.  The rows of a skipped position stay.
__global__ __launch_bounds__(kPlanThreads) void plan_jitter_kernel(LaunchList list, int per, unsigned long long seed,
                                                                   int attempt, const int *__restrict__ stream_ids,
                                                                   double *__restrict__ noise) {
#pragma clang fp contract(off)
  const size_t v = (size_t)blockIdx.x * kPlanThreads + threadIdx.x;
  const size_t p = v / (size_t)per;
  if (p >= (size_t)list.size()) return;
  const int b = list.request((int)p);
  if (b < 0) return;
  const uint32_t e = (uint32_t)(v - p * (size_t)per);
  const uint32_t id = (uint32_t)(stream_ids ? stream_ids[b] : b);
  const double z = counter_normal(seed, id, (uint32_t)attempt, 0u, kRngDomainRetry, e);
  noise[v] = 0.5 * z;
}

// One attempt's results, packed [P] rows, into the request-indexed arrays, with BatchPlanner.plan's bookkeeping:
//   attempts += 1 (`reset`: = 1, the chain's first attempt); nit_total += nit unless the run overflowed
//   ((status & 0xff) >= NEO_TRAJ_NUMERIC_RANGE: the reference raises before it counts such a run; `reset`: =);
//   failed = ((status & 0xff) > NEO_TRAJ_MAXITER and != NEO_TRAJ_BAD_SCENE) or NEO_TRAJ_FLAG_COLLISION; solved = !failed.
// The request-indexed x has rows of `ldx` >= n doubles: the row's n values, then NaN (a group of a mixed chain in rows
// of the longest group's length; ldx == n: no tail).
// `pending[p]` gets the request's index when it failed, -1 otherwise: batch_compact_kernel, or adaptive_compact_kernel
// over the groups' segments, packs it afterwards.
// `bad_scene` (zeroed before the chain's first launch) becomes 1 when a launched request ended with
// NEO_TRAJ_BAD_SCENE -- every wavefront that sees one stores the same 1.
__global__ __launch_bounds__(kWave) void plan_merge_kernel(
    LaunchList list, int n, int ldx, int reset, RunRowsIn packed, RunRows out, int *__restrict__ attempts,
    long long *__restrict__ nit_total, int *__restrict__ solved, int *__restrict__ pending, int *__restrict__ bad_scene) {
  const int p = blockIdx.x;
  const int lane = lane_id();
  const int b = list.request(p);  // wave-uniform
  if (b < 0) {
    if (lane == 0 && p < list.size()) pending[p] = -1;
    return;
  }
  const int st = packed.status[p], its = packed.nit[p];  // (wave-uniform loads, ahead of the scatter's stores)
  scatter_run_row(lane, n, ldx, packed, (size_t)p, out, b);
  double *xr = out.x + (size_t)b * ldx;
  for (int i = n + lane; i < ldx; i += kWave) xr[i] = __builtin_nan("");
  if (lane == 0) {
    const int code = st & 0xff;
    const bool failed = (code > NEO_TRAJ_MAXITER && code != NEO_TRAJ_BAD_SCENE) || (st & NEO_TRAJ_FLAG_COLLISION);
    const long long counted = code >= NEO_TRAJ_NUMERIC_RANGE ? 0 : its;
    attempts[b] = reset ? 1 : attempts[b] + 1;
    nit_total[b] = reset ? counted : nit_total[b] + counted;
    solved[b] = failed ? 0 : 1;
    pending[p] = failed ? b : -1;
    if (code == NEO_TRAJ_BAD_SCENE) *bad_scene = 1;
  }
}

}  // namespace neo
