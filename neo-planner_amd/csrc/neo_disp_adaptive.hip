// neo_disp_adaptive.hip -- adaptive waypoint counts on resident arrays (neo_adaptive.hpp): every request's count, the
// launch list grouped by count, and the segmented compaction of BatchPlanner.plan's retry chain over the groups
// (traj_planner/expert_planner.py:86-88, :186-203).  A group's merge is the plan unit's (plan_merge, neo_disp_plan.hip).
#include "neo_host.hpp"
#include "neo_adaptive.hpp"

namespace neo {

int adaptive_count(neo_ctx *c, const LaunchList &l, int D, const double *head, const double *tail, double seg_len,
                   int max_waypoints, int *counts, int *clamped) {
  const dim3 grid((unsigned)((l.n + kAdaptiveThreads - 1) / kAdaptiveThreads)), block(kAdaptiveThreads);
  if (D == 2)
    hipLaunchKernelGGL(adaptive_count_kernel<2>, grid, block, 0, c->stream, l, head, tail, seg_len, max_waypoints, counts,
                       clamped);
  else
    hipLaunchKernelGGL(adaptive_count_kernel<3>, grid, block, 0, c->stream, l, head, tail, seg_len, max_waypoints, counts,
                       clamped);
  return NEO_OK;
}

int adaptive_bucket(neo_ctx *c, const LaunchList &l, const int *counts, int *order, int *bucket_begin, int *total) {
  hipLaunchKernelGGL(adaptive_bucket_kernel, dim3(1), dim3(kBucketThreads), 0, c->stream, l, counts, order, bucket_begin,
                     total);
  return NEO_OK;
}

int adaptive_compact(neo_ctx *c, const int *seg_begin, const int *seg_len, int *pending, int *n_failed) {
  AdaptiveSegs segs{};
  for (int g = 0; g < kBuckets; ++g) {
    segs.begin[g] = seg_begin[g];
    segs.len[g] = seg_len[g];
  }
  hipLaunchKernelGGL(adaptive_compact_kernel, dim3(kBuckets), dim3(kAdaptiveThreads), 0, c->stream, segs, pending, n_failed);
  return NEO_OK;
}

}  // namespace neo
