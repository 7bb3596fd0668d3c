// neo_disp_plan.hip -- BatchPlanner.plan's retry chain on resident arrays (neo_plan.hpp): the guess of one attempt
// packed for the optimiser launch, and the merge of its results with the compacted list of the requests to launch
// again (traj_planner/expert_planner.py:186-203).  The compaction is the batch unit's (batch_compact); the chain over
// mixed waypoint counts merges group by group through the same launcher and compacts on its own (neo_disp_adaptive.hip).
#include "neo_host.hpp"
#include "neo_plan.hpp"

namespace neo {

int plan_guess(neo_ctx *c, const LaunchList &l, int D, const PlanGuessArgs &a) {
  PlanFrac frac{};
  PlanTau tau{};
  if (!a.x_init) {
    for (int k = 0; k < a.M - 1; ++k) frac.v[k] = a.frac[k];
    for (int i = 0; i < a.M; ++i) tau.v[i] = a.tau[i];
  }
  const dim3 grid((unsigned)((l.n + kPlanThreads - 1) / kPlanThreads)), block(kPlanThreads);
  if (D == 2)
    hipLaunchKernelGGL(plan_guess_kernel<2>, grid, block, 0, c->stream, l, a.M, a.head, a.tail, a.slots, a.x_init,
                       a.noise, frac, tau, a.x0, a.head_k, a.tail_k, a.slots_k);
  else
    hipLaunchKernelGGL(plan_guess_kernel<3>, grid, block, 0, c->stream, l, a.M, a.head, a.tail, a.slots, a.x_init,
                       a.noise, frac, tau, a.x0, a.head_k, a.tail_k, a.slots_k);
  return NEO_OK;
}

int plan_jitter(neo_ctx *c, const LaunchList &l, int M, int D, uint64_t seed, int attempt, const int *stream_ids,
                double *noise) {
  const int per = D * (M - 1);
  const size_t values = (size_t)l.n * per;
  hipLaunchKernelGGL(plan_jitter_kernel, dim3((unsigned)((values + kPlanThreads - 1) / kPlanThreads)), dim3(kPlanThreads), 0,
                     c->stream, l, per, (unsigned long long)seed, attempt, stream_ids, noise);
  return NEO_OK;
}

int plan_merge(neo_ctx *c, const LaunchList &l, const PlanMergeArgs &a) {
  hipLaunchKernelGGL(plan_merge_kernel, dim3(l.n), dim3(kWave), 0, c->stream, l, a.n, a.ldx, a.reset, a.packed, a.out,
                     a.attempts, a.nit_total, a.solved, a.failed, a.bad_scene);
  return a.n_failed ? batch_compact(c, l.n, a.failed, a.n_failed) : NEO_OK;
}

}  // namespace neo
