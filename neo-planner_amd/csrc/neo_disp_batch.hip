// neo_disp_batch.hip -- the `batch` planner mode on resident arrays (neo_batch.hpp): the K lateral candidates of P
// requests packed for one optimiser launch, and the choice among its P * K results with the compacted list of the
// requests that need the host's retries (traj_planner/expert_planner.py:103-168).  D = 2: one instantiation each.
#include "neo_host.hpp"
#include "neo_batch.hpp"

namespace neo {

int batch_candidates(neo_ctx *c, const LaunchList &l, const BatchCandArgs &a) {
  BatchTau tau{};
  BatchOffsets off{};
  for (int i = 0; i < a.M; ++i) tau.v[i] = a.tau[i];
  for (int k = 0; k < a.K; ++k) off.v[k] = a.off[k];
  const long long rows = (long long)l.n * a.K;
  hipLaunchKernelGGL(batch_candidates_kernel, dim3((unsigned)((rows + kBatchThreads - 1) / kBatchThreads)),
                     dim3(kBatchThreads), 0, c->stream, l, a.M, a.K, a.head, a.tail, a.slots, tau, off, a.x0, a.head_k, a.tail_k,
                     a.slots_k);
  return NEO_OK;
}

int batch_select(neo_ctx *c, const LaunchList &l, const BatchSelectArgs &a) {
  BatchWeights w{};
  for (int i = 0; i < 4; ++i) w.v[i] = a.w[i];
  hipLaunchKernelGGL(batch_select_kernel, dim3(l.n), dim3(kWave), 0, c->stream, l, a.n, a.K, a.packed, w, a.chosen,
                     a.cand_cost, a.solved, a.out, a.nit_total, a.opt_runs, a.fallback);
  return batch_compact(c, l.n, a.fallback, a.n_fallback);
}

int batch_compact(neo_ctx *c, int P, int *pending, int *n_pending) {
  hipLaunchKernelGGL(batch_compact_kernel, dim3(1), dim3(kCompactThreads), 0, c->stream, P, pending, n_pending);
  return NEO_OK;
}

}  // namespace neo
