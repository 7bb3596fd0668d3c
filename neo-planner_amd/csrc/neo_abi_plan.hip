// neo_abi_plan.hip -- C ABI of libneo_planner_hip.so (include/neo_planner.h), the unit of the batch planner on resident
// arrays: the lateral candidates and their selection, the plan retry chain (guess, jitter, merge) and the adaptive
// waypoint counts (count, bucket, merge, compact).  Argument checks here, the skeletons in neo_abi_util.hpp, the kernels
// behind the launchers of neo_disp_batch.hip, neo_disp_plan.hip and neo_disp_adaptive.hip.
#include "neo_abi_util.hpp"

using namespace neo;
using namespace neo::abi;

extern "C" {

// ---- the `batch` planner mode on resident arrays (traj_planner/expert_planner.py:103-168; kernels: neo_batch.hpp)
static const double kBatchOffset = 0.6;  // :135
static int batch_check(neo_ctx *c, const char *who, int B, const int32_t *subset, int n_subset, int M, int D, int K) {
  int rc = list_check(c, "fleet", B, 0, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  if (D != 2) return fail_locked(c, NEO_ERR_INVALID, (std::string(who) + ": D must be 2 (the reference's lateral candidates are 2-D)").c_str());
  if (K < 1 || K > NEO_BATCH_MAX_CANDIDATES)
    return fail_locked(c, NEO_ERR_INVALID, (std::string(who) + ": K must be in 1 .. 8").c_str());
  rc = check_shape(c, B, M, D);
  if (rc) return rc;
  if (M < 2) return fail_locked(c, NEO_ERR_INVALID, (std::string(who) + ": M must be >= 2 (at least one waypoint)").c_str());
  if ((long long)launch_list(B, subset, n_subset).n * K > (long long)INT32_MAX)
    return fail_locked(c, NEO_ERR_INVALID, (std::string(who) + ": more than 2^31 - 1 candidate rows").c_str());
  return NEO_OK;
}
// the reference's offsets 0, +0.6, -0.6, +0.6, ... (lateral_dir[(k - 1) % 2], :131-137)
static void batch_default_offsets(int K, double *off) {
  for (int k = 0; k < K; ++k) off[k] = k == 0 ? 0.0 : (k % 2 ? kBatchOffset : -kBatchOffset);
}

int neo_batch_candidates_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, int K, const double *head,
                             const double *tail, const int32_t *slots, const double *tau, const double *lateral_offsets,
                             double *x0, double *head_k, double *tail_k, int32_t *slots_k) {
  int rc = batch_check(c, "batch candidates", B, subset, n_subset, M, D, K);
  if (rc) return rc;
  if ((rc = null_check(c, "batch candidates: null buffer", {head, tail, tau, x0, head_k, tail_k}))) return rc;
  return list_launch(c, B, subset, n_subset, [&](const LaunchList &list) {
    double off[NEO_BATCH_MAX_CANDIDATES];
    batch_default_offsets(K, off);
    if (lateral_offsets)
      for (int k = 0; k < K; ++k) off[k] = lateral_offsets[k];
    return batch_candidates(c, list, {M, K, head, tail, slots, tau, off, x0, head_k, tail_k, slots_k});
  });
}

int neo_batch_candidates(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, int K, const double *head,
                         const double *tail, const int32_t *slots, const double *tau, const double *lateral_offsets,
                         double *x0, double *head_k, double *tail_k, int32_t *slots_k) {
  int rc = batch_check(c, "batch candidates", B, subset, n_subset, M, D, K);
  if (rc) return rc;
  if ((rc = null_check(c, "batch candidates: null buffer", {head, tail, tau, x0, head_k, tail_k}))) return rc;
  const size_t bs = (size_t)B, rows = (size_t)launch_list(B, subset, n_subset).n * K, n = (size_t)D * (M - 1) + M;
  if (rows == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  // the packed outputs go up too: the rows of a skipped index come back as they were
  HostStage st(c, kStagedUpTo);
  const auto fh = st.in(head, bs * 6), ft = st.in(tail, bs * 6);
  const auto fs = st.in_optional(slots, bs), fsub = st.in_optional(subset, (size_t)n_subset);
  const auto fx = st.inout(x0, rows * n), fhk = st.inout(head_k, rows * 6), ftk = st.inout(tail_k, rows * 6);
  const auto fsk = st.inout_optional(slots_k, rows);
  return st.run([&] {
    return neo_batch_candidates_dev(c, B, st.dev(fsub), n_subset, M, D, K, st.dev(fh), st.dev(ft), st.dev(fs), tau,
                                    lateral_offsets, st.dev(fx), st.dev(fhk), st.dev(ftk), st.dev(fsk));
  });
}

static int batch_select_check(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, const BatchSelectArgs &a) {
  int rc = batch_check(c, "batch select", B, subset, n_subset, M, D, a.K);
  if (rc) return rc;
  const RunRowsIn &k = a.packed;
  const RunRows &o = a.out;
  rc = null_check(c, "batch select: null buffer",
                  {k.x, k.costs4, k.costs4_last, k.nit, k.status, a.chosen, a.cand_cost, a.solved, o.x, o.costs4, o.costs4_last,
                   o.status, a.nit_total, a.opt_runs, a.fallback, a.n_fallback});
  if (rc) return rc;
  if (o.nfev && !k.nfev) return fail_locked(c, NEO_ERR_INVALID, "batch select: nfev without nfev_k");
  return NEO_OK;
}

int neo_batch_select_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, int K, const double *x_k,
                         const double *costs4_k, const double *costs4_last_k, const int32_t *nit_k, const int32_t *nfev_k,
                         const int32_t *status_k, const double *weights4, int32_t *chosen, double *cand_cost,
                         int32_t *solved, double *x, double *costs4, double *costs4_last, int32_t *nit, int32_t *nfev,
                         int32_t *status, int32_t *nit_total, int32_t *opt_runs, int32_t *fallback, int32_t *n_fallback) {
  BatchSelectArgs a{D * (M - 1) + M, K, {x_k, costs4_k, costs4_last_k, nit_k, nfev_k, status_k}, weights4, chosen, cand_cost,
                    solved, {x, costs4, costs4_last, nit, nfev, status}, nit_total, opt_runs, fallback, n_fallback};
  int rc = batch_select_check(c, B, subset, n_subset, M, D, a);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  if (list.n == 0) {
    HIPCHK(c, hipMemsetAsync(n_fallback, 0, sizeof(int32_t), c->stream));
    return NEO_OK;
  }
  if (!a.w) a.w = c->params.weights;
  return launched(c, batch_select(c, list, a));
}

int neo_batch_select(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, int K, const double *x_k,
                     const double *costs4_k, const double *costs4_last_k, const int32_t *nit_k, const int32_t *nfev_k,
                     const int32_t *status_k, const double *weights4, int32_t *chosen, double *cand_cost, int32_t *solved,
                     double *x, double *costs4, double *costs4_last, int32_t *nit, int32_t *nfev, int32_t *status,
                     int32_t *nit_total, int32_t *opt_runs, int32_t *fallback, int32_t *n_fallback) {
  const BatchSelectArgs a{D * (M - 1) + M, K, {x_k, costs4_k, costs4_last_k, nit_k, nfev_k, status_k}, weights4, chosen,
                          cand_cost, solved, {x, costs4, costs4_last, nit, nfev, status}, nit_total, opt_runs, fallback,
                          n_fallback};
  int rc = batch_select_check(c, B, subset, n_subset, M, D, a);
  if (rc) return rc;
  const size_t bs = (size_t)B, P = (size_t)launch_list(B, subset, n_subset).n;
  if (P == 0) {
    *n_fallback = 0;
    return NEO_OK;
  }
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  // the request-indexed outputs go up too: requests outside the subset, and x of a request without a choice, stay
  HostStage st(c, kStagedUpTo);
  const RowRefs fk = stage_rows_in(st, a.packed, P * K, (size_t)a.n);
  const auto fsub = st.in_optional(subset, (size_t)n_subset);
  const auto och = st.inout(chosen, bs);
  const auto occ = st.inout(cand_cost, bs * K);
  const auto oso = st.inout(solved, bs);
  const RowRefs fo = stage_rows_inout(st, a.out, bs, (size_t)a.n);
  const auto ont = st.inout(nit_total, bs), oru = st.inout(opt_runs, bs);
  // (the whole list comes back; its entries from n_fallback on are scratch)
  const auto ofb = st.out(fallback, P), onb = st.out(n_fallback, 1);
  return st.run([&] {
    const RunRowsIn k = as_const(staged_rows(st, fk));
    const RunRows o = staged_rows(st, fo);
    return neo_batch_select_dev(c, B, st.dev(fsub), n_subset, M, D, K, k.x, k.costs4, k.costs4_last, k.nit, k.nfev, k.status,
                                weights4, st.dev(och), st.dev(occ), st.dev(oso), o.x, o.costs4, o.costs4_last, o.nit, o.nfev,
                                o.status, st.dev(ont), st.dev(oru), st.dev(ofb), st.dev(onb));
  });
}

// ---- BatchPlanner.plan's retry chain on resident arrays (traj_planner/expert_planner.py:186-203; kernels: neo_plan.hpp)
static int plan_check(neo_ctx *c, const char *who, int B, const int32_t *subset, int n_subset, int M, int D) {
  int rc = list_check(c, "fleet", B, 0, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  rc = check_shape(c, B, M, D);
  if (rc) return rc;
  if (M < 2) return fail_locked(c, NEO_ERR_INVALID, (std::string(who) + ": M must be >= 2 (at least one waypoint)").c_str());
  return NEO_OK;
}

static int plan_guess_check(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, const void *head,
                            const void *tail, const void *x_init, const void *frac, const void *tau, const void *x0,
                            const void *head_k, const void *tail_k) {
  int rc = plan_check(c, "plan guess", B, subset, n_subset, M, D);
  if (rc) return rc;
  if ((rc = null_check(c, "plan guess: null buffer", {head, tail, x0, head_k, tail_k}))) return rc;
  if (!x_init && (!frac || !tau)) return fail_locked(c, NEO_ERR_INVALID, "plan guess: frac and tau are needed without x_init");
  return NEO_OK;
}

int neo_plan_guess_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, const double *head,
                       const double *tail, const int32_t *slots, const double *x_init, const double *noise,
                       const double *frac, const double *tau, double *x0, double *head_k, double *tail_k,
                       int32_t *slots_k) {
  int rc = plan_guess_check(c, B, subset, n_subset, M, D, head, tail, x_init, frac, tau, x0, head_k, tail_k);
  if (rc) return rc;
  return list_launch(c, B, subset, n_subset, [&](const LaunchList &list) {
    return plan_guess(c, list, D, {M, head, tail, slots, x_init, noise, frac, tau, x0, head_k, tail_k, slots_k});
  });
}

int neo_plan_guess(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, const double *head,
                   const double *tail, const int32_t *slots, const double *x_init, const double *noise, const double *frac,
                   const double *tau, double *x0, double *head_k, double *tail_k, int32_t *slots_k) {
  int rc = plan_guess_check(c, B, subset, n_subset, M, D, head, tail, x_init, frac, tau, x0, head_k, tail_k);
  if (rc) return rc;
  const size_t bs = (size_t)B, P = (size_t)launch_list(B, subset, n_subset).n, n = (size_t)D * (M - 1) + M, hd = (size_t)3 * D;
  if (P == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  // the packed outputs go up too: the rows of a skipped index come back as they were
  HostStage st(c, kStagedUpTo);
  const auto fh = st.in(head, bs * hd), ft = st.in(tail, bs * hd);
  const auto fs = st.in_optional(slots, bs), fsub = st.in_optional(subset, (size_t)n_subset);
  const auto fxi = st.in_optional(x_init, bs * n), fno = st.in_optional(noise, P * (size_t)D * (M - 1));
  const auto fx = st.inout(x0, P * n), fhk = st.inout(head_k, P * hd), ftk = st.inout(tail_k, P * hd);
  const auto fsk = st.inout_optional(slots_k, P);
  return st.run([&] {
    return neo_plan_guess_dev(c, B, st.dev(fsub), n_subset, M, D, st.dev(fh), st.dev(ft), st.dev(fs), st.dev(fxi),
                              st.dev(fno), frac, tau, st.dev(fx), st.dev(fhk), st.dev(ftk), st.dev(fsk));
  });
}

static int plan_jitter_check(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, int attempt,
                             const double *noise) {
  int rc = plan_check(c, "plan jitter", B, subset, n_subset, M, D);
  if (rc) return rc;
  if ((rc = null_check(c, "plan jitter: null buffer", {noise}))) return rc;
  if (attempt < 0) return fail_locked(c, NEO_ERR_INVALID, "plan jitter: attempt must be >= 0");
  return NEO_OK;
}

int neo_plan_jitter_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, uint64_t seed, int attempt,
                        const int32_t *stream_ids, double *noise) {
  int rc = plan_jitter_check(c, B, subset, n_subset, M, D, attempt, noise);
  if (rc) return rc;
  return list_launch(c, B, subset, n_subset, [&](const LaunchList &list) {
    return plan_jitter(c, list, M, D, seed, attempt, stream_ids, noise);
  });
}

int neo_plan_jitter(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, uint64_t seed, int attempt,
                    const int32_t *stream_ids, double *noise) {
  int rc = plan_jitter_check(c, B, subset, n_subset, M, D, attempt, noise);
  if (rc) return rc;
  const size_t bs = (size_t)B, P = (size_t)launch_list(B, subset, n_subset).n;
  if (P == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  // the packed rows go up too: the rows of a skipped index come back as they were
  HostStage st(c, kStagedUpTo);
  const auto fi = st.in_optional(stream_ids, bs), fsub = st.in_optional(subset, (size_t)n_subset);
  const auto fno = st.inout(noise, P * (size_t)D * (M - 1));
  return st.run([&] { return neo_plan_jitter_dev(c, B, st.dev(fsub), n_subset, M, D, seed, attempt, st.dev(fi), st.dev(fno)); });
}

// the arrays of the three merge entry points as the launcher takes them (x in rows of n), their one check -- `compacts`:
// n_failed is needed -- and the body of the two device ones: the merge, then with n_failed the compaction
static PlanMergeArgs plan_merge_args(int M, int D, int reset, const double *x_k, const double *costs4_k, const double *costs4_last_k,
                                     const int32_t *nit_k, const int32_t *nfev_k, const int32_t *status_k, double *x, double *costs4,
                                     double *costs4_last, int32_t *nit, int32_t *nfev, int32_t *status, int32_t *attempts,
                                     int64_t *nit_total, int32_t *solved, int32_t *failed, int32_t *n_failed, int32_t *bad_scene) {
  static_assert(sizeof(long long) == sizeof(int64_t), "nit_total is a 64-bit integer on both sides");
  const int n = D * (M - 1) + M;
  return {n, n, reset ? 1 : 0, {x_k, costs4_k, costs4_last_k, nit_k, nfev_k, status_k}, {x, costs4, costs4_last, nit, nfev, status},
          attempts, reinterpret_cast<long long *>(nit_total), solved, failed, n_failed, bad_scene};
}

static int plan_merge_check(neo_ctx *c, const std::string &who, int B, const int32_t *subset, int n_subset, int M, int D,
                            const PlanMergeArgs &a, bool compacts) {
  int rc = plan_check(c, who.c_str(), B, subset, n_subset, M, D);
  if (rc) return rc;
  if (a.ldx < a.n) return fail_locked(c, NEO_ERR_INVALID, (who + ": x_stride must be >= n = D (M - 1) + M").c_str());
  const RunRowsIn &k = a.packed;
  const RunRows &o = a.out;
  return null_check(c, (who + ": null buffer").c_str(),
                    {k.x, k.costs4, k.costs4_last, k.nit, k.nfev, k.status, o.x, o.costs4, o.costs4_last, o.nit, o.nfev, o.status,
                     a.attempts, a.nit_total, a.solved, a.failed, a.bad_scene},
                    compacts && !a.n_failed);
}

static int plan_merge_dev(neo_ctx *c, const char *who, int B, const int32_t *subset, int n_subset, int M, int D,
                          const PlanMergeArgs &a, bool compacts, bool clear_bad) {
  if (int rc = plan_merge_check(c, who, B, subset, n_subset, M, D, a, compacts)) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  if (clear_bad) HIPCHK(c, hipMemsetAsync(a.bad_scene, 0, sizeof(int32_t), c->stream));
  if (list.n > 0) return launched(c, plan_merge(c, list, a));
  if (compacts) HIPCHK(c, hipMemsetAsync(a.n_failed, 0, sizeof(int32_t), c->stream));
  return NEO_OK;
}

int neo_plan_merge_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, int reset, const double *x_k,
                       const double *costs4_k, const double *costs4_last_k, const int32_t *nit_k, const int32_t *nfev_k,
                       const int32_t *status_k, double *x, double *costs4, double *costs4_last, int32_t *nit, int32_t *nfev,
                       int32_t *status, int32_t *attempts, int64_t *nit_total, int32_t *solved, int32_t *failed,
                       int32_t *n_failed, int32_t *bad_scene) {
  const PlanMergeArgs a = plan_merge_args(M, D, reset, x_k, costs4_k, costs4_last_k, nit_k, nfev_k, status_k, x, costs4, costs4_last,
                                          nit, nfev, status, attempts, nit_total, solved, failed, n_failed, bad_scene);
  return plan_merge_dev(c, "plan merge", B, subset, n_subset, M, D, a, true, true);
}

int neo_plan_merge(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, int reset, const double *x_k,
                   const double *costs4_k, const double *costs4_last_k, const int32_t *nit_k, const int32_t *nfev_k,
                   const int32_t *status_k, double *x, double *costs4, double *costs4_last, int32_t *nit, int32_t *nfev,
                   int32_t *status, int32_t *attempts, int64_t *nit_total, int32_t *solved, int32_t *failed,
                   int32_t *n_failed, int32_t *bad_scene) {
  const PlanMergeArgs a = plan_merge_args(M, D, reset, x_k, costs4_k, costs4_last_k, nit_k, nfev_k, status_k, x, costs4, costs4_last,
                                          nit, nfev, status, attempts, nit_total, solved, failed, n_failed, bad_scene);
  int rc = plan_merge_check(c, "plan merge", B, subset, n_subset, M, D, a, true);
  if (rc) return rc;
  const size_t bs = (size_t)B, P = (size_t)launch_list(B, subset, n_subset).n;
  if (P == 0) {
    *n_failed = 0;
    *bad_scene = 0;
    return NEO_OK;
  }
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  // the request-indexed arrays go up too: requests outside the subset stay, attempts and nit_total accumulate
  HostStage st(c, kStagedUpTo);
  const RowRefs fk = stage_rows_in(st, a.packed, P, (size_t)a.n);
  const auto fsub = st.in_optional(subset, (size_t)n_subset);
  const RowRefs fo = stage_rows_inout(st, a.out, bs, (size_t)a.n);
  const auto oat = st.inout(attempts, bs);
  const auto ont = st.inout(nit_total, bs);
  const auto oso = st.inout(solved, bs);
  // (the whole list comes back; its entries from n_failed on are scratch)
  const auto ofl = st.out(failed, P), onl = st.out(n_failed, 1), obs = st.out(bad_scene, 1);
  return st.run([&] {
    const RunRowsIn k = as_const(staged_rows(st, fk));
    const RunRows o = staged_rows(st, fo);
    return neo_plan_merge_dev(c, B, st.dev(fsub), n_subset, M, D, reset, k.x, k.costs4, k.costs4_last, k.nit, k.nfev, k.status,
                              o.x, o.costs4, o.costs4_last, o.nit, o.nfev, o.status, st.dev(oat), st.dev(ont), st.dev(oso),
                              st.dev(ofl), st.dev(onl), st.dev(obs));
  });
}

// ---- adaptive waypoint counts and the plan chain over groups of one count (expert_planner.py:86-88; kernels:
// neo_adaptive.hpp)
static int adaptive_list_check(neo_ctx *c, const char *who, int B, const int32_t *subset, int n_subset) {
  return list_check(c, who, B, 1, INT32_MAX, subset, n_subset);
}

static int adaptive_count_check(neo_ctx *c, int B, const int32_t *subset, int n_subset, int D, const double *head,
                                const double *tail, double seg_len, int max_waypoints, const int32_t *counts,
                                const int32_t *clamped) {
  int rc = adaptive_list_check(c, "adaptive count", B, subset, n_subset);
  if (rc) return rc;
  if (D < 2 || D > NEO_MAX_DIM) return fail_locked(c, NEO_ERR_INVALID, "adaptive count: D must be 2 or 3");
  if (max_waypoints < 1 || max_waypoints > NEO_MAX_PIECES - 1)
    return fail_locked(c, NEO_ERR_INVALID, "adaptive count: max_waypoints must be in 1 .. NEO_MAX_PIECES - 1");
  if (!std::isfinite(seg_len) || !(seg_len > 0.0))
    return fail_locked(c, NEO_ERR_INVALID, "adaptive count: seg_len must be finite and > 0");
  return null_check(c, "adaptive count: null buffer", {head, tail, counts, clamped});
}

int neo_adaptive_count_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, int D, const double *head,
                           const double *tail, double seg_len, int max_waypoints, int32_t *counts, int32_t *clamped) {
  int rc = adaptive_count_check(c, B, subset, n_subset, D, head, tail, seg_len, max_waypoints, counts, clamped);
  if (rc) return rc;
  return list_launch(c, B, subset, n_subset, [&](const LaunchList &list) {
    return adaptive_count(c, list, D, head, tail, seg_len, max_waypoints, counts, clamped);
  });
}

int neo_adaptive_count(neo_ctx *c, int B, const int32_t *subset, int n_subset, int D, const double *head,
                       const double *tail, double seg_len, int max_waypoints, int32_t *counts, int32_t *clamped) {
  int rc = adaptive_count_check(c, B, subset, n_subset, D, head, tail, seg_len, max_waypoints, counts, clamped);
  if (rc) return rc;
  const size_t bs = (size_t)B, hd = (size_t)3 * D;
  if (launch_list(B, subset, n_subset).n == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  // the results go up too: the rows of requests not launched come back as they were
  HostStage st(c, kStagedUpTo);
  const auto fh = st.in(head, bs * hd), ft = st.in(tail, bs * hd);
  const auto fsub = st.in_optional(subset, (size_t)n_subset);
  const auto oc = st.inout(counts, bs), ocl = st.inout(clamped, bs);
  return st.run([&] {
    return neo_adaptive_count_dev(c, B, st.dev(fsub), n_subset, D, st.dev(fh), st.dev(ft), seg_len, max_waypoints, st.dev(oc),
                                  st.dev(ocl));
  });
}

static int adaptive_bucket_check(neo_ctx *c, int B, const int32_t *subset, int n_subset, const int32_t *counts,
                                 const int32_t *order, const int32_t *bucket_begin, const int32_t *total) {
  int rc = adaptive_list_check(c, "adaptive bucket", B, subset, n_subset);
  if (rc) return rc;
  if ((rc = null_check(c, "adaptive bucket: null buffer", {counts, order, bucket_begin, total}))) return rc;
  if (subset && order == subset) return fail_locked(c, NEO_ERR_INVALID, "adaptive bucket: order must not be the subset");
  return NEO_OK;
}

int neo_adaptive_bucket_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, const int32_t *counts, int32_t *order,
                            int32_t *bucket_begin, int32_t *total) {
  int rc = adaptive_bucket_check(c, B, subset, n_subset, counts, order, bucket_begin, total);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  if (list.n == 0) {
    HIPCHK(c, hipMemsetAsync(bucket_begin, 0, (NEO_MAX_PIECES + 1) * sizeof(int32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(total, 0, sizeof(int32_t), c->stream));
    return NEO_OK;
  }
  return launched(c, adaptive_bucket(c, list, counts, order, bucket_begin, total));
}

int neo_adaptive_bucket(neo_ctx *c, int B, const int32_t *subset, int n_subset, const int32_t *counts, int32_t *order,
                        int32_t *bucket_begin, int32_t *total) {
  int rc = adaptive_bucket_check(c, B, subset, n_subset, counts, order, bucket_begin, total);
  if (rc) return rc;
  const size_t bs = (size_t)B, P = (size_t)launch_list(B, subset, n_subset).n;
  if (P == 0) {
    std::memset(bucket_begin, 0, (NEO_MAX_PIECES + 1) * sizeof(int32_t));
    *total = 0;
    return NEO_OK;
  }
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  // the order goes up too: its entries from total on come back as they were
  HostStage st(c, kStagedUpTo);
  const auto fc = st.in(counts, bs);
  const auto fsub = st.in_optional(subset, (size_t)n_subset);
  const auto oo = st.inout(order, P);
  const auto ob = st.out(bucket_begin, (size_t)NEO_MAX_PIECES + 1), ot = st.out(total, 1);
  return st.run([&] { return neo_adaptive_bucket_dev(c, B, st.dev(fsub), n_subset, st.dev(fc), st.dev(oo), st.dev(ob), st.dev(ot)); });
}

int neo_adaptive_merge_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, int x_stride, int reset,
                           int clear_bad, const double *x_k, const double *costs4_k, const double *costs4_last_k,
                           const int32_t *nit_k, const int32_t *nfev_k, const int32_t *status_k, double *x, double *costs4,
                           double *costs4_last, int32_t *nit, int32_t *nfev, int32_t *status, int32_t *attempts,
                           int64_t *nit_total, int32_t *solved, int32_t *pending, int32_t *bad_scene) {
  if (int rc = adaptive_list_check(c, "adaptive merge", B, subset, n_subset)) return rc;
  PlanMergeArgs a = plan_merge_args(M, D, reset, x_k, costs4_k, costs4_last_k, nit_k, nfev_k, status_k, x, costs4, costs4_last,
                                    nit, nfev, status, attempts, nit_total, solved, pending, nullptr, bad_scene);
  a.ldx = x_stride;
  return plan_merge_dev(c, "adaptive merge", B, subset, n_subset, M, D, a, false, clear_bad != 0);
}

static int adaptive_compact_check(neo_ctx *c, const int32_t *seg_begin, const int32_t *seg_len, long long rows,
                                  const int32_t *pending, const int32_t *n_failed) {
  if (!c) return NEO_ERR_INVALID;
  if (int rc = null_check(c, "adaptive compact: null buffer", {seg_begin, seg_len, pending, n_failed})) return rc;
  for (int g = 0; g < NEO_MAX_PIECES; ++g)
    if (seg_begin[g] < 0 || seg_len[g] < 0 || (rows >= 0 && (long long)seg_begin[g] + seg_len[g] > rows))
      return fail_locked(c, NEO_ERR_INVALID, "adaptive compact: a segment is negative or ends beyond pending");
  return NEO_OK;
}

int neo_adaptive_compact_dev(neo_ctx *c, const int32_t *seg_begin, const int32_t *seg_len, int32_t *pending,
                             int32_t *n_failed) {
  int rc = adaptive_compact_check(c, seg_begin, seg_len, -1, pending, n_failed);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  return launched(c, adaptive_compact(c, seg_begin, seg_len, pending, n_failed));
}

int neo_adaptive_compact(neo_ctx *c, const int32_t *seg_begin, const int32_t *seg_len, int rows, int32_t *pending,
                         int32_t *n_failed) {
  if (c && rows < 0) return fail_locked(c, NEO_ERR_INVALID, "adaptive compact: rows must be >= 0");
  int rc = adaptive_compact_check(c, seg_begin, seg_len, rows, pending, n_failed);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  HostStage st(c, kStagedUpTo);
  const auto fp = st.inout(pending, (size_t)rows);
  const auto on = st.out(n_failed, (size_t)NEO_MAX_PIECES);
  return st.run([&] { return neo_adaptive_compact_dev(c, seg_begin, seg_len, st.dev(fp), st.dev(on)); });
}

}  // extern "C"

