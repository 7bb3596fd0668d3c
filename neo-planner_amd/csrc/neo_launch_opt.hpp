// neo_launch_opt.hpp -- launch of one optimize_kernel family member (shared by the neo_disp_opt*.hip units)
#pragma once
#include "neo_host.hpp"
#include "neo_kernels.hpp"

namespace neo {

// the dynamic LDS of one optimize_kernel workgroup: [stage doubles of staging][the L-BFGS pairs][the cyclic reduction's
// multipliers from double pcr_off, or none: pcr_off = 0]
struct OptLds {
  int stage, pcr_off;
  size_t dyn;  // bytes
};

// stash: bytes of the staging the sample loop itself uses, beside the fold and the exchange table (the gather-ahead form's
// two rounds of velocity, velocity_stash_bytes; 0: none)
template <int D, int NS, typename Real, int WAVES, class LG, typename Num>
OptLds opt_lds_plan(int M, int flags, int stash = 0) {
  const size_t pair_elems = (size_t)2 * NEO_LBFGS_M * (D * (M - 1) + M);  // L-BFGS pairs in LDS
  // staging in front of the pairs: the full size (with the rows of the per-piece fold) unless that costs the two-waves
  // variant occupancy -- eight wavefronts per CU want 160 KB / 8 each, less ~0.5 KB of static LDS.  The one-wave
  // variant follows the same rule so that both sum the partials in the same order (bit-identical results).
  // (static LDS beside the dynamic part: line-search state, cost terms, boundary states; the all-fp32 kernels'
  //  lane-assignment cache kSlCacheInts * 4 = 336 bytes more)
  // The chip hands out LDS in granules of 1 280 bytes (measured in round 5: a workgroup of 13 152 bytes runs eleven to a
  // CU, one of 12 704 twelve): the share of a wavefront is 160 KB / waves rounded DOWN to that.
  const size_t cache = sizeof(Num) == 4 ? kSlCacheInts * sizeof(int) : 0;
  const size_t statics = 400;  // line-search state 160 + cost terms 96 + boundary states 72 / 144 (fp32 / fp64), padded
  const size_t lds_share8 = (size_t)160 * 1024 / 8 / 1280 * 1280 - statics - cache,
               lds_share12 = (size_t)160 * 1024 / (4 * NEO_X_OCC) / 1280 * 1280 - statics - cache;
  const size_t pairs = pair_elems * ((pairs_in_f32<Real, NS, WAVES>() || sizeof(Num) == 4) ? sizeof(float) : sizeof(double));
  const int full = stage_doubles<D, NS, Real>(), small = NS * kWave;
  const size_t lds_share = (sizeof(Num) == 4 && NS <= 2) ? lds_share12 : lds_share8;  // all-fp32: twelve per CU
  OptLds l{pairs + (size_t)full * 8 <= lds_share ? full : small, 0, 0};
  l.dyn = pairs + (size_t)l.stage * 8;
  if (sizeof(Num) == 4 && LG::S > 1 && !(flags & 4096)) {
    // all-fp32, lane = (piece, dimension): room for the reduction's multipliers next to the pairs when the fold runs on
    // per-piece accumulators (80 B a piece at D = 3) instead of rows (96 B a lane); flags bit 4096: off (comparison runs)
    // (the stash is the largest of the four below M = 20 at D = 3: there the pairs behind it shrink faster than it grows)
    const int acc = std::max(std::max(std::max(small, (M * fold_acc_stride(D) * 4 + 7) / 8), (pcr_xch_elems(M, 1) * 4 + 7) / 8),
                             (stash + 7) / 8);
    const size_t off = ((size_t)acc * 8 + pairs + 15) / 16 * 2;
    const size_t need = off * 8 + (size_t)pcr_mult_elems(M) * sizeof(float);
    if (need <= lds_share) {
      l.stage = acc;
      l.pcr_off = (int)off;
      l.dyn = need;
    }
  }
  return l;
}

// The launch may run optimize_kernel's fixed plan (neo_kernels.hpp opt_plan_t): accumulator fold and multipliers in LDS
// (pcr_off), the exchange table and the velocity stash within the staging buffer, and the written-out recursion's reads of
// the partly filled FLAT slot -- which run past the last pair by hist_over_read_elems elements (neo_lbfgs_dir.hpp) --
// inside the launch's own dynamic LDS: they land in the multipliers behind the pairs.  (M = 2 with one FLAT slot: 472 bytes
// against 48 of multipliers -- not fixed.)  `plain`: no trace buffer, no flags bit 4096.
template <int D, int NS, class LG, typename Num>
bool opt_plan_fixed(const OptLds &l, int M, int stash, bool plain) {
  const int n = D * (M - 1) + M;
  const size_t pairs_end = (size_t)l.stage * 8 + (size_t)2 * NEO_LBFGS_M * n * sizeof(Num);  // (a fixed plan's pairs are Num = float)
  return l.pcr_off != 0 && pcr_xch_elems(M, LG::dl(D)) * (int)sizeof(Num) <= l.stage * 8 && stash <= l.stage * 8 &&
         pairs_end + (size_t)hist_over_read_elems(n, NS * kWave) * sizeof(Num) <= l.dyn && plain;
}

// one optimize_kernel instantiation on the context's stream
template <int D, int NS, typename Real, class MapT, class LookupT, int WAVES, class LG, typename Num, bool BUDGET>
int launch_opt_kernel(neo_ctx *c, const OptArgs &a) {
  // (a budgeted launch may cover a subset of the batch: workgroup i then works on trajectory subset[i])
  const int n_launch = a.subset ? a.n_subset : a.B;
  const int *launch_order = a.subset ? a.subset : (c->order_B == a.B ? c->dispatch_order : nullptr);
  // (the gather-ahead sample loop keeps two rounds of velocity in the staging buffer, in front of the L-BFGS pairs)
  constexpr int stash = opt_gather_ahead<D, NS, Real, MapT, LookupT, WAVES, LG, Num, BUDGET>() ? velocity_stash_bytes(D) : 0;
  const OptLds l = opt_lds_plan<D, NS, Real, WAVES, LG, Num>(a.M, c->params.flags, stash);
  // optimize_kernel is compiled for ONE plan (neo_kernels.hpp opt_plan_t).  Where that is a fixed plan, it runs only the
  // launches whose plan -- decided here, on the host -- is that one (opt_plan_fixed).  Everything else (flags bit 4096,
  // traces, an M whose multipliers do not fit or do not cover the recursion's reads behind the pairs) goes to
  // optimize_dyn_kernel, which tests the selectors at run time.  The kernel checks nothing.
  using Plan = opt_plan_t<NS, LG, Num, BUDGET>;
  bool fixed = !Plan::dynamic;
  if constexpr (!Plan::dynamic)
    fixed = opt_plan_fixed<D, NS, LG, Num>(l, a.M, stash, !c->trace && !c->trace_xg && !(c->params.flags & 4096));
  auto kernel = optimize_kernel<D, NS, Real, MapT, LookupT, WAVES, LG, Num, BUDGET>;
  if constexpr (!Plan::dynamic)  // (only the members with a fixed plan have the second form)
    if (!fixed) kernel = optimize_dyn_kernel<D, NS, Real, MapT, LookupT, WAVES, LG, Num, BUDGET>;
  ++c->opt_plan_launches[fixed ? 0 : 1];
  hipLaunchKernelGGL(kernel, dim3(n_launch), dim3(kWave), l.dyn,
                     c->stream, n_launch, a.M, c->dev, static_cast<const MapT *>(a.table), a.slots, a.nmaps,
                     a.x0 ? a.x0 : a.x, a.x, a.head, a.tail, a.costs4, a.costs4_last, a.nit, a.nfev, a.status,
                     c->sample_counter, launch_order, c->trace, c->trace_xg, c->trace_cap, l.stage, l.pcr_off,
                     BUDGET ? a.state : reinterpret_cast<double *>(c->progress) /* (plain launches: the progress counter) */,
                     a.state_doubles, a.budget, a.resume, a.traj_total);
  return NEO_OK;
}

// Num = float: the all-fp32 mode (NEO_FLAG_F32_SOLVE) -- solve, adjoint and optimiser vectors in fp32, pairs in fp32
template <int D, typename Real, class MapT, class LookupT, int WAVES = 1, typename Num = double, bool BUDGET = false>
int launch_opt(neo_ctx *c, const OptArgs &a) {
  // the resumable form of the run exists for n <= 128 variables (neo_kernels.hpp NEO_SM_MAX_SLOTS); two waves only up
  // to NEO_W2_MAX_SLOTS
  constexpr int max_ns = BUDGET ? 2 : (WAVES == 1 || NEO_W2_MAX_SLOTS >= 4) ? 4 : 2;
  if (const int ns = slots_for(a.M, D); ns > max_ns) {
    if (BUDGET) return fail(c, NEO_ERR_INVALID, "budgeted launches: n <= 128 variables");
    if (ns == 3) return fail(c, NEO_ERR_INVALID, "n > 128 variables: this build has no two-waves kernel for three FLAT slots");
    return fail(c, NEO_ERR_INVALID, "n > 128 variables: this build has no two-waves kernel for four FLAT slots "
                                    "(NEO_W2_MAX_SLOTS < 4)");
  }
  return visit_slots<D, max_ns>(a.M, c->params.flags, [&](auto ns, auto lg) {
    return launch_opt_kernel<D, decltype(ns)::value, Real, MapT, LookupT, WAVES, type_of<decltype(lg)>, Num, BUDGET>(c, a);
  });
}

}  // namespace neo
