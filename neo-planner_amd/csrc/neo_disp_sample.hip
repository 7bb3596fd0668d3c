// neo_disp_sample.hip -- sample_kernel family: the ESDF-lookup kernel (expert_planner.py:392-466) as a launch of its own
// (the experiment bodies of rounds 3 - 6 -- workgroup-per-trajectory, contiguous chunks, shared tail lanes, the sample
// sequence with a candidate list -- live under tools/probe/ with their measurements; HISTORY.md)
#include "neo_host.hpp"
#include "neo_kernels.hpp"

namespace neo {

template <int D, typename Real, class MapT, class LookupT, typename IO>
int launch_sample_io(neo_ctx *c, const MapT &map, const SampleArgs &a) {
  // (round 6, measured and dropped: unused dynamic LDS on small launches so that the dispatcher spreads 4096 workgroups
  //  over all 256 CUs instead of filling 205 of them to their limit of 20 -- 26.45 us with and without)
  hipLaunchKernelGGL((sample_kernel<D, Real, MapT, LookupT, IO>), dim3(a.B), dim3(kWave), 0, c->stream, a.B, a.M, c->dev, map,
                     static_cast<const IO *>(a.coeffs), a.ts, a.costs2, static_cast<IO *>(a.grad_C), static_cast<IO *>(a.grad_T),
                     (c->sample_order_B == a.B ? c->sample_order : nullptr));
  return NEO_OK;
}

// fp32 coefficient / partials buffers (neo_sampled_terms_batch_f32[_dev]) exist for the fp32 sampling arithmetic only
template <int D, typename Real, class MapT, class LookupT>
int launch_sample(neo_ctx *c, const MapT &map, const SampleArgs &a) {
  if constexpr (sizeof(Real) == 4) {
    if (a.io32) return launch_sample_io<D, Real, MapT, LookupT, float>(c, map, a);
  }
  return launch_sample_io<D, Real, MapT, LookupT, double>(c, map, a);
}

template <typename Real>
int sample_any(neo_ctx *c, const MapEntry &e, int D, const SampleArgs &a) {
  if (e.kind == 0)
    return D == 2 ? launch_sample<2, Real, Map2D, Lookup2D<Real>>(c, e.m2, a) : launch_sample<3, Real, Map2D, Lookup2D<Real>>(c, e.m2, a);
  if (D != 3) return fail(c, NEO_ERR_INVALID, "a 3-D map needs D = 3");
  return visit_field<Real>(c, e.elem, e.m3.layout,
                           [&](auto lk) { return launch_sample<3, Real, Map3D, type_of<decltype(lk)>>(c, e.m3, a); });
}

int dispatch_sample(neo_ctx *c, const MapEntry &e, int D, const SampleArgs &a) {
  const bool f32 = c->params.sample_dtype == NEO_F32;
  if (a.io32 && !f32) return fail(c, NEO_ERR_INVALID, "fp32 coefficient / partials buffers need sample_dtype = NEO_F32");
  return f32 ? sample_any<float>(c, e, D, a) : sample_any<double>(c, e, D, a);
}

}  // namespace neo
