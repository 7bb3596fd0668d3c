// neo_disp_eval.hip -- eval_kernel family: get_cost + get_grad for a batch (expert_planner.py:539-585)
#include "neo_host.hpp"
#include "neo_kernels.hpp"

namespace neo {

template <int D, typename Real, class MapT, class LookupT, typename Num = double>
int launch_eval(neo_ctx *c, const MapT &map, const EvalArgs &a) {
  return visit_slots<D>(a.M, c->params.flags, [&](auto ns, auto lg) {  // (the slots and the lane layout of launch_opt)
    hipLaunchKernelGGL((eval_kernel<D, decltype(ns)::value, Real, MapT, LookupT, type_of<decltype(lg)>, Num>), dim3(a.B),
                       dim3(kWave), 0, c->stream, a.B, a.M, c->dev, map, a.x, a.head, a.tail, a.cost, a.costs4, a.grad,
                       a.coeffs, a.status);
    return NEO_OK;
  });
}

// Real: the sampling arithmetic; Num = float: the all-fp32 mode (the optimiser of neo_disp_opt2d_x.hip / neo_disp_opt3d_x.hip)
template <int D, typename Real, typename Num>
int eval_2d(neo_ctx *c, const MapEntry &e, const EvalArgs &a) {
  return launch_eval<D, Real, Map2D, Lookup2D<Real>, Num>(c, e.m2, a);
}
template <typename Real, typename Num>
int eval_any(neo_ctx *c, const MapEntry &e, int D, const EvalArgs &a) {
  if (e.kind == 0) return D == 2 ? eval_2d<2, Real, Num>(c, e, a) : eval_2d<3, Real, Num>(c, e, a);
  if (D != 3) return fail(c, NEO_ERR_INVALID, "a 3-D map needs D = 3");
  return visit_field<Real>(c, e.elem, e.m3.layout,
                           [&](auto lk) { return launch_eval<3, Real, Map3D, type_of<decltype(lk)>, Num>(c, e.m3, a); });
}

int dispatch_eval(neo_ctx *c, const MapEntry &e, int D, const EvalArgs &a) {
  const bool f32 = c->params.sample_dtype == NEO_F32;
  if (f32 && (c->params.flags & NEO_FLAG_F32_SOLVE)) return eval_any<float, float>(c, e, D, a);
  return f32 ? eval_any<float, double>(c, e, D, a) : eval_any<double, double>(c, e, D, a);
}

}  // namespace neo
