// neo_disp_opt3d_w2.hip -- optimize_kernel on 3-D fields, fp32 sampling, register allocation for two wavefronts per SIMD
#include "neo_launch_opt.hpp"

namespace neo {

int launch_opt_3d_w2(neo_ctx *c, int elem, int layout, const OptArgs &a) {
  return visit_field<float>(c, elem, layout, [&](auto lk) { return launch_opt<3, float, Map3D, type_of<decltype(lk)>, 2>(c, a); });
}

}  // namespace neo
