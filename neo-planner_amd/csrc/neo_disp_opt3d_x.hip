// neo_disp_opt3d_x.hip -- optimize_kernel on 3-D fields in the all-fp32 mode (NEO_FLAG_F32_SOLVE): fp32 sampling, fp32
// coefficient solve / adjoint / optimiser vectors / stored pairs, register allocation for two wavefronts per SIMD
#include "neo_launch_opt.hpp"

namespace neo {

int launch_opt_3d_x(neo_ctx *c, int elem, int layout, const OptArgs &a) {
  return visit_field<float>(c, elem, layout,
                            [&](auto lk) { return launch_opt<3, float, Map3D, type_of<decltype(lk)>, 2, float>(c, a); });
}

}  // namespace neo
