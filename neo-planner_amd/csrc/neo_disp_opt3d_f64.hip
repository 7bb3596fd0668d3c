// neo_disp_opt3d_f64.hip -- optimize_kernel on 3-D fields, fp64 sampling (parity mode), one wavefront per SIMD
#include "neo_launch_opt.hpp"

namespace neo {

int launch_opt_3d_f64(neo_ctx *c, int elem, int layout, const OptArgs &a) {
  return visit_field<double>(c, elem, layout, [&](auto lk) { return launch_opt<3, double, Map3D, type_of<decltype(lk)>>(c, a); });
}

// the same in the two-wavefronts-per-SIMD register allocation (256 registers: the lane = (piece, dimension) kernels
// spill 25 - 31 of them), for batches that queue for the SIMDs anyway
int launch_opt_3d_f64_w2(neo_ctx *c, int elem, int layout, const OptArgs &a) {
  return visit_field<double>(c, elem, layout, [&](auto lk) { return launch_opt<3, double, Map3D, type_of<decltype(lk)>, 2>(c, a); });
}

}  // namespace neo
