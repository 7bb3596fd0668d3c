// neo_disp_onboard.hip -- onboard mapping (neo_onboard.hpp): one launch of the integration kernel per
// neo_onboard_integrate_batch_dev call, on the context's stream; every pointer is a device array, the arguments were
// checked by the C ABI (neo_abi_fleet.hip), which also sized the window.
#include "neo_host.hpp"
#include "neo_onboard.hpp"

namespace neo {

// cells from the eye's cell to the window's edge: a point of a ray lies t along the optical axis and t u across it, so
// within range * sqrt(1 + u_max^2) of the eye in either axis for a unit heading (1e-6 of slack for the fp32 directions),
// plus one cell for the eye's place inside its own cell.  tests/onboard_oracle_np.py window_half is the same expression.
int onboard_window_half(int width, double focal, double range, double res) {
  const float u0 = (float)((0.0 - (double)(width - 1) / 2.0) / focal);
  const float u1 = (float)(((double)(width - 1) - (double)(width - 1) / 2.0) / focal);
  const double umax = std::max(std::fabs((double)u0), std::fabs((double)u1));
  const double ext = range * std::sqrt(1.0 + umax * umax) * (1.0 + 1e-6);
  const double cells = std::ceil(ext / res) + 1.0;
  return cells < 1.0e6 ? (int)cells : 1000000;
}

size_t onboard_lds_need(int half, int N, int height) { return onboard_lds_bytes(half, N, height); }
size_t onboard_lds_limit() { return kOnboardLds; }

int onboard_integrate(neo_ctx *c, const OnboardCall &k) {
  OnboardArgs a{};
  a.list = k.list;
  a.depth_m = k.depth_m, a.pose = k.pose;
  a.W = k.W, a.H = k.H, a.focal = k.focal;
  a.grid_w = k.grid_w, a.grid_h = k.grid_h, a.res = k.res, a.origins = k.origins;
  a.range = k.range, a.z_lo = k.z_lo, a.z_hi = k.z_hi;
  a.l_hit = k.l_hit, a.l_miss = k.l_miss, a.l_lo = k.l_lo, a.l_hi = k.l_hi;
  a.N = k.N, a.half = k.half;
  a.logodds = k.logodds, a.occupancy = k.occupancy, a.changed = k.changed;
  const size_t lds = onboard_lds_bytes(k.half, k.N, k.H);
  // one workgroup a launched mission (the C ABI admits at most 2^20 missions a call)
  hipLaunchKernelGGL(onboard_integrate_kernel, dim3(k.list.n), dim3(kOnboardThreads), lds, c->stream, a);
  HIPCHK(c, hipGetLastError());
  return NEO_OK;
}

}  // namespace neo
