// neo_disp_audit.hip -- the kernels over a planned trajectory's piece table: traj_state_kernel, its sample rows
// (neo_pieces.hpp), and the audit_kernel family, the reference's flight metric (ros_node/traj_planner_node.py:333-363) for
// a batch of trajectories (neo_audit.hpp), one instantiation per map kind, D, element type and layout
#include "neo_host.hpp"
#include "neo_audit.hpp"

namespace neo {

template <int D>
static int launch_traj_state(neo_ctx *c, const TrajStateArgs &a) {
  hipLaunchKernelGGL((traj_state_kernel<D>), dim3(a.B), dim3(kWave), 0, c->stream, a.B, a.M, c->dev, a.x, a.head, a.tail,
                     a.hz, a.K, a.state, a.count);
  return NEO_OK;
}

int dispatch_traj_state(neo_ctx *c, int D, const TrajStateArgs &a) {
  return D == 2 ? launch_traj_state<2>(c, a) : launch_traj_state<3>(c, a);
}

template <int D, class MapT, class LookupT>
static int launch_audit(neo_ctx *c, const AuditArgs &a) {
  hipLaunchKernelGGL((audit_kernel<D, MapT, LookupT>), dim3(a.B), dim3(kWave), 0, c->stream, a.B, a.M, c->dev,
                     static_cast<const MapT *>(a.maps.table), a.maps.slots, a.maps.nmaps, a.x, a.head, a.tail, a.hz, a.w[0],
                     a.w[1], a.w[2], a.audit, a.count, a.flags);
  return NEO_OK;
}

int dispatch_audit(neo_ctx *c, int kind, int elem, int layout, int D, const AuditArgs &a) {
  if (kind == 0) {  // the 2-D reference map: D = 2, or D = 3 looked up on its first two axes (as the sampled cost does)
    if (D == 2) return launch_audit<2, Map2D, Lookup2D<double>>(c, a);
    return launch_audit<3, Map2D, Lookup2D<double>>(c, a);
  }
  if (D != 3) return fail(c, NEO_ERR_INVALID, "audit: a 3-D map needs D = 3");
  return visit_field<double>(c, elem, layout, [&](auto lk) { return launch_audit<3, Map3D, type_of<decltype(lk)>>(c, a); });
}

}  // namespace neo
