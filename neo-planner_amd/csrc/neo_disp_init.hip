// neo_disp_init.hip -- the learned warm start on resident arrays (neo_init.hpp): the motion vector the network is fed,
// PlannerNet's dense layers, and the network's output as the optimiser's first guess (traj_planner/neo_planner.py:10-51
// for the requests of a launch list).  On the context's stream; every pointer is a device array.
#include "neo_host.hpp"
#include "neo_init.hpp"

namespace neo {

int init_motion(neo_ctx *c, const LaunchList &l, const double *pose, const double *cur_vel, const double *head,
                const double *tail, float *motion) {
  hipLaunchKernelGGL(init_motion_kernel, dim3((l.n + kInitThreads - 1) / kInitThreads), dim3(kInitThreads), 0, c->stream, l,
                     pose, cur_vel, head, tail, motion);
  return NEO_OK;
}

int init_head(neo_ctx *c, const LaunchList &l, const float *weights, const float *feature, int feature_rows,
              const float *motion, float *out) {
  hipLaunchKernelGGL(init_head_kernel, dim3((l.n + kInitTile - 1) / kInitTile), dim3(kInitThreads), 0, c->stream, l, weights,
                     feature, feature_rows, motion, out);
  return NEO_OK;
}

int init_guess(neo_ctx *c, const LaunchList &l, const float *out, const double *pose, double *x0) {
  hipLaunchKernelGGL(init_guess_kernel, dim3((l.n + kInitThreads - 1) / kInitThreads), dim3(kInitThreads), 0, c->stream, l,
                     out, pose, c->params.T_min, c->params.T_max, x0);
  return NEO_OK;
}

}  // namespace neo
