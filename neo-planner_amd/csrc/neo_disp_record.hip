// neo_disp_record.hip -- the fleet's record mode (neo_record.hpp): the velocity a mission has now, and per target round
// the rows of the missions that solved, ranked in one workgroup and written by one workgroup a mission
// (traj_planner/record_planner.py:13-72 for B missions).  On the context's stream; every pointer is a device array.
#include "neo_host.hpp"
#include "neo_record.hpp"

namespace neo {

int record_state(neo_ctx *c, const LaunchList &l, const double *cmd, int cap, const int *cmd_len, const int *cmd_index,
                 const double *head, double *cur_vel) {
  hipLaunchKernelGGL(record_state_kernel, dim3((l.n + kRecordThreads - 1) / kRecordThreads), dim3(kRecordThreads), 0,
                     c->stream, l, cmd, cap, cmd_len, cmd_index, head, cur_vel);
  return NEO_OK;
}

int record_commit(neo_ctx *c, const LaunchList &l, const RecordCommitArgs &a) {
  hipLaunchKernelGGL(record_rank_kernel, dim3(1), dim3(kRecordRankThreads), 0, c->stream, l, a.solved, a.capacity, a.row_of,
                     a.n_rows, a.dropped);
  const RecordData d{a.motion, a.wpts_local, a.tau, a.pose_rows, a.meta, a.images};
  hipLaunchKernelGGL(record_commit_kernel, dim3(l.n), dim3(kRecordThreads), 0, c->stream, l, a.row_of, a.capacity, a.M,
                     a.x, a.head, a.tail, a.pose, a.cur_vel, a.staging, (size_t)a.W * a.H, a.mission_ids, a.tick, a.round, d);
  return NEO_OK;
}

}  // namespace neo
