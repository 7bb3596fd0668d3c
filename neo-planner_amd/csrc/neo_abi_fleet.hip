// neo_abi_fleet.hip -- C ABI of libneo_planner_hip.so (include/neo_planner.h), the unit of the closed-loop missions: the
// depth camera, onboard integration, the fleet replan loop, its goal routes and its campaigns, record mode and the learned warm start.
// Argument checks here, the skeletons in neo_abi_util.hpp, the kernels behind the launchers of neo_disp_depth.hip,
// neo_disp_onboard.hip, neo_disp_fleet.hip, neo_disp_record.hip, neo_disp_init.hip and neo_disp_backbone.hip.
#include "neo_abi_util.hpp"

using namespace neo;
using namespace neo::abi;

extern "C" {

// ---- batched depth camera (neo_planner_amd/initializer.py raycast_depth for B requests; kernels: neo_depth.hpp)
// the argument checks both forms make before anything is copied or launched (context unlocked)
static int depth_check(neo_ctx *c, int width, int height, double focal_px, double max_range, const double *boxes,
                       const int32_t *box_begin, int n_scenes, int B, const double *pose, const float *depth_m) {
  if (!c) return NEO_ERR_INVALID;
  if (B < 1) return fail_locked(c, NEO_ERR_INVALID, "depth: B must be >= 1");
  if (width < 1 || width > 4096 || height < 1 || height > 4096)
    return fail_locked(c, NEO_ERR_INVALID, "depth: width and height must be in 1..4096");
  if (!std::isfinite(focal_px) || !(focal_px > 0.0)) return fail_locked(c, NEO_ERR_INVALID, "depth: focal_px must be finite and > 0");
  if (!std::isfinite(max_range) || !(max_range > 0.0)) return fail_locked(c, NEO_ERR_INVALID, "depth: max_range must be finite and > 0");
  if (n_scenes < 1) return fail_locked(c, NEO_ERR_INVALID, "depth: n_scenes must be >= 1");
  return null_check(c, "depth: null buffer", {boxes, box_begin, pose, depth_m});
}

int neo_depth_render_batch_dev(neo_ctx *c, int width, int height, double focal_px, double max_range, const double *boxes,
                               const int32_t *box_begin, int n_scenes, const int32_t *scene_index, int B,
                               const double *pose, float *depth_m, uint8_t *depth_u8, float *depth_max) {
  int rc = depth_check(c, width, height, focal_px, max_range, boxes, box_begin, n_scenes, B, pose, depth_m);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  return depth_render(c, DepthCall{width, height, focal_px, max_range, boxes, box_begin, n_scenes, scene_index, B, pose,
                                   depth_m, depth_u8, depth_max});
}

int neo_depth_render_batch(neo_ctx *c, int width, int height, double focal_px, double max_range, const double *boxes,
                           const int32_t *box_begin, int n_scenes, const int32_t *scene_index, int B, const double *pose,
                           float *depth_m, uint8_t *depth_u8, float *depth_max) {
  int rc = depth_check(c, width, height, focal_px, max_range, boxes, box_begin, n_scenes, B, pose, depth_m);
  if (rc) return rc;
  // what the device form cannot read on the host
  if (box_begin[0] != 0) return fail_locked(c, NEO_ERR_INVALID, "depth: box_begin must start at 0");
  for (int s = 0; s < n_scenes; ++s) {
    if (box_begin[s + 1] < box_begin[s]) return fail_locked(c, NEO_ERR_INVALID, "depth: box_begin must be non-decreasing");
    if (box_begin[s + 1] - box_begin[s] > NEO_DEPTH_MAX_BOXES)
      return fail_locked(c, NEO_ERR_INVALID, "depth: a scene has more than NEO_DEPTH_MAX_BOXES boxes");
  }
  if (scene_index)
    for (int b = 0; b < B; ++b)
      if (scene_index[b] < 0 || scene_index[b] >= n_scenes)
        return fail_locked(c, NEO_ERR_INVALID, "depth: a scene_index is outside 0 .. n_scenes - 1");
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  const size_t bs = (size_t)B, hw = (size_t)width * height, nbox = (size_t)box_begin[n_scenes];
  HostStage st(c, 0);
  const auto fb = st.in(nbox ? boxes : nullptr, nbox * 6, 6);  // (without any box: a valid pointer nothing is read from)
  const auto fbb = st.in(box_begin, (size_t)n_scenes + 1);
  const auto fsi = st.in(scene_index, bs);
  const auto fp = st.in(pose, bs * 5);
  const auto fm = st.out(depth_m, bs * hw);
  const auto fu = st.out(depth_u8, depth_u8 ? bs * hw : 0);
  const auto fx = st.out(depth_max, bs);
  return st.run([&] {
    return neo_depth_render_batch_dev(c, width, height, focal_px, max_range, st.dev(fb), st.dev(fbb), n_scenes,
                                      scene_index ? st.dev(fsi) : nullptr, B, st.dev(fp), st.dev(fm),
                                      depth_u8 ? st.dev(fu) : nullptr, st.dev(fx));
  });
}

int neo_depth_box_test_counter(neo_ctx *c, uint64_t *dev_count) {
  if (!c) return NEO_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  c->depth.box_tests = reinterpret_cast<unsigned long long *>(dev_count);
  return NEO_OK;
}

// ---- onboard mapping (launch/map_server_onboard.launch: octomap_server's scan insertion projected to 2-D; kernel:
// neo_onboard.hpp).  The checks both forms make before anything is copied or launched (context unlocked); N and half
// are the samples a ray and the window's reach in cells.
static int onboard_check(neo_ctx *c, int B, const int32_t *subset, int n_subset, const float *depth_m, const double *pose,
                         int width, int height, double focal_px, double max_range, int grid_w, int grid_h, double res,
                         const double *origins, double sensor_range, double z_lo, double z_hi, int l_hit, int l_miss,
                         int l_lo, int l_hi, const int8_t *logodds, const int8_t *occupancy, const int32_t *changed, int &N,
                         int &half) {
  int rc = list_check(c, "onboard", B, 1, 1 << 20, subset, n_subset);
  if (rc) return rc;
  if (width < 1 || width > 4096 || height < 1 || height > 4096)
    return fail_locked(c, NEO_ERR_INVALID, "onboard: width and height must be in 1..4096");
  if (!std::isfinite(focal_px) || !(focal_px > 0.0)) return fail_locked(c, NEO_ERR_INVALID, "onboard: focal_px must be finite and > 0");
  if (!std::isfinite(res) || !(res > 0.0)) return fail_locked(c, NEO_ERR_INVALID, "onboard: resolution must be finite and > 0");
  if (!std::isfinite(sensor_range) || !(sensor_range > 0.0))
    return fail_locked(c, NEO_ERR_INVALID, "onboard: sensor_range must be finite and > 0");
  if (!(max_range >= sensor_range))
    return fail_locked(c, NEO_ERR_INVALID, "onboard: the camera's max_range must reach sensor_range (a depth clipped below "
                                           "it would read as a hit)");
  if (!std::isfinite(z_lo) || !std::isfinite(z_hi) || !(z_lo <= z_hi))
    return fail_locked(c, NEO_ERR_INVALID, "onboard: the band needs finite z_lo <= z_hi");
  if (grid_w < 1 || grid_h < 1 || (size_t)grid_w * grid_h > (size_t)1 << 30)
    return fail_locked(c, NEO_ERR_INVALID, "onboard: grid width and height >= 1, at most 2^30 cells");
  if (l_lo < -127 || l_hi > 127 || l_lo > l_hi || l_hit < 0 || l_hit > 127 || l_miss > 0 || l_miss < -127)
    return fail_locked(c, NEO_ERR_INVALID, "onboard: log-odds need -127 <= lo <= hi <= 127, 0 <= hit <= 127, -127 <= miss <= 0");
  if ((rc = null_check(c, "onboard: null buffer", {depth_m, pose, origins, logodds, occupancy, changed}))) return rc;
  const double nd = std::ceil(sensor_range / (res / 2.0));
  half = onboard_window_half(width, focal_px, sensor_range, res);
  if (!(nd <= 32767.0) || half > 4096 || onboard_lds_need(half, (int)nd, height) > onboard_lds_limit())
    return fail_locked(c, NEO_ERR_INVALID, "onboard: the window a scan can touch (sensor_range against the resolution and "
                                           "the camera's field of view) does not fit the 64 KB of LDS a workgroup has");
  N = (int)nd;
  return NEO_OK;
}

int neo_onboard_integrate_batch_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, const float *depth_m,
                                    const double *pose, int width, int height, double focal_px, double max_range, int grid_w,
                                    int grid_h, double res, const double *origins, double sensor_range, double z_lo,
                                    double z_hi, int l_hit, int l_miss, int l_lo, int l_hi, int8_t *logodds,
                                    int8_t *occupancy, int32_t *changed) {
  int N = 0, half = 0;
  int rc = onboard_check(c, B, subset, n_subset, depth_m, pose, width, height, focal_px, max_range, grid_w, grid_h, res,
                         origins, sensor_range, z_lo, z_hi, l_hit, l_miss, l_lo, l_hi, logodds, occupancy, changed, N, half);
  if (rc) return rc;
  return list_launch(c, B, subset, n_subset, [&](const LaunchList &list) {
    return onboard_integrate(c, OnboardCall{list, depth_m, pose, width, height, focal_px, grid_w, grid_h, res, origins,
                                            sensor_range, z_lo, z_hi, l_hit, l_miss, l_lo, l_hi, N, half, logodds,
                                            occupancy, changed});
  });
}

int neo_onboard_integrate_batch(neo_ctx *c, int B, const int32_t *subset, int n_subset, const float *depth_m,
                                const double *pose, int width, int height, double focal_px, double max_range, int grid_w,
                                int grid_h, double res, const double *origins, double sensor_range, double z_lo, double z_hi,
                                int l_hit, int l_miss, int l_lo, int l_hi, int8_t *logodds, int8_t *occupancy,
                                int32_t *changed) {
  int N = 0, half = 0;
  int rc = onboard_check(c, B, subset, n_subset, depth_m, pose, width, height, focal_px, max_range, grid_w, grid_h, res,
                         origins, sensor_range, z_lo, z_hi, l_hit, l_miss, l_lo, l_hi, logodds, occupancy, changed, N, half);
  if (rc) return rc;
  if (subset) {
    std::vector<char> seen((size_t)B, 0);
    for (int i = 0; i < n_subset; ++i) {
      if (subset[i] < 0 || subset[i] >= B) return fail_locked(c, NEO_ERR_INVALID, "onboard: a subset entry is outside 0 .. B - 1");
      if (seen[subset[i]]) return fail_locked(c, NEO_ERR_INVALID, "onboard: a mission is listed twice in the subset");
      seen[subset[i]] = 1;
    }
  }
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  const size_t bs = (size_t)B, nl = (size_t)launch_list(B, subset, n_subset).n, hw = (size_t)width * height;
  const size_t ncell = (size_t)grid_w * grid_h;
  if (nl == 0) return NEO_OK;
  HostStage st(c, 0);
  const auto fsub = st.in_optional(subset, nl);
  const auto fd = st.in(depth_m, nl * hw);
  const auto fp = st.in(pose, nl * 5);
  const auto fo = st.in(origins, bs * 2);
  const auto fl = st.inout(logodds, bs * ncell);    // (missions outside the subset keep their grids)
  const auto fc = st.inout(occupancy, bs * ncell);
  const auto fg = st.inout(changed, bs);
  return st.run([&] {
    return neo_onboard_integrate_batch_dev(c, B, st.dev(fsub), n_subset, st.dev(fd), st.dev(fp), width, height, focal_px,
                                           max_range, grid_w, grid_h, res, st.dev(fo), sensor_range, z_lo, z_hi, l_hit,
                                           l_miss, l_lo, l_hi, st.dev(fl), st.dev(fc), st.dev(fg));
  });
}

// ---- fleet replan loop (ros_node/traj_planner_node.py:390-578; kernels: neo_fleet.hpp)
static bool fleet_positive(double v) { return std::isfinite(v) && v > 0.0; }

static int fleet_target_check(neo_ctx *c, int B, const int32_t *subset, int n_subset, const double *cur_pos,
                              const double *goal, const double *jitter, double longitu, double lateral, double move_vel,
                              const double *tail, const int32_t *near_goal, const int32_t *lateral_steps,
                              const int32_t *flags) {
  int rc = list_check(c, "fleet", B, 0, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  rc = null_check(c, "fleet target: null buffer", {cur_pos, goal, jitter, tail, near_goal, lateral_steps, flags});
  if (rc) return rc;
  if (!fleet_positive(longitu) || !fleet_positive(lateral) || !std::isfinite(move_vel))
    return fail_locked(c, NEO_ERR_INVALID, "fleet target: longitu_step_dis and lateral_step_length must be finite and > 0, "
                                           "move_vel finite");
  return NEO_OK;
}

int neo_fleet_target_batch_dev(neo_ctx *c, int scene_id, const int32_t *scene_ids, int B, const int32_t *subset,
                               int n_subset, const double *cur_pos, const double *goal, const double *jitter,
                               double longitu_step_dis, double lateral_step_length, double move_vel, double *tail,
                               int32_t *near_goal, int32_t *lateral_steps, int32_t *flags) {
  int rc = fleet_target_check(c, B, subset, n_subset, cur_pos, goal, jitter, longitu_step_dis, lateral_step_length,
                              move_vel, tail, near_goal, lateral_steps, flags);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  MapRef maps;
  rc = fleet_maps(c, scene_id, scene_ids, maps);
  if (rc) return rc;
  if (list.n < 1) return NEO_OK;  // (only after the maps resolved: a call without a map fails on an empty list too)
  return launched(c, fleet_target(c, list, maps, {cur_pos, goal, jitter, longitu_step_dis, lateral_step_length, move_vel,
                                                  tail, near_goal, lateral_steps, flags}));
}

int neo_fleet_target_batch(neo_ctx *c, int scene_id, const int32_t *scene_ids, int B, const int32_t *subset, int n_subset,
                           const double *cur_pos, const double *goal, const double *jitter, double longitu_step_dis,
                           double lateral_step_length, double move_vel, double *tail, int32_t *near_goal,
                           int32_t *lateral_steps, int32_t *flags) {
  int rc = fleet_target_check(c, B, subset, n_subset, cur_pos, goal, jitter, longitu_step_dis, lateral_step_length,
                              move_vel, tail, near_goal, lateral_steps, flags);
  if (rc) return rc;
  if (B == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  const size_t bs = (size_t)B;
  SceneList scenes(scene_ids);
  if ((rc = scenes.resolve(c, bs))) return rc;
  // all arrays small: the pinned mirror.  The outputs go up too: missions outside the subset keep their rows
  HostStage st(c, kStagedUpTo);
  const auto fp = st.in(cur_pos, bs * 2), fg = st.in(goal, bs * 2), fj = st.in(jitter, bs * 2);
  scenes.stage(st, bs);
  const auto fsub = st.in_optional(subset, (size_t)n_subset);
  const auto ft = st.inout(tail, bs * 6);
  const auto fn = st.inout(near_goal, bs), fl = st.inout(lateral_steps, bs), ff = st.inout(flags, bs);
  return st.run([&] {
    return neo_fleet_target_batch_dev(c, scenes.scene(scene_id), scenes.slots(st), B, st.dev(fsub), n_subset, st.dev(fp),
                                      st.dev(fg), st.dev(fj), longitu_step_dis, lateral_step_length, move_vel, st.dev(ft),
                                      st.dev(fn), st.dev(fl), st.dev(ff));
  });
}

static int fleet_jitter_check(neo_ctx *c, int B, const int32_t *subset, int n_subset, int tick, int target,
                              const double *jitter) {
  int rc = list_check(c, "fleet jitter", B, 0, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  if ((rc = null_check(c, "fleet jitter: null buffer", {jitter}))) return rc;
  if (tick < 0 || target < 0) return fail_locked(c, NEO_ERR_INVALID, "fleet jitter: tick and target must be >= 0");
  return NEO_OK;
}

int neo_fleet_jitter_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, uint64_t seed, int tick, int target,
                         const int32_t *mission_ids, double *jitter) {
  int rc = fleet_jitter_check(c, B, subset, n_subset, tick, target, jitter);
  if (rc) return rc;
  return list_launch(c, B, subset, n_subset, [&](const LaunchList &list) {
    return fleet_jitter(c, list, seed, tick, target, mission_ids, jitter);
  });
}

int neo_fleet_jitter(neo_ctx *c, int B, const int32_t *subset, int n_subset, uint64_t seed, int tick, int target,
                     const int32_t *mission_ids, double *jitter) {
  int rc = fleet_jitter_check(c, B, subset, n_subset, tick, target, jitter);
  if (rc) return rc;
  if (launch_list(B, subset, n_subset).n == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  const size_t bs = (size_t)B;
  // the rows go up too: missions outside the subset keep theirs
  HostStage st(c, kStagedUpTo);
  const auto fi = st.in_optional(mission_ids, bs), fsub = st.in_optional(subset, (size_t)n_subset);
  const auto fj = st.inout(jitter, bs * 2);
  return st.run([&] { return neo_fleet_jitter_dev(c, B, st.dev(fsub), n_subset, seed, tick, target, st.dev(fi), st.dev(fj)); });
}

static int fleet_cmd_check(neo_ctx *c, const char *who, const double *cmd, int cap, const int32_t *cmd_len,
                           const int32_t *cmd_index, const int32_t *future_index) {
  if (int rc = null_check(c, (std::string(who) + ": null buffer").c_str(), {cmd, cmd_len, cmd_index, future_index})) return rc;
  if (cap <= 0) return fail_locked(c, NEO_ERR_INVALID, (std::string(who) + ": cap must be > 0").c_str());
  return NEO_OK;
}

int neo_fleet_advance_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, const double *cmd, int cap,
                          const int32_t *cmd_len, int32_t *cmd_index, int32_t *future_index, int step, int ahead,
                          double *cur_pos, double *head) {
  int rc = list_check(c, "fleet", B, 0, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  rc = fleet_cmd_check(c, "fleet advance", cmd, cap, cmd_len, cmd_index, future_index);
  if (rc) return rc;
  if ((rc = null_check(c, "fleet advance: null buffer", {cur_pos, head}))) return rc;
  if (step < 0 || step > (1 << 30) || ahead < 0 || ahead > (1 << 30))
    return fail_locked(c, NEO_ERR_INVALID, "fleet advance: step and ahead must be in 0 .. 2^30");
  return list_launch(c, B, subset, n_subset, [&](const LaunchList &list) {
    return fleet_advance(c, list, {const_cast<double *>(cmd), cap, const_cast<int32_t *>(cmd_len), cmd_index, future_index},
                         step, ahead, cur_pos, head);
  });
}

int neo_fleet_pose_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, const double *cmd, int cap,
                       const int32_t *cmd_len, const int32_t *cmd_index, const double *cur_pos, const double *goal,
                       double eye_z, double *pose) {
  int rc = list_check(c, "fleet", B, 0, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  if ((rc = null_check(c, "fleet pose: null buffer", {cmd, cmd_len, cmd_index, cur_pos, goal, pose}))) return rc;
  if (cap <= 0) return fail_locked(c, NEO_ERR_INVALID, "fleet pose: cap must be > 0");
  if (!std::isfinite(eye_z)) return fail_locked(c, NEO_ERR_INVALID, "fleet pose: eye_z must be finite");
  return list_launch(c, B, subset, n_subset, [&](const LaunchList &list) {
    return fleet_pose(c, list, {const_cast<double *>(cmd), cap, const_cast<int32_t *>(cmd_len),
                                const_cast<int32_t *>(cmd_index), nullptr}, cur_pos, goal, eye_z, pose);
  });
}

int neo_fleet_splice_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, const double *x, const double *head,
                         const double *tail, const int32_t *solved, double hz, int first, double *cmd, int cap,
                         int32_t *cmd_len, int32_t *cmd_index, int32_t *future_index, int32_t *flags) {
  int rc = list_check(c, "fleet", B, 0, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  rc = check_shape(c, B, M, 2);
  if (rc) return rc;
  rc = fleet_cmd_check(c, "fleet splice", cmd, cap, cmd_len, cmd_index, future_index);
  if (rc) return rc;
  if ((rc = null_check(c, "fleet splice: null buffer", {x, head, tail, flags}))) return rc;
  if (!fleet_positive(hz)) return fail_locked(c, NEO_ERR_INVALID, "fleet splice: hz must be finite and > 0");
  return list_launch(c, B, subset, n_subset, [&](const LaunchList &list) {
    return fleet_splice(c, list, {cmd, cap, cmd_len, cmd_index, future_index},
                        {M, x, head, tail, solved, hz, first ? 1 : 0, flags});
  });
}

// mode "warmstart": the state a mission carries from one plan to the next
static int fleet_warm_check(neo_ctx *c, const char *who, int B, const int32_t *subset, int n_subset, int M) {
  int rc = list_check(c, who, B, 1, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  if (M < 2 || M > NEO_MAX_PIECES) return fail_locked(c, NEO_ERR_INVALID, (std::string(who) + ": M must be in 2 .. 64").c_str());
  return NEO_OK;
}

int neo_fleet_warm_guess_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, const double *head,
                             const double *wpts_local, const double *ts_carry, double *x0) {
  int rc = fleet_warm_check(c, "fleet warm guess", B, subset, n_subset, M);
  if (rc) return rc;
  if ((rc = null_check(c, "fleet warm guess: null buffer", {head, wpts_local, ts_carry, x0}))) return rc;
  return list_launch(c, B, subset, n_subset, [&](const LaunchList &list) {
    return fleet_warm_guess(c, list, M, head, wpts_local, ts_carry, x0);
  });
}

int neo_fleet_warm_carry_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, const double *x,
                             const double *head, const int32_t *solved, const int32_t *status, const int32_t *attempts,
                             const double *init_ts, double *wpts_local, double *ts_carry) {
  int rc = fleet_warm_check(c, "fleet warm carry", B, subset, n_subset, M);
  if (rc) return rc;
  rc = null_check(c, "fleet warm carry: null buffer", {x, head, solved, status, attempts, init_ts, wpts_local, ts_carry});
  if (rc) return rc;
  return list_launch(c, B, subset, n_subset, [&](const LaunchList &list) {
    return fleet_warm_carry(c, list, {M, x, head, solved, status, attempts, init_ts, wpts_local, ts_carry});
  });
}

static int fleet_audit_check(neo_ctx *c, int B, const int32_t *subset, int n_subset, const double *cmd, int cap,
                             const int32_t *n_flown, int stride, double cmd_hz, const double *audit, const int32_t *count,
                             const int32_t *flags) {
  int rc = list_check(c, "fleet", B, 0, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  if ((rc = null_check(c, "fleet audit: null buffer", {cmd, n_flown, audit, count, flags}))) return rc;
  if (cap <= 0) return fail_locked(c, NEO_ERR_INVALID, "fleet audit: cap must be > 0");
  if (stride <= 0) return fail_locked(c, NEO_ERR_INVALID, "fleet audit: stride must be > 0");
  if (!fleet_positive(cmd_hz)) return fail_locked(c, NEO_ERR_INVALID, "fleet audit: cmd_hz must be finite and > 0");
  return NEO_OK;
}

int neo_fleet_audit_batch_dev(neo_ctx *c, int scene_id, const int32_t *scene_ids, int B, const int32_t *subset, int n_subset,
                              const double *cmd, int cap, const int32_t *n_flown, int stride, double cmd_hz,
                              const double *weights3, double *audit, int32_t *count, int32_t *flags) {
  int rc = fleet_audit_check(c, B, subset, n_subset, cmd, cap, n_flown, stride, cmd_hz, audit, count, flags);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  MapRef maps;
  rc = fleet_maps(c, scene_id, scene_ids, maps);
  if (rc) return rc;
  if (list.n < 1) return NEO_OK;  // (only after the maps resolved: a call without a map fails on an empty list too)
  FleetAuditArgs aa{cmd, cap, n_flown, stride, cmd_hz, {1.0, 1.0, 100.0}, audit, count, flags};
  if (weights3)
    for (int k = 0; k < 3; ++k) aa.w[k] = weights3[k];
  return launched(c, fleet_audit(c, list, maps, aa));
}

int neo_fleet_audit_batch(neo_ctx *c, int scene_id, const int32_t *scene_ids, int B, const int32_t *subset, int n_subset,
                          const double *cmd, int cap, const int32_t *n_flown, int stride, double cmd_hz,
                          const double *weights3, double *audit, int32_t *count, int32_t *flags) {
  int rc = fleet_audit_check(c, B, subset, n_subset, cmd, cap, n_flown, stride, cmd_hz, audit, count, flags);
  if (rc) return rc;
  if (B == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  const size_t bs = (size_t)B;
  SceneList scenes(scene_ids);
  if ((rc = scenes.resolve(c, bs))) return rc;
  HostStage st(c, 0);
  const auto fc = st.in(cmd, bs * cap * 6);
  const auto fnf = st.in(n_flown, bs);
  scenes.stage(st, bs);
  const auto fsub = st.in_optional(subset, (size_t)n_subset);
  const auto fa = st.inout(audit, bs * NEO_AUDIT_FIELDS);  // (missions outside the subset keep their records)
  const auto fcnt = st.inout(count, bs), ffl = st.inout(flags, bs);
  return st.run([&] {
    return neo_fleet_audit_batch_dev(c, scenes.scene(scene_id), scenes.slots(st), B, st.dev(fsub), n_subset, st.dev(fc), cap,
                                     st.dev(fnf), stride, cmd_hz, weights3, st.dev(fa), st.dev(fcnt), st.dev(ffl));
  });
}

// ---- fleet goal routes (ros_node/tracker_planner_node.py; kernels: neo_track.hpp)
static int fleet_routes_check(neo_ctx *c, const char *who, const double *vertices, int n_vertices,
                              const int32_t *route_begin, const double *speed) {
  if (int rc = null_check(c, (std::string(who) + ": null buffer").c_str(), {vertices, route_begin, speed})) return rc;
  if (n_vertices < 0) return fail_locked(c, NEO_ERR_INVALID, (std::string(who) + ": n_vertices must be >= 0").c_str());
  return NEO_OK;
}

static int fleet_goal_check(neo_ctx *c, int B, const int32_t *subset, int n_subset, const double *vertices, int n_vertices,
                            const int32_t *route_begin, const double *speed, double t, const double *goal) {
  int rc = list_check(c, "fleet goal", B, 0, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  rc = fleet_routes_check(c, "fleet goal", vertices, n_vertices, route_begin, speed);
  if (rc) return rc;
  if ((rc = null_check(c, "fleet goal: null buffer", {goal}))) return rc;
  if (!std::isfinite(t)) return fail_locked(c, NEO_ERR_INVALID, "fleet goal: t must be finite");
  return NEO_OK;
}

int neo_fleet_goal_route_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, const double *vertices, int n_vertices,
                             const int32_t *route_begin, const double *speed, const int32_t *closed, double t,
                             double *goal) {
  int rc = fleet_goal_check(c, B, subset, n_subset, vertices, n_vertices, route_begin, speed, t, goal);
  if (rc) return rc;
  return list_launch(c, B, subset, n_subset, [&](const LaunchList &list) {
    return fleet_goal(c, list, {vertices, n_vertices, route_begin, speed, closed}, t, goal);
  });
}

int neo_fleet_goal_route(neo_ctx *c, int B, const int32_t *subset, int n_subset, const double *vertices, int n_vertices,
                         const int32_t *route_begin, const double *speed, const int32_t *closed, double t, double *goal) {
  int rc = fleet_goal_check(c, B, subset, n_subset, vertices, n_vertices, route_begin, speed, t, goal);
  if (rc) return rc;
  if (launch_list(B, subset, n_subset).n == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  const size_t bs = (size_t)B;
  // the rows go up too: missions outside the subset keep theirs
  HostStage st(c, kStagedUpTo);
  const auto fv = st.in(vertices, (size_t)n_vertices * 2, 2), fs = st.in(speed, bs);
  const auto fb = st.in(route_begin, bs + 1);
  const auto fc = st.in_optional(closed, bs), fsub = st.in_optional(subset, (size_t)n_subset);
  const auto fg = st.inout(goal, bs * 2);
  return st.run([&] {
    return neo_fleet_goal_route_dev(c, B, st.dev(fsub), n_subset, st.dev(fv), n_vertices, st.dev(fb), st.dev(fs), st.dev(fc),
                                    t, st.dev(fg));
  });
}

int neo_fleet_hold_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, double *cmd, int cap, int32_t *cmd_len,
                       const int32_t *cmd_index, int step, int32_t *flags) {
  int rc = list_check(c, "fleet hold", B, 0, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  if ((rc = null_check(c, "fleet hold: null buffer", {cmd, cmd_len, cmd_index, flags}))) return rc;
  if (cap < 1) return fail_locked(c, NEO_ERR_INVALID, "fleet hold: cap must be >= 1");
  if (step < 1 || step > (1 << 30)) return fail_locked(c, NEO_ERR_INVALID, "fleet hold: step must be in 1 .. 2^30");
  if (reinterpret_cast<uintptr_t>(cmd) & 15) return fail_locked(c, NEO_ERR_INVALID, "fleet hold: cmd must be 16-byte aligned");
  return list_launch(c, B, subset, n_subset, [&](const LaunchList &list) {
    return fleet_hold(c, list, {cmd, cap, cmd_len, const_cast<int32_t *>(cmd_index), nullptr}, step, flags);
  });
}

static int fleet_track_check(neo_ctx *c, int B, const int32_t *subset, int n_subset, const double *cmd, int cap,
                             const int32_t *n_flown, int stride, double cmd_hz, const double *vertices, int n_vertices,
                             const int32_t *route_begin, const double *speed, double radius, const double *track,
                             const int32_t *count, const int32_t *flags) {
  int rc = list_check(c, "fleet track audit", B, 0, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  rc = fleet_routes_check(c, "fleet track audit", vertices, n_vertices, route_begin, speed);
  if (rc) return rc;
  if ((rc = null_check(c, "fleet track audit: null buffer", {cmd, n_flown, track, count, flags}))) return rc;
  if (cap < 1) return fail_locked(c, NEO_ERR_INVALID, "fleet track audit: cap must be >= 1");
  if (stride < 1) return fail_locked(c, NEO_ERR_INVALID, "fleet track audit: stride must be >= 1");
  if (!fleet_positive(cmd_hz)) return fail_locked(c, NEO_ERR_INVALID, "fleet track audit: cmd_hz must be finite and > 0");
  if (!std::isfinite(radius)) return fail_locked(c, NEO_ERR_INVALID, "fleet track audit: radius must be finite");
  return NEO_OK;
}

int neo_fleet_track_audit_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, const double *cmd, int cap,
                              const int32_t *n_flown, int stride, double cmd_hz, const double *vertices, int n_vertices,
                              const int32_t *route_begin, const double *speed, const int32_t *closed, double radius,
                              double *track, int32_t *count, int32_t *flags) {
  int rc = fleet_track_check(c, B, subset, n_subset, cmd, cap, n_flown, stride, cmd_hz, vertices, n_vertices, route_begin,
                             speed, radius, track, count, flags);
  if (rc) return rc;
  return list_launch(c, B, subset, n_subset, [&](const LaunchList &list) {
    return fleet_track_audit(c, list, {vertices, n_vertices, route_begin, speed, closed},
                             {cmd, cap, n_flown, stride, cmd_hz, radius, track, count, flags});
  });
}

int neo_fleet_track_audit(neo_ctx *c, int B, const int32_t *subset, int n_subset, const double *cmd, int cap,
                          const int32_t *n_flown, int stride, double cmd_hz, const double *vertices, int n_vertices,
                          const int32_t *route_begin, const double *speed, const int32_t *closed, double radius,
                          double *track, int32_t *count, int32_t *flags) {
  int rc = fleet_track_check(c, B, subset, n_subset, cmd, cap, n_flown, stride, cmd_hz, vertices, n_vertices, route_begin,
                             speed, radius, track, count, flags);
  if (rc) return rc;
  if (launch_list(B, subset, n_subset).n == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  const size_t bs = (size_t)B;
  HostStage st(c, 0);
  const auto fc = st.in(cmd, bs * cap * 6);
  const auto fnf = st.in(n_flown, bs);
  const auto fv = st.in(vertices, (size_t)n_vertices * 2, 2), fs = st.in(speed, bs);
  const auto fb = st.in(route_begin, bs + 1);
  const auto fcl = st.in_optional(closed, bs), fsub = st.in_optional(subset, (size_t)n_subset);
  const auto ft = st.inout(track, bs * NEO_TRACK_FIELDS);  // (missions outside the subset keep their records)
  const auto fcnt = st.inout(count, bs), ffl = st.inout(flags, bs);
  return st.run([&] {
    return neo_fleet_track_audit_dev(c, B, st.dev(fsub), n_subset, st.dev(fc), cap, st.dev(fnf), stride, cmd_hz, st.dev(fv),
                                     n_vertices, st.dev(fb), st.dev(fs), st.dev(fcl), radius, st.dev(ft), st.dev(fcnt),
                                     st.dev(ffl));
  });
}

// ---- the fleet's flight model (kernels: neo_flight.hpp)
int neo_fleet_fly_dev(neo_ctx *c, int B, const neo_flight_model *model, const int32_t *subset, int n_subset, const double *cmd,
                      int cap, const int32_t *cmd_len, int32_t *cmd_index, int32_t *future_index, int step, int ahead,
                      int first, int settle, double reach, const int32_t *mission_ids, const double *goal, double *drone,
                      double *flown, int32_t *flown_len, int32_t *saturated, int32_t *flags, double *cur_pos, double *head) {
  int rc = list_check(c, "fleet fly", B, 0, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  rc = fleet_cmd_check(c, "fleet fly", cmd, cap, cmd_len, cmd_index, future_index);
  if (rc) return rc;
  rc = null_check(c, "fleet fly: null buffer", {model, goal, drone, flown, flown_len, saturated, flags, cur_pos, head});
  if (rc) return rc;
  // (sums of two of them stay below 2^31: the kernel's index arithmetic cannot overflow)
  if (step < 0 || step > (1 << 30) || ahead < 0 || ahead > (1 << 30) || settle < 0 || settle > (1 << 30))
    return fail_locked(c, NEO_ERR_INVALID, "fleet fly: step, ahead and settle must be in 0 .. 2^30");
  if (!std::isfinite(reach)) return fail_locked(c, NEO_ERR_INVALID, "fleet fly: reach must be finite");
  for (double v : {model->h, model->kp, model->kv, model->a_max, model->alpha, model->drag, model->rho, model->scale})
    if (!std::isfinite(v)) return fail_locked(c, NEO_ERR_INVALID, "fleet fly: the model has a field that is not finite");
  if (!(model->h > 0.0) || !(model->a_max > 0.0) || !(model->alpha > 0.0))
    return fail_locked(c, NEO_ERR_INVALID, "fleet fly: the model's h, a_max and alpha must be > 0");
  if (model->gust_every < 1) return fail_locked(c, NEO_ERR_INVALID, "fleet fly: the model's gust_every must be >= 1");
  return list_launch(c, B, subset, n_subset, [&](const LaunchList &list) {
    return fleet_fly(c, list, *model, {const_cast<double *>(cmd), cap, const_cast<int32_t *>(cmd_len), cmd_index, future_index},
                     {step, ahead, first ? 1 : 0, settle, reach, mission_ids, goal, drone, flown, flown_len, saturated, flags,
                      cur_pos, head});
  });
}

int neo_fleet_fly_error_dev(neo_ctx *c, int B, const int32_t *flown_len, const int32_t *subset, int n_subset,
                            const double *flown, const double *cmd, int cap, const int32_t *cmd_len, int stride, double *fly,
                            int32_t *count, int32_t *flags) {
  int rc = list_check(c, "fleet fly error", B, 0, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  if ((rc = null_check(c, "fleet fly error: null buffer", {flown_len, flown, cmd, cmd_len, fly, count, flags}))) return rc;
  if (cap <= 0) return fail_locked(c, NEO_ERR_INVALID, "fleet fly error: cap must be > 0");
  if (stride < 1) return fail_locked(c, NEO_ERR_INVALID, "fleet fly error: stride must be >= 1");
  return list_launch(c, B, subset, n_subset, [&](const LaunchList &list) {
    return fleet_fly_error(c, list, {flown, cmd, cap, flown_len, cmd_len, stride, fly, count, flags});
  });
}

// ---- fleet campaigns (ros_node/manager_node.py:153-193; kernels: neo_legs.hpp)
// what can be said of the goal lists without reading them (the _dev forms hold device pointers)
static int fleet_legs_seq_check(neo_ctx *c, const char *who, const neo_leg_sequences *seq, int B) {
  const std::string w(who);
  if (!seq) return fail_locked(c, NEO_ERR_INVALID, (w + ": null buffer").c_str());
  if (seq->kind == NEO_LEGS_TABLE) {
    if (int rc = null_check(c, (w + ": null buffer").c_str(), {seq->goals, seq->seq_begin})) return rc;
    if (seq->n_goals < B)
      return fail_locked(c, NEO_ERR_INVALID, (w + ": the table has fewer goals than missions: every mission needs at least 1").c_str());
  } else if (seq->kind == NEO_LEGS_FLAP) {
    if (seq->legs < 1 || seq->legs > NEO_FLEET_LEGS_MAX)
      return fail_locked(c, NEO_ERR_INVALID, (w + ": a flap campaign has 1 .. NEO_FLEET_LEGS_MAX legs").c_str());
    if (!std::isfinite(seq->x_pair[0]) || !std::isfinite(seq->x_pair[1]) || !std::isfinite(seq->y_scale) ||
        !std::isfinite(seq->y_shift))
      return fail_locked(c, NEO_ERR_INVALID, (w + ": x_pair, y_scale and y_shift must be finite").c_str());
  } else {
    return fail_locked(c, NEO_ERR_INVALID, (w + ": kind must be NEO_LEGS_TABLE or NEO_LEGS_FLAP").c_str());
  }
  return NEO_OK;
}

int neo_fleet_leg_close_dev(neo_ctx *c, int B, const int32_t *outcome, const int32_t *subset, int n_subset, const double *cmd,
                            int cap, const int32_t *cmd_len, const int32_t *cmd_index, const double *head, const double *goal,
                            int32_t *n_flown, double *leg_end, double *final_dist) {
  int rc = list_check(c, "fleet leg close", B, 0, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  rc = null_check(c, "fleet leg close: null buffer", {outcome, cmd, cmd_len, cmd_index, head, goal, n_flown, leg_end, final_dist});
  if (rc) return rc;
  if (cap < 1) return fail_locked(c, NEO_ERR_INVALID, "fleet leg close: cap must be >= 1");
  return list_launch(c, B, subset, n_subset, [&](const LaunchList &list) {
    return fleet_leg_close(c, list, {outcome, cmd, cap, cmd_len, cmd_index, head, goal, n_flown, leg_end, final_dist});
  });
}

int neo_fleet_leg_open_dev(neo_ctx *c, int B, const int32_t *outcome, const int32_t *subset, int n_subset,
                           const neo_leg_sequences *seq, int max_legs, double threshold, const int32_t *n_flown, const double *leg_end,
                           const double *final_dist, const int32_t *count, const int32_t *audit_flags, const double *audit,
                           int32_t *leg, double *leg_log, double *leg_start, double *goal, double *cur_pos, double *head,
                           int32_t *cmd_len, int32_t *cmd_index, int32_t *future_index, int32_t *flags) {
  int rc = list_check(c, "fleet leg open", B, 0, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  rc = null_check(c, "fleet leg open: null buffer", {outcome, n_flown, leg_end, final_dist, count, audit_flags, audit, leg, leg_log,
                                                     leg_start, goal, cur_pos, head, cmd_len, cmd_index, future_index, flags});
  if (rc) return rc;
  if (!std::isfinite(threshold) || !(threshold >= 0.0))
    return fail_locked(c, NEO_ERR_INVALID, "fleet leg open: the threshold must be finite and >= 0");
  if ((rc = fleet_legs_seq_check(c, "fleet leg open", seq, B))) return rc;
  if (max_legs < 1 || max_legs > NEO_FLEET_LEGS_MAX)
    return fail_locked(c, NEO_ERR_INVALID, "fleet leg open: max_legs must be in 1 .. NEO_FLEET_LEGS_MAX");
  return list_launch(c, B, subset, n_subset, [&](const LaunchList &list) {
    return fleet_leg_open(c, list, *seq, {max_legs, threshold, outcome, n_flown, leg_end, final_dist, count, audit_flags, audit,
                                          leg, leg_log, leg_start, goal, cur_pos, head, cmd_len, cmd_index, future_index, flags});
  });
}

int neo_fleet_leg_goal(neo_ctx *c, const neo_leg_sequences *seq, int B, int n, const int32_t *mission, const int32_t *leg_of,
                       double *goal, int32_t *exists) {
  if (!c) return NEO_ERR_INVALID;
  if (B < 0 || n < 0) return fail_locked(c, NEO_ERR_INVALID, "fleet leg goal: B and n must be >= 0");
  int rc = fleet_legs_seq_check(c, "fleet leg goal", seq, B);
  if (rc) return rc;
  if ((rc = null_check(c, "fleet leg goal: null buffer", {mission, leg_of, goal, exists}))) return rc;
  const bool table = seq->kind == NEO_LEGS_TABLE;
  if (table) {  // what the device forms cannot read on the host
    if (seq->seq_begin[0] != 0 || seq->seq_begin[B] != seq->n_goals)
      return fail_locked(c, NEO_ERR_INVALID, "fleet leg goal: seq_begin must run from 0 to n_goals");
    for (int b = 0; b < B; ++b) {
      const long long k = (long long)seq->seq_begin[b + 1] - (long long)seq->seq_begin[b];
      if (k < 1 || k > NEO_FLEET_LEGS_MAX)
        return fail_locked(c, NEO_ERR_INVALID, "fleet leg goal: every mission needs 1 .. NEO_FLEET_LEGS_MAX goals");
    }
  }
  if (n == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  const size_t bs = (size_t)B, ns = (size_t)n;
  HostStage st(c, kStagedUpTo);
  const auto fg = st.in(table ? seq->goals : nullptr, table ? (size_t)seq->n_goals * 2 : 0, 2);
  const auto fb = st.in(table ? seq->seq_begin : nullptr, table ? bs + 1 : 0, 2);
  const auto fi = st.in_optional(table ? nullptr : seq->mission_ids, bs);
  const auto fm = st.in(mission, ns), fl = st.in(leg_of, ns);
  const auto fo = st.out(goal, ns * 2);
  const auto fe = st.out(exists, ns);
  return st.run([&] {
    neo_leg_sequences dv = *seq;
    dv.goals = st.dev(fg);
    dv.seq_begin = st.dev(fb);
    dv.mission_ids = st.dev(fi);
    return launched(c, fleet_leg_goal(c, dv, B, n, st.dev(fm), st.dev(fl), st.dev(fo), st.dev(fe)));
  });
}

// ---- the fleet's record mode (traj_planner/record_planner.py:13-72; kernels: neo_record.hpp)
int neo_record_state_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, const double *cmd, int cap,
                         const int32_t *cmd_len, const int32_t *cmd_index, const double *head, double *cur_vel) {
  int rc = list_check(c, "record", B, 1, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  if ((rc = null_check(c, "record state: null buffer", {cmd, cmd_len, cmd_index, head, cur_vel}))) return rc;
  if (cap <= 0) return fail_locked(c, NEO_ERR_INVALID, "record state: cap must be > 0");
  return list_launch(c, B, subset, n_subset, [&](const LaunchList &list) {
    return record_state(c, list, cmd, cap, cmd_len, cmd_index, head, cur_vel);
  });
}

int neo_record_commit_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, const double *x, const double *head,
                          const double *tail, const int32_t *solved, const double *pose, const double *cur_vel,
                          const uint8_t *staging, int width, int height, const int32_t *mission_ids, int tick, int round,
                          int capacity, double *motion, double *wpts_local, double *tau, double *pose_rows, int32_t *meta,
                          uint8_t *images, int32_t *row_of, int32_t *n_rows, int32_t *dropped) {
  int rc = list_check(c, "record", B, 1, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  if (M < 2 || M > NEO_MAX_PIECES) return fail_locked(c, NEO_ERR_INVALID, "record commit: M must be in 2 .. 64");
  if (capacity < 1) return fail_locked(c, NEO_ERR_INVALID, "record commit: capacity must be >= 1");
  if (width < 1 || width > 4096 || height < 1 || height > 4096)
    return fail_locked(c, NEO_ERR_INVALID, "record commit: width and height must be in 1 .. 4096");
  rc = null_check(c, "record commit: null buffer", {x, head, tail, pose, cur_vel, staging, motion, wpts_local, tau, pose_rows,
                                                     meta, images, row_of, n_rows, dropped});
  if (rc) return rc;
  return list_launch(c, B, subset, n_subset, [&](const LaunchList &list) {
    return record_commit(c, list, RecordCommitArgs{M, x, head, tail, solved, pose, cur_vel, staging, width, height,
                                                   mission_ids, tick, round, capacity, motion, wpts_local, tau, pose_rows,
                                                   meta, images, row_of, n_rows, dropped});
  });
}

// ---- the learned warm start on resident arrays (traj_planner/neo_planner.py:10-51; kernels: neo_init.hpp)
int neo_init_motion_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, const double *pose, const double *cur_vel,
                        const double *head, const double *tail, float *motion) {
  int rc = list_check(c, "init motion", B, 1, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  if ((rc = null_check(c, "init motion: null buffer", {pose, cur_vel, head, tail, motion}))) return rc;
  return list_launch(c, B, subset, n_subset, [&](const LaunchList &list) {
    return init_motion(c, list, pose, cur_vel, head, tail, motion);
  });
}

int neo_init_head_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, const float *weights, size_t n_weights,
                      const float *feature, int feature_rows, const float *motion, float *out) {
  int rc = list_check(c, "init head", B, 1, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  if ((rc = null_check(c, "init head: null buffer", {weights, feature, motion, out}))) return rc;
  if (n_weights != (size_t)NEO_INIT_HEAD_FLOATS)
    return fail_locked(c, NEO_ERR_INVALID, "init head: n_weights must be NEO_INIT_HEAD_FLOATS (20817)");
  if (feature_rows != 1 && feature_rows != B)
    return fail_locked(c, NEO_ERR_INVALID, "init head: feature_rows must be 1 or B");
  return list_launch(c, B, subset, n_subset, [&](const LaunchList &list) {
    return init_head(c, list, weights, feature, feature_rows, motion, out);
  });
}

int neo_init_guess_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, const float *out, const double *pose,
                       double *x0) {
  int rc = list_check(c, "init guess", B, 1, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  if ((rc = null_check(c, "init guess: null buffer", {out, pose, x0}))) return rc;
  return list_launch(c, B, subset, n_subset, [&](const LaunchList &list) { return init_guess(c, list, out, pose, x0); });
}

// ---- the image backbone in front of the warm start (nn_trainer/nn_trainer.py:119-122; kernels: neo_backbone.hpp)
size_t neo_backbone_workspace_bytes(int n, int H, int W) {
  if (n <= 0 || H < 1 || W < 1 || (size_t)n * H * W > (size_t)INT32_MAX) return 0;
  return backbone_workspace_bytes(n, H, W);
}

// the checks of a backbone call (context unlocked); n = 0 passes them
static int backbone_check(neo_ctx *c, const float *weights, size_t n_weights, const uint8_t *images_u8, int n, int H, int W,
                          void *workspace, size_t workspace_bytes, float *feature_out) {
  if (!c) return NEO_ERR_INVALID;
  if (n < 0 || H < 1 || W < 1) return fail_locked(c, NEO_ERR_INVALID, "backbone: n must be >= 0, H and W >= 1");
  if ((size_t)n * H * W > (size_t)INT32_MAX)
    return fail_locked(c, NEO_ERR_INVALID, "backbone: n * H * W must stay below 2^31 (split the images over several calls)");
  int rc = null_check(c, "backbone: null buffer", {weights, images_u8, workspace, feature_out});
  if (rc) return rc;
  if (n_weights != (size_t)NEO_BACKBONE_FLOATS)
    return fail_locked(c, NEO_ERR_INVALID, "backbone: n_weights must be NEO_BACKBONE_FLOATS (11177752)");
  if (reinterpret_cast<uintptr_t>(workspace) % 16 || reinterpret_cast<uintptr_t>(weights) % 4)
    return fail_locked(c, NEO_ERR_INVALID, "backbone: workspace must be 16-byte aligned, weights 4-byte");
  if (n > 0 && workspace_bytes < backbone_workspace_bytes(n, H, W))
    return fail_locked(c, NEO_ERR_INVALID, "backbone: workspace smaller than neo_backbone_workspace_bytes(n, H, W)");
  return NEO_OK;
}

int neo_backbone_features_dev(neo_ctx *c, const float *weights, size_t n_weights, const uint8_t *images_u8, int n, int H,
                              int W, void *workspace, size_t workspace_bytes, float *feature_out) {
  const int rc = backbone_check(c, weights, n_weights, images_u8, n, H, W, workspace, workspace_bytes, feature_out);
  if (rc || n == 0) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  return launched(c, backbone_features(c, weights, images_u8, n, H, W, workspace, feature_out));
}

int neo_backbone_launch_times(neo_ctx *c, const float *weights, size_t n_weights, const uint8_t *images_u8, int n, int H, int W,
                              void *workspace, size_t workspace_bytes, float *feature_out, float *launch_ms) {
  int rc = backbone_check(c, weights, n_weights, images_u8, n, H, W, workspace, workspace_bytes, feature_out);
  if (rc) return rc;
  if (!launch_ms || n == 0) return fail_locked(c, NEO_ERR_INVALID, "backbone: launch times need launch_ms and n >= 1");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  // every exit destroys the events created so far; the first failing HIP call is the one reported
  hipEvent_t ev[NEO_BACKBONE_LAUNCHES + 1] = {};
  hipError_t e = hipSuccess;
  const char *what = "hipEventCreate";
  for (int i = 0; e == hipSuccess && i <= NEO_BACKBONE_LAUNCHES; ++i) e = hipEventCreate(&ev[i]);
  if (e == hipSuccess) {
    rc = launched(c, backbone_features(c, weights, images_u8, n, H, W, workspace, feature_out, ev));
    if (!rc) what = "hipStreamSynchronize", e = hipStreamSynchronize(c->stream);
    for (int i = 0; !rc && e == hipSuccess && i < NEO_BACKBONE_LAUNCHES; ++i)
      what = "hipEventElapsedTime", e = hipEventElapsedTime(&launch_ms[i], ev[i], ev[i + 1]);
  }
  for (hipEvent_t &v : ev)
    if (v) hipEventDestroy(v);
  if (!rc && e != hipSuccess) rc = fail(c, NEO_ERR_HIP, std::string("backbone: ") + what + ": " + hipGetErrorString(e));
  return rc;
}

int neo_backbone_activation_shape(int launch, int H, int W, int *h, int *w, int *c) {
  if (launch < 0 || launch >= NEO_BACKBONE_LAUNCHES || H < 1 || W < 1 || !h || !w || !c) return NEO_ERR_INVALID;
  backbone_activation_shape(launch, H, W, h, w, c);
  return NEO_OK;
}

int neo_backbone_activation_dev(neo_ctx *c, const float *weights, size_t n_weights, const uint8_t *images_u8, int n, int H, int W,
                                void *workspace, size_t workspace_bytes, int launch, float *act_out, size_t act_floats) {
  int rc = backbone_check(c, weights, n_weights, images_u8, n, H, W, workspace, workspace_bytes, act_out);
  if (rc) return rc;
  if (launch < 0 || launch >= NEO_BACKBONE_LAUNCHES)
    return fail_locked(c, NEO_ERR_INVALID, "backbone: launch must be 0 .. NEO_BACKBONE_LAUNCHES - 1");
  int h, w, ch;
  backbone_activation_shape(launch, H, W, &h, &w, &ch);
  if (act_floats != (size_t)n * h * w * ch)
    return fail_locked(c, NEO_ERR_INVALID, "backbone: act_floats must be n * h * w * c of neo_backbone_activation_shape");
  if (n == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  // the pool + fc writes act_out itself; a stem's or a convolution's buffer of the workspace is copied behind the launch
  const float *written = nullptr;
  rc = launched(c, backbone_features(c, weights, images_u8, n, H, W, workspace, act_out, nullptr, launch, &written));
  if (rc || written == act_out) return rc;
  HIPCHK(c, hipMemcpyAsync(act_out, written, act_floats * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  return NEO_OK;
}

// ---- the same backbone on bf16 storage and the bf16 matrix cores (kernels: neo_backbone_bf16.hpp)
int neo_backbone_pack_bf16_dev(neo_ctx *c, const float *weights_f32, size_t n_weights, void *packed_out, size_t packed_bytes) {
  if (!c) return NEO_ERR_INVALID;
  int rc = null_check(c, "backbone bf16 pack: null buffer", {weights_f32, packed_out});
  if (rc) return rc;
  if (n_weights != (size_t)NEO_BACKBONE_FLOATS)
    return fail_locked(c, NEO_ERR_INVALID, "backbone bf16 pack: n_weights must be NEO_BACKBONE_FLOATS (11177752)");
  if (packed_bytes != (size_t)NEO_BACKBONE_BF16_BYTES)
    return fail_locked(c, NEO_ERR_INVALID, "backbone bf16 pack: packed_bytes must be NEO_BACKBONE_BF16_BYTES (22396000)");
  if (reinterpret_cast<uintptr_t>(packed_out) % 16 || reinterpret_cast<uintptr_t>(weights_f32) % 4)
    return fail_locked(c, NEO_ERR_INVALID, "backbone bf16 pack: packed_out must be 16-byte aligned, weights 4-byte");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  return launched(c, backbone_bf16_pack(c, weights_f32, packed_out));
}

size_t neo_backbone_bf16_workspace_bytes(int n, int H, int W) {
  if (n <= 0 || H < 1 || W < 1 || (size_t)n * H * W > (size_t)INT32_MAX) return 0;
  return backbone_bf16_workspace_bytes(n, H, W);
}

// the checks of a bf16 backbone call (context unlocked); n = 0 passes them.  `out`: the call's required output
static int backbone_bf16_check(neo_ctx *c, const void *packed, size_t packed_bytes, const uint8_t *images_u8, int n, int H,
                               int W, void *workspace, size_t workspace_bytes, const void *out) {
  if (!c) return NEO_ERR_INVALID;
  if (n < 0 || H < 1 || W < 1) return fail_locked(c, NEO_ERR_INVALID, "backbone bf16: n must be >= 0, H and W >= 1");
  if ((size_t)n * H * W > (size_t)INT32_MAX)
    return fail_locked(c, NEO_ERR_INVALID, "backbone bf16: n * H * W must stay below 2^31 (split the images over several calls)");
  int rc = null_check(c, "backbone bf16: null buffer", {packed, images_u8, workspace, out});
  if (rc) return rc;
  if (packed_bytes != (size_t)NEO_BACKBONE_BF16_BYTES)
    return fail_locked(c, NEO_ERR_INVALID, "backbone bf16: packed_bytes must be NEO_BACKBONE_BF16_BYTES (22396000)");
  if (reinterpret_cast<uintptr_t>(workspace) % 16 || reinterpret_cast<uintptr_t>(packed) % 16)
    return fail_locked(c, NEO_ERR_INVALID, "backbone bf16: workspace and packed must be 16-byte aligned");
  if (n > 0 && workspace_bytes < backbone_bf16_workspace_bytes(n, H, W))
    return fail_locked(c, NEO_ERR_INVALID, "backbone bf16: workspace smaller than neo_backbone_bf16_workspace_bytes(n, H, W)");
  return NEO_OK;
}

int neo_backbone_features_bf16_dev(neo_ctx *c, const void *packed, size_t packed_bytes, const uint8_t *images_u8, int n, int H,
                                   int W, void *workspace, size_t workspace_bytes, float *feature_out) {
  const int rc = backbone_bf16_check(c, packed, packed_bytes, images_u8, n, H, W, workspace, workspace_bytes, feature_out);
  if (rc || n == 0) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  return launched(c, backbone_bf16_features(c, packed, images_u8, n, H, W, workspace, feature_out));
}

int neo_backbone_bf16_launch_times(neo_ctx *c, const void *packed, size_t packed_bytes, const uint8_t *images_u8, int n, int H,
                                   int W, void *workspace, size_t workspace_bytes, float *feature_out, float *launch_ms) {
  int rc = backbone_bf16_check(c, packed, packed_bytes, images_u8, n, H, W, workspace, workspace_bytes, feature_out);
  if (rc) return rc;
  if (!launch_ms || n == 0) return fail_locked(c, NEO_ERR_INVALID, "backbone bf16: launch times need launch_ms and n >= 1");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  // every exit destroys the events created so far; the first failing HIP call is the one reported
  hipEvent_t ev[NEO_BACKBONE_LAUNCHES + 1] = {};
  hipError_t e = hipSuccess;
  const char *what = "hipEventCreate";
  for (int i = 0; e == hipSuccess && i <= NEO_BACKBONE_LAUNCHES; ++i) e = hipEventCreate(&ev[i]);
  if (e == hipSuccess) {
    rc = launched(c, backbone_bf16_features(c, packed, images_u8, n, H, W, workspace, feature_out, ev));
    if (!rc) what = "hipStreamSynchronize", e = hipStreamSynchronize(c->stream);
    for (int i = 0; !rc && e == hipSuccess && i < NEO_BACKBONE_LAUNCHES; ++i)
      what = "hipEventElapsedTime", e = hipEventElapsedTime(&launch_ms[i], ev[i], ev[i + 1]);
  }
  for (hipEvent_t &v : ev)
    if (v) hipEventDestroy(v);
  if (!rc && e != hipSuccess) rc = fail(c, NEO_ERR_HIP, std::string("backbone bf16: ") + what + ": " + hipGetErrorString(e));
  return rc;
}

int neo_backbone_bf16_activation_dev(neo_ctx *c, const void *packed, size_t packed_bytes, const uint8_t *images_u8, int n, int H,
                                     int W, void *workspace, size_t workspace_bytes, int launch, uint16_t *act_bf16_out,
                                     float *act_f32_out, size_t act_elems) {
  const void *some = act_bf16_out ? static_cast<const void *>(act_bf16_out) : act_f32_out;
  int rc = backbone_bf16_check(c, packed, packed_bytes, images_u8, n, H, W, workspace, workspace_bytes, some);
  if (rc) return rc;
  if (launch < 0 || launch >= NEO_BACKBONE_LAUNCHES)
    return fail_locked(c, NEO_ERR_INVALID, "backbone bf16: launch must be 0 .. NEO_BACKBONE_LAUNCHES - 1");
  const bool fc = launch == NEO_BACKBONE_LAUNCHES - 1;
  if (fc && (act_bf16_out || !act_f32_out))
    return fail_locked(c, NEO_ERR_INVALID, "backbone bf16: the pool and fc write fp32 only: act_bf16_out NULL, act_f32_out given");
  int h, w, ch;
  backbone_activation_shape(launch, H, W, &h, &w, &ch);
  if (act_elems != (size_t)n * h * w * ch)
    return fail_locked(c, NEO_ERR_INVALID, "backbone bf16: act_elems must be n * h * w * c of neo_backbone_activation_shape");
  if (n == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  // the pool + fc writes act_f32_out itself; a stem or a convolution writes its fp32 values there through its debug
  // epilogue, and its bf16 buffer of the workspace is copied behind the launch
  const void *written = nullptr;
  rc = launched(c, backbone_bf16_features(c, packed, images_u8, n, H, W, workspace, fc ? act_f32_out : nullptr, nullptr, launch,
                                          &written, fc ? nullptr : act_f32_out));
  if (rc || fc || !act_bf16_out) return rc;
  HIPCHK(c, hipMemcpyAsync(act_bf16_out, written, act_elems * sizeof(uint16_t), hipMemcpyDeviceToDevice, c->stream));
  return NEO_OK;
}

}  // extern "C"
