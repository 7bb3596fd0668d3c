// neo_host.hpp -- host-side state shared by the translation units of libneo_planner_hip.so: the context behind
// the opaque neo_ctx of include/neo_planner.h, the argument packs of the kernel families and the per-family
// dispatch entry points (defined in neo_disp_*.hip, one family per translation unit so they build in parallel).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/neo_planner.h"
#include "neo_map.hpp"
#include "neo_launch_list.hpp"

namespace neo {
// the lane-group policies of neo_device.hpp: visit_slots below only names them, the units that launch MINCO kernels
// include their definitions
struct WaveLanes;
template <int>
struct WaveLanesPD;

struct MapEntry {
  int kind = -1;  // 0 = 2-D reference map, 1 = 3-D field
  int elem = NEO_F64;
  void *data = nullptr;  // device
  Map2D m2{};
  Map3D m3{};
  int slot = -1;  // index into the device-side map table
  unsigned long long version = 0;  // 2-D maps: a new value at every upload / build (keys the geo blocked mask)
};

// the geo warm start's device state (neo_disp_geo.hip)
struct GeoMask {
  void *bits = nullptr;
  unsigned long long version = 0;
};
struct GeoState {
  std::map<int, GeoMask> masks;  // by scene id
  void *cells = nullptr, *heap = nullptr;
  unsigned *epochs = nullptr;
  int *work = nullptr;
  size_t cells_cap = 0;          // cells per slot
  int nslots = 0;
  unsigned long long searches = 0;  // requests launched since the stamps were last cleared
  size_t budget = size_t(2) << 30;
  // device GeoScene[] and what it holds: [0] with the scenes' masks, [1] the direct form's, without any
  void *table[2] = {nullptr, nullptr};
  std::vector<char> table_host[2];
  long long mask_builds = 0;     // geo_mask_kernel launches since the context was created (neo_geo_mask_builds)
};

// the depth camera's device state (neo_disp_depth.hip): the pixel tables of a call, and the images' maxima when the
// caller keeps none
struct DepthState {
  float *uv = nullptr;          // u (padded) then v of the call in flight
  unsigned *max_bits = nullptr;
  size_t max_cap = 0;           // images `max_bits` has room for
  unsigned long long *box_tests = nullptr;  // optional device counter (neo_depth_box_test_counter)
};

struct ProfileSlot {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
  int64_t launches = 0;
  double ms = 0.0;
};

}  // namespace neo

struct neo_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipStream_t home_stream = nullptr;  // the stream of neo_ctx_create (neo_ctx_set_stream(NULL) returns to it)
  neo_params params{};
  neo::DevParams dev{};
  std::map<int, neo::MapEntry> maps;
  std::string err;
  std::recursive_mutex mu;  // recursive: the host-pointer entry points hold it across their *_dev call
  int *tickets = nullptr;  // ring of work counters for optimize_group_kernel launches (one per launch in flight)
  unsigned ticket_next = 0;
  // device-side table of maps (rebuilt when a map changes)
  void *table2d = nullptr, *table3d = nullptr;
  int n2d = 0, n3d = 0;
  bool table_dirty = true;
  // scratch for the host-pointer entry points
  void *scratch = nullptr;
  size_t scratch_bytes = 0;
  // pinned mirror of the scratch layout of neo_optimize_batch: ONE copy in and ONE copy out per call instead of four
  // and six from pageable memory (each of those stages through the runtime and waits)
  void *pinned = nullptr;
  size_t pinned_bytes = 0;
  bool profile = false;
  neo::ProfileSlot prof[NEO_KERNEL_COUNT];
  long long *sample_counter = nullptr;  // optional device array [B] (neo_optimize_sample_counter)
  // optimize_kernel launches since the context was created, by wrapper: [0] the one compiled for its member's fixed plan,
  // [1] the one with run-time selectors (neo_launch_opt.hpp; read by neo_optimize_plan_launches)
  int64_t opt_plan_launches[2] = {0, 0};
  int *progress = nullptr;              // optional device-accessible counter of finished trajectories (neo_optimize_progress_counter)
  const int *dispatch_order = nullptr;  // optional device permutation [B] (neo_optimize_dispatch_order)
  int order_B = 0;                      // batch size the permutation was given for (ignored for any other B)
  double *trace = nullptr;              // optional device array [B][trace_cap][4] (neo_optimize_trace)
  double *trace_xg = nullptr;           // optional device array [B][trace_cap][2][n] (neo_optimize_trace_xg)
  int trace_cap = 0;
  int *order_buf = nullptr;             // device copy of a host permutation (neo_optimize_dispatch_order_host)
  size_t order_cap = 0;
  int *sample_order = nullptr;          // context-owned device copy of the ESDF-lookup kernel's permutation
  size_t sample_order_cap = 0;          // (neo_sampled_terms_dispatch_order; never the optimiser's, never caller-owned)
  int sample_order_B = 0;
  int edt_flags = 0;                    // NEO_EDT_* (neo_esdf_build_config)
  unsigned long long map_serial = 0;    // MapEntry::version source
  neo::GeoState geo;
  neo::DepthState depth;
};

namespace neo {

inline int fail(neo_ctx *c, int code, const std::string &msg) {
  if (c) c->err = msg;
  return code;
}

#define HIPCHK(c, call)                                                                     \
  do {                                                                                      \
    hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return fail(c, NEO_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));       \
  } while (0)

// device allocation released on every exit path unless release()d into a longer-lived owner
struct DevBuf {
  void *p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() {
    if (p) hipFree(p);
  }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
  void *release() {
    void *q = p;
    p = nullptr;
    return q;
  }
  template <typename T>
  T *as() const { return static_cast<T *>(p); }
};

struct ProfScope {
  neo_ctx *c;
  int k;
  hipEvent_t a = nullptr, b = nullptr;
  ProfScope(neo_ctx *c_, int k_) : c(c_), k(k_) {
    if (c->profile) {
      hipEventCreate(&a);
      hipEventCreate(&b);
      hipEventRecord(a, c->stream);
    }
  }
  ~ProfScope() {
    if (c->profile) {
      hipEventRecord(b, c->stream);
      c->prof[k].pending.emplace_back(a, b);
    }
  }
};

struct EvalArgs {
  int B, M;
  const double *x, *head, *tail;
  double *cost, *costs4, *grad, *coeffs;
  int *status;
};

struct OptArgs {
  int B, M;
  const void *table;
  const int *slots;  // device array [B] of map-table slots, or NULL (all trajectories use table[0])
  int nmaps;         // entries of `table` (slots are checked against it on the device)
  const double *x0;  // start points (NULL: read from x, the in-place form)
  double *x;
  const double *head, *tail;
  double *costs4, *costs4_last;
  int *nit, *nfev, *status;
  // budgeted launches (neo_optimize_batch_budget_dev); all zero otherwise
  double *state = nullptr;       // [B][state_doubles] optimiser state of suspended runs
  int state_doubles = 0;
  int budget = 0;                // evaluations per trajectory and launch
  int resume = 0;                // continue suspended runs instead of starting from x0
  const int *subset = nullptr;   // device array of n_subset trajectory indices: launch these only (workgroup i -> subset[i])
  int n_subset = 0;
  int traj_total = 0;            // B of the arrays (subset entries are checked against it on the device)
};

struct SampleArgs {
  int B, M;
  const void *coeffs;  // [B][6M][D] doubles, or floats when io32
  const double *ts;
  double *costs2;
  void *grad_C, *grad_T;  // doubles, or floats when io32
  bool io32 = false;      // neo_sampled_terms_batch_f32_dev (fp32 sampling only)
};

// neo_eval_traj_batch: one traj_state_kernel launch (neo_disp_audit.hip)
struct TrajStateArgs {
  int B, M;
  const double *x, *head, *tail;
  double hz;
  int K;
  double *state;
  int *count;
};

// neo_audit_traj_batch_dev: one audit_kernel launch (neo_disp_audit.hip)
struct AuditArgs {
  int B, M;
  MapRef maps;  // of the call's kind
  const double *x, *head, *tail;
  double hz, w[3];
  double *audit;
  int *count, *flags;
};

// neo_fleet_*_dev: one launch of a fleet kernel each (neo_disp_fleet.hip, kernels in neo_fleet.hpp).  Every array is
// indexed by mission; the LaunchList picks the missions launched, the MapRef (target, audit) is the 2-D map table.
struct FleetTargetArgs {
  const double *cur_pos, *goal, *jitter;
  double longitu, lateral, move_vel;
  double *tail;
  int *near_goal, *lateral_steps, *flags;
};
struct FleetCmd {  // the resident command arrays
  double *cmd;
  int cap;
  int *cmd_len, *cmd_index, *future_index;
};
struct FleetSpliceArgs {
  int M;
  const double *x, *head, *tail;
  const int *solved;
  double hz;
  int first;
  int *flags;
};
struct FleetAuditArgs {
  const double *cmd;
  int cap;
  const int *n_flown;
  int stride;
  double hz, w[3];
  double *audit;
  int *count, *flags;
};
int fleet_target(neo_ctx *c, const LaunchList &l, const MapRef &m, const FleetTargetArgs &a);
// jitter [B][2] by mission: the re-targeting draws of (tick, target) from the missions' own counter streams
int fleet_jitter(neo_ctx *c, const LaunchList &l, uint64_t seed, int tick, int target, const int *mission_ids,
                 double *jitter);
int fleet_advance(neo_ctx *c, const LaunchList &l, const FleetCmd &m, int step, int ahead, double *cur_pos, double *head);
int fleet_splice(neo_ctx *c, const LaunchList &l, const FleetCmd &m, const FleetSpliceArgs &a);
int fleet_audit(neo_ctx *c, const LaunchList &l, const MapRef &m, const FleetAuditArgs &a);
// the missions' camera poses (eye x y z, cos, sin) from where they are on their command arrays
int fleet_pose(neo_ctx *c, const LaunchList &l, const FleetCmd &m, const double *cur_pos, const double *goal, double eye_z,
               double *pose);
// mode "warmstart": the carried plan as x0 [B][n], and what a mission keeps of a target round's plan.  T_min, T_max: the
// context's; init_ts: a HOST array of M durations, handed to the kernel by value
struct FleetWarmCarryArgs {
  int M;
  const double *x, *head;                 // [B][n], [B][3][2] by mission
  const int *solved, *status, *attempts;  // [B]: plan_dev's
  const double *init_ts;                  // host
  double *wpts_local, *ts_carry;          // [B][2][M - 1], [B][M]
};
int fleet_warm_guess(neo_ctx *c, const LaunchList &l, int M, const double *head, const double *wpts_local,
                     const double *ts_carry, double *x0);
int fleet_warm_carry(neo_ctx *c, const LaunchList &l, const FleetWarmCarryArgs &a);
// goal routes (kernels in neo_track.hpp): the ragged route table, by mission
struct FleetRoutes {
  const double *vertices;  // [n_vertices][2]
  int n_vertices;
  const int *route_begin;  // [B + 1]
  const double *speed;     // [B]
  const int *closed;       // [B], or NULL: all open
};
struct FleetTrackArgs {
  const double *cmd;
  int cap;
  const int *n_flown;
  int stride;
  double hz, radius;
  double *track;
  int *count, *flags;
};
int fleet_goal(neo_ctx *c, const LaunchList &l, const FleetRoutes &r, double t, double *goal);
// rows appended to a command array that ends before cmd_index + step + 1 (m.future_index is not used)
int fleet_hold(neo_ctx *c, const LaunchList &l, const FleetCmd &m, int step, int *flags);
int fleet_track_audit(neo_ctx *c, const LaunchList &l, const FleetRoutes &r, const FleetTrackArgs &a);
// the flight model (kernels in neo_flight.hpp): the advance with a drone that lags, and its tracking-error record
struct FleetFlyArgs {
  int step, ahead, first, settle;
  double reach;
  const int *mission_ids;              // [B], or NULL: the mission's index
  const double *goal;                  // [B][2]
  double *drone, *flown;               // [B][8], [B][cap][3][2]
  int *flown_len, *saturated, *flags;  // [B]
  double *cur_pos, *head;              // [B][2], [B][3][2]
};
struct FleetFlyErrorArgs {
  const double *flown, *cmd;
  int cap;
  const int *flown_len, *cmd_len;
  int stride;
  double *fly;
  int *count, *flags;
};
int fleet_fly(neo_ctx *c, const LaunchList &l, const neo_flight_model &model, const FleetCmd &m, const FleetFlyArgs &a);
int fleet_fly_error(neo_ctx *c, const LaunchList &l, const FleetFlyErrorArgs &a);
// campaigns (kernels in neo_legs.hpp): what a leg was, then its row of the log and the next leg's start
struct FleetLegCloseArgs {
  const int *outcome;                  // [B]: NEO_LEG_*
  const double *cmd;
  int cap;
  const int *cmd_len, *cmd_index;
  const double *head, *goal;           // [B][3][2], [B][2]
  int *n_flown;
  double *leg_end, *final_dist;        // [B][2][2], [B]
};
struct FleetLegOpenArgs {
  int max_legs;
  double threshold;                    // target_reach_threshold
  const int *outcome, *n_flown;        // [B]: the caller's, close's
  const double *leg_end, *final_dist;  // [B][2][2], [B]: close's
  const int *count, *audit_flags;      // [B]: the audit's
  const double *audit;                 // [B][NEO_AUDIT_FIELDS]
  int *leg;                            // [B]: the index of the leg being flown
  double *leg_log;                     // [B][max_legs][NEO_LEG_FIELDS]
  double *leg_start;                   // [B][2]: where the leg being flown began
  double *goal, *cur_pos, *head;       // [B][2], [B][2], [B][3][2]
  int *cmd_len, *cmd_index, *future_index, *flags;
};
int fleet_leg_close(neo_ctx *c, const LaunchList &l, const FleetLegCloseArgs &a);
int fleet_leg_open(neo_ctx *c, const LaunchList &l, const neo_leg_sequences &seq, const FleetLegOpenArgs &a);
// goal[n][2], exists[n] for the n pairs (mission[p], leg_of[p]); every pointer, seq's too, a device array
int fleet_leg_goal(neo_ctx *c, const neo_leg_sequences &seq, int B, int n, const int *mission, const int *leg_of,
                   double *goal, int *exists);

// neo_record_*_dev: the fleet's `record` mode (neo_disp_record.hip, kernels in neo_record.hpp).  Every pointer is a
// device array; the arguments were checked by the C ABI.
struct RecordCommitArgs {
  int M;
  const double *x, *head, *tail;  // [B][n], [B][3][2], [B][3][2] by mission
  const int *solved;              // [B], or NULL: every launched mission
  const double *pose, *cur_vel;   // [B][5], [B][2]
  const unsigned char *staging;   // [B][H][W]
  int W, H;
  const int *mission_ids;         // [B], or NULL: the mission's index
  int tick, round, capacity;
  double *motion, *wpts_local, *tau, *pose_rows;  // the dataset, `capacity` rows each
  int *meta;
  unsigned char *images;
  int *row_of, *n_rows, *dropped;  // [launched], [1], [1]
};
int record_state(neo_ctx *c, const LaunchList &l, const double *cmd, int cap, const int *cmd_len, const int *cmd_index,
                 const double *head, double *cur_vel);
int record_commit(neo_ctx *c, const LaunchList &l, const RecordCommitArgs &a);  // rank, then commit

// neo_init_*_dev: the learned warm start on resident arrays (neo_disp_init.hip, kernels in neo_init.hpp): one launch
// each.  Every pointer is a device array indexed by request; the arguments were checked by the C ABI.
int init_motion(neo_ctx *c, const LaunchList &l, const double *pose, const double *cur_vel, const double *head,
                const double *tail, float *motion);
int init_head(neo_ctx *c, const LaunchList &l, const float *weights, const float *feature, int feature_rows,
              const float *motion, float *out);
int init_guess(neo_ctx *c, const LaunchList &l, const float *out, const double *pose, double *x0);  // T_min, T_max: the context's

// neo_backbone_*: the image backbone in front of them (neo_disp_backbone.hip, kernels in neo_backbone.hpp): n uint8
// images of H x W -> feature_out [n][24], 21 launches; `workspace` holds backbone_workspace_bytes(n, H, W) bytes.
// events: NULL, or NEO_BACKBONE_LAUNCHES + 1 events recorded in front of the chain and behind every launch
// last: the chain ends behind launch `last` (neo_backbone_activation_dev; 0 .. NEO_BACKBONE_LAUNCHES - 1, the default is the
// whole chain); written: NULL, or where the buffer that launch wrote is returned (feature_out for the pool + fc)
size_t backbone_workspace_bytes(int n, int H, int W);
int backbone_features(neo_ctx *c, const float *weights, const unsigned char *images, int n, int H, int W, void *workspace,
                      float *feature_out, hipEvent_t *events = nullptr, int last = NEO_BACKBONE_LAUNCHES - 1,
                      const float **written = nullptr);
// h, w, c of what launch `launch` writes an image of H x W ([h][w][c] channels-last; 1, 1, 24 for the pool + fc)
void backbone_activation_shape(int launch, int H, int W, int *h, int *w, int *c);

// neo_backbone_*bf16*: the same chain on bf16 storage and the bf16 matrix cores (neo_disp_backbone_bf16.hip, kernels in
// neo_backbone_bf16.hpp).  packed: NEO_BACKBONE_BF16_BYTES bytes (backbone_bf16_pack makes them from the fp32 blob);
// `workspace` holds backbone_bf16_workspace_bytes(n, H, W) bytes.  events, last, written: as above (a bf16 buffer of the
// workspace, or feature_out); dbg_last: NULL, or where launch `last` (a stem or a convolution) also writes its fp32
// values before the rounding
size_t backbone_bf16_workspace_bytes(int n, int H, int W);
int backbone_bf16_pack(neo_ctx *c, const float *weights, void *packed);
int backbone_bf16_features(neo_ctx *c, const void *packed, const unsigned char *images, int n, int H, int W, void *workspace,
                           float *feature_out, hipEvent_t *events = nullptr, int last = NEO_BACKBONE_LAUNCHES - 1,
                           const void **written = nullptr, float *dbg_last = nullptr);

// neo_batch_*_dev: the `batch` planner mode on resident arrays (neo_disp_batch.hip, kernels in neo_batch.hpp).  P =
// the list's n requests; tau, off and w are HOST arrays (M, K and 4 values), handed to the kernels by value.
struct BatchCandArgs {
  int M, K;
  const double *head, *tail;  // [B][3][2], by request
  const int *slots;           // [B] by request, or NULL
  const double *tau, *off;    // host
  double *x0, *head_k, *tail_k;  // packed [P * K] rows
  int *slots_k;                  // packed, or NULL
};
struct BatchSelectArgs {
  int n, K;
  RunRowsIn packed;                       // [P * K] rows: the optimiser's results (nfev: or NULL)
  const double *w;                        // host, 4 weights
  int *chosen;                            // everything below by request
  double *cand_cost;
  int *solved;
  RunRows out;                            // nit, nfev: or NULL
  int *nit_total, *opt_runs;
  int *fallback, *n_fallback;             // [P] and [1]
};
int batch_candidates(neo_ctx *c, const LaunchList &l, const BatchCandArgs &a);
int batch_select(neo_ctx *c, const LaunchList &l, const BatchSelectArgs &a);
// pending[P] (request indices, or -1) packed in place in position order, *n_pending their number: one launch
int batch_compact(neo_ctx *c, int P, int *pending, int *n_pending);

// neo_plan_*_dev: BatchPlanner.plan's retry chain on resident arrays (neo_disp_plan.hip, kernels in neo_plan.hpp).
// P = the list's n requests; frac and tau are HOST arrays (M - 1 and M values), handed to the kernel by value.
struct PlanGuessArgs {
  int M;
  const double *head, *tail;     // [B][3][D], by request
  const int *slots;              // [B] by request, or NULL
  const double *x_init;          // [B][n] by request, or NULL: the caller's start points instead of the straight line
  const double *noise;           // packed [P][D][M - 1], or NULL
  const double *frac, *tau;      // host (not read with x_init)
  double *x0, *head_k, *tail_k;  // packed [P] rows
  int *slots_k;                  // packed, or NULL
};
struct PlanMergeArgs {
  int n, ldx, reset;                      // ldx >= n: the row length of out.x (NaN behind a row's n values)
  RunRowsIn packed;                       // [P] rows: the optimiser's results
  RunRows out;                            // everything below by request
  int *attempts;
  long long *nit_total;
  int *solved;
  int *failed, *n_failed, *bad_scene;     // [P], [1] and [1] (not zeroed here); n_failed NULL: the merge alone, no
                                          // compaction launch after it (a group of a mixed chain)
};
int plan_guess(neo_ctx *c, const LaunchList &l, int D, const PlanGuessArgs &a);
int plan_merge(neo_ctx *c, const LaunchList &l, const PlanMergeArgs &a);
// noise [P][D][M - 1] packed: the retry jitter of attempt `attempt` from the requests' own counter streams
int plan_jitter(neo_ctx *c, const LaunchList &l, int M, int D, uint64_t seed, int attempt, const int *stream_ids,
                double *noise);

// neo_adaptive_*_dev: per-request waypoint counts and the plan chain over groups of one count (neo_disp_adaptive.hip,
// kernels in neo_adaptive.hpp; a group's merge is plan_merge above): one launch each on the context's stream.  Every
// pointer is a device array but seg_begin / seg_len (HOST, NEO_MAX_PIECES values each, handed to the kernel by value);
// the arguments were checked.
int adaptive_count(neo_ctx *c, const LaunchList &l, int D, const double *head, const double *tail, double seg_len,
                   int max_waypoints, int *counts, int *clamped);
int adaptive_bucket(neo_ctx *c, const LaunchList &l, const int *counts, int *order, int *bucket_begin, int *total);
int adaptive_compact(neo_ctx *c, const int *seg_begin, const int *seg_len, int *pending, int *n_failed);

// neo_geo_search_batch_dev / neo_geo_guess_dev / neo_geo_prune_batch (neo_disp_geo.hip); the context is locked and its
// tables rebuilt.  The requests are `list` over rows of start / target with `stride` doubles a request (2: dense (B, 2)
// arrays; 6: head / tail [B][3][2] where they lie); x0 [B][7] or NULL; tau: the three start values of x0 (HOST, read
// with x0 only); direct: the search reads the maps' records, and no mask is built or read
struct GeoArgs {
  LaunchList list;
  const int *slots;  // device array [B] of 2-D map-table slots, or NULL (all requests use scene_id)
  const double *start, *target;
  int stride;
  int max_exp, path_cap;
  double *key_pts, *path, *path_cost;
  int *path_len, *expansions, *flags;
  double *x0;
  const double *tau;
  bool direct;
};
int geo_search(neo_ctx *c, int scene_id, const GeoArgs &a);
int geo_prune(neo_ctx *c, int scene_id, int B, const int *slots, const double *paths, const int *path_len, int stride,
              double *key_pts);
void geo_release(neo_ctx *c);             // frees every geo buffer (neo_ctx_destroy)
void geo_forget(neo_ctx *c, int scene_id);  // frees the scene's mask (map drop)

// neo_depth_render_batch_dev (neo_disp_depth.hip, kernels in neo_depth.hpp): the tables, the render pass and, with
// depth_u8, the normalise pass, on the context's stream; every pointer is a device array, the arguments are checked
struct DepthCall {
  int W, H;
  double focal, max_range;
  const double *boxes;
  const int *box_begin;
  int n_scenes;
  const int *scene_index;  // or NULL
  int B;
  const double *pose;
  float *depth_m;
  unsigned char *depth_u8;  // or NULL
  float *depth_max;         // or NULL
};
int depth_render(neo_ctx *c, const DepthCall &a);
void depth_release(neo_ctx *c);  // frees the camera's buffers (neo_ctx_destroy)

// neo_onboard_integrate_batch_dev (neo_disp_onboard.hip, kernel in neo_onboard.hpp): one launch on the context's
// stream; every pointer is a device array, the arguments are checked, N and half sized by the caller
struct OnboardCall {
  LaunchList list;
  const float *depth_m;
  const double *pose;
  int W, H;
  double focal;
  int grid_w, grid_h;
  double res;
  const double *origins;
  double range, z_lo, z_hi;
  int l_hit, l_miss, l_lo, l_hi;
  int N, half;
  int8_t *logodds, *occupancy;
  int *changed;
};
int onboard_window_half(int width, double focal, double range, double res);  // cells from the eye's cell to the window's edge
size_t onboard_lds_need(int half, int N, int height);                         // LDS bytes of a launch
size_t onboard_lds_limit();
int onboard_integrate(neo_ctx *c, const OnboardCall &k);

// the map kernels' launches (neo_disp_esdf.hip, kernels in neo_esdf.hpp), on the context's stream.  Every pointer is a
// device array the caller owns -- the C ABI carves the work arrays from the context's scratch -- and nothing is
// allocated; the arguments are the ones neo_esdf_* checked.
struct Edt2DWork {  // work arrays of a W x H build: v and z are the sweeps' stacks (maps beyond 512 x 512 only)
  const int8_t *occ;
  int *g, *v;        // [W * H] each
  double *z;         // [H * (W + 1)]
  double *dist, *gx, *gy;  // [W * H] each: the results, as the reference's arrays
};
void esdf_build_2d(neo_ctx *c, const Edt2DWork &w, int W, int H, double res, double4 *rec);  // EDT, gradient, records
// the same kernels for `nmap` maps of one size in one set of launches: occ and the work arrays hold the maps back to
// back (z: H * (W + 1) a map), recs[nmap] (device) names each map's record buffer; gx and gy are not kept
void esdf_build_2d_batch(neo_ctx *c, const Edt2DWork &w, int nmap, int W, int H, double res, double4 *const *recs);
void esdf_pack_2d(neo_ctx *c, const double *dist, const double *gx, const double *gy, size_t ncell, double4 *rec);
void esdf_pack_3d(neo_ctx *c, const void *src, int src_dtype, int nx, int ny, int nz, int store_dtype, int layout, int nbx,
                  int nby, int nbz, void *dst);  // nbx, nby, nbz: bricks per axis (NEO_LAYOUT_BRICK only)
// x, y and z pass of the exact 3-D EDT: occupancy -> gx (row distances) -> sq (squared plane distances) -> dist
void esdf_edt_3d(neo_ctx *c, const uint8_t *occ, int nx, int ny, int nz, double res, uint16_t *gx, uint32_t *sq, float *dist);
void esdf_query(neo_ctx *c, const MapEntry &e, int n, const double *pts, double *dist, double *grad);

// FLAT slots of the optimiser vectors: n <= 64, 128, 192 or 256 variables
inline int slots_for(int M, int D) {
  const int n = D * (M - 1) + M;
  const int ns = (n + kWave - 1) / kWave;
  return ns <= 3 ? (ns < 1 ? 1 : ns) : 4;  // (3: cfg5's n = 161 -- a quarter fewer optimiser-vector instructions than 4 slots)
}

// doubles of a suspended run's state (neo_optimize_batch_budget_dev; layout: neo_kernels.hpp save_run), n variables and m pairs
inline size_t opt_state_doubles(int n, int m) { return 64 + 5 * (size_t)n + kWave + 2 * (size_t)m * (size_t)n; }

// ---- run-time values to template arguments: the one place where a field's (element type, layout) and a problem's
// (FLAT slots, lane layout) become types.  Each visitor calls f with empty tag values; the unit's lambda reads the types
// off them and names the kernel it owns.  Templates and inlined lambdas only: nothing is allocated, no std::function.
template <class T>
struct Type {
  using type = T;
};
template <class Tag>
using type_of = typename Tag::type;  // type_of<decltype(tag)>
template <int V>
using Int = std::integral_constant<int, V>;
template <typename... E>
struct Elems {};
template <int... LAY>
struct Layouts {};
template <typename E>
constexpr int elem_code = std::is_same<E, float>::value ? NEO_F32 : NEO_F16;  // float | __half

template <typename Real, typename E, class F, int... LAY>
bool visit_layout(int layout, int &rc, F &f, Layouts<LAY...>) {
  return ((layout == LAY && (rc = f(Type<Lookup3D<Real, E, LAY>>{}), true)) || ...);
}
// f(Type<Lookup3D<Real, E, LAY>>) for the stored element type and layout of a 3-D field, out of the ones the family has
// kernels for: only those are instantiated.  Anything else -- nothing neo_esdf_upload_3d admits -- is NEO_ERR_INVALID.
template <typename Real, class F, typename... E, int... LAY>
int visit_field(neo_ctx *c, int elem, int layout, Elems<E...>, Layouts<LAY...> lays, F f) {
  int rc = NEO_OK;
  if (((elem == elem_code<E> && visit_layout<Real, E>(layout, rc, f, lays)) || ...)) return rc;
  return fail(c, NEO_ERR_INVALID, "unknown 3-D field layout / element type");
}
// every field neo_esdf_upload_3d admits: fp32 or fp16 elements in any of the four layouts
template <typename Real, class F>
int visit_field(neo_ctx *c, int elem, int layout, F f) {
  return visit_field<Real>(c, elem, layout, Elems<float, __half>{},
                           Layouts<NEO_LAYOUT_LINEAR, NEO_LAYOUT_YZ4, NEO_LAYOUT_CELL8, NEO_LAYOUT_BRICK>{}, f);
}

// lane = (piece, dimension) whenever D * M fits the wavefront (cfg2: 63 lanes busy in the PIECE-layout phases instead of
// 21, a third of the per-dimension state per lane); lane = piece otherwise.  flags bit 512 forces the latter (comparison
// runs).
inline bool lane_piece_dim(int D, int M, int flags) { return D * M <= kWave && !(flags & 512); }

// f(Int<NS>, Type<LG>) for the FLAT slots and the lane layout of an M-piece problem: one or two slots on either lane
// layout, three and four on WaveLanes (n > 128 means D * M > 64: lane = piece).  A family without kernels beyond MAX_NS
// slots instantiates none and checks slots_for() first, with its own message.
template <int D, int MAX_NS = 4, class F>
int visit_slots(int M, int flags, F f) {
  const bool pd = lane_piece_dim(D, M, flags);
  switch (slots_for(M, D)) {
    case 1: return pd ? f(Int<1>{}, Type<WaveLanesPD<D>>{}) : f(Int<1>{}, Type<WaveLanes>{});
    case 2: return pd ? f(Int<2>{}, Type<WaveLanesPD<D>>{}) : f(Int<2>{}, Type<WaveLanes>{});
    case 3:
      if constexpr (MAX_NS >= 3) return f(Int<3>{}, Type<WaveLanes>{});
      break;
    default:
      if constexpr (MAX_NS >= 4) return f(Int<4>{}, Type<WaveLanes>{});
      break;
  }
  return NEO_ERR_INVALID;
}

// ---- per-family dispatch (neo_disp_*.hip; the fleet, batch, geo and map units' entry points are declared with their
// argument packs above)
int dispatch_eval(neo_ctx *c, const MapEntry &e, int D, const EvalArgs &a);
int dispatch_sample(neo_ctx *c, const MapEntry &e, int D, const SampleArgs &a);
int dispatch_audit(neo_ctx *c, int kind, int elem, int layout, int D, const AuditArgs &a);  // neo_disp_audit.hip
int dispatch_traj_state(neo_ctx *c, int D, const TrajStateArgs &a);                         // neo_disp_audit.hip
// the families behind dispatch_opt (neo_abi.hip)
int launch_opt_2d(neo_ctx *c, int D, bool f32, const OptArgs &a);           // neo_disp_opt2d.hip
int launch_opt_3d_f32(neo_ctx *c, int elem, int layout, const OptArgs &a);  // neo_disp_opt3d_f32.hip
int launch_opt_3d_f64(neo_ctx *c, int elem, int layout, const OptArgs &a);  // neo_disp_opt3d_f64.hip
int launch_opt_3d_w2(neo_ctx *c, int elem, int layout, const OptArgs &a);   // neo_disp_opt3d_w2.hip
int launch_opt_3d_x(neo_ctx *c, int elem, int layout, const OptArgs &a);    // neo_disp_opt3d_x.hip
int launch_opt_groups(neo_ctx *c, int elem, int layout, const OptArgs &a);  // neo_disp_group.hip
int launch_opt_3d_f64_w2(neo_ctx *c, int elem, int layout, const OptArgs &a);
int launch_opt_3d_budget(neo_ctx *c, int elem, int layout, const OptArgs &a);  // neo_disp_opt3d_b.hip
int launch_opt_2d_w2(neo_ctx *c, bool f32, const OptArgs &a);
int launch_opt_2d_x(neo_ctx *c, int D, const OptArgs &a);                   // neo_disp_opt2d_x.hip (all-fp32 mode)
int launch_opt_groups_2d(neo_ctx *c, bool f32, const OptArgs &a);           // neo_disp_group.hip (D = 2, nearest-cell map)

}  // namespace neo
