/*
 * neo_planner.h -- C ABI of libneo_planner_hip.so (MI355X / gfx950).
 *
 * The reference (Amos-Chen98/neo-planner) has no FFI: its boundary is the Python
 * object protocol between ros_node/traj_planner_node.py and
 * traj_planner/expert_planner.py:MinJerkPlanner, and between MinJerkPlanner and
 * map_server/esdf.py:ESDF.  This header is the boundary the MI355X path puts
 * underneath that protocol; neo_planner_amd/planner.py binds it with ctypes and
 * keeps the reference's method names.  Every entry point cites the reference code
 * it replaces (paths relative to src/planner/scripts/).
 *
 * Conventions: plain C, int status return (0 = NEO_OK), caller-owned buffers,
 * opaque context, no exceptions.  All arrays are C-contiguous.  A context owns one
 * HIP stream; calls on one context are serialised, different contexts are
 * independent.  Pointers are HOST pointers unless the argument is documented as a
 * device pointer (the *_dev entry points take device pointers and are asynchronous
 * on the context's stream).
 *
 * Decision vector layout (expert_planner.py:211, :540-541):
 *   x[n] = [ int_wpts row-major (D, M-1) ; tau (M) ],  n = D*(M-1) + M.
 * Boundary states: head[3][D], tail[3][D] = position, velocity, acceleration
 *   (expert_planner.py:170-181).
 */
#ifndef NEO_PLANNER_H
#define NEO_PLANNER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NEO_ABI_VERSION 1
#define NEO_MAX_PIECES 64 /* M: one lane per piece */
#define NEO_MAX_DIM 3     /* D */
#define NEO_LBFGS_M 10    /* maxcor (expert_planner.py:221) */

typedef struct neo_ctx neo_ctx; /* opaque */

/* status codes: per call (return value) and per trajectory (status[] arrays) */
enum {
  NEO_OK = 0,
  NEO_ERR_INVALID = 1,      /* bad argument */
  NEO_ERR_HIP = 2,          /* HIP runtime failure, see neo_last_error */
  NEO_ERR_NO_MAP = 3,       /* scene id has no ESDF uploaded */
  NEO_ERR_UNSUPPORTED = 4,
};

/* per-trajectory termination codes (neo_optimize_*): the ctypes host maps them to
 * the reference's exceptions (expert_planner.py:236-237, :481). */
enum {
  NEO_TRAJ_CONVERGED_GRAD = 0,   /* max|g| <= gtol                 (L-BFGS-B "NORM OF PROJECTED GRADIENT") */
  NEO_TRAJ_CONVERGED_F = 1,      /* rel. reduction of f <= ftol    (L-BFGS-B "REL_REDUCTION_OF_F")          */
  NEO_TRAJ_ABNORMAL = 2,         /* line search failed with empty memory (L-BFGS-B "ABNORMAL")             */
  NEO_TRAJ_MAXITER = 3,          /* iteration / evaluation cap                                                */
  NEO_TRAJ_NUMERIC_RANGE = 4,    /* exp(-tau) overflow: the reference raises OverflowError (:481)            */
  NEO_TRAJ_NONFINITE = 5,        /* NaN/Inf objective                                                         */
  NEO_TRAJ_BAD_SCENE = 6,        /* its map-table slot is outside the table (neo_optimize_batch_dev): left untouched */
  NEO_TRAJ_SUSPENDED = 7,        /* out of its launch's evaluation budget (neo_optimize_batch_budget_dev): resumable */
};
/* OR-ed into the code above when weighted collision cost > collision_cost_tol
 * (expert_planner.py:235-237 raises ValueError("collision cost too large")). */
#define NEO_TRAJ_FLAG_COLLISION 0x100

/* ESDF lookup mode */
enum {
  NEO_INTERP_NEAREST_2D_REF = 0, /* esdf.py:53-82: nearest cell, int() truncation, gradient in m/cell */
  NEO_INTERP_TRILINEAR_3D = 1,   /* north-star mode: trilinear distance + analytic gradient (m/m)     */
};

/* element type of an uploaded distance field / arithmetic of the sampling phase */
enum { NEO_F64 = 0, NEO_F32 = 1, NEO_F16 = 2 };

/* voxel order of a 3-D field in HBM */
enum {
  NEO_LAYOUT_LINEAR = 0, /* [z][y][x] */
  NEO_LAYOUT_YZ4 = 1,    /* yz-quads: voxel (x,y,z) stores d(y,z), d(y+1,z), d(y,z+1), d(y+1,z+1) contiguously, records in
                            [z][y][x] order: the 8 corners of a cell are 2 adjacent records (32 contiguous bytes), one
                            cache line per lookup and x-adjacent cells share half their bytes (4x the memory) */
  NEO_LAYOUT_CELL8 = 2,  /* cell-packed: the 2x2x2 corners of every interpolation cell contiguous (8x the
                            memory; one aligned 32-byte read per lookup instead of four gathers) */
  NEO_LAYOUT_BRICK = 3,  /* corner bricks: one 128-byte line per block of 2 x 2 x 2 cells holding the block's 27 corners
                            (fp32; fp16: 4 x 2 x 2 cells, 45 corners) -- a lookup reads one line, and a path stays on it
                            for two cells in every direction (4x the memory in fp32, like NEO_LAYOUT_YZ4) */
};

/* planner parameters: DefaultConfig / PlannerConfig fields (expert_planner.py:12-25,
 * ros_node/traj_planner_node.py:32-46); real values launch/config/planner_config.yaml:2-13 */
typedef struct neo_params {
  double v_max;
  double T_min;
  double T_max;
  double safe_dis;
  double delta_t;
  double weights[4]; /* energy, time, feasibility, collision */
  double collision_cost_tol;
  /* L-BFGS-B options, expert_planner.py:213-225 (tol=1e-4 -> ftol = gtol = 1e-4) */
  double ftol;
  double gtol;
  int32_t maxls;   /* 20 */
  int32_t maxiter; /* 15000 */
  int32_t maxfun;  /* 15000 */
  int32_t bugcompat_stale_T; /* 1 = reproduce expert_planner.py:528-533 */
  int32_t sample_dtype;      /* NEO_F64 | NEO_F32: arithmetic of the sampled cost terms */
  int32_t flags;             /* NEO_FLAG_* below; 0 = defaults */
} neo_params;

/* neo_params.flags.  The optimiser kernel exists in two register allocations with bit-identical results:
 * one wavefront per SIMD (shortest evaluation; default below 1024 trajectories per call) and two per SIMD
 * (slower evaluations, higher throughput once the trajectories queue for the SIMDs: large calls, or several
 * calls in flight on several streams; n <= 128 variables in the fp64 mode and on the 2-D map with D = 2, n <= 256
 * on 3-D fields with fp32 sampling). */
#define NEO_FLAG_ONE_WAVE_PER_SIMD 32
#define NEO_FLAG_TWO_WAVES_PER_SIMD 64
/* small problems (n <= 32 variables, M <= 16, one scene: a 3-D field with fp32 sampling, or the 2-D nearest-cell map
 * with D = 2 in either arithmetic -- the reference's own M = 3 shape): eight trajectories per wavefront, 8
 * lanes each, for n <= 16; four of 16 lanes beyond.  Opt-in: a piece's samples are strided over fewer lanes, so sums associate differently
 * and results agree with the default kernel to fp32 rounding, not bit for bit. */
#define NEO_FLAG_LANE_GROUPS 128
/* all-fp32 evaluation (fp32 sampling; 3-D fields and the 2-D reference map): the coefficient solve, the adjoint pass and the optimiser's vectors
 * and stored pairs in fp32 too -- for n <= 128 variables also the optimiser's scalars and the line search --, three
 * wavefronts per SIMD for n <= 128, two beyond.  Per evaluation the cost and gradient then agree with the
 * fp64 solve to ~1e-5 instead of 2e-6; the optimiser's statistics (evaluations, final costs) are those of the default
 * mode.  Opt-in throughput mode. */
#define NEO_FLAG_F32_SOLVE 2048
/* bits 1..16 switch phases off for timing experiments (tools/), 512 forces lane = piece, 4096 makes the all-fp32
 * adjoint pass reduce the transposed joint system itself instead of reusing the forward reduction's multipliers
 * (comparison runs): leave them 0 */

/* ---- lifetime ------------------------------------------------------------- */
int neo_abi_version(void);
/* device_id: HIP device ordinal.  stream: a hipStream_t to run on, or NULL to let the
 * context create its own. */
int neo_ctx_create(int device_id, void *stream, neo_ctx **out);
int neo_ctx_destroy(neo_ctx *ctx);
const char *neo_last_error(neo_ctx *ctx);
/* fills p with the ROS YAML defaults */
int neo_params_default(neo_params *p);
int neo_params_set(neo_ctx *ctx, const neo_params *p);
int neo_ctx_synchronize(neo_ctx *ctx);
/* stream of the calls that follow (NULL = back to the stream the context was created with).  The `_dev`
 * entry points are asynchronous and only read the context's maps, so a caller may keep several batches in
 * flight on several streams of one context; ordering between the batches' streams is the caller's business.
 * Map updates (neo_esdf_upload_*, neo_esdf_build_*, neo_esdf_drop) wait for ALL work in flight on the device
 * before they rewrite or free a scene's buffer, so a batch launched before the update reads the old map and one
 * launched after it the new map; map-table slots (neo_scene_slot) must be re-read after any update. */
int neo_ctx_set_stream(neo_ctx *ctx, void *stream);

/* ---- maps (map_server/esdf.py) ------------------------------------------- */
/* replaces ESDF.esdf_map / esdf_grad_x / esdf_grad_y (esdf.py:29-33) as looked up by
 * get_edt_dis / get_edt_grad (esdf.py:53-82).  Arrays are [height][width] float64. */
int neo_esdf_upload_2d(neo_ctx *ctx, int scene_id, const double *dist, const double *grad_x,
                       const double *grad_y, int width, int height, double resolution,
                       double origin_x, double origin_y);
/* replaces ESDF.occupancy_map_cb (esdf.py:11-33): int8 occupancy (100 = occupied) ->
 * exact EDT * resolution -> np.gradient, all on the device.  Optionally copies the three
 * arrays back (any of the out pointers may be NULL). */
int neo_esdf_build_2d(neo_ctx *ctx, int scene_id, const int8_t *occupancy, int width, int height,
                      double resolution, double origin_x, double origin_y, double *out_dist,
                      double *out_grad_x, double *out_grad_y);
/* neo_esdf_build_2d for n maps of one size whose occupancy is already on the device (onboard maps: one per mission):
 * scene_ids[n] and origins[n][2] are HOST arrays, occupancy[n][height][width] a DEVICE array, the maps back to back.
 * The same kernels with the maps in the grid -- the column sweep, then the exhaustive row pass up to 512 x 512 and the
 * row sweep beyond; all forms give the same integers -- and so the same records, bit for bit, as n neo_esdf_build_2d
 * calls; they are written straight into each scene's record buffer and nothing is copied back.  A scene that already holds a 2-D map of this width and height is rewritten in place:
 * with an unchanged origin and resolution its descriptor, the map table, every neo_scene_slot value and a caller's
 * resident slot arrays stay valid (its version is bumped as by neo_esdf_build_2d); any other scene gets a new buffer
 * and the table is rebuilt at its next use.  The call waits for the device once before the first record is overwritten
 * (when any map is rewritten) and for the context's stream once at the end: per call, not per map.
 * Device memory: 12 bytes a cell and map of scratch (beyond 512 x 512: 24 bytes and 8 a row), carved once from the
 * context's scratch for as many maps as fit 1 GiB -- 993 maps of 300 x 300 -- and reused by the passes of a larger batch.
 * NEO_ERR_INVALID: n < 0, a NULL buffer with n > 0, width or height < 1, more than 2^28 cells, a resolution that is not
 * finite and > 0, a scene id listed twice.  A call that fails on the device leaves the scenes it was rewriting without
 * a map. */
int neo_esdf_build_2d_batch_dev(neo_ctx *ctx, const int32_t *scene_ids, int n, const int8_t *occupancy, int width,
                                int height, double resolution, const double *origins);
/* 3-D distance field for NEO_INTERP_TRILINEAR_3D.  dist is [nz][ny][nx] of src_dtype
 * (host pointer, or device pointer when src_is_device != 0); it is stored on the device
 * as store_dtype in `layout`. */
int neo_esdf_upload_3d(neo_ctx *ctx, int scene_id, const void *dist, int src_dtype,
                       int src_is_device, int nx, int ny, int nz, double resolution,
                       const double origin[3], int store_dtype, int layout);
/* 3-D counterpart of neo_esdf_build_2d (esdf.py:23-29 in three dimensions): uint8 occupancy
 * [nz][ny][nx] (non-zero = occupied; host pointer, or device pointer when occ_is_device != 0) ->
 * exact Euclidean distance * resolution on the device, stored as for neo_esdf_upload_3d.
 * out_dist: optional HOST buffer [nz][ny][nx] float32 receiving the distances.
 * Device memory: besides the stored field the build needs 10 bytes per voxel of intermediates (NEO_ERR_HIP if they do not
 * fit); they are kept in the context for the next build while they are at most 512 MB and released otherwise.
 * At most 4096 voxels per axis.  Volumes whose squared diagonal leaves room in 31 bits (all of BASELINE.json's) take a
 * faster form of the line passes and, for rows of 4-byte aligned length up to 1024, of the x pass;
 * neo_esdf_build_config(ctx, NEO_EDT_GENERIC_LINES) forces the general form (same results; the tests run both).
 * 300^3 on one MI355X: 0.5 ms. */
int neo_esdf_build_3d(neo_ctx *ctx, int scene_id, const uint8_t *occupancy, int occ_is_device, int nx,
                      int ny, int nz, double resolution, const double origin[3], int store_dtype,
                      int layout, float *out_dist);
/* per-context switches of neo_esdf_build_3d (0 = defaults): comparison runs and tests */
#define NEO_EDT_GENERIC_LINES 1 /* the general form of the y / z line passes for every volume */
int neo_esdf_build_config(neo_ctx *ctx, int flags);
int neo_esdf_drop(neo_ctx *ctx, int scene_id);
/* point queries, replaces get_edt_dis / get_edt_grad called from Python
 * (astar_planner.py:134, traj_planner_node.py:474).  pts[n][D_map], grad[n][D_map]. */
int neo_esdf_query(neo_ctx *ctx, int scene_id, int n, const double *pts, double *dist, double *grad);

/* ---- cost / gradient (expert_planner.py:539-585) --------------------------
 * One evaluation of get_cost(x) and get_grad(x) for B trajectories of one scene.
 *   x[B][n], head[B][3][D], tail[B][3][D]
 *   cost[B]      = dot(costs, weights)                       (:558)
 *   costs4[B][4] = unweighted [energy, time, feasibility, collision] (:549-552)
 *   grad[B][n]                                               (:579)
 *   coeffs[B][6M][D]  polynomial coefficients (:336)         (may be NULL)
 *   status[B]    NEO_TRAJ_NUMERIC_RANGE or 0                 (may be NULL) */
int neo_cost_grad_batch(neo_ctx *ctx, int scene_id, int B, int M, int D, const double *x,
                        const double *head, const double *tail, double *cost, double *costs4,
                        double *grad, double *coeffs, int32_t *status);
/* same, device pointers, asynchronous on the context stream */
int neo_cost_grad_batch_dev(neo_ctx *ctx, int scene_id, int B, int M, int D, const double *x,
                            const double *head, const double *tail, double *cost, double *costs4,
                            double *grad, double *coeffs, int32_t *status);

/* ---- sampled terms alone (expert_planner.py:392-466: add_sampled_cost + add_sampled_grad_CT) ----
 * The ESDF-lookup kernel on its own, as the reference uses it after get_coeffs()
 * (all_planner_demo.py:46-51).  coeffs[B][6M][D], ts[B][M]  ->
 *   costs2[B][2]      unweighted feasibility and collision cost            (:413, :422)
 *   grad_C[B][6M][D]  weighted partials w.r.t. the coefficients            (:450, :465)
 *   grad_T[B][M]      weighted partials w.r.t. the durations               (:451, :466)
 * _dev: coeffs and grad_C must be 16-byte aligned (the kernel moves them as pairs of doubles). */
int neo_sampled_terms_batch(neo_ctx *ctx, int scene_id, int B, int M, int D, const double *coeffs,
                            const double *ts, double *costs2, double *grad_C, double *grad_T);
int neo_sampled_terms_batch_dev(neo_ctx *ctx, int scene_id, int B, int M, int D, const double *coeffs,
                                const double *ts, double *costs2, double *grad_C, double *grad_T);
/* the same with fp32 coefficient and partials buffers (round 6; sample_dtype NEO_F32 only, NEO_ERR_INVALID otherwise):
 * half the operand bytes of the fp32 sampling path and no conversions in the kernel.  coeffs[B][6M][D] and
 * grad_C[B][6M][D], grad_T[B][M] are floats; ts and costs2 stay doubles (int(T / delta_t) of :401 is taken in fp64).
 * _dev: coeffs and grad_C must be 8-byte aligned. */
int neo_sampled_terms_batch_f32(neo_ctx *ctx, int scene_id, int B, int M, int D, const float *coeffs,
                                const double *ts, double *costs2, float *grad_C, float *grad_T);
int neo_sampled_terms_batch_f32_dev(neo_ctx *ctx, int scene_id, int B, int M, int D, const float *coeffs,
                                    const double *ts, double *costs2, float *grad_C, float *grad_T);

/* ---- optimiser (expert_planner.py:205-237: plan_once) ----------------------
 * Runs L-BFGS-B(maxcor 10, no bounds) from x to termination for every trajectory,
 * entirely on the device.  scene_ids[B] selects the map per trajectory (NULL = all
 * use `scene_id`); all maps of one call must be of the same kind (2-D / 3-D), element type
 * and layout: NEO_ERR_INVALID otherwise.
 * The *_dev variant takes a DEVICE array of map-table slots (neo_scene_slot) in
 * place of scene ids, and `scene_id` then only names the kind of map; since the slots cannot
 * be inspected from the host, every map of that kind held by the context must then share
 * `scene_id`'s element type and layout (NEO_ERR_INVALID otherwise), and a slot outside the
 * table ends that trajectory with NEO_TRAJ_BAD_SCENE.
 *   x[B][n]         in: x0, out: final x (res.x)
 *   costs4[B][4]    unweighted costs at the final x
 *   costs4_last[B][4] unweighted costs at the LAST EVALUATED x -- what the reference
 *                   reports as weighted_cost / final_cost (:233-234)   (may be NULL)
 *   nit[B], nfev[B] L-BFGS-B iteration / evaluation counts (res.nit, res.nfev)
 *   status[B]       NEO_TRAJ_* | NEO_TRAJ_FLAG_COLLISION */
int neo_optimize_batch(neo_ctx *ctx, int scene_id, const int32_t *scene_ids, int B, int M, int D,
                       double *x, const double *head, const double *tail, double *costs4,
                       double *costs4_last, int32_t *nit, int32_t *nfev, int32_t *status);
int neo_optimize_batch_dev(neo_ctx *ctx, int scene_id, const int32_t *scene_ids, int B, int M,
                           int D, double *x, const double *head, const double *tail,
                           double *costs4, double *costs4_last, int32_t *nit, int32_t *nfev,
                           int32_t *status);
/* the same with separate start points: x0[B][n] is only read, the results go to x[B][n] (x0 == x is the in-place
 * form above).  A caller that optimises the same requests again (benchmarks, re-planning from a stored guess) keeps
 * x0 resident and needs no copy per launch. */
int neo_optimize_batch_from_dev(neo_ctx *ctx, int scene_id, const int32_t *scene_ids, int B, int M,
                                int D, const double *x0, double *x, const double *head,
                                const double *tail, double *costs4, double *costs4_last, int32_t *nit,
                                int32_t *nfev, int32_t *status);
/* ---- launches with an evaluation budget (round 5) ----------------------------
 * The duration of one launch is the duration of its LONGEST run (cfg2: 633 evaluations against a mean of 135), which the
 * other trajectories' results wait for.  neo_optimize_batch_budget_dev is neo_optimize_batch_from_dev for ONE scene with
 * a cap on the evaluations a trajectory may make IN THIS LAUNCH: a run that needs more is suspended -- status
 * NEO_TRAJ_SUSPENDED, its complete optimiser state (iterate, gradient, direction, line-search interval, the stored
 * pairs) in state[b] -- and a later launch with resume != 0 continues it exactly where it stopped: the finished run is
 * bit for bit the run of an unbudgeted launch (tests/test_gpu_budget.py).  The reference's own caps keep their meaning:
 * maxiter / maxfun of expert_planner.py:213-225 count over all launches of a run (NEO_TRAJ_MAXITER).
 *   state      DEVICE buffer of B * neo_optimize_state_bytes(M, D) bytes, the caller's, kept between the launches of a run
 *   subset     optional DEVICE array of n_subset trajectory indices: only these are launched -- the compacted re-launch of
 *              the stragglers; NULL = all B.  Arrays are always indexed by trajectory, never by position; an index
 *              outside 0 .. B - 1 is skipped
 *   resume     0: the launched trajectories start from x0; 1: those among them with status NEO_TRAJ_SUSPENDED continue
 *              from state, the others are left untouched
 * A suspended trajectory's x holds the point it evaluates next, costs4 the terms at its last iterate, nit / nfev its
 * counts so far.  3-D fp32 fields in the linear or brick layout, n <= 128 variables, every arithmetic mode. */
size_t neo_optimize_state_bytes(int M, int D);
int neo_optimize_batch_budget_dev(neo_ctx *ctx, int scene_id, int B, int M, int D, const double *x0, double *x,
                                  const double *head, const double *tail, double *costs4, double *costs4_last,
                                  int32_t *nit, int32_t *nfev, int32_t *status, void *state, int eval_budget,
                                  const int32_t *subset, int n_subset, int resume);
/* slot of a scene in the device-side map table, -1 if it has no map.  Slots change
 * whenever a map is uploaded or dropped. */
int neo_scene_slot(neo_ctx *ctx, int scene_id);
/* bytes of device (HBM) workspace neo_optimize_batch_dev keeps for B trajectories.  Currently 0:
 * the L-BFGS history (2 * maxcor * n doubles per trajectory) lives in LDS. */
size_t neo_optimize_workspace_bytes(int B, int M, int D);

/* ---- trajectory evaluation (traj_utils.py:85-222) --------------------------
 * state[B][K][3][D] = position, velocity, acceleration at t_k = k / hz, k < K; rows with
 * t_k >= sum(ts) are left zero and count[B] returns the valid number
 * (= len(np.arange(0, sum(ts), 1/hz)), traj_utils.py:185).  x as above. */
int neo_eval_traj_batch(neo_ctx *ctx, int B, int M, int D, const double *x, const double *head,
                        const double *tail, double hz, int K, double *state, int32_t *count);

/* ---- trajectory audit (ros_node/traj_planner_node.py:333-363: get_weighted_metric) ----
 * The reference's flight metric of every planned trajectory under perfect tracking, one record per trajectory:
 *   1. the coefficients are solved from x, head, tail as neo_eval_traj_batch solves them (fp64);
 *   2. samples at t_k = k * (1 / hz), k < count[b] = len(np.arange(0, sum(T), 1/hz)) -- any number of them;
 *   3. the sample states are those of neo_eval_traj_batch's rows at the same hz, bit for bit (one piece table for
 *      both, csrc/neo_pieces.hpp: the same solve, piece search and expressions);
 *   4. d_k = the map's point lookup of the sample position in neo_esdf_query's arithmetic: the nearest cell on the
 *      2-D reference map (the first two axes, as the sampled cost projects them; 10000 outside), trilinear on 3-D
 *      fields (fp32 / fp16, every layout);
 *   5. the record audit[b][NEO_AUDIT_FIELDS] of doubles (fields below), count[b] and flags[b] (NEO_AUDIT_FLAG_*).
 * v_max, safe_dis and collision_cost_tol come from neo_params.  With D = 2 on the 2-D map every field is the
 * reference's get_weighted_metric of the planned trajectory (sample interval metric_eva_interval = 0.1 s at hz = 10,
 * :119; metric weights [1, 1, 100], :204).  D = 3 (3-D fields, or the 2-D map with the first two axes looked up) is this
 * project's extension: the same formulas over all D axes.  The same call returns the same bits whatever the launch
 * configuration; ties of MIN_CLEARANCE go to the earliest sample.
 * Validity: hz must be finite and > 0, and M * T_max * hz < 2^30 (the most samples a trajectory can have); output
 * buffers must not be NULL; the (map kind, D) pair must be (2-D, 2), (2-D, 3) or (3-D, 3).  NEO_ERR_INVALID with a
 * neo_last_error message otherwise, before anything is launched.
 * scene_ids, maps and slots as in neo_optimize_batch / neo_optimize_batch_dev (NULL = all use scene_id; one kind,
 * element type and layout per call).  weights3: host pointer to the three metric weights, NULL = {1, 1, 100}. */
enum {
  NEO_AUDIT_PATH_LENGTH = 0,     /* sum_{k>=1} |p_k - p_{k-1}| over all D axes                        (:341-343) */
  NEO_AUDIT_FEASIBILITY = 1,     /* sum_k (|v_k|^2 - v_max^2)^3 over the samples where it is > 0       (:346-348) */
  NEO_AUDIT_COLLISION = 2,       /* sum_k (safe_dis - d_k)^3 over the samples where it is > 0          (:351-355) */
  NEO_AUDIT_WEIGHTED = 3,        /* w0 * [0] + w1 * [1] + w2 * [2]                                     (:357)     */
  NEO_AUDIT_MIN_CLEARANCE = 4,   /* min_k d_k (+inf without samples)                                              */
  NEO_AUDIT_T_MIN_CLEARANCE = 5, /* t_k of the first sample attaining [4] (-1 without samples)                    */
  NEO_AUDIT_MAX_SPEED = 6,       /* max_k |v_k|                                                                   */
  NEO_AUDIT_MAX_ACC = 7,         /* max_k |a_k|                                                                   */
  NEO_AUDIT_T_FIRST_UNSAFE = 8,  /* first t_k with d_k < safe_dis, or -1                                          */
  NEO_AUDIT_DURATION = 9,        /* sum(T)                                                                        */
  NEO_AUDIT_FIELDS = 10,
};
#define NEO_AUDIT_FLAG_UNSAFE 1      /* some d_k < safe_dis */
#define NEO_AUDIT_FLAG_METRIC_FAIL 2 /* WEIGHTED > 10 * collision_cost_tol: the reference's failed flight (:359-361) */
#define NEO_AUDIT_FLAG_OUTSIDE_MAP 4 /* some sample lies outside the map (its d_k is 10000) */
#define NEO_AUDIT_FLAG_NONFINITE 8   /* the solve failed (exp(-tau) overflow), a state is not finite, or the map-table
                                        slot is outside the table (_dev): every field NaN, count 0 */
int neo_audit_traj_batch(neo_ctx *ctx, int scene_id, const int32_t *scene_ids, int B, int M, int D,
                         const double *x, const double *head, const double *tail, double hz,
                         const double *weights3, double *audit, int32_t *count, int32_t *flags);
/* the same with DEVICE pointers, asynchronous on the context's stream; scene_ids is then a device array of map-table
 * slots (neo_scene_slot) as in neo_optimize_batch_dev, and weights3 stays a host pointer */
int neo_audit_traj_batch_dev(neo_ctx *ctx, int scene_id, const int32_t *scene_ids, int B, int M, int D,
                             const double *x, const double *head, const double *tail, double hz,
                             const double *weights3, double *audit, int32_t *count, int32_t *flags);

/* ---- geo warm start (traj_planner/astar_planner.py, geo_planner.py:19-101) ----
 * For each request b on a 2-D map: the reference's AstarPlanner.plan(map, start[b], target[b]) -- an 8-connected A* on
 * the map's grid expanded by 10 m (W + int(10 / res) by H + int(10 / res) cells, origin - 5 m), a cell blocked where the
 * map's nearest-cell distance of its position is < 0.5 (esdf.py has_collision) -- then
 * GeoPlanner.prune_path_nodes(map, path), the four key nodes.  Results, all equal to the reference's:
 *   key_pts[b][4][2]   the pruned nodes (int_wpts = key_pts[b][1:3].T for warm_start_plan);
 *   path_len[b]        nodes of the reference's path (1 when there is none: [calc_real_pos(target cell)]);
 *   path_cost[b]       target_node.cost (0 without a path);
 *   path[b][path_cap][2] the first min(path_len, path_cap) nodes when path is not NULL, NaN after them;
 *   expansions[b]      nodes the search closed (0 for the short cuts below);
 *   flags[b]           NEO_GEO_FLAG_*.
 * Short cuts, exact: start cell == target cell gives the one-node path at once; a target cell that is blocked or outside
 * the grid gives NO_PATH without a search.  One divergence: a start whose key x + y * W_e falls outside [0, W_e * H_e)
 * (the reference would search from it) gives START_OUTSIDE and the one-node result.  max_expansions > 0 ends a search
 * after that many expansions with CAPPED and the one-node result -- NOT the reference's answer; 0 = unbounded.
 * Each search runs on one slot of a context-owned workspace of 32 bytes per expanded cell and slot, sized from a byte
 * budget (neo_geo_workspace_budget; default 2 GiB, at most 1024 slots); NEO_ERR_HIP when not even one slot fits or the
 * allocation fails.  A scene's blocked mask (one bit per expanded cell) is built on first use and kept until the map
 * changes.  Results do not depend on the slot, the launch or the batch.  The geo calls of one context share the
 * workspace: issue them on one stream.
 * Errors, before anything is launched: B < 1, path_cap < 0, path != NULL with path_cap < 1, max_expansions < 0 or a NULL
 * required buffer: NEO_ERR_INVALID; a scene without a map: NEO_ERR_NO_MAP; a 3-D scene: NEO_ERR_UNSUPPORTED.
 * scene_ids: NULL (all use scene_id) or B scene ids (host form). */
#define NEO_GEO_FLAG_NO_PATH 1        /* the open set emptied, or the target cell is blocked or outside the grid */
#define NEO_GEO_FLAG_START_OUTSIDE 2  /* the start cell's key is outside the grid: not searched */
#define NEO_GEO_FLAG_CAPPED 4         /* max_expansions reached: not the reference's result */
#define NEO_GEO_FLAG_PATH_TRUNCATED 8 /* only the copied path was cut to path_cap */
#define NEO_GEO_FLAG_BAD_SCENE 16     /* _dev: the map-table slot is outside the table; key_pts and path_cost NaN */
int neo_geo_search_batch(neo_ctx *ctx, int scene_id, const int32_t *scene_ids, int B, const double *start,
                         const double *target, int max_expansions, int path_cap, double *key_pts, double *path,
                         int32_t *path_len, double *path_cost, int32_t *expansions, int32_t *flags);
/* the same with DEVICE pointers, asynchronous on the context's stream; scene_ids is then a device array of 2-D map-table
 * slots (neo_scene_slot), as in neo_optimize_batch_dev */
int neo_geo_search_batch_dev(neo_ctx *ctx, int scene_id, const int32_t *scene_ids, int B, const double *start,
                             const double *target, int max_expansions, int path_cap, double *key_pts, double *path,
                             int32_t *path_len, double *path_cost, int32_t *expansions, int32_t *flags);
/* The geo warm start on RESIDENT arrays, ONE launch, asynchronous on the context's stream: search, prune and the pack of
 * the optimiser's first guess over a launch list.  Position p works on request subset[p] (a device array of `count`
 * indices), or on p when subset is NULL (all B; count is then ignored); an index outside 0 .. B - 1 is skipped and its
 * rows stay.  Every pointer
 * is a device array indexed by REQUEST, except tau3:
 *   slots[B]          2-D map-table slots (neo_scene_slot), or NULL: every request uses scene_id;
 *   head, tail        [B][3][2], read where they lie: start = head[b][0], target = tail[b][0]; the velocity and
 *                     acceleration rows are not read;
 *   tau3              HOST pointer to the three start values of tau (map_T2tau of init_T * [1.5, 1, 1.5]), read before
 *                     the call returns;
 *   x0[B][7]          = [k1.x, k2.x, k1.y, k2.y, tau3[0], tau3[1], tau3[2]], k1 and k2 the two inner key nodes: the x
 *                     neo_optimize_batch_from_dev / neo_plan_guess_dev take as a start, with M = 3, D = 2;
 *   key_pts, path_len, path_cost, expansions, flags   as neo_geo_search_batch_dev writes them.  A request without a path
 *                     has four equal key nodes, the target cell; a slot outside the table gives NaN key nodes and
 *                     waypoints (tau as above), path_cost NaN and NEO_GEO_FLAG_BAD_SCENE.
 * direct: 0 -- the search reads the scenes' blocked masks (built on first use, rebuilt when a map changes: an
 * allocation, a wait and a launch per changed scene of the table).  Non-zero -- the DIRECT form: a cell is blocked iff
 * the map's nearest-cell distance at its position is < 0.5, evaluated on the map's 32-byte records where the search needs
 * it, by the very function the mask is built with; no mask is built or read for any scene of the table.  The results of
 * the two forms are equal.  Direct is the form for maps that change between calls (onboard maps); the masked form
 * reads less per expansion on a map that stays.
 * Errors, before anything is launched: B < 1, count outside 0 .. B with a subset, max_expansions < 0 or a NULL
 * required buffer (slots and subset may be NULL): NEO_ERR_INVALID; scene_id without a map: NEO_ERR_NO_MAP; a 3-D scene:
 * NEO_ERR_UNSUPPORTED.  An empty list launches nothing. */
int neo_geo_guess_dev(neo_ctx *ctx, int scene_id, const int32_t *slots, int B, const int32_t *subset, int count,
                      const double *head, const double *tail, const double *tau3, int max_expansions, int direct,
                      double *x0, double *key_pts, int32_t *path_len, double *path_cost, int32_t *expansions,
                      int32_t *flags);
/* blocked masks built since the context was created (a diagnostic: the direct form builds none) */
int neo_geo_mask_builds(neo_ctx *ctx, int64_t *count);
/* prune_path_nodes alone on caller-given host paths[b][path_stride][2] of path_len[b] (1 <= path_len[b] <= path_stride)
 * nodes: key_pts[b][4][2] */
int neo_geo_prune_batch(neo_ctx *ctx, int scene_id, const int32_t *scene_ids, int B, const double *paths,
                        const int32_t *path_len, int path_stride, double *key_pts);
/* the byte budget the geo workspace is sized from (takes effect at the next reallocation) */
int neo_geo_workspace_budget(neo_ctx *ctx, size_t bytes);

/* ---- fleet replan loop (ros_node/traj_planner_node.py:390-578) ----------------
 * What the reference's node does for one mission between two plans, for B missions in lock step.  2-D reference map,
 * D = 2, fp64.  Fleet state, caller-owned DEVICE buffers indexed by MISSION:
 *   cmd[B][cap][3][2]   the command arrays des_state_array (:518, :577): position, velocity, acceleration rows in the
 *                       layout of neo_eval_traj_batch's state;
 *   cmd_len[B]          des_state_length; cmd_index[B] des_state_index (the row being flown); future_index[B] (:531);
 *   flags[B]            NEO_FLEET_FLAG_* below, OR-ed in by the kernels (the caller zeroes them once).
 * Every call takes an optional DEVICE array `subset` of n_subset mission indices: only these are launched, NULL = all
 * B.  Arrays are always indexed by mission, never by position; an index outside 0 .. B - 1 is skipped (the convention
 * of neo_optimize_batch_budget_dev); a mission may appear in a subset once.  scene_id / scene_ids as in
 * neo_optimize_batch (host form) / neo_optimize_batch_dev (_dev: a device array of map-table slots, one per mission).
 * A mission's results depend on neither B, the subset nor the launch: no floating-point atomics, fixed summation order.
 * Errors, before anything is launched, with a neo_last_error message: a NULL required buffer, B < 0, a bad subset size,
 * cap <= 0, stride <= 0, step or ahead outside 0 .. 2^30, a rate or step length that is not finite and > 0, a 3-D map:
 * NEO_ERR_INVALID; a scene without a map: NEO_ERR_NO_MAP. */
#define NEO_FLEET_FLAG_TARGET_CAPPED 1  /* the lateral walk of the target ran into its bound: not the reference's target */
#define NEO_FLEET_FLAG_CMD_FULL 2       /* a spliced trajectory did not fit cmd: its rows from `cap` on were dropped */
#define NEO_FLEET_FLAG_BAD_SCENE 4      /* _dev: the mission's map-table slot is outside the table; its target is NaN */
#define NEO_FLEET_FLAG_SPLICE_FAILED 8  /* the trajectory to splice could not be solved (exp(-tau) overflow): cmd untouched */
#define NEO_FLEET_FLAG_ABANDONED 16     /* set by the host loop (neo_planner_amd.FleetReplanLoop): all targets of a tick failed */
/* set_local_target (:450-488), one lane per mission.  cur_pos[B][2], goal[B][2]; jitter[B][2] is added to the first
 * candidate (:469): zeros for the first target of a tick, the caller's N(0, 1) draws for the re-targeted ones -- the
 * kernel draws nothing.  move_vel = 0.8 v_max (:87).
 *   tail[B][3][2]     target position, velocity (move_vel towards the goal, :480-481), zero acceleration;
 *   near_goal[B]      1 where |goal - cur_pos| < longitu_step_dis: the target is the goal with zero velocity (:456-459);
 *   lateral_steps[B]  steps of the alternating, growing lateral walk (:474-477) out of has_collision -- the map's
 *                     nearest-cell distance in the arithmetic of neo_esdf_query < 0.5, 10000 outside the map, which is
 *                     what ends a walk.  The reference's loop has no bound; here a walk takes at most
 *                     ceil(2 L / lateral_step_length) + 2 steps, L the map's diagonal extent (it cannot take that many:
 *                     after k steps the candidate is ceil(k / 2) step lengths from the first one, and both must lie
 *                     inside the map for the walk to go on), and never more than 2^20: NEO_FLEET_FLAG_TARGET_CAPPED.
 * A target that falls on the goal has the reference's 0 / 0 velocity: NaN. */
int neo_fleet_target_batch(neo_ctx *ctx, int scene_id, const int32_t *scene_ids, int B, const int32_t *subset,
                           int n_subset, const double *cur_pos, const double *goal, const double *jitter,
                           double longitu_step_dis, double lateral_step_length, double move_vel, double *tail,
                           int32_t *near_goal, int32_t *lateral_steps, int32_t *flags);
/* the same with DEVICE pointers, asynchronous on the context's stream.  (The host form above copies the output arrays
 * up first, so the rows of missions outside the subset come back as they were.) */
int neo_fleet_target_batch_dev(neo_ctx *ctx, int scene_id, const int32_t *scene_ids, int B, const int32_t *subset,
                               int n_subset, const double *cur_pos, const double *goal, const double *jitter,
                               double longitu_step_dis, double lateral_step_length, double move_vel, double *tail,
                               int32_t *near_goal, int32_t *lateral_steps, int32_t *flags);
/* the re-targeting's draws on the device, one lane per mission of the subset: jitter[B][2], the array the target
 * kernel reads, from the counter stream of mission_ids[b] (int32, mission-indexed [B], ids in 0 .. 2^31 - 1; NULL: b
 * itself):
 *   jitter[b][i] = z(seed, id, tick, target, value i),   zeros, without drawing, when target == 0,
 * z the unit normal of csrc/neo_counter_rng.hpp with the counter (id, tick, target, 2 << 24) (see neo_plan_jitter):
 * neo_planner_amd.fleet.target_jitter_counter's rows bit for bit.  Missions outside the subset keep their rows (the
 * host form copies jitter up first).  Errors, before anything is launched: a NULL jitter, B < 0, a bad subset size,
 * tick or target < 0: NEO_ERR_INVALID. */
int neo_fleet_jitter(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, uint64_t seed, int tick, int target,
                     const int32_t *mission_ids, double *jitter);
/* the same with DEVICE pointers, asynchronous on the context's stream */
int neo_fleet_jitter_dev(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, uint64_t seed, int tick, int target,
                         const int32_t *mission_ids, double *jitter);
/* perfect tracking for one replan period, then get_drone_state_ahead (:527-537), one lane per mission:
 *   cmd_index = min(cmd_index + step, cmd_len - 1);  cur_pos[B][2] = position of row cmd_index;
 *   future_index = min(ahead + cmd_index, cmd_len - 1);  head[B][3][2] = position and velocity of row future_index, zero
 *   acceleration (the reference hands plan() a 2 x 2 state).
 * step = commands per replan period, ahead = int(planning_time_ahead * cmd_hz), both computed by the caller.  A mission
 * with cmd_len < 1 is left untouched.  Device pointers only: the point is the resident array. */
int neo_fleet_advance_dev(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, const double *cmd, int cap,
                          const int32_t *cmd_len, int32_t *cmd_index, int32_t *future_index, int step, int ahead,
                          double *cur_pos, double *head);
/* the camera pose a mission senses from (onboard maps), one lane per mission: pose[B][5] = cur_pos x, y, eye_z, c, s
 * as neo_depth_render_batch takes it.  (c, s) is the unit vector of the last step of the command array, position of
 * row cmd_index minus that of the row before it (:685-687 without the arctan2 round trip); where there is no such step
 * (cmd_index < 1, nothing planned yet) or it has no length, the unit vector from cur_pos to goal; (1, 0) on the goal.
 * Two squares, their sum, one square root and two divisions, each rounded on its own, so NumPy gives the same bits.
 * Device pointers only. */
int neo_fleet_pose_dev(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, const double *cmd, int cap,
                       const int32_t *cmd_len, const int32_t *cmd_index, const double *cur_pos, const double *goal,
                       double eye_z, double *pose);
/* the splice of replan (:574-578), one wavefront per mission, for the launched missions with solved[b] != 0 (solved: a
 * device array [B], NULL = all launched): the trajectory x[B][n], head[B][3][2], tail[B][3][2] of M pieces is solved as
 * neo_eval_traj_batch solves it and its rows k < count = len(np.arange(0, sum(T), 1 / hz)) -- the rows of
 * neo_eval_traj_batch at the same hz, bit for bit -- are written to cmd[b][future_index[b] + k]; cmd_len[b] =
 * future_index[b] + count; rows before future_index[b] stay.  first != 0 splices at 0 and zeroes cmd_index and
 * future_index (first_plan, :515-519).  Rows from `cap` on are dropped, cmd_len = cap, and NEO_FLEET_FLAG_CMD_FULL is
 * raised: nothing is written past the buffer.  Device pointers only. */
int neo_fleet_splice_dev(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, int M, const double *x,
                         const double *head, const double *tail, const int32_t *solved, double hz, int first,
                         double *cmd, int cap, int32_t *cmd_len, int32_t *cmd_index, int32_t *future_index,
                         int32_t *flags);
/* ---- fleet mode "warmstart" (ros_node/traj_planner_node.py:570-571, :597-611) ----
 * The reference's `selected_planner:=warmstart` starts every replan from the previous plan: its waypoints, carried along
 * relative to the planning start state, and the durations the planner last held.  Per mission, caller-owned DEVICE
 * buffers indexed by MISSION:
 *   wpts_local[B][2][M - 1]   the last SOLVED plan's waypoints minus the position that plan started from (head[b][0]);
 *   ts_carry[B][M]            the durations the planner last held.
 * x rows are a plan's [x_0 .. x_{M-2}, y_0 .. y_{M-2}, tau_0 .. tau_{M-1}], n = 2 (M - 1) + M doubles.  D = 2, fp64, one
 * lane per mission, one launch each.  Device pointers only, asynchronous on the context's stream.  `subset` (n_subset
 * mission indices, a device array) names the missions launched, NULL = all B; an index outside 0 .. B - 1 is skipped
 * and its rows stay.  A mission's values depend on neither B, the subset nor its position.  T_min, T_max: the context's
 * parameters.  Sums, differences and quotients only, each rounded on its own.
 * NEO_ERR_INVALID before any launch, with a neo_last_error message: B < 1, a bad subset size, M outside 2 .. 64, a NULL
 * buffer. */
/* the first guess of a replan: x0[b] (x0[B][n], what neo_plan_guess_dev takes as x_init) from what mission b carries,
 *   x0[b][d (M - 1) + k] = wpts_local[b][d][k] + head[b][0][d]      -- NumPy's bits;
 *   tau_k = -log((T_max - T_min) / (ts_carry[b][k] - T_min) - 1)    -- map_T2tau, the device's fp64 log.
 * Where the reference's map_T2tau raises -- ts_carry - T_min is not > 0, or the log's argument is not > 0 (a duration
 * that saturated to T_min or T_max: |tau| beyond about 37) -- and for a NaN duration, tau_k is NaN: the optimiser ends
 * that attempt NEO_TRAJ_NONFINITE at its first evaluation, uncounted, and the plan chain re-seeds it from the straight
 * line, as the reference does when warm_start_plan catches the exception. */
int neo_fleet_warm_guess_dev(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, int M, const double *head,
                             const double *wpts_local, const double *ts_carry, double *x0);
/* what the launched missions keep of a target round's plan: x[B][n] the plan, head[B][3][2] the state it started from,
 * solved[B], status[B] (NEO_TRAJ_* | NEO_TRAJ_FLAG_COLLISION of the last attempt) and attempts[B] as neo_plan_merge_dev
 * leaves them; init_ts: a HOST array [M], the start durations of a re-seeded attempt (init_T * [1.5, 1, ..., 1, 1.5]).
 *   solved[b] != 0:   wpts_local[b][d][k] = x[b][d (M - 1) + k] - head[b][0][d]   -- NumPy's bits;
 *                     ts_carry[b][k] = (T_max - T_min) / (1 + exp(-tau_k)) + T_min -- map_tau2T, the device's fp64 exp;
 *   solved[b] == 0:   wpts_local[b] stays (the reference raises before :570).  ts_carry[b] is map_tau2T of x[b]'s tau when
 *                     the last attempt ran to an answer ((status & 0xff) <= NEO_TRAJ_MAXITER: its collision was too
 *                     large); when it raised instead ((status & 0xff) >= NEO_TRAJ_NUMERIC_RANGE) ts_carry[b] is that
 *                     attempt's START durations: init_ts with attempts[b] > 1, unchanged with attempts[b] == 1.
 * exp(-tau) overflows to +inf and gives T_min, as it does to rounding from -tau = 37 on; a NaN tau gives NaN. */
int neo_fleet_warm_carry_dev(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, int M, const double *x,
                             const double *head, const int32_t *solved, const int32_t *status, const int32_t *attempts,
                             const double *init_ts, double *wpts_local, double *ts_carry);
/* get_weighted_metric (:333-363) over what was FLOWN, one wavefront per mission: the samples are rows 0, stride,
 * 2 stride, ... < n_flown[b] of cmd[b] (stride = cmd_hz * metric_eva_interval: 6 at the reference's 60 Hz and 0.1 s;
 * n_flown = the final cmd_index + 1, or cmd_len for a mission flown to its end; values outside 0 .. cap are clamped).
 * The record is neo_audit_traj_batch's: audit[B][NEO_AUDIT_FIELDS], count[B] (samples), flags[B] (NEO_AUDIT_FLAG_*, not
 * OR-ed: written), with d_k the nearest-cell lookup of the row's position; sample j has the time (j * stride) / cmd_hz,
 * DURATION = n_flown / cmd_hz, and a row that is not finite gives the NaN record of NEO_AUDIT_FLAG_NONFINITE.
 * NEO_AUDIT_FLAG_METRIC_FAIL is the reference's "planning is considered failed" (:359-361).  v_max, safe_dis and
 * collision_cost_tol come from neo_params; weights3 as in neo_audit_traj_batch.  Same bits whatever the subset, its
 * order and the launch.  The host form takes cmd, n_flown and the outputs as HOST arrays (a flight recorded elsewhere). */
int neo_fleet_audit_batch(neo_ctx *ctx, int scene_id, const int32_t *scene_ids, int B, const int32_t *subset,
                          int n_subset, const double *cmd, int cap, const int32_t *n_flown, int stride, double cmd_hz,
                          const double *weights3, double *audit, int32_t *count, int32_t *flags);
int neo_fleet_audit_batch_dev(neo_ctx *ctx, int scene_id, const int32_t *scene_ids, int B, const int32_t *subset,
                              int n_subset, const double *cmd, int cap, const int32_t *n_flown, int stride,
                              double cmd_hz, const double *weights3, double *audit, int32_t *count, int32_t *flags);

/* ---- fleet goal routes (ros_node/tracker_planner_node.py: a goal that keeps moving) ----------------
 * A mission's goal moves along a polyline at constant speed (csrc/neo_track.hpp; neo_planner_amd.goal_routes.GoalRoutes
 * is its NumPy model, bit for bit).  The routes are a ragged table laid out as the depth camera's box_begin is:
 *   vertices[n_vertices][2]   the points of all routes, one route after the other;
 *   route_begin[B + 1]        mission b's points are vertices[route_begin[b] .. route_begin[b + 1]): 2 to
 *                             NEO_FLEET_ROUTE_MAX of them;
 *   speed[B]                  metres a second along the route, >= 0;
 *   closed[B]                 != 0: the route gets the closing segment back to its first point (NULL: all open).
 * The point at time t: seg_k = sqrt(dx * dx + dy * dy), cum their sequential running sum from cum_0 = 0, s = speed * t,
 * closed: s = fmod(s, total), open: s = min(s, total); k the largest index with cum_k <= s, at most the last segment;
 * v_k + ((s - cum_k) / seg_k) * (v_{k+1} - v_k), and v_k itself where seg_k or the total is 0.  Every operation is
 * rounded on its own.  A mission whose route has fewer than 2 or more than NEO_FLEET_ROUTE_MAX points, or points outside
 * the table, gets a NaN goal / a NaN record; no other row is touched.
 * Everything is indexed by MISSION, fp64; `subset` as for the other fleet calls; same bits whatever the subset, its
 * order and the launch.  NEO_ERR_INVALID before any launch, with a neo_last_error message: a NULL required buffer,
 * B < 0, a bad subset size, n_vertices < 0, step, stride or cap < 1, step > 2^30, a cmd that is not 16-byte aligned
 * (hold), a cmd_hz that is not finite and > 0, a t or radius that is not finite. */
#define NEO_FLEET_ROUTE_MAX 256
#define NEO_TRACK_FIELDS 8
enum {
  NEO_TRACK_GAP_MEAN = 0,       /* mean distance between the flown position and the goal, over the samples */
  NEO_TRACK_GAP_MAX = 1,        /* the largest gap ... */
  NEO_TRACK_T_GAP_MAX = 2,      /* ... and its time; the first sample wins ties */
  NEO_TRACK_GAP_MIN = 3,        /* the smallest gap ... */
  NEO_TRACK_T_GAP_MIN = 4,      /* ... and its time; the first sample wins ties */
  NEO_TRACK_GAP_FINAL = 5,      /* the gap at the last sample */
  NEO_TRACK_T_FIRST_WITHIN = 6, /* time of the first sample with gap <= radius, or -1 */
  NEO_TRACK_FRAC_WITHIN = 7     /* samples with gap <= radius over count */
};
/* goal[b] = the point of mission b's route at time t, one lane per mission: goal[B][2]. */
int neo_fleet_goal_route(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, const double *vertices,
                         int n_vertices, const int32_t *route_begin, const double *speed, const int32_t *closed,
                         double t, double *goal);
/* the same with DEVICE pointers, asynchronous on the context's stream */
int neo_fleet_goal_route_dev(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, const double *vertices,
                             int n_vertices, const int32_t *route_begin, const double *speed, const int32_t *closed,
                             double t, double *goal);
/* a drone that runs out of commands holds the last one (tracker_planner_node.py:387-391 re-reads that row), one
 * wavefront per mission, in front of neo_fleet_advance_dev: with need = cmd_index[b] + step + 1, a mission with
 * 1 <= cmd_len[b] < need gets copies of row cmd_len[b] - 1 (position, velocity and acceleration as they are) appended
 * up to min(need, cap) rows, cmd_len[b] becomes that, and need > cap raises NEO_FLEET_FLAG_CMD_FULL.  After it row i of
 * the mission is its command at time i / cmd_hz.  cmd must be 16-byte aligned.  Device pointers only. */
int neo_fleet_hold_dev(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, double *cmd, int cap,
                       int32_t *cmd_len, const int32_t *cmd_index, int step, int32_t *flags);
/* how well the flown rows followed the moving goal, one wavefront per mission: sample j is row j * stride of cmd[b],
 * j * stride < n_flown[b] (clamped to 0 .. cap), at time t_j = (j * stride) / cmd_hz; its gap is the square root of the
 * squared distance between the row's position and the route's point at t_j.  track[B][NEO_TRACK_FIELDS] as the enum
 * above, count[B] the samples, flags[B] written (not OR-ed): 0, or NEO_AUDIT_FLAG_NONFINITE with a NaN record and count 0
 * for a sampled row or gap that is not finite and for a bad route.  No samples: a NaN record, count 0, flags 0.  The
 * mean is the sum over count; each lane sums its own samples in time order, the lanes are combined in a fixed order. */
int neo_fleet_track_audit(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, const double *cmd, int cap,
                          const int32_t *n_flown, int stride, double cmd_hz, const double *vertices, int n_vertices,
                          const int32_t *route_begin, const double *speed, const int32_t *closed, double radius,
                          double *track, int32_t *count, int32_t *flags);
int neo_fleet_track_audit_dev(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, const double *cmd, int cap,
                              const int32_t *n_flown, int stride, double cmd_hz, const double *vertices,
                              int n_vertices, const int32_t *route_begin, const double *speed, const int32_t *closed,
                              double radius, double *track, int32_t *count, int32_t *flags);

/* ---- fleet flight model (a drone that tracks its commands with lag and gusts, in place of PX4 / Gazebo) ----------------
 * The reference reads the drone's odometry, not the command, for set_local_target (:452), the reach test (:183), the
 * camera pose, the flight metric (:333-363) and save_tracking_err (:310-331); only the planning start state comes from
 * the command array (:527-537).  csrc/neo_flight.hpp is the model, neo_planner_amd.flight_model its NumPy twin and its
 * definition, bit for bit.  Per mission, caller-owned DEVICE buffers indexed by MISSION:
 *   drone[B][8]          position p, velocity v, lagged thrust acceleration a, gust acceleration g, 2-D each;
 *   flown[B][cap][3][2]  the flown rows, in the command rows' layout: row t is the drone at t / cmd_hz;
 *   flown_len[B]         rows flown so far; saturated[B] sub-steps whose command was clipped to a_max.
 * Sub-step t (one command period h; t the absolute row) takes the drone from row t - 1 to row t against the command it
 * holds during that period, r = cmd[min(t - 1, cmd_len - 1)] = (p_d, v_d, a_d):
 *   u = a_d + kp (p_d - p) + kv (v_d - v);  n = |u| > a_max: u *= a_max / n, saturated += 1;  a += alpha (u - a);
 *   t % gust_every == 0 and scale != 0: g = rho g + scale z, z values 0 and 1 of csrc/neo_counter_rng.hpp's stream with
 *   the key `seed` and the counter (mission_ids[b], t / gust_every, 0, 4 << 24);  v += h (a + g - drag v);  p += h v;
 *   flown row t = (p, v, a + g - drag v).  fp64, + - * / and sqrt, every operation rounded on its own.
 * The caller computes the derived values once: h = 1 / cmd_hz, alpha = h / (tau + h), rho = exp(-gust_every h / gust_tau),
 * scale = gust_sigma sqrt(1 - rho^2).  The draw index is the absolute row: a flight does not depend on how launches cut
 * it, nor on B, the subset or its order.
 * The launch parameter stands next to B in both calls (the model, a HOST struct read before the launch; flown_len, a device
 * array); subset and n_subset follow it.
 * NEO_ERR_INVALID before any launch, with a neo_last_error message: a NULL required buffer, B < 0, a bad subset size,
 * cap <= 0, step, ahead or settle outside 0 .. 2^30, stride < 1, a model with a field that is not finite, h, a_max or
 * alpha not > 0, or gust_every < 1, a reach that is not finite. */
typedef struct neo_flight_model {
  double h;            /* 1 / cmd_hz */
  double kp, kv;       /* gains on the position and the velocity error */
  double a_max;        /* the largest commanded acceleration */
  double alpha;        /* h / (tau + h): the thrust lag */
  double drag;         /* linear drag, 1 / s */
  double rho, scale;   /* the gust's AR(1) step; scale 0: no gusts, nothing is drawn */
  int32_t gust_every;  /* sub-steps between two draws */
  uint64_t seed;       /* the key of the gust streams */
} neo_flight_model;
#define NEO_FLY_FIELDS 6
enum {
  NEO_FLY_POS_ERR_RMS = 0,    /* sqrt(sum(e^2) / count), e the distance between the flown and the commanded position */
  NEO_FLY_POS_ERR_MAX = 1,    /* the largest e ... */
  NEO_FLY_POS_ERR_MAX_AT = 2, /* ... and its row; the first sample wins ties */
  NEO_FLY_VEL_ERR_RMS = 3,    /* the same of the velocities */
  NEO_FLY_VEL_ERR_MAX = 4,
  NEO_FLY_POS_ERR_FINAL = 5   /* e at row flown_len - 1, whatever the stride */
};
/* neo_fleet_advance_dev with the model in place of perfect tracking, one lane per mission.  For a mission with
 * cmd_len >= 1 (clamped to cap): `first` != 0 (or flown_len[b] < 1: nothing of it flown yet) writes flown row cmd_index
 * from the state as it stands, so row 0 is the start state; the sub-steps cmd_index + 1 .. min(cmd_index + step,
 * cmd_len - 1) follow, each writing its flown row; cmd_index, future_index and head[B][3][2] are exactly
 * neo_fleet_advance_dev's -- the planning start state comes from the COMMAND array -- cur_pos[B][2] is the actual
 * position and flown_len = cmd_index + 1.  settle > 0 is the last launch of a landed mission: on the array's last row the
 * last command is held for at most `settle` more sub-steps, up to the first that starts with sqrt(dx * dx + dy * dy) <
 * reach, measured to goal[B][2]; those rows are appended to flown (flown_len counts them).  Nothing is written at or past
 * row cap: a flight that would go past it stops there and raises NEO_FLEET_FLAG_CMD_FULL in flags[B].  A mission with
 * cmd_len < 1 keeps every row and word it has.  mission_ids: int32 [B], ids in 0 .. 2^31 - 1; NULL: b itself.  Device
 * pointers only. */
int neo_fleet_fly_dev(neo_ctx *ctx, int B, const neo_flight_model *model, const int32_t *subset, int n_subset,
                      const double *cmd, int cap, const int32_t *cmd_len, int32_t *cmd_index, int32_t *future_index,
                      int step, int ahead, int first, int settle, double reach, const int32_t *mission_ids,
                      const double *goal, double *drone, double *flown, int32_t *flown_len, int32_t *saturated,
                      int32_t *flags, double *cur_pos, double *head);
/* save_tracking_err's table (:310-331) reduced per mission, one wavefront per mission: sample j is flown row j * stride
 * < flown_len[b] (clamped to 0 .. cap) against command row min(j * stride, cmd_len[b] - 1) -- the settle rows against the
 * last command.  fly[B][NEO_FLY_FIELDS] as the enum above, count[B] the samples, flags[B] written (not OR-ed): 0, or
 * NEO_AUDIT_FLAG_NONFINITE with a NaN record and count 0 for a sampled position, velocity or result that is not finite.
 * No samples or no commands: a NaN record, count 0, flags 0.  Each lane sums its own samples in time order, the lanes are
 * combined in a fixed order.  Device pointers only. */
int neo_fleet_fly_error_dev(neo_ctx *ctx, int B, const int32_t *flown_len, const int32_t *subset, int n_subset,
                            const double *flown, const double *cmd, int cap, const int32_t *cmd_len, int stride,
                            double *fly, int32_t *count, int32_t *flags);

/* ---- fleet campaigns (ros_node/manager_node.py:153-193: the next goal as soon as one is reached or given up) --------
 * A mission flies a sequence of goals; each goal is a LEG (csrc/neo_legs.hpp; neo_planner_amd.goal_sequences.GoalSequences
 * is the NumPy model of the goal lists, bit for bit).  When a leg ends the caller uploads outcome[b] for the closing
 * missions and runs, on the same subset: neo_fleet_leg_close_dev, neo_fleet_audit_batch_dev with close's n_flown (a leg's
 * rows start at row 0 of the mission's command array), neo_fleet_leg_open_dev.  One lane per mission, fp64, everything
 * indexed by MISSION; `subset` as for the other fleet calls; same bits whatever the subset, its order and the launch.
 * outcome[B], the one input a leg's end adds, stands next to B in both calls; subset and n_subset follow it.
 * The goal lists, struct neo_leg_sequences -- DEVICE pointers for the _dev calls, HOST pointers for neo_fleet_leg_goal:
 *   kind NEO_LEGS_TABLE   goals[n_goals][2] and seq_begin[B + 1], laid out as the route table is: mission b's goals are
 *                         goals[seq_begin[b] .. seq_begin[b + 1]), 1 to NEO_FLEET_LEGS_MAX of them;
 *   kind NEO_LEGS_FLAP    the reference's set_random_goal: `legs` goals a mission, goal k = (x_pair[k & 1],
 *                         y_scale * (u - y_shift)), u the 52-bit uniform of csrc/neo_counter_rng.hpp with the key `seed`
 *                         and the counter (mission_ids[b], k, 0, 3 << 24), words 0 and 1 (mission_ids: int32 [B], ids in
 *                         0 .. 2^31 - 1; NULL: b itself).
 * NEO_ERR_INVALID before any launch, with a neo_last_error message: a NULL required buffer, B < 0, a bad subset size,
 * cap < 1, max_legs outside 1 .. NEO_FLEET_LEGS_MAX, a threshold that is not finite and >= 0, a kind that is none of the
 * two, a table with fewer goals than missions (some mission would have none) or a flap with legs outside
 * 1 .. NEO_FLEET_LEGS_MAX, x_pair, y_scale or y_shift not finite; neo_fleet_leg_goal, which reads the table on the host,
 * also for any mission with fewer than 1 or more than NEO_FLEET_LEGS_MAX goals.  (On the device a mission whose list is
 * not one has no next goal.) */
#define NEO_FLEET_LEGS_MAX 64
#define NEO_LEGS_TABLE 0
#define NEO_LEGS_FLAP 1
typedef struct neo_leg_sequences {
  int32_t kind;               /* NEO_LEGS_TABLE or NEO_LEGS_FLAP */
  int32_t legs;               /* flap: goals a mission */
  int32_t n_goals;            /* table */
  const double *goals;        /* table */
  const int32_t *seq_begin;   /* table */
  uint64_t seed;              /* flap */
  const int32_t *mission_ids; /* flap, or NULL */
  double x_pair[2];           /* flap: x of the even and of the odd legs */
  double y_scale, y_shift;    /* flap */
} neo_leg_sequences;
/* how a leg ended: outcome[b] */
#define NEO_LEG_LANDED 1    /* the plan near the goal was spliced */
#define NEO_LEG_ABANDONED 2 /* all 11 targets of a tick failed */
#define NEO_LEG_TIMEOUT 3   /* the leg ran past its time limit (max_target_find_time) */
#define NEO_LEG_STUCK 4     /* NEO_FLEET_FLAG_CMD_FULL or NEO_FLEET_FLAG_SPLICE_FAILED was raised */
#define NEO_LEG_OPEN 5      /* the run ended first: logged, and nothing is opened */
/* a row of leg_log[B][max_legs][NEO_LEG_FIELDS]; the integers are stored as doubles */
#define NEO_LEG_FIELDS 21
enum {
  NEO_LEG_GOAL_X = 0,
  NEO_LEG_GOAL_Y = 1,
  NEO_LEG_START_X = 2,      /* where the leg began: leg_start[b] */
  NEO_LEG_START_Y = 3,
  NEO_LEG_OUTCOME = 4,      /* NEO_LEG_* */
  NEO_LEG_N_FLOWN = 5,
  NEO_LEG_FINAL_DIST = 6,
  NEO_LEG_FLAGS = 7,        /* the mission's NEO_FLEET_FLAG_* of this leg, NEO_FLEET_FLAG_ABANDONED with that outcome */
  NEO_LEG_COUNT = 8,        /* the audit's count ... */
  NEO_LEG_AUDIT_FLAGS = 9,  /* ... and flags */
  NEO_LEG_AUDIT = 10,       /* the NEO_AUDIT_FIELDS values of the audit record, in its order */
  NEO_LEG_SUCCESS = 20      /* 1: LANDED, final_dist < threshold, no METRIC_FAIL | NONFINITE, flags == 0 */
};
/* what a leg was: n_flown[b] = cmd_len[b] for NEO_LEG_LANDED, else min(cmd_index[b] + 1, cmd_len[b]), clamped to 0 .. cap;
 * leg_end[B][2][2] = position and velocity of row n_flown - 1, head[b][0 .. 1] when n_flown == 0 (a leg that never got a
 * plan); final_dist[b] = sqrt(dx * dx + dy * dy) from there to goal[b], each operation rounded on its own
 * (np.linalg.norm's bits), inf when n_flown == 0.  outcome[B] is read for the launched missions only. */
int neo_fleet_leg_close_dev(neo_ctx *ctx, int B, const int32_t *outcome, const int32_t *subset, int n_subset,
                            const double *cmd, int cap, const int32_t *cmd_len, const int32_t *cmd_index,
                            const double *head, const double *goal, int32_t *n_flown, double *leg_end,
                            double *final_dist);
/* logs the leg and starts the next.  With k = leg[b] (outside 0 .. max_legs - 1: the mission is skipped): row k of
 * leg_log from goal[b], leg_start[b], outcome, close's n_flown / leg_end / final_dist, flags[b], the audit's count /
 * audit_flags / audit[B][NEO_AUDIT_FIELDS] and `threshold` (target_reach_threshold); leg[b] = k + 1; then, unless the
 * outcome is NEO_LEG_OPEN, if the mission has a goal k + 1 and k + 1 < max_legs: that goal into goal[b], cur_pos[b] =
 * leg_start[b] = the end position, head[b] = [end position, end velocity, 0], cmd_len = cmd_index = future_index = 0,
 * flags[b] = 0 (first_plan plans from drone_state, :491-504; init_mission zeroes des_state_index).  Otherwise nothing
 * more changes: the last leg's command array stays.  The caller writes leg_start of leg 0 (head[b][0] is the look-ahead
 * state once a leg has flown a tick, so a leg's start has a row of its own). */
int neo_fleet_leg_open_dev(neo_ctx *ctx, int B, const int32_t *outcome, const int32_t *subset, int n_subset,
                           const neo_leg_sequences *seq, int max_legs, double threshold, const int32_t *n_flown,
                           const double *leg_end, const double *final_dist, const int32_t *count,
                           const int32_t *audit_flags, const double *audit, int32_t *leg, double *leg_log,
                           double *leg_start, double *goal, double *cur_pos, double *head, int32_t *cmd_len,
                           int32_t *cmd_index, int32_t *future_index, int32_t *flags);
/* the goal model alone, HOST pointers (seq's too), evaluated on the device: goal[n][2] = goal leg_of[p] of mission
 * mission[p] and exists[p] = 1; NaN and 0 where the mission has no such goal or is outside 0 .. B - 1. */
int neo_fleet_leg_goal(neo_ctx *ctx, const neo_leg_sequences *seq, int B, int n, const int32_t *mission,
                       const int32_t *leg_of, double *goal, int32_t *exists);

/* ---- fleet record mode (traj_planner/record_planner.py:13-72, :152-185) ----------------
 * What the reference's `record` planner saves of every successful plan, for the missions of a fleet: one row of a
 * RESIDENT dataset of `capacity` rows, caller-owned DEVICE buffers:
 *   motion[capacity][24]            form_nn_input's vector (:13-58), see below;
 *   wpts_local[capacity][3 (M - 1)] form_nn_output (:61-72): the waypoints in the body frame, waypoint-major (x, y, z);
 *   tau[capacity][M]                the last M entries of the plan's x -- the durations are
 *                                   ts = (T_max - T_min) / (1 + exp(-tau)) + T_min (expert_planner.py:477-483), which the
 *                                   HOST derives: the device's exp is not libm's;
 *   pose_rows[capacity][5]          the sensed pose (eye x, y, z, c, s) the row was formed with;
 *   meta[capacity][3]               int32: mission id, tick, target round;
 *   images[capacity][H][W]          the mission's uint8 depth image (neo_depth_render_batch's depth_u8);
 *   n_rows[1], dropped[1]           int32 device words: rows filled so far, and rows that found no place.  The caller
 *                                   zeroes them once and reads them when it wants to know.
 * Fleet state as in the section above (device arrays indexed by MISSION, `subset` of n_subset mission indices or NULL
 * = all B, an index outside 0 .. B - 1 is skipped, a mission may appear once).  fp64, every operation rounded on its
 * own, so NumPy gives the same bits; no atomics: a mission's row depends on neither B, the subset nor its position,
 * and its row NUMBER only on the launched missions before it.  Nothing is written outside rows 0 .. capacity - 1 of
 * any dataset array.  Device pointers only, asynchronous on the context's stream.
 * NEO_ERR_INVALID before any launch, with a neo_last_error message: B < 1, a bad subset size, M outside 2 .. 64,
 * capacity < 1, cap <= 0, width or height outside 1 .. 4096, a NULL required buffer. */
/* drone_state.global_vel at the time of a tick's plans, one lane per mission: cur_vel[B][2] = the velocity of row
 * cmd_index[b] of cmd[b] (clamped into 0 .. cmd_len - 1) for a mission with cmd_len >= 1, else head[b][1] -- before
 * the first plan drone_state is plan_init_state (ros_node/traj_planner_node.py first_plan).  Call it once a tick before
 * any plan: the splice of a later target round may overwrite row cmd_index. */
int neo_record_state_dev(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, const double *cmd, int cap,
                         const int32_t *cmd_len, const int32_t *cmd_index, const double *head, double *cur_vel);
/* One target round's rows, two launches.  Rank (one workgroup, ballot and prefix counts): the launched mission at
 * position k with solved[b] != 0 (solved NULL: every launched mission) gets row_of[k] = *n_rows + its rank among
 * them; the others -1; a row at or beyond `capacity` is -1 too and counted in *dropped; *n_rows advances by the rows
 * given.  row_of is a device array of at least the launched missions, written for every position.  Commit (one
 * workgroup of 256 lanes per launched mission, returns at once on row -1) writes the row from x[B][3 M - 2],
 * head[B][3][2], tail[B][3][2], pose[B][5] (neo_fleet_pose_dev), cur_vel[B][2] and staging[B][H][W], the tick's images
 * by mission.  With R = [[c, -s, 0], [s, c, 0], [0, 0, 1]] of the pose, R^T v = (c vx + s vy, -s vx + c vy, vz) and
 * p = (px, py, pz) the eye, the 24 values of motion are: R^T (cur_vel, 0); R row-major; R^T ((head pos, pz) - p);
 * R^T ((head vel, 0) - (cur_vel, 0)); the same two for tail.  Waypoint i is R^T ((q_x[i], q_y[i], pz) - p), q the
 * first 2 (M - 1) entries of x[b], row-major by dimension.  meta = (mission_ids[b], or b with mission_ids NULL; tick;
 * round).  The image is copied with 16-byte loads and stores over the aligned middle of the destination row and bytes
 * at both ends: H * W need not be a multiple of 16. */
int neo_record_commit_dev(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, int M, const double *x,
                          const double *head, const double *tail, const int32_t *solved, const double *pose,
                          const double *cur_vel, const uint8_t *staging, int width, int height,
                          const int32_t *mission_ids, int tick, int round, int capacity, double *motion,
                          double *wpts_local, double *tau, double *pose_rows, int32_t *meta, uint8_t *images,
                          int32_t *row_of, int32_t *n_rows, int32_t *dropped);

/* ---- the learned warm start on resident arrays (traj_planner/neo_planner.py:10-51) ----------------------------
 * What NeoPlanner.enhanced_traj_plan does between the depth image's 24 features and the optimiser, for B requests:
 *   motion (form_nn_input's vector) -> head (PlannerNet's dense layers) -> guess (the first guess neo_plan_guess_dev
 *   takes as x_init).
 * The image backbone is not part of it: its features come in as an array (neo_backbone_features_dev, below, makes
 * them from the depth images).  Device pointers only, asynchronous on the
 * context's stream, one launch each.  Every array is indexed by REQUEST; `subset` (n_subset request indices, a device
 * array) names the requests launched, NULL = all B; an index outside 0 .. B - 1 is skipped and its rows stay.  A
 * request's results depend on neither B, the subset nor its position.  M = 3 pieces, D = 2.
 * NEO_ERR_INVALID before any launch, with a neo_last_error message: B < 1, a bad subset size, a NULL buffer,
 * n_weights != NEO_INIT_HEAD_FLOATS, feature_rows not 1 or B. */
#define NEO_INIT_MOTION 24  /* form_nn_input's vector */
#define NEO_INIT_FEATURE 24 /* features of an image, and of the motion branch */
#define NEO_INIT_OUTPUT 9   /* 2 body-frame waypoints (x, y, z) and 3 durations */
#define NEO_INIT_X 7        /* x0 of a request: D (M - 1) + M */
/* floats of the weight blob: the eight Linear layers of PlannerNet.head in forward order -- the motion branch
 * 24 -> 48 -> 24 -> 24 -> 24, then the fusion MLP 48 -> 48 -> 96 -> 96 -> 9 -- each as W row-major [out][in], then
 * b[out] */
#define NEO_INIT_HEAD_FLOATS 20817
/* One lane per request: motion[B][24] = the 24 doubles neo_record_commit_dev writes into a row's motion, from the same
 * pose[B][5], cur_vel[B][2] (neo_record_state_dev), head[B][3][2] and tail[B][3][2] with the same fp64 operations, each
 * then converted to fp32 once: the network is fed in flight the bits it was trained on. */
int neo_init_motion_dev(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, const double *pose,
                        const double *cur_vel, const double *head, const double *tail, float *motion);
/* PlannerNet.head: out[B][9] = mlp([feature, motion_backbone(motion)]), LeakyReLU (v > 0 ? v : 0.01f v) after every
 * layer but the last of each stack.  feature[feature_rows][24]: one row per request (feature_rows = B) or one shared
 * row (feature_rows = 1).  fp32; a lane computes a whole dot product as acc = b[j], then for k ascending
 * acc = acc + W[j][k] * a[k], product and sum rounded on their own: the result is reproducible bit for bit on the
 * host.  A workgroup of 256 lanes per 32 requests, weights and activations in LDS. */
int neo_init_head_dev(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, const float *weights, size_t n_weights,
                      const float *feature, int feature_rows, const float *motion, float *out);
/* One lane per request: x0[B][7] = [x_0, x_1, y_0, y_1, tau_0, tau_1, tau_2] from out[B][9] and pose[B][5].  With
 * (lx, ly) the doubles of out[3 i], out[3 i + 1] (the body-frame z is dropped): x_i = (c lx - s ly) + px,
 * y_i = (s lx + c ly) + py.  Duration t = (double) out[6 + j] is clamped to [T_min + e, T_max - e],
 * e = 1e-3 (T_max - T_min), T_min and T_max the context's parameters (a NaN stays a NaN), and
 * tau_j = -log((T_max - T_min) / (t - T_min) - 1) (map_T2tau).  The waypoints are NumPy's bits; tau is the device's
 * fp64 log of the same argument. */
int neo_init_guess_dev(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, const float *out, const double *pose,
                       double *x0);

/* ---- the image backbone in front of the warm start (nn_trainer/nn_trainer.py:119-122) --------------------------
 * The `feature` rows neo_init_head_dev takes, from the depth images: the inference form of PlannerNet.img_backbone, a
 * ResNet-18 with a one-channel stem and a 24-wide fc, in eval mode, all fp32.  Every BatchNorm is folded into the
 * convolution in front of it when the blob is packed (w' = w g / sqrt(var + eps), b' = beta - mean g / sqrt(var + eps)):
 * the device sees convolutions with a bias.  Activations are channels-last, [image][y][x][c].
 * NEO_BACKBONE_FLOATS floats of the weight blob, in forward order:
 *   the stem            W[7][7][1][64], b[64]
 *   layer1 .. layer4    (64, 128, 256, 512 channels), two blocks each; a block is conv1 W[3][3][cin][cout], b[cout];
 *                       conv2 W[3][3][cout][cout], b[cout]; and, in the first block of layers 2 .. 4 (stride 2), the
 *                       downsample branch W[1][1][cin][cout], b[cout]
 *   fc                  W[24][512] row-major, b[24]
 * A convolution's W is [ky][kx][ci][co], the output channel fastest (torch's weight[co][ci][ky][kx], permuted).
 * Summation: an output element of a convolution is one fp32 fmaf chain from its bias over the taps (ky, kx) row-major
 * and, inside a tap, over the input channels in groups of 32, a group in the order 0, 16, 1, 17, ..., 15, 31; a padding tap
 * contributes products with +0.  The average pool adds a channel's pixels in ascending order and divides by their count;
 * the fc is one fmaf chain from its bias over k ascending.  So an image's features depend on neither n nor the image's
 * position among the n: they are the same bits in any batch.  (The rule is tested launch by launch against a plain host
 * restatement of it, through neo_backbone_activation_dev below: the MI355X's f32 matrix instruction is such a chain.) */
#define NEO_BACKBONE_FLOATS 11177752
/* bytes of `workspace` for n images of H x W: three activation buffers of the largest layer output (the 64-channel
 * output of the stem's pool for every but the smallest images).  0 for n <= 0, H or W < 1, or n * H * W >= 2^31. */
size_t neo_backbone_workspace_bytes(int n, int H, int W);
/* feature_out[n][24] from images_u8[n][H][W]: device pointers, 21 launches, asynchronous on the context's stream.  The
 * stem (uint8 -> float, 7 x 7 stride 2, ReLU, 3 x 3 stride-2 max pool) is one fused kernel; the 3 x 3 and 1 x 1
 * convolutions are implicit GEMMs on the f32 matrix instructions, columns = the flattened (image, y, x) of the output,
 * with bias, residual and ReLU in the epilogue; the last kernel is the global average pool and the fc.  `workspace`
 * (16-byte aligned, at least neo_backbone_workspace_bytes(n, H, W) bytes) is written and holds nothing afterwards; no other
 * memory is touched.  Any H, W >= 1 is valid.  n = 0 launches nothing.
 * NEO_ERR_INVALID before any launch, with a neo_last_error message: a NULL pointer, n < 0, H or W < 1,
 * n * H * W >= 2^31, n_weights != NEO_BACKBONE_FLOATS, a misaligned or too small workspace. */
int neo_backbone_features_dev(neo_ctx *ctx, const float *weights, size_t n_weights, const uint8_t *images_u8, int n, int H,
                              int W, void *workspace, size_t workspace_bytes, float *feature_out);
/* The same call for measurements: an event in front of the chain and one behind every launch, then it WAITS for the stream
 * and writes the NEO_BACKBONE_LAUNCHES times between them, in milliseconds, to the HOST array launch_ms -- the stem;
 * conv1, [downsample,] conv2 of the eight blocks in forward order; the pool and fc.  n >= 1. */
#define NEO_BACKBONE_LAUNCHES 21
int neo_backbone_launch_times(neo_ctx *ctx, const float *weights, size_t n_weights, const uint8_t *images_u8, int n, int H,
                              int W, void *workspace, size_t workspace_bytes, float *feature_out, float *launch_ms);
/* One launch's output, for tests and measurements: runs launches 0 .. `launch` of the same chain (in the order of
 * launch_ms above: 0 the stem, 1 .. 19 the convolutions, 20 the pool and fc) and copies what launch `launch` wrote to the
 * device array act_out on the context's stream: [n][h][w][c] fp32 channels-last for the stem (after its max pool) and a
 * convolution (after its residual and ReLU), [n][24] for the pool and fc.  act_floats must be n * h * w * c of
 * neo_backbone_activation_shape.  The refusals of neo_backbone_features_dev, and NEO_ERR_INVALID before any launch for
 * a launch outside 0 .. NEO_BACKBONE_LAUNCHES - 1, a NULL act_out, another act_floats. */
int neo_backbone_activation_dev(neo_ctx *ctx, const float *weights, size_t n_weights, const uint8_t *images_u8, int n, int H,
                                int W, void *workspace, size_t workspace_bytes, int launch, float *act_out, size_t act_floats);
/* h, w, c of launch `launch`'s output an image of H x W (1, 1, 24 for the pool and fc).  Host only, no context.
 * NEO_ERR_INVALID: a launch outside 0 .. NEO_BACKBONE_LAUNCHES - 1, H or W < 1, a NULL pointer. */
int neo_backbone_activation_shape(int launch, int H, int W, int *h, int *w, int *c);

/* ---- the same backbone with bf16 storage, on the bf16 matrix instructions: a second, opt-in route ----------------
 * The same network, the same 21 launches in the same order and the same fp32 features out; the fp32 calls above keep
 * their bits.  Weights of the 19 convolutions and every stored activation are bf16 (fp32's exponent range: no input and
 * no set of weights overflows a stored activation); accumulators, biases, the residual sum, the ReLU, the stem's
 * arithmetic, the average pool and the fc are fp32.
 * NEO_BACKBONE_BF16_BYTES bytes of the PACKED blob, made from the fp32 blob by neo_backbone_pack_bf16_dev, the parts in
 * the fp32 blob's order, back to back (every part's size is a multiple of 16 bytes, so every part starts 16-byte aligned):
 *   the stem           W[49][64] fp32, b[64] fp32, verbatim
 *   a convolution      W as bf16 (round to nearest even) in the layout [ky][kx][cin / 8][cout][8], the value at
 *                      [ky][kx][g][co][j] being the fp32 blob's W[ky][kx][ci = 8 g + j][co]; then b[cout] fp32, verbatim
 *   the fc             W[24][512] fp32, b[24] fp32, verbatim
 * 11 157 504 bf16 values and 20 248 floats.  Activations are channels-last bf16, [image][y][x][c].
 * Summation: an output element of a convolution is accumulated in fp32 from its fp32 bias over the taps (ky, kx)
 * row-major and, inside a tap, over the input channels ascending, 16 a matrix instruction; K is never split, a padding tap
 * contributes zeros, and an image's features depend on neither n nor the image's position among the n.  The products
 * are exact in fp32, so a launch's fp32 value differs from the exact sum of its products by the accumulation's rounding
 * alone; HOW the instruction adds its 16 products is not promised (it is held to the bound of any fp32 accumulation,
 * launch by launch, through neo_backbone_bf16_activation_dev).  The residual is added and the ReLU applied in fp32, and
 * the result is rounded to bf16 once, to nearest even, at the store; so is the stem's pooled value. */
#define NEO_BACKBONE_BF16_BYTES 22396000
/* packed_out[NEO_BACKBONE_BF16_BYTES] (16-byte aligned) from weights_f32[NEO_BACKBONE_FLOATS]: device pointers,
 * asynchronous on the context's stream.  NEO_ERR_INVALID before any launch: a NULL pointer, another n_weights or
 * packed_bytes, a misaligned pointer. */
int neo_backbone_pack_bf16_dev(neo_ctx *ctx, const float *weights_f32, size_t n_weights, void *packed_out, size_t packed_bytes);
/* bytes of `workspace` for n images of H x W: three bf16 activation buffers of the largest layer output.  0 where
 * neo_backbone_workspace_bytes returns 0. */
size_t neo_backbone_bf16_workspace_bytes(int n, int H, int W);
/* feature_out[n][24] fp32 from images_u8[n][H][W] and the packed blob: device pointers, NEO_BACKBONE_LAUNCHES launches,
 * asynchronous on the context's stream.  `workspace` (16-byte aligned, at least neo_backbone_bf16_workspace_bytes(n, H, W)
 * bytes) is written and holds nothing afterwards; no other memory is touched.  Any H, W >= 1 is valid.  n = 0 launches
 * nothing.  NEO_ERR_INVALID before any launch, with a neo_last_error message: a NULL pointer, n < 0, H or W < 1,
 * n * H * W >= 2^31, packed_bytes != NEO_BACKBONE_BF16_BYTES, a misaligned blob, a misaligned or too small workspace. */
int neo_backbone_features_bf16_dev(neo_ctx *ctx, const void *packed, size_t packed_bytes, const uint8_t *images_u8, int n, int H,
                                   int W, void *workspace, size_t workspace_bytes, float *feature_out);
/* The same call for measurements, as neo_backbone_launch_times: it WAITS for the stream and writes the
 * NEO_BACKBONE_LAUNCHES times, in milliseconds, to the HOST array launch_ms.  n >= 1. */
int neo_backbone_bf16_launch_times(neo_ctx *ctx, const void *packed, size_t packed_bytes, const uint8_t *images_u8, int n, int H,
                                   int W, void *workspace, size_t workspace_bytes, float *feature_out, float *launch_ms);
/* One launch's output, for tests: runs launches 0 .. `launch` of the chain and hands out what launch `launch` stored, as
 * uint16 bf16 bits in act_bf16_out, and the fp32 values it rounded (written by the same launch, on the same path up to
 * the store) in act_f32_out; both device arrays of act_elems = n * h * w * c elements of neo_backbone_activation_shape.
 * Either pointer may be NULL, not both.  Launch 20 (the pool and fc) has fp32 values only: act_bf16_out must be NULL.
 * The refusals of neo_backbone_features_bf16_dev, and NEO_ERR_INVALID before any launch for a launch outside
 * 0 .. NEO_BACKBONE_LAUNCHES - 1 and another act_elems. */
int neo_backbone_bf16_activation_dev(neo_ctx *ctx, const void *packed, size_t packed_bytes, const uint8_t *images_u8, int n,
                                     int H, int W, void *workspace, size_t workspace_bytes, int launch, uint16_t *act_bf16_out,
                                     float *act_f32_out, size_t act_elems);

/* ---- the `batch` planner mode on resident arrays (traj_planner/expert_planner.py:103-168) ----------------
 * MinJerkPlanner.batch_plan optimises K laterally shifted initial guesses of one request and keeps the cheapest
 * feasible one.  These two calls are what surrounds the optimiser launch for P requests at once, 2-D (D = 2), fp64:
 *   candidates -> neo_optimize_batch_from_dev over the P * K packed rows -> select.
 * Two kinds of arrays:
 *   REQUEST-INDEXED [B]...   head, tail, slots, and everything select writes: indexed by request b;
 *   PACKED [P * K]...        x0, head_k, tail_k, slots_k and the optimiser's results: row p * K + k holds candidate k
 *                            of the request at position p of the launch (request-major).
 * `subset` (n_subset request indices; a DEVICE array in the _dev forms, a host array in the host forms) names the
 * requests launched, P = n_subset; NULL = all B, P = B, position p is request p.  An index outside 0 .. B - 1 in
 * `subset` is skipped: candidates leaves its packed rows as they are, select writes nothing for it.  A request may
 * appear in a subset once.  tau, lateral_offsets and weights4 are always HOST arrays (a few values, handed to the
 * kernels by value).  A request's results depend on neither B, the subset nor the launch.
 * Errors, before anything is launched, with a neo_last_error message: D != 2, K < 1, K > NEO_BATCH_MAX_CANDIDATES,
 * M < 2, a shape neo_optimize_batch refuses, a NULL required buffer, B < 0, a bad subset size: NEO_ERR_INVALID. */
#define NEO_BATCH_MAX_CANDIDATES 8
/* batch_generate_init_variables (:103-140), one lane per packed row.  head / tail [B][3][2] request-indexed; slots [B]
 * request-indexed map-table slots or NULL; tau[M] = map_T2tau of the shared durations init_T * [1.5, 1, ..., 1, 1.5];
 * lateral_offsets[K] signed offsets along lateral_dir[0] = (f_y, -f_x), f the unit vector from start to target -- NULL:
 * the reference's 0, +0.6, -0.6, +0.6, ... (its 0.6 * lateral_dir[(k - 1) % 2]; the distance does not grow).
 *   x0[P * K][n]          n = 2 (M - 1) + M: the M - 1 waypoints of np.linspace(start + stride, target, M - 1,
 *                         endpoint=False) by dimension, shifted by the candidate's offset, then tau -- every value with
 *                         the bits NumPy computes (an offset of exactly 0 adds nothing: with start == target the
 *                         direction is 0 / 0, candidates with an offset are NaN and candidate 0 is finite, as in the
 *                         reference);
 *   head_k, tail_k [P * K][3][2]   the request's head and tail, once per candidate;
 *   slots_k[P * K]        slots[b] per candidate (0 without slots); NULL: not written.
 * The host form copies x0, head_k, tail_k and slots_k up first, so rows of skipped indices come back as they were. */
int neo_batch_candidates(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, int M, int D, int K,
                         const double *head, const double *tail, const int32_t *slots, const double *tau,
                         const double *lateral_offsets, double *x0, double *head_k, double *tail_k, int32_t *slots_k);
/* the same with DEVICE pointers (tau and lateral_offsets stay host arrays), asynchronous on the context's stream */
int neo_batch_candidates_dev(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, int M, int D, int K,
                             const double *head, const double *tail, const int32_t *slots, const double *tau,
                             const double *lateral_offsets, double *x0, double *head_k, double *tail_k,
                             int32_t *slots_k);
/* the choice (:160-165), one wavefront per request, from the optimiser's PACKED results x_k [P * K][n], costs4_k,
 * costs4_last_k [P * K][4], nit_k, nfev_k (or NULL), status_k [P * K] and weights4 (NULL: neo_params' weights).
 * Candidate k is feasible when (status & 0xff) <= NEO_TRAJ_MAXITER and neither NEO_TRAJ_FLAG_COLLISION nor
 * NEO_TRAJ_BAD_SCENE is set; its cost is (costs4_last * weights4).sum() in NumPy's order ((p0 + p1) + p2) + p3, +inf
 * when it is not feasible.  REQUEST-INDEXED results:
 *   chosen[B]        np.argmin of the costs (the first index of the minimum); -1 when no candidate is feasible or the
 *                    minimum is NaN (the reference falls back to warm_start_plan then);
 *   cand_cost[B][K]  the costs; solved[B] = chosen >= 0;
 *   x[B][n], costs4[B][4], costs4_last[B][4], status[B], nit[B], nfev[B] (the last two or NULL)   the chosen
 *                    candidate's results; a request with chosen = -1 leaves them untouched;
 *   nit_total[B]     sum of nit over the candidates with (status & 0xff) < NEO_TRAJ_NUMERIC_RANGE, opt_runs[B] their
 *                    number: what the reference adds to iter_num and opt_running_times (an overflowed run raises
 *                    before it is counted).
 *   fallback[P], n_fallback[1]   the requests with chosen = -1, compacted, in the order of their positions in the
 *                    launch (ascending with an ascending subset or none); entries from n_fallback on are scratch.  No
 *                    atomics decide a position: the list is the same from launch to launch.  A caller copies 4 bytes
 *                    and the list, not B statuses.
 * The host form copies the request-indexed arrays up first: what select does not write comes back as it was. */
int neo_batch_select(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, int M, int D, int K, const double *x_k,
                     const double *costs4_k, const double *costs4_last_k, const int32_t *nit_k, const int32_t *nfev_k,
                     const int32_t *status_k, const double *weights4, int32_t *chosen, double *cand_cost,
                     int32_t *solved, double *x, double *costs4, double *costs4_last, int32_t *nit, int32_t *nfev,
                     int32_t *status, int32_t *nit_total, int32_t *opt_runs, int32_t *fallback, int32_t *n_fallback);
int neo_batch_select_dev(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, int M, int D, int K,
                         const double *x_k, const double *costs4_k, const double *costs4_last_k, const int32_t *nit_k,
                         const int32_t *nfev_k, const int32_t *status_k, const double *weights4, int32_t *chosen,
                         double *cand_cost, int32_t *solved, double *x, double *costs4, double *costs4_last,
                         int32_t *nit, int32_t *nfev, int32_t *status, int32_t *nit_total, int32_t *opt_runs,
                         int32_t *fallback, int32_t *n_fallback);

/* ---- BatchPlanner.plan's retry chain on resident arrays (traj_planner/expert_planner.py:186-203) --------
 * warm_start_plan gives a request up to five plan_once runs: an attempt that ends the way the reference raises on is
 * re-seeded (straight line + N(0, 0.5) jitter, :94, :201) and optimised again.  These two calls are what surrounds the
 * optimiser launch of ONE attempt for P requests at once, D = 2 or 3, fp64:
 *   guess -> neo_optimize_batch_from_dev over the P packed rows -> merge,
 * and merge's list of failed requests is the next attempt's `subset`.  Between two attempts a host reads the count
 * (4 bytes) and the list, and draws the jitter of those requests; everything else stays on the device.
 * Two kinds of arrays, as in the neo_batch_* block:
 *   REQUEST-INDEXED [B]...   head, tail, slots, x_init and everything merge writes: indexed by request b;
 *   PACKED [P]...            x0, head_k, tail_k, slots_k, noise and the optimiser's results: row p belongs to the
 *                            request at position p of the launch.
 * `subset` (n_subset request indices; a DEVICE array in the _dev forms, a host array in the host forms) names the
 * requests launched, P = n_subset; NULL = all B, P = B, position p is request p.  An index outside 0 .. B - 1 in
 * `subset` is skipped: guess leaves its packed rows as they are, merge writes nothing for it.  A request may appear
 * in a subset once.  frac and tau are always HOST arrays (a few values, handed to the kernel by value).  A request's
 * results depend on neither B, the subset nor the launch.
 * Errors, before anything is launched, with a neo_last_error message: M < 2, a shape neo_optimize_batch refuses
 * (D outside {2, 3} among them), a NULL required buffer, B < 0, a bad subset size: NEO_ERR_INVALID. */
/* generate_init_variables (:82-101), one lane per launched request.  head / tail [B][3][D] request-indexed; slots [B]
 * request-indexed map-table slots or NULL; frac[M - 1] = (k + 1) / M, the waypoints' places along the line;
 * tau[M] = map_T2tau of the durations init_T * [1.5, 1, ..., 1, 1.5].
 *   x0[P][n]           n = D (M - 1) + M: waypoint k of dimension d is start + (target - start) * frac[k], then
 *                      + noise[p][d][k] when noise (PACKED [P][D][M - 1], the re-seeded attempts' jitter) is given --
 *                      every operation rounded on its own, no fused multiply-add: the bits of NumPy's
 *                      start + (target - start) * f (+ noise) -- by dimension, then tau.
 *                      With x_init ([B][n] request-indexed, or NULL) the row is x_init[b] copied instead: a caller's
 *                      own start points (a warm start); frac, tau and noise are not read then;
 *   head_k, tail_k [P][3][D]   the request's head and tail;
 *   slots_k[P]         slots[b] (0 without slots); NULL: not written.
 * The host form copies x0, head_k, tail_k and slots_k up first, so rows of skipped indices come back as they were. */
int neo_plan_guess(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, int M, int D, const double *head,
                   const double *tail, const int32_t *slots, const double *x_init, const double *noise,
                   const double *frac, const double *tau, double *x0, double *head_k, double *tail_k, int32_t *slots_k);
/* the same with DEVICE pointers (frac and tau stay host arrays), asynchronous on the context's stream */
int neo_plan_guess_dev(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, int M, int D, const double *head,
                       const double *tail, const int32_t *slots, const double *x_init, const double *noise,
                       const double *frac, const double *tau, double *x0, double *head_k, double *tail_k,
                       int32_t *slots_k);
/* the re-seeded attempts' jitter drawn on the device, one lane per value: the PACKED noise[P][D][M - 1] that guess
 * adds, without a host draw, a read-back of the list or an upload.  Position p takes the counter stream of
 * stream_ids[b], b its request (stream_ids: int32, REQUEST-INDEXED [B], ids in 0 .. 2^31 - 1; NULL: b itself):
 *   noise[p][d][k] = 0.5 * z(seed, id, attempt, value d (M - 1) + k),
 * z the unit normal of csrc/neo_counter_rng.hpp -- Philox4x32-10 with the key (seed's low word, seed's high word) and
 * the counter (id, attempt, 0, 1 << 24 | value / 2), a 52-bit uniform from two output words, Wichura's AS241 -- which
 * neo_planner_amd/counter_rng.py restates in NumPy bit for bit (BatchPlanner.retry_noise_counter).  A value depends on
 * (seed, id, attempt, d, k) alone: not on B, the subset or the launch.  The rows of a skipped index stay (the host form
 * copies the P rows up first).  Further errors, before anything is launched: attempt < 0: NEO_ERR_INVALID. */
int neo_plan_jitter(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, int M, int D, uint64_t seed, int attempt,
                    const int32_t *stream_ids, double *noise);
/* the same with DEVICE pointers, asynchronous on the context's stream */
int neo_plan_jitter_dev(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, int M, int D, uint64_t seed,
                        int attempt, const int32_t *stream_ids, double *noise);
/* one attempt's bookkeeping, one wavefront per launched request, from the optimiser's PACKED results x_k [P][n],
 * costs4_k, costs4_last_k [P][4], nit_k, nfev_k, status_k [P].  REQUEST-INDEXED results, written for every launched
 * request (requests not launched keep theirs):
 *   x[B][n], costs4[B][4], costs4_last[B][4], nit[B], nfev[B], status[B]   the attempt's results (status with its
 *                    NEO_TRAJ_FLAG_COLLISION bit);
 *   attempts[B]      += 1;
 *   nit_total[B]     (64-bit) += nit unless (status & 0xff) >= NEO_TRAJ_NUMERIC_RANGE: what the reference adds to
 *                    iter_num (an overflowed run raises before it is counted);
 *                    reset != 0 starts a chain instead: attempts = 1, nit_total = the counted nit;
 *   solved[B]        0 when the attempt FAILED -- ((status & 0xff) > NEO_TRAJ_MAXITER and != NEO_TRAJ_BAD_SCENE) or
 *                    NEO_TRAJ_FLAG_COLLISION -- 1 otherwise;
 *   failed[P], n_failed[1]   the failed requests, compacted, in the order of their positions in the launch (ascending
 *                    with an ascending subset or none); entries from n_failed on are scratch.  No atomics decide a
 *                    position.  It must not be the array `subset` points to: two attempts in a row alternate
 *                    between two lists;
 *   bad_scene[1]     1 when a launched request ended with NEO_TRAJ_BAD_SCENE (a map-table slot without a map: no
 *                    planning failure, retrying cannot help -- the caller's error to raise), 0 otherwise.
 * The host form copies the request-indexed arrays up first: what merge does not write comes back as it was. */
int neo_plan_merge(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, int M, int D, int reset, const double *x_k,
                   const double *costs4_k, const double *costs4_last_k, const int32_t *nit_k, const int32_t *nfev_k,
                   const int32_t *status_k, double *x, double *costs4, double *costs4_last, int32_t *nit, int32_t *nfev,
                   int32_t *status, int32_t *attempts, int64_t *nit_total, int32_t *solved, int32_t *failed,
                   int32_t *n_failed, int32_t *bad_scene);
int neo_plan_merge_dev(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, int M, int D, int reset,
                       const double *x_k, const double *costs4_k, const double *costs4_last_k, const int32_t *nit_k,
                       const int32_t *nfev_k, const int32_t *status_k, double *x, double *costs4, double *costs4_last,
                       int32_t *nit, int32_t *nfev, int32_t *status, int32_t *attempts, int64_t *nit_total,
                       int32_t *solved, int32_t *failed, int32_t *n_failed, int32_t *bad_scene);

/* ---- adaptive waypoint counts: mixed M in one plan chain (traj_planner/expert_planner.py:86-88) ----------
 * With init_wpts_mode 'adaptive' the reference places one waypoint per init_seg_len metres of straight-line distance:
 * max(ceil(L / init_seg_len - 1), 1).  These calls give every request of a launch list its own count, group the list
 * by count on the device, and carry BatchPlanner.plan's retry chain over the groups: per attempt and group
 *   neo_plan_guess_dev -> neo_optimize_batch_from_dev (M = count + 1) -> neo_adaptive_merge_dev,
 * then ONE neo_adaptive_compact_dev for all groups.  A host reads the group table once and the groups' failed counts
 * once per attempt; it never waits per group.  REQUEST-INDEXED and PACKED arrays, `subset` and skipped indices as in
 * the neo_plan_* block; a group is `count` = 0 .. NEO_MAX_PIECES - 1 (0 stays empty: a count is at least 1).
 * Errors, before anything is launched and with every output untouched, with a neo_last_error message: B < 1, a bad
 * subset size, D outside {2, 3}, max_waypoints outside 1 .. NEO_MAX_PIECES - 1, a seg_len that is not finite or not
 * > 0, a NULL required buffer, and for merge a shape neo_plan_merge refuses or x_stride < n: NEO_ERR_INVALID. */
/* the count of every launched request, one lane per position.  head / tail [B][3][D] request-indexed; only the
 * positions head[b][0], tail[b][0] are read.  Every operation rounded on its own, no fused multiply-add:
 *   d_k = tail[b][0][k] - head[b][0][k];  s = d_0 d_0 + d_1 d_1 (+ d_2 d_2), left to right;  L = sqrt(s);
 *   c = ceil(L / seg_len - 1.0);  counts[b] = max(c, 1), and 1 when L is not finite;
 *   above max_waypoints: counts[b] = max_waypoints and clamped[b] = 1 (0 otherwise)
 * -- BatchPlanner.adaptive_counts, bit for bit.  counts, clamped [B] request-indexed: rows of requests not launched
 * stay (the host form copies both up first). */
int neo_adaptive_count(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, int D, const double *head,
                       const double *tail, double seg_len, int max_waypoints, int32_t *counts, int32_t *clamped);
int neo_adaptive_count_dev(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, int D, const double *head,
                           const double *tail, double seg_len, int max_waypoints, int32_t *counts, int32_t *clamped);
/* the launch list grouped by count: a stable counting sort by ONE workgroup (a histogram pass, a scan over the
 * NEO_MAX_PIECES counters, a placement pass; ballots and per-wavefront counters in LDS, no atomics -- nothing depends
 * on scheduling).  counts [B] request-indexed.
 *   order[P]         the launched request indices by ascending count, in launch-list order within a count: what
 *                    np.argsort(counts[list], kind="stable") gives.  Skipped indices, and requests whose count is
 *                    outside 0 .. NEO_MAX_PIECES - 1, are dropped; entries from total on stay.  Must not be `subset`;
 *   bucket_begin[NEO_MAX_PIECES + 1]   group c is order[bucket_begin[c] .. bucket_begin[c + 1] - 1];
 *   total[1]         the entries kept (= bucket_begin[NEO_MAX_PIECES]).
 * An empty list (n_subset = 0 with a subset) writes an all-zero table and total 0. */
int neo_adaptive_bucket(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, const int32_t *counts, int32_t *order,
                        int32_t *bucket_begin, int32_t *total);
int neo_adaptive_bucket_dev(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, const int32_t *counts,
                            int32_t *order, int32_t *bucket_begin, int32_t *total);
/* neo_plan_merge_dev's bookkeeping for ONE group of a mixed chain (DEVICE pointers, asynchronous), two differences:
 * the request-indexed x has rows of x_stride >= n doubles -- row b gets the group's n = D (M - 1) + M values, then NaN
 * up to x_stride -- and nothing is compacted: pending[P] gets the request's index where it failed, -1 elsewhere
 * (skipped positions too), for neo_adaptive_compact_dev.  bad_scene[1] is set to 1 as in merge but zeroed only when
 * clear_bad != 0 (the first group a chain issues): it gathers over the groups.  An empty list launches nothing. */
int neo_adaptive_merge_dev(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, int M, int D, int x_stride,
                           int reset, int clear_bad, const double *x_k, const double *costs4_k,
                           const double *costs4_last_k, const int32_t *nit_k, const int32_t *nfev_k,
                           const int32_t *status_k, double *x, double *costs4, double *costs4_last, int32_t *nit,
                           int32_t *nfev, int32_t *status, int32_t *attempts, int64_t *nit_total, int32_t *solved,
                           int32_t *pending, int32_t *bad_scene);
/* the segmented compaction of an attempt: one workgroup per group, the in-place ordered walk of the plan chain's
 * compaction.  seg_begin, seg_len: HOST arrays [NEO_MAX_PIECES] (handed to the kernel by value): group c owns
 * pending[seg_begin[c] .. seg_begin[c] + seg_len[c] - 1]; segments must not overlap.  Its entries >= 0 are packed to the
 * front of the segment in position order and n_failed[c] is their number (0 for an empty segment); entries behind
 * them are scratch.  pending [rows], n_failed [NEO_MAX_PIECES]: device arrays in the _dev form; the host form takes
 * `rows`, the length of pending, and checks the segments against it.  Further errors: a negative seg_begin or seg_len:
 * NEO_ERR_INVALID. */
int neo_adaptive_compact(neo_ctx *ctx, const int32_t *seg_begin, const int32_t *seg_len, int rows, int32_t *pending,
                         int32_t *n_failed);
int neo_adaptive_compact_dev(neo_ctx *ctx, const int32_t *seg_begin, const int32_t *seg_len, int32_t *pending,
                             int32_t *n_failed);

/* ---- batched depth camera ---------------------------------------------------
 * B pinhole depth images of box scenes in one call: neo_planner_amd/initializer.py raycast_depth, the sensor in front
 * of the initializer network (traj_planner/record_planner.py:16-18 scales the image to uint8 by its maximum), for B
 * requests that each see their own scene from their own pose.
 *   boxes[NB][6]             doubles, lo xyz then hi xyz, the boxes of all scenes back to back
 *   box_begin[n_scenes + 1]  scene s owns the boxes box_begin[s] .. box_begin[s + 1]; at most NEO_DEPTH_MAX_BOXES each
 *   scene_index[B]           the scene of each request, or NULL: every request sees scene 0
 *   pose[B][5]               eye x y z, cos(yaw), sin(yaw): the caller takes the cosine and sine (the device calls no
 *                            trigonometric function)
 *   focal_px                 (width / 2) / tan(hfov / 2), in pixels; max_range in metres
 *   depth_m[B][height][width]   float32 metres along the optical axis, clipped to [0, max_range]
 *   depth_u8[B][height][width]  (uint8)(depth / max(depth_max, 1e-9f) * 255.0f), the network's input; may be NULL
 *   depth_max[B]                float32 maximum of each image; may be NULL
 * Camera frame: x forward, y left, z up; the ground is the plane z = 0.  Every ray is computed in fp32 with each
 * product rounded on its own (tests/depth_oracle_np.py restates it in NumPy, bit for bit), the pixel coordinates and
 * the boxes' corners relative to the eye in fp64 rounded once.  An image's bytes depend on its own pose, its scene's
 * boxes and the camera only: not on B, its place in the batch, the packing of the scenes or the launch.
 * NEO_ERR_INVALID before anything is copied or launched: B < 1, width or height outside 1..4096, focal_px or max_range
 * not finite or <= 0, n_scenes < 1, a NULL boxes / box_begin / pose / depth_m; host form also: box_begin not
 * non-decreasing from 0, a scene with more than NEO_DEPTH_MAX_BOXES boxes, a scene_index outside 0 .. n_scenes - 1.
 * The _dev form cannot read its index arrays: a request whose scene index (or box range) is out of range gets depth_m
 * NaN, depth_u8 0 and depth_max NaN, and reads no box. */
#define NEO_DEPTH_MAX_BOXES 1024
int neo_depth_render_batch(neo_ctx *ctx, int width, int height, double focal_px, double max_range, const double *boxes,
                           const int32_t *box_begin, int n_scenes, const int32_t *scene_index, int B, const double *pose,
                           float *depth_m, uint8_t *depth_u8, float *depth_max);
int neo_depth_render_batch_dev(neo_ctx *ctx, int width, int height, double focal_px, double max_range,
                               const double *boxes, const int32_t *box_begin, int n_scenes, const int32_t *scene_index,
                               int B, const double *pose, float *depth_m, uint8_t *depth_u8, float *depth_max);
/* diagnostics: optional DEVICE counter (64-bit, the caller zeroes it) to which the next render passes add, per tile, the
 * boxes left after culling times the tile's pixels: box tests per ray = counter / (B * height * width).  NULL switches it
 * off. */
int neo_depth_box_test_counter(neo_ctx *ctx, uint64_t *dev_count);

/* ---- onboard mapping (launch/map_server_onboard.launch) ---------------------------------
 * The depth images of B missions into B 2-D occupancy grids of their own: what octomap_server (0.1 m leaves,
 * sensor_model/max_range 6.0, projected_map of the band occupancy_min_z .. occupancy_max_z) gives ESDF.occupancy_map_cb
 * on the vehicle, as a fixed model: octomap's scan insertion (within a scan a hit wins over a miss, clamped log-odds,
 * occupied from probability 0.5) projected to 2-D.  tests/onboard_oracle_np.py is the model in NumPy; the kernel equals
 * it bit for bit.  Per mission and scan, with the ray directions of neo_depth_render_batch widened to fp64 --
 * dx_j = c + u_j s, dy_j = s - u_j c, dz_i = -v_i, each fp32 product and sum rounded on its own -- and every further
 * operation fp64, rounded on its own:
 *   cell of a point  fx = (px - ox) / res, fy = (py - oy) / res; outside the grid, and ignored, unless 0 <= fx < grid_w
 *                    and 0 <= fy < grid_h; else cell (int)fy * grid_w + (int)fx (map_server/esdf.py:61-62);
 *   hit              pixel (i, j) of depth d when d < sensor_range and z_lo <= ez + d dz_i <= z_hi: the cell of
 *                    (ex + d dx_j, ey + d dy_j).  A NaN depth marks nothing;
 *   passed           for the samples t_n = n (res / 2), n < ceil(sensor_range / (res / 2)), with t_n < min(d, sensor_range)
 *                    and z_lo <= ez + t_n dz_i <= z_hi: the cell of (ex + t_n dx_j, ey + t_n dy_j);
 *   update           the scan's marks are the union over its pixels, then every marked cell is updated once, from L0 = 0
 *                    if it was never updated: a hit cell to min(L0 + hit, hi), a cell passed but not hit to
 *                    max(L0 + miss, lo).  Unmarked cells keep their state.
 * Log-odds are integers in units of 0.05 (octomap's 0.7 / 0.4 / 0.12 / 0.97 are hit 17, miss -8, lo -40, hi 70),
 * stored as int8 with -128 = never updated.
 *   subset[n_subset]   DEVICE (host form: host) mission indices, NULL = all B; n = n_subset or B missions are launched
 *   depth_m[n][height][width], pose[n][5]   the image and the pose (neo_depth_render_batch's) of each LAUNCHED mission,
 *                      by position in the subset -- a caller renders only the missions that sense.  (c, s) must be a
 *                      unit vector to fp32 rounding: marks further from the eye than a unit heading reaches are dropped
 *   width, height, focal_px, max_range   the camera of neo_depth_render_batch; max_range < sensor_range is an error (a
 *                      depth clipped below sensor_range would read as a hit)
 *   origins[B][2]      the grids' origins, by mission; grid_w, grid_h, res are shared
 *   logodds[B][grid_h][grid_w]    int8, in and out, by mission (all -128 before the first scan)
 *   occupancy[B][grid_h][grid_w]  int8 as nav_msgs/OccupancyGrid.data: 100 where L >= 0, 0 where updated and L < 0,
 *                      -1 never updated.  Only the cells a scan marks are written: hand in the previous call's array
 *                      (all -1 before the first scan)
 *   changed[B]         1 where the set of cells with value 100 changed in this scan, else 0 (launched missions only)
 * A mission outside the subset keeps every byte.  Results do not depend on the order of pixels, launches or missions.
 * A mission may appear in a subset once: two workgroups on one mission would update its grids unordered (the host
 * form rejects a repeated entry, the _dev form cannot see it).
 * One workgroup per mission holds two bits a cell of the window a scan can touch in LDS: (2 h + 1)^2 cells around the
 * eye's cell, h = ceil(sensor_range sqrt(1 + u_max^2) (1 + 1e-6) / res) + 1 with u_max the outermost column's |u| (a
 * point lies d along the axis and d u across it) -- 169^2 cells for the 87 degree camera at the defaults.
 * NEO_ERR_INVALID before anything is copied or launched, with a message: B outside 1 .. 2^20, a bad subset size, width
 * or height outside 1..4096, focal_px, res or sensor_range not finite or <= 0, max_range < sensor_range, a band that is
 * not finite or has z_lo > z_hi, grid_w or grid_h < 1 or more than 2^30 cells, log-odds outside -127 <= lo <= hi <= 127,
 * 0 <= hit <= 127, -127 <= miss <= 0, a NULL buffer, a window that does not fit the 64 KB of LDS of a workgroup; host
 * form also: a subset entry outside 0 .. B - 1 (the _dev form skips it) or listed twice. */
int neo_onboard_integrate_batch(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, const float *depth_m,
                                const double *pose, int width, int height, double focal_px, double max_range, int grid_w,
                                int grid_h, double res, const double *origins, double sensor_range, double z_lo,
                                double z_hi, int hit, int miss, int lo, int hi, int8_t *logodds, int8_t *occupancy,
                                int32_t *changed);
/* the same with DEVICE pointers, asynchronous on the context's stream */
int neo_onboard_integrate_batch_dev(neo_ctx *ctx, int B, const int32_t *subset, int n_subset, const float *depth_m,
                                    const double *pose, int width, int height, double focal_px, double max_range,
                                    int grid_w, int grid_h, double res, const double *origins, double sensor_range,
                                    double z_lo, double z_hi, int hit, int miss, int lo, int hi, int8_t *logodds,
                                    int8_t *occupancy, int32_t *changed);

/* ---- timing of the device work (bench.py) ----------------------------------
 * When enabled, every kernel launch of the named family is bracketed by HIP events on
 * the context stream; neo_profile_read returns launches and summed milliseconds. */
enum { NEO_KERNEL_EVAL = 0, NEO_KERNEL_OPTIMIZE = 1, NEO_KERNEL_ESDF_BUILD = 2, NEO_KERNEL_ESDF_SAMPLE = 3, NEO_KERNEL_COUNT = 4 };
int neo_profile_enable(neo_ctx *ctx, int on);
/* optional DEVICE array [B] that the next neo_optimize_batch_dev launches fill with the number of
 * quadrature samples (ESDF lookups) each trajectory evaluated; NULL switches it off. */
int neo_optimize_sample_counter(neo_ctx *ctx, int64_t *dev_counts);
/* results as they finish (round 6).  One launch lasts as long as its LONGEST run (cfg2: 527 evaluations against a mean of
 * 135) while 80 % of its trajectories are complete after ~2/3 of that time.  `counter` is a device-accessible int32 (device
 * memory, or pinned host memory the device can add to) that the caller zeroes; every later neo_optimize_batch_dev /
 * _from_dev launch on this context then adds 1 to it -- a system-scope release, after the trajectory's x, cost terms,
 * counts and status are stored -- for each trajectory it completes.  A host that sees the counter reach k may copy the result
 * arrays on another stream: the k finished trajectories are final (preset status[] to -1 to tell them apart, and copy status[]
 * FIRST: a trajectory marked finished in that copy is final in every array copied after it), bit for bit what the
 * completed launch leaves.  NULL switches it off.  Plain launches of optimize_kernel only: while a counter is set, a
 * launch that would run the lane-group kernel (NEO_FLAG_LANE_GROUPS) and every neo_optimize_batch_budget_dev call (budgeted
 * launches exist to END a launch early instead) return NEO_ERR_INVALID with a neo_last_error message, before anything is
 * launched; the context stays usable. */
int neo_optimize_progress_counter(neo_ctx *ctx, int32_t *counter);
/* diagnostics: optional DEVICE array [B][cap][4] that the next neo_optimize_batch[_dev] launches fill with one record
 * per counted evaluation of every trajectory -- (f, line-search step, quadrature samples, iteration) -- so that a run
 * can be laid beside the CPU optimiser's evaluation by evaluation (tools/classify_divergence.py); NULL switches it off.
 * Not supported by the lane-group kernel: while a trace (or trace_xg) is set, a launch that would run it
 * (NEO_FLAG_LANE_GROUPS) returns NEO_ERR_INVALID with a neo_last_error message, before anything is launched; budgeted
 * launches refuse it the same way. */
int neo_optimize_trace(neo_ctx *ctx, double *dev_trace, int cap);
/* diagnostics: optional DEVICE array [B][cap][2][n] that receives, per counted evaluation, the evaluated point x_k
 * and its gradient g_k (as doubles, whatever arithmetic the kernel ran in).  With neo_optimize_trace's (f, step, ...)
 * records this is everything needed to re-evaluate a device run point by point on the CPU oracle and to re-derive
 * every line-search / restart decision on the host (tests/test_gpu_replay.py).  `cap` must equal neo_optimize_trace's
 * when both are on; NULL switches it off.  Refused like neo_optimize_trace by lane-group and budgeted launches. */
int neo_optimize_trace_xg(neo_ctx *ctx, double *dev_xg, int cap);
/* optional DEVICE permutation [B] for the next neo_optimize_batch_dev launches: workgroup i works on
 * trajectory order[i].  Results stay in the caller's order.  Workgroups start in index order, so
 * putting the runs expected to be long first shortens the launch (a late long run is its tail);
 * NULL = identity; it must be a permutation of 0..B-1 and is ignored by launches of another batch size.
 * neo_planner_amd.BatchPlanner sorts by time slack (sum(ts) * v_max / distance).
 * LIFETIME: the array is the caller's and is read by every later neo_optimize_batch[_dev | _from_dev] launch of B
 * trajectories on this context until another order (or NULL) is set: keep it allocated until those launches have
 * completed.  Only the optimiser kernels read it. */
int neo_optimize_dispatch_order(neo_ctx *ctx, const int32_t *dev_order, int B);
/* the expected-effort order computed ON THE DEVICE from a batch's resident start points (round 6): key = time slack of the
 * guess, sum(T) v_max / |goal - start|, largest first, ties by index -- what neo_planner_amd.BatchPlanner.expected_effort_order
 * computes on the host (a key that is not finite -- NaN or infinite start, goal or duration -- is 0 on both): a keys kernel and
 * a stable descending radix sort (rocPRIM) on the context's stream.  `scratch`
 * (neo_effort_order_scratch_bytes(B) bytes, 256-byte aligned; the B keys stay in its first B doubles) and order[B] are the
 * caller's device buffers (several batches in flight on several streams: one pair per batch).  Hand `order` to
 * neo_optimize_dispatch_order. */
size_t neo_effort_order_scratch_bytes(int B);
int neo_effort_order_dev(neo_ctx *ctx, int B, int M, int D, const double *x0, const double *head, const double *tail,
                         void *scratch, int32_t *order);
/* the same from a HOST permutation (copied into a context-owned device buffer); NULL or B = 0 resets.
 * Either way the permutation only applies to launches of exactly B trajectories. */
int neo_optimize_dispatch_order_host(neo_ctx *ctx, const int32_t *host_order, int B);
/* results of a batch as fp32 rows [x (n) | weighted total cost | 4 cost terms] -- what the ranks of a scene-sharded job
 * gather (neo_planner_amd/sharding.py): one launch on the context's stream, device pointers, weights4 on
 * the host.  out[B][n + 5]. */
int neo_pack_results_dev(neo_ctx *ctx, int B, int n, const double *x, const double *costs4, const double *weights4,
                         float *out);
/* the ESDF-lookup kernel's own permutation (neo_sampled_terms_batch[_dev] launches of exactly B trajectories; results stay
 * in the caller's order, bit-identical): there the lever is locality -- workgroup i runs on XCD i mod 8, each XCD has its
 * own L2, and BatchPlanner.spatial_order deals requests that fly through the same part of the field to the same XCD.
 * `order` is a host (on_device = 0) or device (on_device = 1) array of B ints; it is COPIED into a context-owned buffer
 * before the call returns (the call synchronises the context's stream), so the caller may free it right away.  NULL or
 * B = 0 resets.  Independent of neo_optimize_dispatch_order. */
int neo_sampled_terms_dispatch_order(neo_ctx *ctx, const int32_t *order, int on_device, int B);
int neo_profile_read(neo_ctx *ctx, int kernel, int64_t *launches, double *total_ms);
/* diagnostics, read-only: optimiser launches of this context since it was created, by the form of the kernel that ran
 * them.  The all-fp32 kernels with one lane per (piece, dimension) and n <= 128 variables exist twice: compiled for the one
 * launch plan the launcher always chooses for them (fixed_plan), and with the plan's selectors tested at run time
 * (dynamic_plan) -- the latter runs comparison launches (flags bit 4096), launches with a trace buffer, budgeted launches
 * and every kernel family that has no fixed plan.  Same results bit for bit; either pointer may be NULL. */
int neo_optimize_plan_launches(neo_ctx *ctx, int64_t *fixed_plan, int64_t *dynamic_plan);
int neo_profile_reset(neo_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* NEO_PLANNER_H */
