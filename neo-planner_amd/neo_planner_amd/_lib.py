"""ctypes binding of include/neo_planner.h.  Loading fails loudly: there is no CPU fallback."""
import ctypes
import os
import sys

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
# NEO_PLANNER_LIB: another build of the same library (kernel experiments in tools/)
LIB_PATH = os.environ.get("NEO_PLANNER_LIB") or os.path.join(PKG, "libneo_planner_hip.so")

NEO_OK = 0
NEO_F64, NEO_F32, NEO_F16 = 0, 1, 2
NEO_LAYOUT_LINEAR, NEO_LAYOUT_YZ4, NEO_LAYOUT_CELL8, NEO_LAYOUT_BRICK = 0, 1, 2, 3
LAYOUTS = {"linear": NEO_LAYOUT_LINEAR, "yz4": NEO_LAYOUT_YZ4, "cell8": NEO_LAYOUT_CELL8, "brick": NEO_LAYOUT_BRICK}
NEO_TRAJ_CONVERGED_GRAD, NEO_TRAJ_CONVERGED_F, NEO_TRAJ_ABNORMAL = 0, 1, 2
NEO_TRAJ_MAXITER, NEO_TRAJ_NUMERIC_RANGE, NEO_TRAJ_NONFINITE, NEO_TRAJ_BAD_SCENE, NEO_TRAJ_SUSPENDED = 3, 4, 5, 6, 7
NEO_TRAJ_FLAG_COLLISION = 0x100
NEO_EDT_GENERIC_LINES = 1
NEO_KERNEL_EVAL, NEO_KERNEL_OPTIMIZE, NEO_KERNEL_ESDF_BUILD, NEO_KERNEL_ESDF_SAMPLE = 0, 1, 2, 3
NEO_FLAG_ONE_WAVE_PER_SIMD, NEO_FLAG_TWO_WAVES_PER_SIMD, NEO_FLAG_LANE_GROUPS = 32, 64, 128
NEO_FLAG_F32_SOLVE = 2048
# neo_audit_traj_batch: fields of a record and flag bits
AUDIT_FIELDS = ("path_length", "feasibility", "collision", "weighted", "min_clearance", "t_min_clearance", "max_speed",
                "max_acc", "t_first_unsafe", "duration")
NEO_AUDIT_FIELDS = len(AUDIT_FIELDS)
NEO_AUDIT_FLAG_UNSAFE, NEO_AUDIT_FLAG_METRIC_FAIL, NEO_AUDIT_FLAG_OUTSIDE_MAP, NEO_AUDIT_FLAG_NONFINITE = 1, 2, 4, 8
# neo_geo_search_batch: flag bits
NEO_GEO_FLAG_NO_PATH, NEO_GEO_FLAG_START_OUTSIDE, NEO_GEO_FLAG_CAPPED, NEO_GEO_FLAG_PATH_TRUNCATED = 1, 2, 4, 8
NEO_GEO_FLAG_BAD_SCENE = 16
# neo_fleet_*: flag bits of a mission
NEO_FLEET_FLAG_TARGET_CAPPED, NEO_FLEET_FLAG_CMD_FULL, NEO_FLEET_FLAG_BAD_SCENE, NEO_FLEET_FLAG_SPLICE_FAILED = 1, 2, 4, 8
NEO_FLEET_FLAG_ABANDONED = 16
# neo_fleet_goal_route / neo_fleet_track_audit: vertices a route, fields of a tracking record
NEO_FLEET_ROUTE_MAX = 256
TRACK_FIELDS = ("gap_mean", "gap_max", "t_gap_max", "gap_min", "t_gap_min", "gap_final", "t_first_within", "frac_within")
NEO_TRACK_FIELDS = len(TRACK_FIELDS)
# neo_fleet_fly_error_dev: fields of a tracking-error record (flight_model.py)
FLY_FIELDS = ("pos_err_rms", "pos_err_max", "pos_err_max_at", "vel_err_rms", "vel_err_max", "pos_err_final")
NEO_FLY_FIELDS = len(FLY_FIELDS)
# neo_fleet_leg_*: goals a mission, the kinds of goal lists, how a leg ended, fields of a row of the leg log
NEO_FLEET_LEGS_MAX = 64
NEO_LEGS_TABLE, NEO_LEGS_FLAP = 0, 1
NEO_LEG_LANDED, NEO_LEG_ABANDONED, NEO_LEG_TIMEOUT, NEO_LEG_STUCK, NEO_LEG_OPEN = 1, 2, 3, 4, 5
LEG_FIELDS = ("goal_x", "goal_y", "start_x", "start_y", "outcome", "n_flown", "final_dist", "flags", "count",
              "audit_flags") + AUDIT_FIELDS + ("success",)
LEG_INT_FIELDS = ("outcome", "n_flown", "flags", "count", "audit_flags", "success")      # stored as doubles, exact
NEO_LEG_FIELDS = len(LEG_FIELDS)
NEO_MAX_PIECES = 64                # M of any trajectory; neo_adaptive_*: one group per waypoint count below it
NEO_BATCH_MAX_CANDIDATES = 8       # neo_batch_*: candidates a request
NEO_DEPTH_MAX_BOXES = 1024         # neo_depth_*: boxes a scene
# neo_init_*: sizes of the motion vector, a feature row, the network's output, x0, and the head's weight blob
NEO_INIT_MOTION, NEO_INIT_FEATURE, NEO_INIT_OUTPUT, NEO_INIT_X, NEO_INIT_HEAD_FLOATS = 24, 24, 9, 7, 20817
NEO_BACKBONE_FLOATS, NEO_BACKBONE_LAUNCHES = 11177752, 21     # neo_backbone_*: the weight blob, launches a call
NEO_BACKBONE_BF16_BYTES = 22396000                            # neo_backbone_*bf16*: the packed blob

# every symbol include/neo_planner.h declares (tests check the library exports them all)
EXPORTS = [
    "neo_abi_version", "neo_ctx_create", "neo_ctx_destroy", "neo_last_error", "neo_params_default",
    "neo_params_set", "neo_ctx_synchronize", "neo_esdf_upload_2d", "neo_esdf_build_2d",
    "neo_esdf_upload_3d", "neo_esdf_drop", "neo_esdf_query", "neo_cost_grad_batch",
    "neo_cost_grad_batch_dev", "neo_optimize_batch", "neo_optimize_batch_dev", "neo_scene_slot",
    "neo_optimize_workspace_bytes", "neo_eval_traj_batch", "neo_profile_enable", "neo_profile_read",
    "neo_profile_reset", "neo_optimize_sample_counter", "neo_optimize_dispatch_order",
    "neo_sampled_terms_batch", "neo_sampled_terms_batch_dev", "neo_esdf_build_3d",
    "neo_optimize_dispatch_order_host", "neo_ctx_set_stream", "neo_optimize_trace",
    "neo_optimize_batch_from_dev", "neo_optimize_trace_xg", "neo_sampled_terms_dispatch_order",
    "neo_esdf_build_config", "neo_pack_results_dev", "neo_optimize_state_bytes", "neo_optimize_batch_budget_dev",
    "neo_sampled_terms_batch_f32", "neo_sampled_terms_batch_f32_dev", "neo_effort_order_dev",
    "neo_optimize_progress_counter", "neo_effort_order_scratch_bytes", "neo_audit_traj_batch",
    "neo_audit_traj_batch_dev", "neo_geo_search_batch", "neo_geo_search_batch_dev", "neo_geo_prune_batch",
    "neo_geo_workspace_budget", "neo_fleet_target_batch", "neo_fleet_target_batch_dev", "neo_fleet_advance_dev",
    "neo_fleet_splice_dev", "neo_fleet_audit_batch", "neo_fleet_audit_batch_dev", "neo_batch_candidates",
    "neo_batch_candidates_dev", "neo_batch_select", "neo_batch_select_dev", "neo_plan_guess", "neo_plan_guess_dev",
    "neo_plan_merge", "neo_plan_merge_dev", "neo_depth_render_batch", "neo_depth_render_batch_dev",
    "neo_depth_box_test_counter", "neo_onboard_integrate_batch", "neo_onboard_integrate_batch_dev",
    "neo_esdf_build_2d_batch_dev", "neo_fleet_pose_dev", "neo_record_state_dev", "neo_record_commit_dev",
    "neo_optimize_plan_launches", "neo_init_motion_dev", "neo_init_head_dev", "neo_init_guess_dev",
    "neo_plan_jitter", "neo_plan_jitter_dev", "neo_fleet_jitter", "neo_fleet_jitter_dev",
    "neo_adaptive_count", "neo_adaptive_count_dev", "neo_adaptive_bucket", "neo_adaptive_bucket_dev",
    "neo_adaptive_merge_dev", "neo_adaptive_compact", "neo_adaptive_compact_dev",
    "neo_fleet_warm_guess_dev", "neo_fleet_warm_carry_dev",
    "neo_fleet_goal_route", "neo_fleet_goal_route_dev", "neo_fleet_hold_dev", "neo_fleet_track_audit",
    "neo_fleet_track_audit_dev",
    "neo_fleet_leg_close_dev", "neo_fleet_leg_open_dev", "neo_fleet_leg_goal",
    "neo_fleet_fly_dev", "neo_fleet_fly_error_dev",
    "neo_geo_guess_dev", "neo_geo_mask_builds",
    "neo_backbone_workspace_bytes", "neo_backbone_features_dev", "neo_backbone_launch_times",
    "neo_backbone_activation_dev", "neo_backbone_activation_shape",
    "neo_backbone_pack_bf16_dev", "neo_backbone_bf16_workspace_bytes", "neo_backbone_features_bf16_dev",
    "neo_backbone_bf16_launch_times", "neo_backbone_bf16_activation_dev",
]


class NeoParams(ctypes.Structure):
    _fields_ = [("v_max", ctypes.c_double), ("T_min", ctypes.c_double), ("T_max", ctypes.c_double),
                ("safe_dis", ctypes.c_double), ("delta_t", ctypes.c_double), ("weights", ctypes.c_double * 4),
                ("collision_cost_tol", ctypes.c_double), ("ftol", ctypes.c_double), ("gtol", ctypes.c_double),
                ("maxls", ctypes.c_int32), ("maxiter", ctypes.c_int32), ("maxfun", ctypes.c_int32),
                ("bugcompat_stale_T", ctypes.c_int32), ("sample_dtype", ctypes.c_int32),
                ("flags", ctypes.c_int32)]


class NeoLegSequences(ctypes.Structure):
    """neo_leg_sequences: the goal lists of a campaign (goal_sequences.GoalSequences fills it)"""
    _fields_ = [("kind", ctypes.c_int32), ("legs", ctypes.c_int32), ("n_goals", ctypes.c_int32),
                ("goals", ctypes.c_void_p), ("seq_begin", ctypes.c_void_p), ("seed", ctypes.c_uint64), ("mission_ids", ctypes.c_void_p),
                ("x_pair", ctypes.c_double * 2), ("y_scale", ctypes.c_double), ("y_shift", ctypes.c_double)]


class NeoFlightModel(ctypes.Structure):
    """neo_flight_model: the derived constants of a flight (flight_model.FlightModel.derived fills it)"""
    _fields_ = [(k, ctypes.c_double) for k in ("h", "kp", "kv", "a_max", "alpha", "drag", "rho", "scale")] + \
               [("gust_every", ctypes.c_int32), ("seed", ctypes.c_uint64)]


_lib = None


class NeoError(RuntimeError):
    pass


def load():
    """dlopen the HIP library (no compute).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NeoError(f"{LIB_PATH} is missing: build it with `python -m neo_planner_amd.build` "
                       "(hipcc, gfx950).  There is no CPU fallback.")
    # PyTorch-ROCm wheels bundle their own HIP runtime under the same soname as /opt/rocm's.  Whichever is loaded
    # first serves the whole process; torch does not find its GPUs on the system one ("No HIP GPUs are
    # available"), while this library runs on either.  So: torch first, if it is installed at all.
    if "torch" not in sys.modules and not os.environ.get("NEO_NO_TORCH_PRELOAD"):
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = ctypes.CDLL(LIB_PATH)
    c_p, c_i, c_d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    L.neo_abi_version.restype = c_i
    L.neo_ctx_create.argtypes = [c_i, c_p, ctypes.POINTER(c_p)]
    L.neo_ctx_destroy.argtypes = [c_p]
    L.neo_last_error.argtypes = [c_p]
    L.neo_last_error.restype = ctypes.c_char_p
    L.neo_params_default.argtypes = [ctypes.POINTER(NeoParams)]
    L.neo_params_set.argtypes = [c_p, ctypes.POINTER(NeoParams)]
    L.neo_ctx_synchronize.argtypes = [c_p]
    L.neo_ctx_set_stream.argtypes = [c_p, c_p]
    L.neo_esdf_upload_2d.argtypes = [c_p, c_i, c_p, c_p, c_p, c_i, c_i, c_d, c_d, c_d]
    L.neo_esdf_build_2d.argtypes = [c_p, c_i, c_p, c_i, c_i, c_d, c_d, c_d, c_p, c_p, c_p]
    L.neo_esdf_upload_3d.argtypes = [c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_i, c_d, c_p, c_i, c_i]
    L.neo_esdf_build_3d.argtypes = [c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_d, c_p, c_i, c_i, c_p]
    L.neo_esdf_drop.argtypes = [c_p, c_i]
    L.neo_esdf_query.argtypes = [c_p, c_i, c_i, c_p, c_p, c_p]
    L.neo_cost_grad_batch.argtypes = [c_p, c_i, c_i, c_i, c_i] + [c_p] * 8
    L.neo_cost_grad_batch_dev.argtypes = [c_p, c_i, c_i, c_i, c_i] + [c_p] * 8
    L.neo_optimize_batch.argtypes = [c_p, c_i, c_p, c_i, c_i, c_i] + [c_p] * 8
    L.neo_optimize_batch_dev.argtypes = [c_p, c_i, c_p, c_i, c_i, c_i] + [c_p] * 8
    L.neo_optimize_batch_from_dev.argtypes = [c_p, c_i, c_p, c_i, c_i, c_i] + [c_p] * 9
    L.neo_scene_slot.argtypes = [c_p, c_i]
    L.neo_optimize_workspace_bytes.argtypes = [c_i, c_i, c_i]
    L.neo_optimize_workspace_bytes.restype = ctypes.c_size_t
    L.neo_eval_traj_batch.argtypes = [c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_d, c_i, c_p, c_p]
    L.neo_audit_traj_batch.argtypes = [c_p, c_i, c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_d] + [c_p] * 4
    L.neo_audit_traj_batch_dev.argtypes = [c_p, c_i, c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_d] + [c_p] * 4
    L.neo_geo_search_batch.argtypes = [c_p, c_i, c_p, c_i, c_p, c_p, c_i, c_i] + [c_p] * 6
    L.neo_geo_search_batch_dev.argtypes = [c_p, c_i, c_p, c_i, c_p, c_p, c_i, c_i] + [c_p] * 6
    L.neo_geo_prune_batch.argtypes = [c_p, c_i, c_p, c_i, c_p, c_p, c_i, c_p]
    L.neo_geo_workspace_budget.argtypes = [c_p, ctypes.c_size_t]
    L.neo_geo_guess_dev.argtypes = [c_p, c_i, c_p, c_i, c_p, c_i, c_p, c_p, c_p, c_i, c_i] + [c_p] * 6
    L.neo_geo_mask_builds.argtypes = [c_p, ctypes.POINTER(ctypes.c_int64)]
    L.neo_fleet_target_batch.argtypes = [c_p, c_i, c_p, c_i, c_p, c_i, c_p, c_p, c_p, c_d, c_d, c_d] + [c_p] * 4
    L.neo_fleet_target_batch_dev.argtypes = [c_p, c_i, c_p, c_i, c_p, c_i, c_p, c_p, c_p, c_d, c_d, c_d] + [c_p] * 4
    L.neo_fleet_advance_dev.argtypes = [c_p, c_i, c_p, c_i, c_p, c_i, c_p, c_p, c_p, c_i, c_i, c_p, c_p]
    L.neo_fleet_splice_dev.argtypes = [c_p, c_i, c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_d, c_i, c_p, c_i] + [c_p] * 4
    L.neo_fleet_audit_batch.argtypes = [c_p, c_i, c_p, c_i, c_p, c_i, c_p, c_i, c_p, c_i, c_d] + [c_p] * 4
    L.neo_fleet_audit_batch_dev.argtypes = [c_p, c_i, c_p, c_i, c_p, c_i, c_p, c_i, c_p, c_i, c_d] + [c_p] * 4
    L.neo_batch_candidates.argtypes = [c_p, c_i, c_p, c_i, c_i, c_i, c_i] + [c_p] * 9
    L.neo_batch_candidates_dev.argtypes = [c_p, c_i, c_p, c_i, c_i, c_i, c_i] + [c_p] * 9
    L.neo_batch_select.argtypes = [c_p, c_i, c_p, c_i, c_i, c_i, c_i] + [c_p] * 20
    L.neo_batch_select_dev.argtypes = [c_p, c_i, c_p, c_i, c_i, c_i, c_i] + [c_p] * 20
    L.neo_plan_guess.argtypes = [c_p, c_i, c_p, c_i, c_i, c_i] + [c_p] * 11
    L.neo_plan_guess_dev.argtypes = [c_p, c_i, c_p, c_i, c_i, c_i] + [c_p] * 11
    L.neo_plan_merge.argtypes = [c_p, c_i, c_p, c_i, c_i, c_i, c_i] + [c_p] * 18
    L.neo_plan_merge_dev.argtypes = [c_p, c_i, c_p, c_i, c_i, c_i, c_i] + [c_p] * 18
    L.neo_plan_jitter.argtypes = [c_p, c_i, c_p, c_i, c_i, c_i, ctypes.c_uint64, c_i, c_p, c_p]
    L.neo_plan_jitter_dev.argtypes = [c_p, c_i, c_p, c_i, c_i, c_i, ctypes.c_uint64, c_i, c_p, c_p]
    L.neo_fleet_jitter.argtypes = [c_p, c_i, c_p, c_i, ctypes.c_uint64, c_i, c_i, c_p, c_p]
    L.neo_fleet_jitter_dev.argtypes = [c_p, c_i, c_p, c_i, ctypes.c_uint64, c_i, c_i, c_p, c_p]
    L.neo_fleet_warm_guess_dev.argtypes = [c_p, c_i, c_p, c_i, c_i] + [c_p] * 4
    L.neo_fleet_warm_carry_dev.argtypes = [c_p, c_i, c_p, c_i, c_i] + [c_p] * 8
    L.neo_fleet_goal_route.argtypes = [c_p, c_i, c_p, c_i, c_p, c_i, c_p, c_p, c_p, c_d, c_p]
    L.neo_fleet_goal_route_dev.argtypes = [c_p, c_i, c_p, c_i, c_p, c_i, c_p, c_p, c_p, c_d, c_p]
    L.neo_fleet_hold_dev.argtypes = [c_p, c_i, c_p, c_i, c_p, c_i, c_p, c_p, c_i, c_p]
    L.neo_fleet_track_audit.argtypes = [c_p, c_i, c_p, c_i, c_p, c_i, c_p, c_i, c_d, c_p, c_i, c_p, c_p, c_p, c_d] + [c_p] * 3
    L.neo_fleet_track_audit_dev.argtypes = [c_p, c_i, c_p, c_i, c_p, c_i, c_p, c_i, c_d, c_p, c_i, c_p, c_p, c_p, c_d] + [c_p] * 3
    L.neo_fleet_leg_close_dev.argtypes = [c_p, c_i, c_p, c_p, c_i, c_p, c_i] + [c_p] * 7
    L.neo_fleet_leg_open_dev.argtypes = [c_p, c_i, c_p, c_p, c_i, ctypes.POINTER(NeoLegSequences), c_i, c_d] + [c_p] * 16
    L.neo_fleet_leg_goal.argtypes = [c_p, ctypes.POINTER(NeoLegSequences), c_i, c_i] + [c_p] * 4
    L.neo_fleet_fly_dev.argtypes = [c_p, c_i, ctypes.POINTER(NeoFlightModel), c_p, c_i, c_p, c_i, c_p, c_p, c_p, c_i, c_i, c_i, c_i,
                                    c_d] + [c_p] * 9
    L.neo_fleet_fly_error_dev.argtypes = [c_p, c_i, c_p, c_p, c_i, c_p, c_p, c_i, c_p, c_i, c_p, c_p, c_p]
    L.neo_adaptive_count.argtypes = [c_p, c_i, c_p, c_i, c_i, c_p, c_p, c_d, c_i, c_p, c_p]
    L.neo_adaptive_count_dev.argtypes = [c_p, c_i, c_p, c_i, c_i, c_p, c_p, c_d, c_i, c_p, c_p]
    L.neo_adaptive_bucket.argtypes = [c_p, c_i, c_p, c_i] + [c_p] * 4
    L.neo_adaptive_bucket_dev.argtypes = [c_p, c_i, c_p, c_i] + [c_p] * 4
    L.neo_adaptive_merge_dev.argtypes = [c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_i, c_i] + [c_p] * 17
    L.neo_adaptive_compact.argtypes = [c_p, c_p, c_p, c_i, c_p, c_p]
    L.neo_adaptive_compact_dev.argtypes = [c_p, c_p, c_p, c_p, c_p]
    L.neo_depth_render_batch.argtypes = [c_p, c_i, c_i, c_d, c_d, c_p, c_p, c_i, c_p, c_i] + [c_p] * 4
    L.neo_depth_render_batch_dev.argtypes = [c_p, c_i, c_i, c_d, c_d, c_p, c_p, c_i, c_p, c_i] + [c_p] * 4
    L.neo_depth_box_test_counter.argtypes = [c_p, c_p]
    _onboard = [c_p, c_i, c_p, c_i, c_p, c_p, c_i, c_i, c_d, c_d, c_i, c_i, c_d, c_p, c_d, c_d, c_d, c_i, c_i, c_i, c_i, c_p, c_p, c_p]
    L.neo_onboard_integrate_batch.argtypes = list(_onboard)
    L.neo_onboard_integrate_batch_dev.argtypes = list(_onboard)
    L.neo_esdf_build_2d_batch_dev.argtypes = [c_p, c_p, c_i, c_p, c_i, c_i, c_d, c_p]
    L.neo_fleet_pose_dev.argtypes = [c_p, c_i, c_p, c_i, c_p, c_i, c_p, c_p, c_p, c_p, c_d, c_p]
    L.neo_record_state_dev.argtypes = [c_p, c_i, c_p, c_i, c_p, c_i, c_p, c_p, c_p, c_p]
    L.neo_record_commit_dev.argtypes = [c_p, c_i, c_p, c_i, c_i] + [c_p] * 7 + [c_i, c_i, c_p, c_i, c_i, c_i] + [c_p] * 9
    L.neo_init_motion_dev.argtypes = [c_p, c_i, c_p, c_i] + [c_p] * 5
    L.neo_init_head_dev.argtypes = [c_p, c_i, c_p, c_i, c_p, ctypes.c_size_t, c_p, c_i, c_p, c_p]
    L.neo_init_guess_dev.argtypes = [c_p, c_i, c_p, c_i] + [c_p] * 3
    L.neo_backbone_workspace_bytes.argtypes = [c_i, c_i, c_i]
    L.neo_backbone_workspace_bytes.restype = ctypes.c_size_t
    L.neo_backbone_features_dev.argtypes = [c_p, c_p, ctypes.c_size_t, c_p, c_i, c_i, c_i, c_p, ctypes.c_size_t, c_p]
    L.neo_backbone_launch_times.argtypes = L.neo_backbone_features_dev.argtypes + [c_p]
    L.neo_backbone_activation_dev.argtypes = L.neo_backbone_features_dev.argtypes[:-1] + [c_i, c_p, ctypes.c_size_t]
    L.neo_backbone_activation_shape.argtypes = [c_i, c_i, c_i] + [ctypes.POINTER(ctypes.c_int)] * 3
    L.neo_backbone_pack_bf16_dev.argtypes = [c_p, c_p, ctypes.c_size_t, c_p, ctypes.c_size_t]
    L.neo_backbone_bf16_workspace_bytes.argtypes = [c_i, c_i, c_i]
    L.neo_backbone_bf16_workspace_bytes.restype = ctypes.c_size_t
    L.neo_backbone_features_bf16_dev.argtypes = list(L.neo_backbone_features_dev.argtypes)
    L.neo_backbone_bf16_launch_times.argtypes = L.neo_backbone_features_bf16_dev.argtypes + [c_p]
    L.neo_backbone_bf16_activation_dev.argtypes = L.neo_backbone_features_bf16_dev.argtypes[:-1] + [c_i, c_p, c_p, ctypes.c_size_t]
    L.neo_profile_enable.argtypes = [c_p, c_i]
    L.neo_profile_read.argtypes = [c_p, c_i, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(c_d)]
    L.neo_profile_reset.argtypes = [c_p]
    L.neo_optimize_plan_launches.argtypes = [c_p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    L.neo_optimize_sample_counter.argtypes = [c_p, c_p]
    L.neo_optimize_trace.argtypes = [c_p, c_p, c_i]
    L.neo_optimize_trace_xg.argtypes = [c_p, c_p, c_i]
    L.neo_optimize_dispatch_order.argtypes = [c_p, c_p, c_i]
    L.neo_optimize_dispatch_order_host.argtypes = [c_p, c_p, c_i]
    L.neo_sampled_terms_dispatch_order.argtypes = [c_p, c_p, c_i, c_i]
    L.neo_esdf_build_config.argtypes = [c_p, c_i]
    L.neo_pack_results_dev.argtypes = [c_p, c_i, c_i, c_p, c_p, c_p, c_p]
    L.neo_optimize_state_bytes.argtypes = [c_i, c_i]
    L.neo_optimize_state_bytes.restype = ctypes.c_size_t
    L.neo_optimize_batch_budget_dev.argtypes = [c_p, c_i, c_i, c_i, c_i] + [c_p] * 10 + [c_i, c_p, c_i, c_i]
    L.neo_sampled_terms_batch.argtypes = [c_p, c_i, c_i, c_i, c_i] + [c_p] * 5
    L.neo_sampled_terms_batch_dev.argtypes = [c_p, c_i, c_i, c_i, c_i] + [c_p] * 5
    L.neo_sampled_terms_batch_f32.argtypes = [c_p, c_i, c_i, c_i, c_i] + [c_p] * 5
    L.neo_sampled_terms_batch_f32_dev.argtypes = [c_p, c_i, c_i, c_i, c_i] + [c_p] * 5
    L.neo_effort_order_dev.argtypes = [c_p, c_i, c_i, c_i] + [c_p] * 5
    L.neo_optimize_progress_counter.argtypes = [c_p, c_p]
    L.neo_effort_order_scratch_bytes.argtypes = [c_i]
    L.neo_effort_order_scratch_bytes.restype = ctypes.c_size_t
    for name in EXPORTS:
        fn = getattr(L, name)
        if fn.restype is ctypes.c_int or name in ("neo_abi_version",):
            fn.restype = c_i
    _lib = L
    return L


def ptr(a):
    """host pointer of a C-contiguous NumPy array (None -> NULL)"""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.c_void_p)


def as_f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def dev_ptr(t, first=0):
    """device pointer of a torch tensor, from its element `first` on (None -> NULL)"""
    return ctypes.c_void_p(t.data_ptr() + first * t.element_size()) if t is not None else None


def launch_count(subset, B):
    """positions a launch covers: the subset's entries, or all B requests without one"""
    return B if subset is None else int(subset.numel())


class Context:
    """one neo_ctx: a device, a HIP stream, the uploaded maps"""

    def __init__(self, device=0, stream=None):
        self.lib = load()
        h = ctypes.c_void_p()
        self.device = int(device)
        rc = self.lib.neo_ctx_create(int(device), ctypes.c_void_p(stream) if stream else None, ctypes.byref(h))
        if rc != NEO_OK:
            raise NeoError(f"neo_ctx_create(device={device}) failed with {rc}: no usable MI355X? "
                           "(the product path has no CPU fallback)")
        self.h = h
        self.params = NeoParams()
        self.lib.neo_params_default(ctypes.byref(self.params))
        self._next_scene = 0

    def check(self, rc):
        if rc != NEO_OK:
            raise NeoError(f"libneo_planner_hip error {rc}: {self.lib.neo_last_error(self.h).decode()}")

    def call(self, name, *args):
        """the status-returning entry point `name` on this context; raises on its error code.  `lib` is looked up at
        call time: a recording proxy stands in by replacing it"""
        self.check(getattr(self.lib, name)(self.h, *args))

    def backbone_workspace_bytes(self, n, H, W):
        """neo_backbone_workspace_bytes: what neo_backbone_features_dev needs for n images of H x W"""
        return int(self.lib.neo_backbone_workspace_bytes(int(n), int(H), int(W)))

    def backbone_bf16_workspace_bytes(self, n, H, W):
        """neo_backbone_bf16_workspace_bytes: what neo_backbone_features_bf16_dev needs for n images of H x W"""
        return int(self.lib.neo_backbone_bf16_workspace_bytes(int(n), int(H), int(W)))

    def set_params(self, **kw):
        for k, v in kw.items():
            if k == "weights":
                for i in range(4):
                    self.params.weights[i] = float(v[i])
            else:
                setattr(self.params, k, v)
        self.check(self.lib.neo_params_set(self.h, ctypes.byref(self.params)))

    def new_scene_id(self):
        self._next_scene += 1
        return self._next_scene

    def synchronize(self):
        self.check(self.lib.neo_ctx_synchronize(self.h))

    def set_stream(self, stream=None):
        """HIP stream handle for the calls that follow (None: the stream the context was created with)"""
        self.check(self.lib.neo_ctx_set_stream(self.h, ctypes.c_void_p(stream) if stream else None))

    def close(self):
        if self.h:
            self.lib.neo_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = {}


def default_context(device=0):
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]
