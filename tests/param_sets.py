"""
Planner parameter sets away from the ROS YAML defaults, shared by tests/test_params_cpu.py, tests/test_gpu_params.py and
the non-default rows of the GPU tests (a plain helper module).

  A: 1 / delta_t is inexact in fp32 and fp64, T_min is no multiple of delta_t, every fp32 copy in DevParams is rounded;
  B: delta_t = 0.013 -- up to floor(3.1 / 0.013) = 238 samples per piece (the defaults never pass 50);
  C: T_min an exact multiple of delta_t, a zero weight (feasibility), at most 47 samples per piece;
     T_max = 11.9 keeps T_max / delta_t off an integer.

The optimiser options (ftol, gtol, maxls, maxiter, maxfun) are extra attributes that planner._push_params and
oracle/cpu_native.make_params read with getattr; OPTION_SETS are the non-default ones the tests use.
"""
import numpy as np

SETS = {
    "A": dict(v_max=2.5, T_min=0.33, T_max=7.3, safe_dis=1.1, delta_t=0.07, weights=[0.5, 3.0, 7.0, 2500.0],
              collision_cost_tol=40.0),
    "B": dict(v_max=0.6, T_min=0.21, T_max=3.1, safe_dis=0.45, delta_t=0.013, weights=[2.0, 0.25, 40.0, 300.0],
              collision_cost_tol=0.5),
    "C": dict(v_max=1.7, T_min=1.0, T_max=11.9, safe_dis=0.9, delta_t=0.25, weights=[1.0, 2.0, 0.0, 500.0],
              collision_cost_tol=5.0),
}

OPTION_SETS = [dict(maxiter=1), dict(maxiter=3), dict(maxfun=1), dict(maxfun=6), dict(maxiter=4, maxfun=5),
               dict(maxls=2), dict(ftol=1e-2, gtol=1e-1)]


def _with(obj, opts):
    for k, v in opts.items():
        assert k in ("ftol", "gtol", "maxls", "maxiter", "maxfun"), k
        setattr(obj, k, v)
    return obj


def oracle_params(name=None, **opts):
    """oracle.minco_np.PlannerParams of set `name` (None: the defaults) plus optimiser options"""
    from oracle import minco_np as onp
    return _with(onp.PlannerParams(**(SETS[name] if name else {})), opts)


def planner_config(name=None, **opts):
    """neo_planner_amd.PlannerConfig of set `name` (None: the defaults) plus optimiser options"""
    import neo_planner_amd as npa
    return _with(npa.PlannerConfig(**(SETS[name] if name else {})), opts)


def durations(rng, name, shape, lo=0.05, hi=0.6):
    """piece durations T_min + [lo, hi] * (T_max - T_min) of the set"""
    s = SETS[name]
    return s["T_min"] + rng.uniform(lo, hi, shape) * (s["T_max"] - s["T_min"])


def sample_count(ts, name):
    """floor(T / delta_t) summed over the pieces: the reference's int(T / delta_t) per piece (expert_planner.py:398)"""
    return np.floor(np.asarray(ts) / SETS[name]["delta_t"]).sum(axis=-1)


def random_requests(rng, B, M, D, lo, hi):
    """tests/test_gpu_parity._random_requests without its durations (they come from `durations`): start and goal at
    opposite ends of the box [lo, hi], every boundary row non-zero, jittered waypoints on the straight line"""
    head = np.zeros((B, 3, D)); tail = np.zeros((B, 3, D))
    head[:, 0] = rng.uniform(lo, lo + 0.2 * (hi - lo), (B, D))
    tail[:, 0] = rng.uniform(lo + 0.7 * (hi - lo), hi, (B, D))
    head[:, 1] = rng.normal(0, 0.4, (B, D)); head[:, 2] = rng.normal(0, 0.3, (B, D))
    tail[:, 1] = rng.normal(0, 0.4, (B, D)); tail[:, 2] = rng.normal(0, 0.3, (B, D))
    k = np.arange(1, M)[None, None, :] / M
    wp = head[:, 0, :, None] + (tail[:, 0] - head[:, 0])[:, :, None] * k + rng.normal(0, 0.5, (B, D, M - 1))
    return head, tail, wp


def field32(shift=0):
    """the 32^3 field of tests/test_gpu_trace_parity._field: a floor ramp and one box"""
    n = 32
    dist = np.full((n, n, n), 4.0, np.float32)
    dist[:, :, :6] = np.linspace(0.0, 1.2, 6)[None, None, :]
    dist[10:14, 12 + shift:18 + shift, :] = 0.05
    return dist


RES3, ORIGIN3 = 0.4, (0.0, -6.4, 0.0)
BOX3 = (np.array([1.0, -5.0, 1.0]), np.array([11.5, 5.0, 10.0]))
BOX2 = (np.array([1.0, -10.0, 0.5]), np.array([26.0, 10.0, 3.0]))


# duration fractions [lo, hi] of (T_max - T_min) per set for the per-evaluation cases: A and C are shortened so that the
# sampled terms are at work (at 0.6 of their long T_max every speed is far below v_max and the feasibility term vanishes)
DUR = {"A": (0.01, 0.1), "B": (0.05, 0.6), "C": (0.02, 0.25)}
# ... and for the start points of whole runs: the share of the range that the default rows' 0.8 .. 2.5 s take of theirs
RUN_DUR = {"A": (0.05, 0.3), "B": (0.2, 0.8), "C": (0.02, 0.25)}


def case_inputs(name, kind, M, D, B=6, seed=0):
    """(head, tail, wp, ts) of one per-evaluation case at set `name` on map `kind` ("2d" / "3d")"""
    import zlib
    rng = np.random.default_rng(zlib.crc32(f"{name}-{kind}-{M}-{D}-{seed}".encode()))
    lo, hi = BOX2 if kind == "2d" else BOX3
    head, tail, wp = random_requests(rng, B, M, D, lo[:D], hi[:D])
    return head, tail, wp, durations(rng, name, (B, M), *DUR[name])


def pack_x(name, wp, ts):
    """BatchPlanner.pack_x at the set's T_min / T_max"""
    s = SETS[name]
    tau = -np.log((s["T_max"] - s["T_min"]) / (ts - s["T_min"]) - 1.0)
    return np.concatenate([np.asarray(wp, dtype=np.float64).reshape(ts.shape[0], -1), tau], axis=1)


def small_requests(name, kind, M, D, B, seed=4):
    """the gentle small problems of tests/test_gpu_api_edges.test_lane_group_kernel_small_problems -- synth.replan_requests
    over 4 .. 6 m, through the box of the 32^3 field when D = 3 -- with start durations from the set"""
    from neo_planner_amd import synth
    import zlib
    kw = dict(z_range=(3.0, 7.0), pitch=0.25) if D == 3 else {}
    head, tail, wp, _ = synth.replan_requests(seed, B, M - 1, D=D, length_range=(4.0, 6.0), **kw)
    rng = np.random.default_rng(zlib.crc32(f"small-{name}-{kind}-{M}-{seed}".encode()))
    return head, tail, wp, durations(rng, name, (B, M), *RUN_DUR[name])
