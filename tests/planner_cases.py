"""What tools/gen_golden_planner.py, test_gpu_planner_golden.py and test_planner_cpu.py share: short calls that between
them go through every public method of BatchPlanner and MinJerkPlanner and every branch of the retry chains, and what is
kept of each -- a SHA-256 over everything the call returned, the run-length-encoded sequence of library entry points it
made, and the number of context synchronisations (the fleet flights' method, tests/fleet_flight_cases.py, whose recorder
and encoder are used here).

The requests are the fleet flights': three synth 2-D scenes, six start / goal pairs repeated to B = 12, goals 3 and 5 inside
obstacles (every attempt on them fails: retries, the batch mode's fallback, unsolved requests); init_wpts_num = 2 (M = 3).
One 32^3 field carries the D = 3, M = 4 case, and B = 1025 the launches that are dispatched longest-expected first.

REFUSALS is the CPU side: argument sets BatchPlanner refuses before it touches the device, by the first error's type and
message."""
import hashlib

import numpy as np

import fleet_flight_cases as fc

B = 12
BIG = 1025          # above 1024 rows a launch is dispatched in expected-effort order
SEED = 97


# ------------------------------------------------------------------------------------------------ the requests
def requests(fs, n=B, spread=0.0):
    """head / tail (n, 3, 2) and scene ids: the six missions repeated; `spread` > 0 moves every start by its own N(0, spread)"""
    k = np.arange(n) % fc.B
    head, tail = np.zeros((n, 3, 2)), np.zeros((n, 3, 2))
    head[:, 0], tail[:, 0] = fs["start"][k], fs["goals"][k]
    if spread > 0.0:
        head[:, 0] += np.random.default_rng(n).normal(0.0, spread, (n, 2))
    return head, tail, fs["sids"][k].copy()


def setup():
    import torch
    import neo_planner_amd as npa
    import param_sets as ps
    fs = fc.setup()
    fs["head"], fs["tail"], fs["ids"] = requests(fs)
    fs["map"] = fs["maps"][0]
    fs["dev"] = torch.device("cuda", 0)
    fs["field"] = npa.ESDF3D(ps.field32(0), ps.RES3, ps.ORIGIN3, store="f32", layout="brick")
    rng = np.random.default_rng(3)
    lo, hi = ps.BOX3
    h3, t3 = np.zeros((6, 3, 3)), np.zeros((6, 3, 3))
    h3[:, 0], t3[:, 0] = rng.uniform(lo, hi, (6, 3)), rng.uniform(lo, hi, (6, 3))
    fs["head3"], fs["tail3"] = h3, t3
    return fs


def drop(fs):
    from neo_planner_amd import _lib
    fc.drop(fs)
    c = _lib.default_context()
    c.check(c.lib.neo_esdf_drop(c.h, fs["field"].scene_id))


def _bp(**kw):
    import neo_planner_amd as npa
    return npa.BatchPlanner(**kw)


def _up(fs, *arrays):
    """the arrays as device tensors, in place before the context's stream starts"""
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(a)).to(fs["dev"]) for a in arrays]
    torch.cuda.synchronize(fs["dev"])
    return out


def _slots(fs, bp, ids):
    c = bp.ctx
    return np.array([c.lib.neo_scene_slot(c.h, int(s)) for s in ids], dtype=np.int32)


def _x0(bp, head, tail, count=2):
    return bp.pack_x(*bp.init_guess(head, tail, count))


def _result_tensors(fs, n):
    import torch
    f = lambda *s: torch.zeros(s, dtype=torch.float64, device=fs["dev"])
    i = lambda *s: torch.zeros(s, dtype=torch.int32, device=fs["dev"])
    return dict(costs=f(n, 4), costs_last=f(n, 4), nit=i(n), nfev=i(n), status=i(n))


# ------------------------------------------------------------------------------------------------ the cases
def cost_grad(fs):
    bp = _bp()
    return bp.cost_grad(fs["map"], _x0(bp, fs["head"], fs["tail"]), fs["head"], fs["tail"], want_coeffs=True)


def _sampled(fs, bp, **kw):
    _, ts = bp.init_guess(fs["head"], fs["tail"], 2)
    coeffs = bp.cost_grad(fs["map"], _x0(bp, fs["head"], fs["tail"]), fs["head"], fs["tail"], want_coeffs=True)["coeffs"]
    return bp.sampled_terms(fs["map"], coeffs, ts, **kw)


def sampled_terms(fs):
    return _sampled(fs, _bp())


def sampled_terms_order(fs):
    bp = _bp()
    return _sampled(fs, bp, order=bp.spatial_order(fs["head"], fs["tail"]))


def sampled_terms_io32(fs):
    return _sampled(fs, _bp(sample_dtype="f32"), io32=True)


def optimize(fs):
    bp = _bp()
    return bp.optimize(fs["map"], _x0(bp, fs["head"], fs["tail"]), fs["head"], fs["tail"])


def optimize_scene_ids(fs):
    bp = _bp()
    return bp.optimize(fs["map"], _x0(bp, fs["head"], fs["tail"]), fs["head"], fs["tail"], scene_ids=fs["ids"])


def optimize_big(fs):
    bp = _bp()
    head, tail, ids = requests(fs, BIG, spread=0.05)
    return bp.optimize(fs["map"], _x0(bp, head, tail), head, tail, scene_ids=ids)


def audit(fs):
    bp = _bp()
    x = bp.optimize(fs["map"], _x0(bp, fs["head"], fs["tail"]), fs["head"], fs["tail"], scene_ids=fs["ids"])["x"]
    return bp.audit(fs["map"], x, fs["head"], fs["tail"], scene_ids=fs["ids"])


def audit_dev(fs):
    import torch
    bp = _bp()
    bp.cost_grad(fs["map"], _x0(bp, fs["head"], fs["tail"]), fs["head"], fs["tail"])      # (optimize_dev pushes no parameters)
    res = _result_tensors(fs, B)
    rec = dict(audit=torch.zeros((B, 10), dtype=torch.float64, device=fs["dev"]),
               count=torch.zeros(B, dtype=torch.int32, device=fs["dev"]), flags=torch.zeros(B, dtype=torch.int32, device=fs["dev"]))
    x, head, tail, slots = _up(fs, _x0(bp, fs["head"], fs["tail"]), fs["head"], fs["tail"], _slots(fs, bp, fs["ids"]))
    bp.optimize_dev(fs["map"], x, head, tail, res["costs"], res["costs_last"], res["nit"], res["nfev"], res["status"], slots=slots)
    bp.audit_dev(fs["map"], x, head, tail, rec["audit"], rec["count"], rec["flags"], slots=slots, weights=(1.0, 2.0, 50.0))
    bp.ctx.synchronize()
    return dict(res, x=x, **rec)


def geo_init(fs):
    return _bp().geo_init(fs["map"], fs["head"][:, 0], fs["tail"][:, 0], scene_ids=fs["ids"], path_cap=512)


def geo_init_dev(fs):
    import torch
    bp = _bp()
    f = lambda *s: torch.zeros(s, dtype=torch.float64, device=fs["dev"])
    i = lambda: torch.zeros(B, dtype=torch.int32, device=fs["dev"])
    out = dict(key_pts=f(B, 4, 2), path_len=i(), path_cost=f(B), expansions=i(), flags=i(), paths=f(B, 512, 2))
    start, target, slots = _up(fs, fs["head"][:, 0], fs["tail"][:, 0], _slots(fs, bp, fs["ids"]))
    bp.geo_init_dev(fs["map"], start, target, out["key_pts"], out["path_len"], out["path_cost"], out["expansions"], out["flags"],
                    slots=slots, paths=out["paths"])
    bp.ctx.synchronize()
    return out


def geo_prune(fs):
    bp = _bp()
    g = bp.geo_init(fs["map"], fs["head"][:, 0], fs["tail"][:, 0], scene_ids=fs["ids"], path_cap=512)
    ok = np.flatnonzero((g["flags"] == 0) & (g["path_len"] >= 2))
    assert ok.size >= 6
    key_pts = bp.geo_prune(fs["map"], np.nan_to_num(g["paths"][ok]), g["path_len"][ok], scene_ids=fs["ids"][ok])
    return dict(rows=ok, key_pts=key_pts)


def geo_plan(fs):
    return _bp().geo_plan(fs["map"], fs["head"], fs["tail"], scene_ids=fs["ids"], seed=SEED)


def optimize_budgeted(fs):
    """(budgeted launches take 3-D fields only)"""
    bp = _bp()
    return bp.optimize_budgeted(fs["field"], _x0(bp, fs["head3"], fs["tail3"], 3), fs["head3"], fs["tail3"], eval_budget=4)


def optimize_progressive(fs):
    """the union of the yields by request: the partition depends on timing and is not kept"""
    bp = _bp()
    out, seen = {}, np.zeros(B, bool)
    for idx, res in bp.optimize_progressive(fs["map"], _x0(bp, fs["head"], fs["tail"]), fs["head"], fs["tail"], shares=(0.5,)):
        assert not seen[idx].any()
        seen[idx] = True
        for k, v in res.items():
            out.setdefault(k, np.zeros((B,) + v.shape[1:], dtype=v.dtype))[idx] = v
    assert seen.all()
    return out


def _plan(fs, **kw):
    kw.setdefault("seed", SEED)
    return _bp().plan(fs["map"], fs["head"], fs["tail"], return_launch_sizes=True, **kw)


def plan_numpy(fs):
    return _plan(fs)


def plan_counter(fs):
    return _plan(fs, jitter="counter")


def plan_stream_ids(fs):
    return _plan(fs, stream_ids=100 + 7 * np.arange(B))


def plan_scene_ids(fs):
    return _plan(fs, scene_ids=fs["ids"])


def plan_rng(fs):
    return _plan(fs, seed=None, rng=np.random.default_rng(SEED))


def plan_three_waypoints(fs):
    return _plan(fs, waypoints=3)


def plan_adaptive(fs):
    return _plan(fs, waypoints="adaptive", max_waypoints=6, scene_ids=fs["ids"])


def plan_3d(fs):
    return _bp().plan(fs["field"], fs["head3"], fs["tail3"], waypoints=3, seed=SEED, return_launch_sizes=True)


def _plan_dev(fs, n=B, spread=0.0, warm=False, own=False, device_ids=False, bufs=None, **kw):
    import torch
    bp = _bp()
    head, tail, ids = requests(fs, n, spread)
    d_head, d_tail, slots = _up(fs, head, tail, _slots(fs, bp, ids))
    kw.setdefault("seed", SEED)
    if warm:        # a first guess by request: the straight line bent to one side
        wp, ts = bp.init_guess(head, tail, 2)
        kw["x0"] = _up(fs, bp.pack_x(wp + 0.3, ts))[0]
    if device_ids:
        kw["stream_ids"] = _up(fs, (100 + 7 * np.arange(n)).astype(np.int32))[0]
    extra = {}
    if own:         # the caller's own x / solved (the fleet's)
        extra = dict(own_x=torch.full((n, 7), -1.0, dtype=torch.float64, device=fs["dev"]),
                     own_solved=torch.full((n,), -1, dtype=torch.int32, device=fs["dev"]))
        torch.cuda.synchronize(fs["dev"])
        kw.update(x=extra["own_x"], solved=extra["own_solved"])
    out = bp.plan_dev(fs["map"], d_head, d_tail, bufs=bufs, slots=slots, **kw)
    return dict(out, **extra)


def plan_dev_fixed(fs):
    return _plan_dev(fs)


def plan_dev_x0(fs):
    return _plan_dev(fs, warm=True)


def plan_dev_subset(fs):
    return _plan_dev(fs, subset=_up(fs, np.array([1, 3, 4, 5, 8, 9, 11], np.int32))[0])


def plan_dev_own_arrays(fs):
    return _plan_dev(fs, own=True, subset=_up(fs, np.array([0, 2, 3, 5, 10], np.int32))[0])


def plan_dev_counter_device_ids(fs):
    return _plan_dev(fs, jitter="counter", device_ids=True)


def plan_dev_counter_host_ids(fs):
    return _plan_dev(fs, jitter="counter", stream_ids=100 + 7 * np.arange(B))


def plan_dev_adaptive(fs):
    return _plan_dev(fs, waypoints="adaptive", max_waypoints=6)


def plan_dev_adaptive_counter_subset(fs):
    return _plan_dev(fs, waypoints="adaptive", max_waypoints=6, jitter="counter",
                     subset=_up(fs, np.array([0, 1, 3, 4, 5, 7, 9], np.int32))[0])


def plan_dev_big(fs):
    return _plan_dev(fs, n=BIG, spread=0.05)


def plan_dev_guessed(fs):
    """attempt 0 from the packed rows as they lie (the fleet's batch fallback fills them itself): here a one-attempt
    plan_dev leaves its answers there"""
    import torch
    bp = _bp()
    bufs = bp.plan_buffers(B, fs["dev"])
    torch.cuda.synchronize(fs["dev"])
    _plan_dev(fs, bufs=bufs, max_attempts=1)
    first = bufs["x"].clone()
    return dict(_plan_dev(fs, bufs=bufs, _guessed=True), first_x=first)


def warm_start(fs):
    """the fleet's `warmstart` round trip: a plan, what the requests carry of it, the next plan from that, the carry again"""
    import torch
    bp = _bp()
    d_head, d_tail, slots = _up(fs, fs["head"], fs["tail"], _slots(fs, bp, fs["ids"]))
    f = lambda *s: torch.zeros(s, dtype=torch.float64, device=fs["dev"])
    wpts_local, ts_carry, x0 = f(B, 2, 2), f(B, 3), f(B, 7)
    bufs = bp.plan_buffers(B, fs["dev"])
    sub = _up(fs, np.array([0, 1, 2, 3, 4, 6, 7, 8, 10], np.int32))[0]
    bp.plan_dev(fs["map"], d_head, d_tail, bufs=bufs, slots=slots, seed=SEED)
    bp.warm_carry_dev(bufs["x"], d_head, bufs["solved"], bufs["status"], bufs["attempts"], wpts_local, ts_carry)
    bp.ctx.synchronize()
    first = dict(first_x=bufs["x"].clone(), first_wpts_local=wpts_local.clone(), first_ts_carry=ts_carry.clone())
    moved = d_head.clone()
    moved[:, 0] += 0.25
    torch.cuda.synchronize(fs["dev"])
    got = bp.warm_guess_dev(moved, wpts_local, ts_carry, x0, subset=sub)
    bp.plan_dev(fs["map"], moved, d_tail, bufs=bufs, x0=got, slots=slots, subset=sub, seed=SEED + 1)
    bp.warm_carry_dev(bufs["x"], moved, bufs["solved"], bufs["status"], bufs["attempts"], wpts_local, ts_carry, subset=sub)
    bp.ctx.synchronize()
    return dict(bufs, x0=x0, wpts_local=wpts_local, ts_carry=ts_carry, **first)


def batch_plan_dev_subset(fs):
    bp = _bp()
    d_head, d_tail, slots, sub = _up(fs, fs["head"], fs["tail"], _slots(fs, bp, fs["ids"]), np.array([0, 3, 4, 5, 7, 11], np.int32))
    bufs = bp.batch_plan_dev(fs["map"], d_head, d_tail, slots=slots, subset=sub)
    return dict(bufs, fallback_list=np.sort(bp.batch_fallback(bufs)))


def batch_plan(fs):
    return _bp().batch_plan(fs["map"], fs["head"], fs["tail"], scene_ids=fs["ids"], seed=SEED)


def batch_plan_offsets(fs):
    return _bp().batch_plan(fs["map"], fs["head"], fs["tail"], lateral_offsets=(0.0, 0.4, -0.4, 0.9), seed=SEED,
                            stream_ids=100 + 7 * np.arange(B))


def expected_effort_order_dev(fs):
    bp = _bp()
    head, tail, _ = requests(fs, 40, spread=0.5)
    order, keys = bp.expected_effort_order_dev(*_up(fs, _x0(bp, head, tail), head, tail))
    bp.ctx.synchronize()
    return dict(order=order, keys=keys, host_order=bp.expected_effort_order(head, tail, bp.init_guess(head, tail, 2)[1]))


def min_jerk(fs):
    """MinJerkPlanner on request 0: plan, batch_plan, the callbacks, the commands, the audit"""
    import neo_planner_amd as npa
    head, tail = fs["head"][0], fs["tail"][0]
    out = {}
    keep = lambda tag, p: out.update({tag + "_int_wpts": np.array(p.int_wpts), tag + "_ts": np.array(p.ts), tag + "_costs": p.costs,
                                      tag + "_final_cost": p.final_cost, tag + "_iter_num": p.iter_num,
                                      tag + "_runs": p.opt_running_times})
    p = npa.MinJerkPlanner()
    p.plan(fs["map"], head, tail)
    keep("plan", p)
    x = np.concatenate((np.reshape(p.int_wpts, -1), p.tau))
    out.update(cost=p.get_cost(x), cost_terms=p.costs.copy(), grad=p.get_grad(x), coeffs=np.array(p.coeffs),
               cmd=p.get_full_state_cmd(30))
    for k, v in p.audit().items():
        out["audit_" + k] = v
    q = npa.MinJerkPlanner()
    q.batch_plan(fs["map"], head, tail)
    keep("batch", q)
    return out


def min_jerk_no_solution(fs):
    """request 3, whose goal lies inside an obstacle: the reference's exception after five seeds"""
    import neo_planner_amd as npa
    np.random.seed(5)
    p = npa.MinJerkPlanner()
    try:
        p.plan(fs["map"], fs["head"][3], fs["tail"][3])
    except Exception as ex:
        return dict(error="%s: %s" % (type(ex).__name__, ex), iter_num=p.iter_num, runs=p.opt_running_times,
                    int_wpts=np.array(p.int_wpts), ts=np.array(p.ts))
    raise AssertionError("request 3 was planned")


CASES = {f.__name__: f for f in (
    cost_grad, sampled_terms, sampled_terms_order, sampled_terms_io32, optimize, optimize_scene_ids, optimize_big, audit,
    audit_dev, geo_init, geo_init_dev, geo_prune, geo_plan, optimize_budgeted, optimize_progressive, plan_numpy, plan_counter,
    plan_stream_ids, plan_scene_ids, plan_rng, plan_three_waypoints, plan_adaptive, plan_3d, plan_dev_fixed, plan_dev_x0,
    plan_dev_subset, plan_dev_own_arrays, plan_dev_counter_device_ids, plan_dev_counter_host_ids, plan_dev_adaptive,
    plan_dev_adaptive_counter_subset, plan_dev_big, plan_dev_guessed, warm_start, batch_plan_dev_subset, batch_plan,
    batch_plan_offsets, expected_effort_order_dev, min_jerk, min_jerk_no_solution)}

# what a case must have gone through for the fixture to be worth keeping (the generator refuses a recording that misses one)
_retried = lambda o: int(np.max(_host(o["attempts"]))) >= 2 and not np.all(_host(o["solved"]))
_two_counts = lambda o: len(set(_host(o["counts"])[_host(o["attempts"]) > 0].tolist())) >= 2
BRANCHES = {
    **{k: _retried for k in CASES if k.startswith(("plan_", "warm_start", "geo_plan")) and k != "plan_3d"},
    "plan_adaptive": lambda o: _retried(o) and _two_counts(o),
    "plan_dev_adaptive": lambda o: _retried(o) and _two_counts(o),
    "plan_dev_adaptive_counter_subset": lambda o: _retried(o) and _two_counts(o),
    "plan_dev_big": lambda o: _retried(o) and o["launch_sizes"][0] == BIG and o["launch_sizes"][1] > 0,
    "batch_plan": lambda o: bool(np.any(o["chosen"] < 0)) and bool(np.any(o["chosen"] >= 0)),
    "batch_plan_offsets": lambda o: bool(np.any(o["chosen"] < 0)),
    "batch_plan_dev_subset": lambda o: o["fallback_list"].size >= 1,
    "optimize_budgeted": lambda o: len(o["launch_sizes"]) >= 3,
    "geo_init": lambda o: bool(o["no_path"].any()) and not bool(o["no_path"].all()),
}


# ------------------------------------------------------------------------------------------------ what is kept of a case
def _host(v):
    return v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)


# the scratch of plan_buffers / batch_buffers: packed rows of the last launch, lists and sort space -- map-table slots depend
# on what else the process has uploaded, and what lies behind a list's end is whatever the launch before left there
SCRATCH = ("x_k", "head_k", "tail_k", "slots_k", "noise", "costs_k", "last_k", "nit_k", "nfev_k", "status_k", "todo", "order",
           "order_scratch", "group_order", "table", "fallback", "n_fallback")


def flatten(out, prefix=""):
    """the result as {dotted key: array}: nested dicts by key, tensors copied down, lists and numbers as arrays; None
    (an output that was not asked for) and the buffers' SCRATCH are left out"""
    flat = {}
    for k, v in out.items():
        key = prefix + str(k)
        if k in SCRATCH and hasattr(v, "detach"):
            continue
        if isinstance(v, dict):
            flat.update(flatten(v, key + "."))
        elif isinstance(v, str):
            flat[key] = np.frombuffer(v.encode(), dtype=np.uint8)
        elif v is not None:
            flat[key] = _host(v)
    return flat


def digest(out):
    """SHA-256 over every returned array in sorted key order: key, dtype, shape, bytes"""
    h = hashlib.sha256()
    flat = flatten(out)
    for k in sorted(flat):
        h.update(k.encode() + b"=")
        fc._feed(h, flat[k])
    return h.hexdigest()


def run(fs, name):
    """one case with the recording proxy in place of ctx.lib: (what the fixture keeps of it, the result itself)"""
    from neo_planner_amd import _lib
    ctx = _lib.default_context()
    lib, proxy = ctx.lib, fc.RecordingLib(ctx.lib)
    ctx.lib = proxy
    try:
        out = CASES[name](fs)
    finally:
        ctx.lib = lib
    got = dict(digest=digest(out), calls=fc.run_length(proxy.names), synchronizes=proxy.syncs)
    if "error" in out:
        got["error"] = out["error"]
    for k in ("launch_sizes", "group_launch_sizes"):
        if k in out:
            got[k] = {str(c): v for c, v in out[k].items()} if isinstance(out[k], dict) else list(out[k])
    return got, out


# ------------------------------------------------------------------------------------------------ the CPU side
def signatures():
    """str(inspect.signature) of every public method of the two planners and of PlannerConfig"""
    import inspect
    from neo_planner_amd import planner
    table = {}
    for cls in (planner.PlannerConfig, planner.MinJerkPlanner, planner.BatchPlanner):
        table[cls.__name__ + ".__init__"] = str(inspect.signature(cls.__init__))
        for name, member in sorted(vars(cls).items()):
            fn = member.__func__ if isinstance(member, (staticmethod, classmethod)) else member
            if not name.startswith("_") and inspect.isfunction(fn):
                table["%s.%s" % (cls.__name__, name)] = str(inspect.signature(fn))
    return table


class _Tensor:
    """as much of a device tensor as the argument checks look at"""

    def __init__(self, *shape):
        self.shape, self.ndim = tuple(shape), len(shape)


def _cpu_tensor(*shape):
    import torch
    return torch.zeros(shape, dtype=torch.int32)


def _refusals():
    """name -> (method, args, kwargs, planner keywords): calls that are refused before any device use"""
    H = np.zeros((4, 3, 2))
    H[:, 0, 0] = [0.0, 1.0, 2.0, 3.0]
    T = H + 5.0
    H3, T3 = np.zeros((2, 3, 3)), np.ones((2, 3, 3))
    h, t = _Tensor(4, 3, 2), _Tensor(4, 3, 2)
    no_seg = dict(config=dict(init_seg_len=0.0))
    bufs = dict(B=2, D=2, M=3)
    r = {
        "plan.one_of_int_wpts_ts": ("plan", (None, H, T), dict(int_wpts=np.zeros((4, 2, 2))), {}),
        "plan.jitter": ("plan", (None, H, T), dict(jitter="device"), {}),
        "plan.counter_seed": ("plan", (None, H, T), dict(jitter="counter", seed=-1), {}),
        "plan.counter_seed_large": ("plan", (None, H, T), dict(jitter="counter", seed=2 ** 64), {}),
        "plan.counter_ids": ("plan", (None, H, T), dict(jitter="counter", stream_ids=[0, 1, 2, 2 ** 31]), {}),
        "plan.waypoints_word": ("plan", (None, H, T), dict(waypoints="auto"), {}),
        "plan.adaptive_with_guess": ("plan", (None, H, T), dict(waypoints="adaptive", int_wpts=np.zeros((4, 2, 2)), ts=np.ones((4, 3))), {}),
        "plan.adaptive_max_waypoints": ("plan", (None, H, T), dict(waypoints="adaptive", max_waypoints=64), {}),
        "plan.adaptive_max_waypoints_fraction": ("plan", (None, H, T), dict(waypoints="adaptive", max_waypoints=2.5), {}),
        "plan.adaptive_seg_len": ("plan", (None, H, T), dict(waypoints="adaptive"), no_seg),
        "plan.adaptive_jitter": ("plan", (None, H, T), dict(waypoints="adaptive", jitter="device"), {}),
        "plan.adaptive_head_shape": ("plan", (None, np.zeros((4, 3, 4)), np.zeros((4, 3, 4))), dict(waypoints="adaptive"), {}),
        "plan.adaptive_counter_seed": ("plan", (None, H, T), dict(waypoints="adaptive", jitter="counter", seed=-1), {}),
        "plan.adaptive_stream_ids": ("plan", (None, H, T), dict(waypoints="adaptive", stream_ids=[0, 1]), {}),
        "adaptive_counts.max_waypoints": ("adaptive_counts", (H, T), dict(max_waypoints=0), {}),
        "adaptive_counts.seg_len": ("adaptive_counts", (H, T), {}, dict(config=dict(init_seg_len=float("nan")))),
        "adaptive_counts.shape": ("adaptive_counts", (H[:, 0], T[:, 0]), {}, {}),
        "adaptive_counts.tail": ("adaptive_counts", (H, T[:3]), {}, {}),
        "adaptive_groups.row_length": ("adaptive_groups", (dict(counts=np.ones(2, np.int32), x=np.zeros((2, 8)), max_waypoints=2),), {}, {}),
        "adaptive_groups.count": ("adaptive_groups", (dict(counts=np.array([1, 0], np.int32), x=np.zeros((2, 7)), max_waypoints=2),), {}, {}),
        "plan_buffers.waypoints_word": ("plan_buffers", (4, None), dict(waypoints="auto"), {}),
        "plan_buffers.max_waypoints": ("plan_buffers", (4, None), dict(waypoints="adaptive", max_waypoints=0), {}),
        "plan_buffers.seg_len": ("plan_buffers", (4, None), dict(waypoints="adaptive"), no_seg),
        "plan_dev.head_ndim": ("plan_dev", (None, _Tensor(4, 2), _Tensor(4, 2)), {}, {}),
        "plan_dev.head_rows": ("plan_dev", (None, _Tensor(4, 2, 2), _Tensor(4, 2, 2)), {}, {}),
        "plan_dev.tail": ("plan_dev", (None, h, _Tensor(3, 3, 2)), {}, {}),
        "plan_dev.waypoints_word": ("plan_dev", (None, h, t), dict(waypoints="auto"), {}),
        "plan_dev.adaptive_x0": ("plan_dev", (None, h, t), dict(waypoints="adaptive", x0=_Tensor(4, 7)), {}),
        "plan_dev.adaptive_max_waypoints": ("plan_dev", (None, h, t), dict(waypoints="adaptive", max_waypoints=64), {}),
        "plan_dev.adaptive_seg_len": ("plan_dev", (None, h, t), dict(waypoints="adaptive"), no_seg),
        "plan_dev.x0_rows": ("plan_dev", (None, h, t), dict(x0=_Tensor(3, 7)), {}),
        "plan_dev.x0_length": ("plan_dev", (None, h, t), dict(x0=_Tensor(4, 8)), {}),
        "plan_dev.x0_short": ("plan_dev", (None, h, t), dict(x0=_Tensor(4, 2)), {}),
        "plan_dev.x0_waypoints": ("plan_dev", (None, h, t), dict(x0=_Tensor(4, 7), waypoints=3), {}),
        "plan_dev.max_attempts": ("plan_dev", (None, h, t), dict(max_attempts=0), {}),
        "plan_dev.jitter": ("plan_dev", (None, h, t), dict(jitter="device"), {}),
        "plan_dev.stream_ids": ("plan_dev", (None, h, t), dict(stream_ids=[0, 1]), {}),
        "plan_dev.counter_seed": ("plan_dev", (None, h, t), dict(jitter="counter", seed=-1), {}),
        "plan_dev.counter_ids": ("plan_dev", (None, h, t), dict(jitter="counter", stream_ids=[0, 1, 2, -1]), {}),
        "plan_dev.device_stream_ids": ("plan_dev", (None, lambda: _cpu_tensor(4, 3, 2), lambda: _cpu_tensor(4, 3, 2)),
                                       dict(jitter="counter", stream_ids=lambda: _cpu_tensor(4).long()), {}),
        "plan_dev.bufs": ("plan_dev", (None, h, t), dict(bufs=bufs), {}),
        "plan_dev.bufs_waypoints": ("plan_dev", (None, h, t), dict(bufs=dict(B=4, D=2, M=3), waypoints=3), {}),
        "plan_dev.bufs_not_adaptive": ("plan_dev", (None, h, t), dict(bufs=dict(B=4, D=2, M=7), waypoints="adaptive", max_waypoints=6), {}),
        "plan_dev.adaptive_x": ("plan_dev", (None, h, t), dict(waypoints="adaptive", max_waypoints=6, x=_Tensor(4, 7)), {}),
        "geo_init.targets": ("geo_init", (None, np.zeros((3, 2)), np.zeros((2, 2))), {}, {}),
        "batch_init_guess.dimension": ("batch_init_guess", (H3, T3), {}, {}),
        "batch_init_guess.offsets": ("batch_init_guess", (H, T), dict(K=2, lateral_offsets=[0.0, 0.5, -0.5]), {}),
        "batch_init_guess.K": ("batch_init_guess", (H, T), dict(K=9), {}),
        "batch_init_guess.K_zero": ("batch_init_guess", (H, T), dict(K=0), {}),
        "batch_plan.shape": ("batch_plan", (None, H3, T3), {}, {}),
        "batch_plan.tail": ("batch_plan", (None, H, T[:3]), {}, {}),
        "batch_plan.K": ("batch_plan", (None, H, T), dict(K=0), {}),
        "batch_plan.offsets": ("batch_plan", (None, H, T), dict(lateral_offsets=np.zeros(9)), {}),
        "batch_plan.stream_ids": ("batch_plan", (None, H, T), dict(stream_ids=[1, 2]), {}),
        "batch_plan.scene_ids": ("batch_plan", (None, H, T), dict(scene_ids=[1, 2]), {}),
    }
    return r


def refusal(name):
    """the first error of the argument set `name`: "Type: message" (nothing may get as far as the device: the planner's
    context is an object that has none)"""
    from neo_planner_amd import planner
    method, args, kw, made = _refusals()[name]
    made = dict(made)
    made_now = lambda v: v() if callable(v) else v       # (tensors are made here: importing this module imports no torch)
    args, kw = [made_now(v) for v in args], {k: made_now(v) for k, v in kw.items()}
    if "config" in made:
        made["config"] = planner.PlannerConfig(**made["config"])
    bp = planner.BatchPlanner(ctx=object(), **made)
    try:
        got = getattr(bp, method)(*args, **kw)
        if hasattr(got, "__next__"):
            next(got)
    except Exception as ex:
        return "%s: %s" % (type(ex).__name__, ex)
    return "no error"


REFUSALS = tuple(_refusals())
