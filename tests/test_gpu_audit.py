"""Batched trajectory audit (neo_audit_traj_batch[_dev], BatchPlanner.audit / audit_dev, MinJerkPlanner.audit): the
reference's flight metric, ros_node/traj_planner_node.py:333-363 (get_weighted_metric), checked against the project's
own sample states and point lookups, against the NumPy oracle, and on constructed cases."""
import numpy as np
import pytest

import neo_planner_amd as npa
from neo_planner_amd import _lib, synth

pytestmark = pytest.mark.gpu

NEO_ERR_INVALID = 1  # include/neo_planner.h
CLEARANCE = ("min_clearance", "t_min_clearance", "t_first_unsafe")
SUMS = ("path_length", "feasibility", "collision", "weighted")


def _eval_rows(bp, x, head, tail, hz):
    """neo_eval_traj_batch rows (B, K, 3, D) and counts at hz"""
    c = bp.ctx
    bp._sync()
    B, n = x.shape
    D = head.shape[2]
    M = (n + D) // (D + 1)
    _, ts = bp.unpack_x(x, M, D)
    K = int(np.max(np.ceil(ts.sum(axis=1) * hz))) + 4
    state = np.zeros((B, K, 3, D))
    cnt = np.zeros(B, np.int32)
    c.check(c.lib.neo_eval_traj_batch(c.h, B, M, D, _lib.ptr(_lib.as_f64(x)), _lib.ptr(_lib.as_f64(head)),
                                      _lib.ptr(_lib.as_f64(tail)), float(hz), K, _lib.ptr(state), _lib.ptr(cnt)))
    return state, cnt


def _metric(pos, vel, acc, d, hz, total, cfg, weights=(1.0, 1.0, 100.0)):
    """get_weighted_metric (traj_planner_node.py:333-363) restated over sampled states: path length, feasibility and
    collision sums (:341-355), weighted by `weights` (:204, :357), plus the audit's clearance / maxima fields"""
    raw = np.zeros(3)
    if len(pos) > 1:
        raw[0] = np.sqrt(((pos[1:] - pos[:-1]) ** 2).sum(axis=1)).sum()
    vv = (vel ** 2).sum(axis=1) - cfg.v_max ** 2
    raw[1] = (vv[vv > 0.0] ** 3).sum()
    vd = cfg.safe_dis - d
    raw[2] = (vd[vd > 0.0] ** 3).sum()
    weighted = float(np.dot(raw, np.asarray(weights)))
    t = np.minimum(np.arange(len(pos)) * (1.0 / hz), total)
    unsafe = np.nonzero(d < cfg.safe_dis)[0]
    out = dict(path_length=raw[0], feasibility=raw[1], collision=raw[2], weighted=weighted,
               min_clearance=d.min(), t_min_clearance=t[int(np.argmin(d))],
               max_speed=np.sqrt((vel ** 2).sum(axis=1)).max(), max_acc=np.sqrt((acc ** 2).sum(axis=1)).max(),
               t_first_unsafe=t[unsafe[0]] if len(unsafe) else -1.0)
    flags = ((_lib.NEO_AUDIT_FLAG_UNSAFE if len(unsafe) else 0)
             | (_lib.NEO_AUDIT_FLAG_METRIC_FAIL if weighted > 10 * cfg.collision_cost_tol else 0)
             | (_lib.NEO_AUDIT_FLAG_OUTSIDE_MAP if np.any(d == 10000.0) else 0))
    return out, flags


def _same(a, b):
    """bit for bit (a NaN record -- a failed solve -- equals itself)"""
    return np.array_equal(a, b, equal_nan=True)


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def _check_self_consistent(bp, m, x, head, tail, hz):
    out = bp.audit(m, x, head, tail, hz=hz)
    state, cnt = _eval_rows(bp, x, head, tail, hz)
    # a failed solve (exp(-tau) overflow: neo_eval_traj_batch's count -1) is NONFINITE with a NaN record and no samples
    failed = cnt < 0
    assert np.array_equal(out["count"], np.where(failed, 0, cnt))
    assert np.all(out["flags"][failed] == _lib.NEO_AUDIT_FLAG_NONFINITE)
    assert np.all(np.isnan(out["weighted"][failed]) & np.isnan(out["duration"][failed]))
    for b in np.nonzero(~failed)[0]:
        k = cnt[b]
        assert k > 0
        pos, vel, acc = state[b, :k, 0], state[b, :k, 1], state[b, :k, 2]
        d, _ = m.query(pos)
        total = out["duration"][b]
        ref, flags = _metric(pos, vel, acc, d, hz, total, bp.cfg)
        assert out["flags"][b] == flags, b
        for f in CLEARANCE:
            assert out[f][b] == ref[f], (b, f, out[f][b], ref[f])
        for f in ("max_speed", "max_acc"):
            assert _rel(out[f][b], ref[f]) <= 1e-15, (b, f)
        for f in SUMS:
            assert abs(out[f][b] - ref[f]) <= 1e-12 * abs(ref[f]), (b, f, out[f][b], ref[f])
    D = head.shape[2]
    _, ts = bp.unpack_x(x, (x.shape[1] + D) // (D + 1), D)
    assert np.all(np.abs(out["duration"] - ts.sum(axis=1))[~failed] <= 1e-13 * ts.sum(axis=1)[~failed])
    assert np.array_equal(out["unsafe"], (out["flags"] & _lib.NEO_AUDIT_FLAG_UNSAFE) != 0)
    assert np.array_equal(out["metric_fail"], (out["flags"] & _lib.NEO_AUDIT_FLAG_METRIC_FAIL) != 0)
    return out


@pytest.fixture(scope="module")
def map2d():
    m = npa.ESDF()
    m.occupancy_map_cb(synth.OccupancyGridMsg(synth.occupancy_2d(1)))
    return m


@pytest.fixture(scope="module")
def cfg2_2d(map2d):
    bp = npa.BatchPlanner()
    head, tail, wp, ts = synth.replan_requests(1, 256, 20, D=2)
    x0 = bp.pack_x(wp, ts)
    xo = bp.optimize(map2d, x0, head, tail)["x"]
    return bp, head, tail, x0, xo


@pytest.mark.parametrize("hz", [10.0, 60.0])
def test_audit_equals_the_metric_of_eval_rows_and_point_queries_2d(map2d, cfg2_2d, hz):
    bp, head, tail, x0, xo = cfg2_2d
    raw = _check_self_consistent(bp, map2d, x0, head, tail, hz)
    opt = _check_self_consistent(bp, map2d, xo, head, tail, hz)
    # the raw guesses run through obstacles, the optimised trajectories mostly do not
    assert raw["unsafe"].any() and raw["unsafe"].sum() >= opt["unsafe"].sum()


@pytest.mark.parametrize("store,layout", [("f32", "linear"), ("f32", "brick"), ("f16", "brick")])
def test_audit_equals_the_metric_of_eval_rows_and_point_queries_3d(store, layout):
    dist = synth.esdf_3d(2, n=120, res=0.25)
    m = npa.ESDF3D(dist, 0.25, synth.DOMAIN_ORIGIN, store=store, layout=layout)
    bp = npa.BatchPlanner()
    head, tail, wp, ts = synth.replan_requests(2, 96, 20, D=3, **synth.VOLUME)
    x0 = bp.pack_x(wp, ts)
    _check_self_consistent(bp, m, x0, head, tail, 10.0)
    xo = bp.optimize(m, x0[:32], head[:32], tail[:32])["x"]
    _check_self_consistent(bp, m, xo, head[:32], tail[:32], 10.0)


def test_audit_against_the_oracle_and_the_reference_formula(map2d, cfg2_2d):
    """get_full_state_cmd(10) and GridESDF.get_edt_dis of the NumPy oracle through traj_planner_node.py:333-363"""
    from oracle import minco_np as onp
    _check_against_the_oracle(map2d, cfg2_2d, onp.PlannerParams())


@pytest.fixture(scope="module", params=["A", "B"])
def set_2d(request, map2d):
    """64 requests at a parameter set of tests/param_sets.py: a non-default v_max, safe_dis and collision_cost_tol in the
    metric, T_min / T_max in neo_eval_traj_batch's tau -> T map"""
    import param_sets as ps
    name = request.param
    bp = npa.BatchPlanner(config=ps.planner_config(name))
    head, tail, wp, _ = synth.replan_requests(1, 64, 20, D=2)
    ts = ps.durations(np.random.default_rng(7), name, (64, 21), *ps.RUN_DUR[name])
    x0 = bp.pack_x(wp, ts)
    xo = bp.optimize(map2d, x0, head, tail)["x"]
    return name, (bp, head, tail, x0, xo)


def test_audit_equals_the_metric_of_eval_rows_and_point_queries_at_the_sets(map2d, set_2d):
    _, (bp, head, tail, x0, xo) = set_2d
    raw = _check_self_consistent(bp, map2d, x0, head, tail, 10.0)
    opt = _check_self_consistent(bp, map2d, xo, head, tail, 10.0)
    assert raw["unsafe"].any() and raw["unsafe"].sum() >= opt["unsafe"].sum()


def test_audit_against_the_oracle_and_the_reference_formula_at_the_sets(map2d, set_2d):
    import param_sets as ps
    name, run = set_2d
    _check_against_the_oracle(map2d, run, ps.oracle_params(name))


def _check_against_the_oracle(map2d, run, oracle_params):
    from oracle import minco_np as onp
    bp, head, tail, x0, xo = run
    occ = synth.occupancy_2d(1)
    grid = onp.GridESDF(occ, synth.RES, occ.shape[1], occ.shape[0], (synth.DOMAIN_ORIGIN[0], synth.DOMAIN_ORIGIN[1]))
    B, M, D = 48, 21, 2
    x = np.concatenate([x0[:24], xo[:24]])
    hd = np.concatenate([head[:24], head[:24]])
    tl = np.concatenate([tail[:24], tail[:24]])
    out = bp.audit(map2d, x, hd, tl, hz=10.0)
    wp, ts = bp.unpack_x(x, M, D)
    cfg = bp.cfg
    compared = 0
    for b in range(B):
        if np.any(-x[b, D * (M - 1):] > 709.782712893384):   # math.exp(-tau) overflows: the reference raises (:481)
            assert out["flags"][b] == _lib.NEO_AUDIT_FLAG_NONFINITE and out["count"][b] == 0
            continue
        pl = onp.OraclePlanner(oracle_params)
        pl.read_planning_conditions(grid, hd[b], tl[b], wp[b], ts[b])
        st = pl.get_full_state_cmd(10)
        # the reference formula, verbatim in structure (traj_planner_node.py:333-363)
        raw = np.zeros(3)
        for i in range(len(st)):
            pos, vel = st[i][0][:2], st[i][1][:2]
            if i > 0:
                raw[0] += np.linalg.norm(pos - st[i - 1][0][:2])
            violate_vel = sum(vel ** 2) - cfg.v_max ** 2
            if violate_vel > 0:
                raw[1] += violate_vel ** 3
            violate_dis = cfg.safe_dis - grid.get_edt_dis(pos)
            if violate_dis > 0.0:
                raw[2] += violate_dis ** 3
        weighted = np.dot(raw, np.array([1, 1, 100]))
        assert _rel(out["path_length"][b], raw[0]) <= 1e-9
        assert _rel(out["feasibility"][b], raw[1]) <= 1e-6 or abs(out["feasibility"][b] - raw[1]) <= 1e-12
        assert (weighted > 10 * cfg.collision_cost_tol) == bool(out["metric_fail"][b])
        # clearance: equal unless an oracle sample sits within 1e-7 m of a cell face (nearest-cell lookup)
        p = st[:, 0, :2]
        org = np.array(synth.DOMAIN_ORIGIN[:2])
        fr = (p - org) / synth.RES
        if np.min(np.abs(fr - np.round(fr))) * synth.RES < 1e-7 or len(st) != out["count"][b]:
            continue
        compared += 1
        assert _rel(out["collision"][b], raw[2]) <= 1e-12 or (raw[2] == 0.0 and out["collision"][b] == 0.0)
        d = np.array([grid.get_edt_dis(q) for q in p])
        t = np.arange(len(st)) * (1.0 / 10)
        assert out["min_clearance"][b] == d.min()
        assert out["t_min_clearance"][b] == t[int(np.argmin(d))]
        unsafe = np.nonzero(d < cfg.safe_dis)[0]
        assert out["t_first_unsafe"][b] == (t[unsafe[0]] if len(unsafe) else -1.0)
    assert compared >= 0.9 * B, compared


def _straight(bp, p0, p1, M=4, T=4.0):
    """a request whose waypoints lie on the segment p0 -> p1, at rest at both ends: the trajectory stays on the line"""
    p0, p1 = np.asarray(p0, float), np.asarray(p1, float)
    D = len(p0)
    head = np.zeros((1, 3, D)); tail = np.zeros((1, 3, D))
    head[0, 0] = p0; tail[0, 0] = p1
    s = np.arange(1, M) / M
    wp = (p0[:, None] + (p1 - p0)[:, None] * s[None, :])[None]
    return bp.pack_x(wp, np.full((1, M), T)), head, tail


@pytest.fixture(scope="module")
def pillar():
    occ = np.zeros((300, 300), np.int8)
    occ[145:155, 100:110] = 100                  # x in [10, 11), y in [-0.5, 0.5)
    m = npa.ESDF()
    m.occupancy_map_cb(synth.OccupancyGridMsg(occ))
    return m


def test_constructed_cases(pillar):
    bp = npa.BatchPlanner()
    cases = [_straight(bp, (5.0, 0.05), (16.0, 0.05)),      # through the pillar
             _straight(bp, (5.0, 10.0), (15.0, 10.0)),      # open space
             _straight(bp, (25.0, 5.0), (35.0, 5.0)),       # leaves the map at x = 30
             _straight(bp, (35.0, 5.0), (45.0, 5.0))]       # entirely outside
    x = np.concatenate([c[0] for c in cases]); head = np.concatenate([c[1] for c in cases])
    tail = np.concatenate([c[2] for c in cases])
    out = bp.audit(pillar, x, head, tail)
    U, MF, OUT, NF = (_lib.NEO_AUDIT_FLAG_UNSAFE, _lib.NEO_AUDIT_FLAG_METRIC_FAIL, _lib.NEO_AUDIT_FLAG_OUTSIDE_MAP,
                      _lib.NEO_AUDIT_FLAG_NONFINITE)
    assert out["flags"][0] == U | MF and out["min_clearance"][0] == 0.0 and out["collision"][0] > 0.0
    assert 0.0 < out["t_first_unsafe"][0] < out["t_min_clearance"][0]
    assert out["flags"][1] == 0 and out["collision"][1] == 0.0 and out["t_first_unsafe"][1] == -1.0
    assert out["min_clearance"][1] > 5.0
    assert abs(out["path_length"][1] - 10.0) < 1e-2 and abs(out["duration"][1] - 16.0) < 1e-9
    assert out["flags"][2] & OUT and not out["flags"][2] & NF
    assert out["flags"][3] == OUT and out["min_clearance"][3] == 10000.0 and out["collision"][3] == 0.0
    assert all(out["count"][b] == len(np.arange(0, out["duration"][b], 0.1)) for b in range(4))

    # NaN in x and an overflowing tau: NONFINITE, NaN record, no samples; the other trajectories are unaffected
    xb = np.concatenate([x, x[:2], x[:2]])
    hb = np.concatenate([head, head[:2], head[:2]]); tb = np.concatenate([tail, tail[:2], tail[:2]])
    xb[4, 0] = np.nan
    xb[5, -1] = np.nan
    xb[6, -1] = -710.0                               # math.exp(710) overflows (expert_planner.py:481)
    xb[7, 1] = np.inf
    ob = bp.audit(pillar, xb, hb, tb)
    for b in (4, 5, 6, 7):
        assert ob["flags"][b] == NF and ob["count"][b] == 0
        assert all(np.isnan(ob[f][b]) for f in _lib.AUDIT_FIELDS)
    for f in list(_lib.AUDIT_FIELDS) + ["count", "flags"]:
        assert np.array_equal(ob[f][:4], out[f]), f

    # weights: the record's WEIGHTED follows them, the sums do not change
    ow = bp.audit(pillar, x, head, tail, weights=[2.0, 0.0, 1.0])
    assert ow["weighted"][0] == 2.0 * out["path_length"][0] + out["collision"][0]
    assert np.array_equal(ow["collision"], out["collision"])


def test_invalid_arguments_are_refused_and_the_context_stays_usable(pillar):
    bp = npa.BatchPlanner()
    x, head, tail = _straight(bp, (5.0, 10.0), (15.0, 10.0))
    bp._sync()
    c = bp.ctx
    a = np.zeros((1, _lib.NEO_AUDIT_FIELDS)); cnt = np.zeros(1, np.int32); fl = np.zeros(1, np.int32)
    P = _lib.ptr

    def call(hz, audit=a, count=cnt, flags=fl, D=2, h=head, t=tail, xx=x):
        M = (xx.shape[1] + D) // (D + 1)
        return c.lib.neo_audit_traj_batch(c.h, pillar.scene_id, None, 1, M, D, P(xx), P(h), P(t), float(hz), None,
                                          P(audit), P(count), P(flags))

    for hz in (0.0, -10.0, float("nan"), float("inf"), 1e12):
        assert call(hz) == NEO_ERR_INVALID
        assert b"hz" in c.lib.neo_last_error(c.h)
    assert call(10.0, audit=None) == NEO_ERR_INVALID
    assert call(10.0, count=None) == NEO_ERR_INVALID
    assert call(10.0, flags=None) == NEO_ERR_INVALID
    # an unsupported (map kind, D) pair: a 3-D field with D = 2
    g3 = npa.ESDF3D(np.full((8, 8, 8), 1.0, np.float32), 0.5, (0.0, 0.0, 0.0))
    assert c.lib.neo_audit_traj_batch(c.h, g3.scene_id, None, 1, 4, 2, P(x), P(head), P(tail), 10.0, None, P(a), P(cnt),
                                      P(fl)) == NEO_ERR_INVALID
    assert cnt[0] == 0 and fl[0] == 0 and not a.any()     # nothing was launched
    out = bp.audit(pillar, x, head, tail)
    assert out["flags"][0] == 0 and out["count"][0] == len(np.arange(0, out["duration"][0], 0.1))


def test_multi_scene_dev_slots_and_determinism(map2d, cfg2_2d):
    import torch
    bp, head, tail, x0, xo = cfg2_2d
    m2 = npa.ESDF()
    m2.occupancy_map_cb(synth.OccupancyGridMsg(synth.occupancy_2d(4)))
    B = 64
    x, hd, tl = np.concatenate([x0[:32], xo[:32]]), head[:B], tail[:B]
    sid = np.where(np.arange(B) % 2 == 0, map2d.scene_id, m2.scene_id).astype(np.int32)
    multi = bp.audit(map2d, x, hd, tl, scene_ids=sid)
    one = bp.audit(map2d, x, hd, tl)
    two = bp.audit(m2, x, hd, tl)
    even = np.arange(B) % 2 == 0
    for f in list(_lib.AUDIT_FIELDS) + ["count", "flags"]:
        assert _same(multi[f], np.where(even, one[f], two[f])), f
    again = bp.audit(map2d, x, hd, tl, scene_ids=sid)
    for f in list(_lib.AUDIT_FIELDS) + ["count", "flags"]:
        assert _same(again[f], multi[f]), f

    c = bp.ctx
    slots = np.array([c.lib.neo_scene_slot(c.h, int(s)) for s in sid], np.int32)
    slots[5] = 1 << 20                                # outside the table
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    a = torch.zeros((B, _lib.NEO_AUDIT_FIELDS), dtype=torch.float64, device="cuda")
    cnt = torch.zeros(B, dtype=torch.int32, device="cuda"); fl = torch.zeros(B, dtype=torch.int32, device="cuda")
    bp.audit_dev(map2d, dev(x), dev(hd), dev(tl), a, cnt, fl, hz=10.0, slots=dev(slots))
    c.synchronize()
    a, cnt, fl = a.cpu().numpy(), cnt.cpu().numpy(), fl.cpu().numpy()
    keep = np.arange(B) != 5
    assert _same(a[keep], np.stack([multi[f] for f in _lib.AUDIT_FIELDS], axis=1)[keep])
    assert _same(cnt[keep], multi["count"][keep]) and _same(fl[keep], multi["flags"][keep])
    assert fl[5] == _lib.NEO_AUDIT_FLAG_NONFINITE and cnt[5] == 0 and np.all(np.isnan(a[5]))


def test_min_jerk_planner_audit_equals_the_batch_audit():
    occ = synth.occupancy_2d(3)
    m = npa.ESDF()
    m.occupancy_map_cb(synth.OccupancyGridMsg(occ))
    head = np.array([[0.0, 0.0], [0.0, 0.0]])
    tail = np.array([[5.0, 0.3], [0.8, 0.0]])
    pl = npa.MinJerkPlanner(npa.PlannerConfig())
    pl.plan(m, head, tail)
    got = pl.audit()
    x = np.concatenate([np.reshape(pl.int_wpts, -1), pl.map_T2tau(pl.ts)])[None]
    ref = npa.BatchPlanner().audit(m, x, pl.head_state[None], pl.tail_state[None])
    for f in list(_lib.AUDIT_FIELDS) + ["count", "flags", "unsafe", "metric_fail"]:
        assert _same(got[f], ref[f]), f
    assert got["count"][0] == len(pl.get_full_state_cmd(10.0))
    got60 = pl.audit(hz=60.0)
    assert got60["count"][0] == len(pl.get_full_state_cmd(60.0))
