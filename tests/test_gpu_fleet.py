"""Fleet replan loop on the GPU (neo_fleet_*, neo_planner_amd.FleetReplanLoop): each kernel against a NumPy restatement of
the reference lines it replaces (ros_node/traj_planner_node.py:333-363, :450-488, :527-537, :574-578), the fleet's
independence of its composition, one flight against the CPU oracle's, and invariants over a fleet of 512."""
import ctypes
import math

import numpy as np
import pytest

import neo_planner_amd as npa
from neo_planner_amd import _lib, synth
from neo_planner_amd.fleet import draw_missions
from neo_planner_amd.replan import ReplanLoop
from oracle import minco_np as onp

pytestmark = pytest.mark.gpu

ORIGIN = (0.0, -15.0)
SENTINEL = 777.0


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


_ALIVE = []     # device copies handed to a call as bare pointers: kept until the call has run


def _dev(a):
    torch, dev = _torch()
    _ALIVE.append(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
    return _ALIVE[-1]


def _run(ctx, fn, *args):
    """a `_dev` call between torch's stream and the context's"""
    torch, dev = _torch()
    torch.cuda.synchronize(dev)
    ctx.check(fn(ctx.h, *args))
    ctx.synchronize()
    _ALIVE.clear()


@pytest.fixture(scope="module")
def maps():
    """scenes 0 - 7 on the default context, each with the oracle's host grid (the same map values, bit for bit)"""
    out = []
    for s in range(8):
        occ = synth.occupancy_2d(s)
        m = npa.ESDF()
        m.occupancy_map_cb(synth.OccupancyGridMsg(occ))
        g = onp.GridESDF(occ, synth.RES, 300, 300, ORIGIN)
        assert np.array_equal(m.esdf_map, g.esdf_map)
        out.append((m, g))
    return out


# ------------------------------------------------------------------ 1. target
class _EdgeWatch:
    """the oracle's grid behind has_collision, noting how close a queried position came to a cell edge"""

    def __init__(self, grid):
        self.grid, self.edge = grid, np.inf

    def has_collision(self, p):
        f = (np.asarray(p) - np.array(ORIGIN)) / synth.RES
        self.edge = min(self.edge, float(np.min(np.abs(f - np.round(f)))) * synth.RES)
        return self.grid.has_collision(p)


def _target_cases(grid, rng, N=4096):
    """positions uniform over the map; a quarter closer than 5 m to their goal; of the others four in five aim their
    first candidate at the inside of a pillar (so that, un-jittered, they walk); half of all cases jittered"""
    n_near, n_pillar = N // 4, 2400
    cur = np.stack([rng.uniform(0.0, 30.0, N), rng.uniform(-15.0, 15.0, N)], 1)
    th = rng.uniform(0, 2 * np.pi, N)
    u = np.stack([np.cos(th), np.sin(th)], 1)
    goal = cur + rng.uniform(6.0, 28.0, N)[:, None] * u
    goal[:n_near] = cur[:n_near] + rng.uniform(0.1, 4.9, n_near)[:, None] * u[:n_near]
    rows, cols = np.nonzero(grid.esdf_map < 0.3)
    k = n_near
    while k < n_near + n_pillar:      # cur = q - 5 u inside the map, q the centre of a cell well inside a pillar
        pick = rng.integers(0, len(rows), 4 * n_pillar)
        q = np.stack([ORIGIN[0] + (cols[pick] + 0.5) * synth.RES, ORIGIN[1] + (rows[pick] + 0.5) * synth.RES], 1)
        t2 = rng.uniform(0, 2 * np.pi, len(pick))
        u2 = np.stack([np.cos(t2), np.sin(t2)], 1)
        c2 = q - 5.0 * u2
        ok = (c2[:, 0] > 0) & (c2[:, 0] < 30) & (np.abs(c2[:, 1]) < 15)
        take = min(int(ok.sum()), n_near + n_pillar - k)
        cur[k:k + take] = c2[ok][:take]
        goal[k:k + take] = c2[ok][:take] + rng.uniform(6.0, 28.0, take)[:, None] * u2[ok][:take]
        k += take
    jitter = np.where(rng.random(N)[:, None] < 0.5, rng.normal(0.0, 1.0, (N, 2)), 0.0)
    perm = rng.permutation(N)
    return cur[perm], goal[perm], jitter[perm]


def _target_restated(grid, cur, goal, jitter, monkeypatch):
    """ReplanLoop.set_local_target (the line-by-line restatement of :450-488) with its draw replaced by `jitter`"""
    N = len(cur)
    tail = np.zeros((N, 3, 2)); near = np.zeros(N, np.int32); steps = np.zeros(N, np.int32); skip = np.zeros(N, bool)
    watch = _EdgeWatch(grid)
    loop = ReplanLoop(None, watch)
    n_steps = [0]
    real = watch.has_collision

    def counting(p):
        hit = real(p)
        n_steps[0] += bool(hit)
        return hit
    watch.has_collision = counting
    draw = [None]
    monkeypatch.setattr(np.random, "normal", lambda *a: draw[0].copy())
    for i in range(N):
        loop.global_target = goal[i]
        loop.near_global_target = False
        watch.edge, n_steps[0] = np.inf, 0
        draw[0] = jitter[i]
        with np.errstate(invalid="ignore", divide="ignore"):
            loop.set_local_target(cur[i].copy(), seed=1 if jitter[i].any() else 0)
        tail[i, :2] = loop.target_state
        near[i] = loop.near_global_target
        steps[i] = n_steps[0]
        skip[i] = watch.edge < 1e-9 or abs(np.linalg.norm(goal[i] - cur[i]) - 5.0) < 1e-9
    monkeypatch.undo()
    return tail, near, steps, skip


def test_target_equals_set_local_target(maps, monkeypatch):
    ctx = _lib.default_context()
    rng = np.random.default_rng(2024)
    every = []
    for s in range(4):
        m, grid = maps[s]
        cur, goal, jitter = _target_cases(grid, rng)
        ref_tail, ref_near, ref_steps, skip = _target_restated(grid, cur, goal, jitter, monkeypatch)
        N = len(cur)
        tail = np.full((N, 3, 2), SENTINEL); near = np.full(N, -1, np.int32); steps = np.full(N, -1, np.int32)
        flags = np.zeros(N, np.int32)
        ctx.check(ctx.lib.neo_fleet_target_batch(ctx.h, m.scene_id, None, N, None, 0, _lib.ptr(cur), _lib.ptr(goal),
                                                 _lib.ptr(jitter), 5.0, 1.0, 0.8, _lib.ptr(tail), _lib.ptr(near),
                                                 _lib.ptr(steps), _lib.ptr(flags)))
        keep = ~skip
        walked = float((ref_steps > 0).mean())
        err = np.abs(tail[keep, :2] - ref_tail[keep, :2])
        err = np.where(np.isnan(tail[keep, :2]) & np.isnan(ref_tail[keep, :2]), 0.0, err)
        print(f"scene {s}: {int(skip.sum())} of {N} cases left out (cell edge / 5 m boundary), {walked:.1%} walk, "
              f"most steps {ref_steps.max()}, near {ref_near.mean():.1%}, jittered {jitter.any(axis=1).mean():.1%}, "
              f"max |target - restatement| {np.nanmax(err):.2e}")
        assert skip.mean() < 0.01
        assert walked >= 0.20, "inputs too easy: too few cases take a lateral step"
        assert 0.24 <= ref_near.mean() <= 0.26 and 0.45 <= jitter.any(axis=1).mean() <= 0.55
        assert not flags.any()
        assert np.array_equal(near[keep], ref_near[keep])
        assert np.array_equal(steps[keep], ref_steps[keep])
        assert not np.isnan(err).any() and err.max() <= 1e-12
        assert not tail[:, 2].any()           # zero acceleration
        every.append((m, cur, goal, jitter, tail, near, steps))
    # the _dev form over all four scenes at once (map-table slots), on a subset: same bits, the rest untouched
    torch, dev = _torch()
    cur, goal, jitter = (np.concatenate([e[k] for e in every]) for k in (1, 2, 3))
    slots = np.concatenate([np.full(len(e[1]), ctx.lib.neo_scene_slot(ctx.h, e[0].scene_id), np.int32) for e in every])
    N = len(cur)
    sub = np.concatenate([rng.permutation(N)[:N // 2], [-1, N, N + 7]]).astype(np.int32)     # with indices to skip
    d_tail = torch.full((N, 3, 2), SENTINEL, dtype=torch.float64, device=dev)
    d_near = torch.full((N,), -1, dtype=torch.int32, device=dev); d_steps = d_near.clone()
    d_flags = torch.zeros(N, dtype=torch.int32, device=dev)
    _run(ctx, ctx.lib.neo_fleet_target_batch_dev, every[0][0].scene_id, _p(_dev(slots)), N, _p(_dev(sub)), len(sub),
         _p(_dev(cur)), _p(_dev(goal)), _p(_dev(jitter)), 5.0, 1.0, 0.8, _p(d_tail), _p(d_near), _p(d_steps), _p(d_flags))
    inside = np.zeros(N, bool)
    inside[sub[:N // 2]] = True
    tail_all = np.concatenate([e[4] for e in every])
    got = d_tail.cpu().numpy()
    assert np.array_equal(got[inside], tail_all[inside], equal_nan=True)
    assert np.all(got[~inside] == SENTINEL) and np.all(d_near.cpu().numpy()[~inside] == -1)
    assert np.array_equal(d_near.cpu().numpy()[inside], np.concatenate([e[5] for e in every])[inside])
    assert np.array_equal(d_steps.cpu().numpy()[inside], np.concatenate([e[6] for e in every])[inside])
    assert not d_flags.cpu().numpy().any()


def test_target_on_the_goal_has_the_reference_nan_velocity(maps):
    ctx = _lib.default_context()
    m, grid = maps[3]
    # the first candidate IS the goal: cur + 5 (goal - cur) / 5 with |goal - cur| exactly 5 (not < 5: not the near branch)
    jitter = np.zeros((1, 2))
    for cx, cy in [(x0, y0) for x0 in (2.0, 6.0, 10.0, 14.0) for y0 in (-7.0, -3.0, 1.0, 5.0)]:
        cur, goal = np.array([[cx, cy]]), np.array([[cx + 3.0, cy + 4.0]])
        first = cur[0] + 5.0 * ((goal[0] - cur[0]) / np.linalg.norm(goal[0] - cur[0]))
        if np.array_equal(first, goal[0]) and not grid.has_collision(goal[0]):
            break
    else:
        pytest.fail("no free 3-4-5 case on this scene")
    tail = np.zeros((1, 3, 2)); near = np.zeros(1, np.int32); steps = np.zeros(1, np.int32); flags = np.zeros(1, np.int32)
    ctx.check(ctx.lib.neo_fleet_target_batch(ctx.h, m.scene_id, None, 1, None, 0, _lib.ptr(cur), _lib.ptr(goal),
                                             _lib.ptr(jitter), 5.0, 1.0, 0.8, _lib.ptr(tail), _lib.ptr(near),
                                             _lib.ptr(steps), _lib.ptr(flags)))
    assert near[0] == 0 and np.array_equal(tail[0, 0], goal[0]) and np.isnan(tail[0, 1]).all()


def test_fleet_argument_errors(maps):
    ctx = _lib.default_context()
    m, _ = maps[0]
    L = ctx.lib
    a = np.zeros((4, 2)); t = np.zeros((4, 3, 2)); i = np.zeros(4, np.int32)
    ok = lambda **kw: L.neo_fleet_target_batch(ctx.h, m.scene_id, None, 4, None, 0, _lib.ptr(a), _lib.ptr(a), _lib.ptr(a),
                                               kw.get("lon", 5.0), kw.get("lat", 1.0), 0.8, kw.get("tail", _lib.ptr(t)),
                                               _lib.ptr(i), _lib.ptr(i), _lib.ptr(i))
    assert ok() == 0
    for bad in (dict(tail=None), dict(lat=0.0), dict(lat=float("nan")), dict(lon=-1.0)):
        assert ok(**bad) == 1 and L.neo_last_error(ctx.h)
    cmd = np.zeros((4, 8, 3, 2)); rec = np.zeros((4, _lib.NEO_AUDIT_FIELDS))
    au = lambda cap=8, stride=6, hz=60.0, out=_lib.ptr(rec): L.neo_fleet_audit_batch(
        ctx.h, m.scene_id, None, 4, None, 0, _lib.ptr(cmd), cap, _lib.ptr(i), stride, hz, None, out, _lib.ptr(i), _lib.ptr(i))
    assert au() == 0
    assert au(cap=0) == 1 and au(stride=0) == 1 and au(hz=0.0) == 1 and au(out=None) == 1
    assert b"stride" in L.neo_last_error(ctx.h) or b"null" in L.neo_last_error(ctx.h)
    m3 = npa.ESDF3D(np.ones((8, 8, 8), np.float32), 0.5, (0.0, 0.0, 0.0))
    assert L.neo_fleet_audit_batch(ctx.h, m3.scene_id, None, 4, None, 0, _lib.ptr(cmd), 8, _lib.ptr(i), 6, 60.0, None,
                                   _lib.ptr(rec), _lib.ptr(i), _lib.ptr(i)) == 1
    assert b"3-D" in L.neo_last_error(ctx.h)
    L.neo_esdf_drop(ctx.h, m3.scene_id)
    torch, dev = _torch()
    z = torch.zeros(64, dtype=torch.float64, device=dev); zi = torch.zeros(8, dtype=torch.int32, device=dev)
    adv = lambda cap=2, step=1, head=_p(z): L.neo_fleet_advance_dev(ctx.h, 1, None, 0, _p(z), cap, _p(zi), _p(zi), _p(zi),
                                                                     step, 1, _p(z), head)
    assert adv(cap=0) == 1 and adv(step=-1) == 1 and adv(head=None) == 1
    spl = lambda cap=2, hz=60.0, M=3, x=_p(z): L.neo_fleet_splice_dev(ctx.h, 1, None, 0, M, x, _p(z), _p(z), None, hz, 0,
                                                                       _p(z), cap, _p(zi), _p(zi), _p(zi), _p(zi))
    assert spl(cap=0) == 1 and spl(hz=0.0) == 1 and spl(M=0) == 1 and spl(x=None) == 1


# ------------------------------------------------------------------ 2. advance
def test_advance_equals_numpy_indexing():
    ctx = _lib.default_context()
    torch, dev = _torch()
    rng = np.random.default_rng(5)
    B, cap, step, ahead = 97, 400, 60, 60
    cmd = rng.normal(0, 1, (B, cap, 3, 2))
    cmd_len = rng.integers(1, cap + 1, B).astype(np.int32)
    cmd_len[:6] = [1, 1, 2, 59, 61, cap]
    cmd_index = (rng.random(B) * cmd_len).astype(np.int32)
    cmd_index[6:12] = cmd_len[6:12] - 1             # already at the end
    cmd_index[0] = 0
    for sub in (None, np.concatenate([rng.permutation(B)[:40], [B, -3]]).astype(np.int32)):
        d_idx, d_fut = _dev(cmd_index), torch.full((B,), -7, dtype=torch.int32, device=dev)
        d_cur = torch.full((B, 2), SENTINEL, dtype=torch.float64, device=dev)
        d_head = torch.full((B, 3, 2), SENTINEL, dtype=torch.float64, device=dev)
        _run(ctx, ctx.lib.neo_fleet_advance_dev, B, _p(None if sub is None else _dev(sub)), 0 if sub is None else len(sub),
             _p(_dev(cmd)), cap, _p(_dev(cmd_len)), _p(d_idx), _p(d_fut), step, ahead, _p(d_cur), _p(d_head))
        on = np.ones(B, bool) if sub is None else np.isin(np.arange(B), sub)
        idx = np.where(on, np.minimum(cmd_index + step, cmd_len - 1), cmd_index)
        fut = np.minimum(ahead + idx, cmd_len - 1)
        assert np.array_equal(d_idx.cpu().numpy(), idx)
        assert np.array_equal(d_fut.cpu().numpy()[on], fut[on]) and np.all(d_fut.cpu().numpy()[~on] == -7)
        b = np.arange(B)
        assert np.array_equal(d_cur.cpu().numpy()[on], cmd[b, idx, 0][on])
        head = d_head.cpu().numpy()
        assert np.array_equal(head[on, :2], cmd[b, fut, :2][on]) and not head[on, 2].any()
        assert np.all(head[~on] == SENTINEL) and np.all(d_cur.cpu().numpy()[~on] == SENTINEL)


# ------------------------------------------------------------------ 3. splice
def _eval_rows(bp, x, head, tail, hz, K):
    c = bp.ctx
    bp._sync()
    B = x.shape[0]
    state = np.zeros((B, K, 3, 2)); cnt = np.zeros(B, np.int32)
    c.check(c.lib.neo_eval_traj_batch(c.h, B, 3, 2, _lib.ptr(_lib.as_f64(x)), _lib.ptr(_lib.as_f64(head)),
                                      _lib.ptr(_lib.as_f64(tail)), float(hz), K, _lib.ptr(state), _lib.ptr(cnt)))
    return state, cnt


@pytest.mark.parametrize("cap,first", [(1200, 0), (1200, 1), (300, 0)])
def test_splice_writes_eval_traj_rows_at_the_look_ahead_index(cap, first):
    torch, dev = _torch()
    bp = npa.BatchPlanner()
    ctx = bp.ctx
    rng = np.random.default_rng(11)
    B, hz, guard = 48, 60.0, 4096
    head, tail, wp, ts = synth.replan_requests(1, B, 2, D=2)
    ts = ts * rng.uniform(0.4, 1.2, ts.shape)
    x = bp.pack_x(wp, ts)
    rows, cnt = _eval_rows(bp, x, head, tail, hz, 1100)
    assert cnt.min() > 100 and cnt.max() < 1100
    fut = rng.integers(0, 250, B).astype(np.int32)
    fut[0] = 0
    cmd_len = (fut + rng.integers(1, 50, B)).astype(np.int32)
    solved = (rng.random(B) < 0.7).astype(np.int32)
    solved[:2] = [1, 0]
    old = rng.normal(0, 1, (B, cap, 3, 2))
    buf = torch.full((B * cap * 6 + guard,), SENTINEL, dtype=torch.float64, device=dev)
    buf[:B * cap * 6] = _dev(old).reshape(-1)
    d_len, d_idx, d_fut = _dev(cmd_len), torch.full((B,), 5, dtype=torch.int32, device=dev), _dev(fut)
    d_flags = torch.zeros(B, dtype=torch.int32, device=dev)
    _run(ctx, ctx.lib.neo_fleet_splice_dev, B, None, 0, 3, _p(_dev(x)), _p(_dev(head)), _p(_dev(tail)), _p(_dev(solved)), hz,
         first, _p(buf), cap, _p(d_len), _p(d_idx), _p(d_fut), _p(d_flags))
    out = buf.cpu().numpy()
    assert np.all(out[B * cap * 6:] == SENTINEL), "written past the buffer"
    new = out[:B * cap * 6].reshape(B, cap, 3, 2)
    flags, new_len = d_flags.cpu().numpy(), d_len.cpu().numpy()
    full = 0
    for b in range(B):
        if not solved[b]:
            assert np.array_equal(new[b], old[b]) and new_len[b] == cmd_len[b] and flags[b] == 0
            assert d_idx[b].item() == 5 and d_fut[b].item() == fut[b]
            continue
        at = 0 if first else int(fut[b])
        k = min(int(cnt[b]), cap - at)
        assert np.array_equal(new[b, :at], old[b, :at])                    # what was flown and what is being flown stays
        assert np.array_equal(new[b, at:at + k], rows[b, :k])              # neo_eval_traj_batch's rows, bit for bit
        assert np.array_equal(new[b, at + k:], old[b, at + k:])
        assert new_len[b] == at + k
        assert flags[b] == (_lib.NEO_FLEET_FLAG_CMD_FULL if at + cnt[b] > cap else 0)
        full += int(at + cnt[b] > cap)
        assert (d_idx[b].item(), d_fut[b].item()) == ((0, 0) if first else (5, fut[b]))
    assert (full > 0) == (cap == 300)


# ------------------------------------------------------------------ 6. a flight against the CPU oracle (and 4.'s rows)
@pytest.fixture(scope="module")
def flight3(maps):
    m, _ = maps[3]
    loop = npa.FleetReplanLoop(npa.BatchPlanner(), m, [[30.0, 0.0]])
    out = loop.run([[0.0, 0.0]])
    return loop, out


def test_fleet_of_one_flies_the_cpu_oracle_flight(flight3):
    loop, out = flight3
    np.random.seed(503)
    state = np.random.get_state()
    ref = ReplanLoop(onp.OraclePlanner(onp.PlannerParams()), onp.GridESDF(synth.occupancy_2d(3), synth.RES, 300, 300, ORIGIN)).run()
    after = np.random.get_state()
    assert np.array_equal(after[1], state[1]) and after[2:] == state[2:], "the oracle flight drew random numbers: not comparable"
    path = loop.commands(0)[:, 0, :]
    n = min(len(path), len(ref["path"]))
    print(f"fleet: {out['replans'][0]} plans, {out['failed_attempts'][0]} failed, {out['n_cmd'][0]} commands, iterations "
          f"{out['iter_num'][0]}, clearance {out['min_clearance'][0]:.3f}; oracle: {ref['replans']} plans, "
          f"{ref['failed_attempts']} failed, {len(ref['path'])} commands, iterations {ref['iter_num']}, clearance "
          f"{ref['min_clearance']:.3f}; max position difference "
          f"{np.max(np.linalg.norm(path[:n] - ref['path'][:n], axis=1)):.4f} m")
    assert ref["success"] and bool(out["success"][0])
    assert out["replans"][0] == ref["replans"] and out["failed_attempts"][0] == ref["failed_attempts"]
    assert out["n_cmd"][0] == len(path) and abs(len(path) - len(ref["path"])) <= 60
    assert np.max(np.linalg.norm(path[:n] - ref["path"][:n], axis=1)) < 0.25
    assert abs(out["iter_num"][0] - ref["iter_num"]) <= 0.2 * ref["iter_num"] + 5


# ------------------------------------------------------------------ 4. audit
def _audit_restated(m, rows, n_flown, stride, hz, cfg, weights=(1.0, 1.0, 100.0)):
    """get_weighted_metric (:333-363) over rows 0, stride, ... < n_flown, distances from ESDF.query; sums by math.fsum"""
    s = rows[:n_flown:stride]
    pos, vel, acc = s[:, 0], s[:, 1], s[:, 2]
    if len(s) == 0:
        return dict(count=0, flags=0, path_length=0.0, feasibility=0.0, collision=0.0, min_clearance=np.inf,
                    t_min_clearance=-1.0, t_first_unsafe=-1.0, max_speed=0.0, max_acc=0.0, duration=n_flown / hz)
    d, _ = m.query(pos)
    path = [math.sqrt(float(((pos[i] - pos[i - 1]) ** 2).sum())) for i in range(1, len(s))]
    vv = (vel ** 2).sum(axis=1) - cfg.v_max ** 2
    vd = cfg.safe_dis - d
    raw = [math.fsum(path), math.fsum(float(v) ** 3 for v in vv[vv > 0.0]), math.fsum(float(v) ** 3 for v in vd[vd > 0.0])]
    t = np.arange(len(s)) * stride / hz
    unsafe = np.nonzero(d < cfg.safe_dis)[0]
    weighted = float(np.dot(raw, weights))
    flags = ((_lib.NEO_AUDIT_FLAG_UNSAFE if len(unsafe) else 0)
             | (_lib.NEO_AUDIT_FLAG_METRIC_FAIL if weighted > 10 * cfg.collision_cost_tol else 0)
             | (_lib.NEO_AUDIT_FLAG_OUTSIDE_MAP if np.any(d == 10000.0) else 0))
    return dict(count=len(s), flags=flags, path_length=raw[0], feasibility=raw[1], collision=raw[2], weighted=weighted,
                min_clearance=d.min(), t_min_clearance=t[int(np.argmin(d))],
                t_first_unsafe=t[unsafe[0]] if len(unsafe) else -1.0,
                max_speed=np.sqrt((vel ** 2).sum(axis=1)).max(), max_acc=np.sqrt((acc ** 2).sum(axis=1)).max(),
                duration=n_flown / hz)


def test_audit_of_flown_rows_equals_the_reference_metric(maps, flight3):
    _check_audit_of_flown_rows(maps, flight3, npa.BatchPlanner())


def test_audit_of_flown_rows_equals_the_reference_metric_at_set_a(maps, flight3):
    """the same comparison with the context at parameter set A (tests/param_sets.py): v_max 2.5, safe_dis 1.1 and
    collision_cost_tol 40 in the metric and its METRIC_FAIL threshold"""
    import param_sets as ps
    _check_audit_of_flown_rows(maps, flight3, npa.BatchPlanner(config=ps.planner_config("A")))


def _check_audit_of_flown_rows(maps, flight3, bp):
    torch, dev = _torch()
    ctx = bp.ctx
    bp._sync()
    m, _ = maps[3]
    loop, _ = flight3
    flown = loop.commands(0)
    cap, stride, hz = 2400, 6, 60.0
    assert 1000 < len(flown) <= cap
    rng = np.random.default_rng(3)
    cases = [(flown, len(flown)), (flown, len(flown) - 1), (flown, 1207), (flown, 1), (flown, 0), (flown, 7)]
    # synthetic flights: straight lines at 1.3 and 0.7 times v_max through the forest and out of the map
    for k in range(10):
        a = np.array([rng.uniform(0.5, 5.0), rng.uniform(-14.0, 14.0)])
        b = np.array([rng.uniform(31.0, 40.0), rng.uniform(-20.0, 20.0)])
        n = int(rng.integers(600, cap))
        speed = (1.3 if k % 2 == 0 else 0.7) * bp.cfg.v_max
        u = (b - a) / np.linalg.norm(b - a)
        rows = np.zeros((n, 3, 2))
        rows[:, 0] = a + (np.arange(n) / hz * speed)[:, None] * u + 0.3 * np.sin(np.arange(n) / 40.0)[:, None] * u[::-1]
        rows[:, 1] = speed * u * (1.0 + 0.2 * np.sin(np.arange(n) / 25.0))[:, None]
        rows[:, 2] = rng.normal(0, 0.5, (n, 2))
        cases.append((rows, n if k % 3 else n - int(rng.integers(1, 6))))
    B = len(cases)
    cmd = np.zeros((B, cap, 3, 2)); n_flown = np.zeros(B, np.int32)
    for b, (rows, nf) in enumerate(cases):
        cmd[b, :len(rows)] = rows
        n_flown[b] = nf
    ref = [_audit_restated(m, cmd[b], int(n_flown[b]), stride, hz, bp.cfg) for b in range(B)]
    assert any(r["flags"] & _lib.NEO_AUDIT_FLAG_OUTSIDE_MAP for r in ref) and any(r["flags"] & _lib.NEO_AUDIT_FLAG_UNSAFE for r in ref)
    assert any(r["feasibility"] > 0 for r in ref) and any(r["collision"] > 0 for r in ref)

    def device(sub):
        audit = torch.full((B, _lib.NEO_AUDIT_FIELDS), SENTINEL, dtype=torch.float64, device=dev)
        count = torch.full((B,), -1, dtype=torch.int32, device=dev); flags = count.clone()
        _run(ctx, ctx.lib.neo_fleet_audit_batch_dev, m.scene_id, None, B, _p(None if sub is None else _dev(sub)),
             0 if sub is None else len(sub), _p(_dev(cmd)), cap, _p(_dev(n_flown)), stride, hz, None, _p(audit), _p(count),
             _p(flags))
        return audit.cpu().numpy(), count.cpu().numpy(), flags.cpu().numpy()

    audit, count, flags = device(None)
    F = {name: k for k, name in enumerate(_lib.AUDIT_FIELDS)}
    for b, r in enumerate(ref):
        assert count[b] == r["count"] and flags[b] == r["flags"], (b, count[b], r["count"], flags[b], r["flags"])
        for f in ("t_first_unsafe", "t_min_clearance", "min_clearance", "max_speed", "max_acc", "duration"):
            assert audit[b, F[f]] == r[f], (b, f, audit[b, F[f]], r[f])
        for f in ("path_length", "feasibility", "collision"):
            assert abs(audit[b, F[f]] - r[f]) <= 1e-12 * abs(r[f]), (b, f, audit[b, F[f]], r[f])
        if r["count"]:
            w = 1.0 * audit[b, F["path_length"]] + 1.0 * audit[b, F["feasibility"]] + 100.0 * audit[b, F["collision"]]
            assert audit[b, F["weighted"]] == w
    # the same bits for two subset orders and launch sizes, and from host arrays; missions outside a subset untouched
    order1 = np.arange(B, dtype=np.int32)[::-1].copy()
    order2 = np.concatenate([[B + 3], rng.permutation(B)[:B - 4], [-1]]).astype(np.int32)
    a1, c1, f1 = device(order1)
    a2, c2, f2 = device(order2)
    assert np.array_equal(a1, audit) and np.array_equal(c1, count) and np.array_equal(f1, flags)
    on = np.isin(np.arange(B), order2)
    assert np.array_equal(a2[on], audit[on]) and np.array_equal(c2[on], count[on]) and np.array_equal(f2[on], flags[on])
    assert np.all(a2[~on] == SENTINEL) and np.all(c2[~on] == -1)
    ah = np.zeros((B, _lib.NEO_AUDIT_FIELDS)); ch = np.zeros(B, np.int32); fh = np.zeros(B, np.int32)
    ctx.check(ctx.lib.neo_fleet_audit_batch(ctx.h, m.scene_id, None, B, None, 0, _lib.ptr(cmd), cap, _lib.ptr(n_flown), stride,
                                            hz, None, _lib.ptr(ah), _lib.ptr(ch), _lib.ptr(fh)))
    assert np.array_equal(ah, audit) and np.array_equal(ch, count) and np.array_equal(fh, flags)
    # a row that is not finite: the NaN record
    cmd[1, 12, 0, 1] = np.nan
    a3, c3, f3 = device(np.array([1], np.int32))
    assert np.isnan(a3[1]).all() and c3[1] == 0 and f3[1] == _lib.NEO_AUDIT_FLAG_NONFINITE


# ------------------------------------------------------------------ 4b. indices to skip, and the empty subset
SKIP_B = 5
SKIP_SUBSET = np.array([3, -1, 1, SKIP_B, SKIP_B + 7], dtype=np.int32)     # missions 3 and 1; three indices to skip


def _skip_rows(maps, entry):
    """(call, outputs) of one `_dev` entry point for 5 missions: call(sub, n_sub, outs) launches it on fresh sentinel
    outputs made by outputs(); every array a launch may write is among them"""
    torch, dev = _torch()
    rng = np.random.default_rng(77)
    B = SKIP_B
    L = _lib.default_context().lib
    i32 = lambda a: torch.from_numpy(np.asarray(a, np.int32)).to(dev)
    f64 = lambda a: torch.from_numpy(np.asarray(a, np.float64)).to(dev)
    sent = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float64, device=dev)
    if entry in ("advance", "pose"):
        cap = 40
        cmd = f64(rng.normal(0, 1, (B, cap, 3, 2)))
        cmd_len = i32(rng.integers(10, cap + 1, B))
        start = rng.integers(1, 8, B)
        cur, goal = f64(rng.normal(0, 1, (B, 2))), f64(rng.normal(0, 1, (B, 2)))
        if entry == "advance":
            outputs = lambda: [i32(start), i32(np.full(B, -7)), sent(B, 2), sent(B, 3, 2)]
            call = lambda h, sub, n, o: L.neo_fleet_advance_dev(h, B, sub, n, _p(cmd), cap, _p(cmd_len), _p(o[0]), _p(o[1]),
                                                                3, 2, _p(o[2]), _p(o[3]))
        else:
            idx = i32(start)
            outputs = lambda: [sent(B, 5)]
            call = lambda h, sub, n, o: L.neo_fleet_pose_dev(h, B, sub, n, _p(cmd), cap, _p(cmd_len), _p(idx), _p(cur), _p(goal),
                                                             2.0, _p(o[0]))
    elif entry == "splice":
        cap, M = 1200, 3
        head, tail, wp, ts = synth.replan_requests(1, B, M - 1, D=2)
        x = f64(npa.BatchPlanner().pack_x(wp, ts))
        head, tail = f64(head), f64(tail)
        outputs = lambda: [sent(B, cap, 3, 2), i32(np.full(B, 9)), i32(np.full(B, 5)), i32(np.full(B, 4)), i32(np.zeros(B))]
        call = lambda h, sub, n, o: L.neo_fleet_splice_dev(h, B, sub, n, M, _p(x), _p(head), _p(tail), None, 60.0, 0, _p(o[0]),
                                                           cap, _p(o[1]), _p(o[2]), _p(o[3]), _p(o[4]))
    else:
        cap = 2400
        rows = np.zeros((B, cap, 3, 2))
        rows[:, :, 0, 0] = np.linspace(1.0, 29.0, cap)
        rows[:, :, 0, 1] = np.linspace(-9.0, 9.0, B)[:, None]
        rows[:, :, 1:] = rng.normal(0, 0.5, (B, cap, 2, 2))
        cmd, n_flown = f64(rows), i32(rng.integers(600, cap, B))
        sid = maps[3][0].scene_id
        outputs = lambda: [sent(B, _lib.NEO_AUDIT_FIELDS), i32(np.full(B, -1)), i32(np.full(B, -1))]
        call = lambda h, sub, n, o: L.neo_fleet_audit_batch_dev(h, sid, None, B, sub, n, _p(cmd), cap, _p(n_flown), 6, 60.0,
                                                                None, _p(o[0]), _p(o[1]), _p(o[2]))
    return call, outputs


@pytest.mark.parametrize("entry", ["advance", "pose", "splice", "audit"])
def test_indices_to_skip_and_the_empty_subset(maps, entry):
    """subset [3, -1, 1, B, B + 7] of 5 missions: missions 3 and 1 get the bits of the call without a subset, every
    other row keeps its sentinel; a subset of no entries returns 0 and writes nothing"""
    torch, dev = _torch()
    bp = npa.BatchPlanner()
    bp._sync()
    ctx = bp.ctx
    call, outputs = _skip_rows(maps, entry)
    sub = torch.from_numpy(SKIP_SUBSET).to(dev)

    def run(s, n):
        outs = outputs()
        torch.cuda.synchronize(dev)
        assert call(ctx.h, _p(s), n, outs) == 0
        ctx.synchronize()
        return [o.cpu().numpy() for o in outs]

    fresh = [o.cpu().numpy() for o in outputs()]
    full, part, none = run(None, 0), run(sub, len(SKIP_SUBSET)), run(sub, 0)
    on = np.isin(np.arange(SKIP_B), [3, 1])
    assert all(any(not np.array_equal(f[b], s[b]) for f, s in zip(full, fresh)) for b in range(SKIP_B)), \
        "the call without a subset left a mission as it was: its rows would check nothing"
    for f, p, e, s in zip(full, part, none, fresh):
        assert np.array_equal(p[on], f[on], equal_nan=True)
        assert np.array_equal(p[~on], s[~on])
        assert np.array_equal(e, s)


# ------------------------------------------------------------------ 5. fleet independence
@pytest.mark.parametrize("mode", ["basic", "geo"])
def test_a_mission_flies_the_same_alone_and_in_a_fleet(maps, mode):
    ys = np.array([0.0, -7.0, -4.5, -2.0, 2.5, 4.0, 6.5, 9.0])
    goals = np.tile(np.stack([np.full(8, 30.0), ys], 1), (8, 1))
    sids = np.repeat([m.scene_id for m, _ in maps], 8).astype(np.int32)
    start = np.zeros((64, 2))
    kw = dict(mode=mode, seed=41, max_cmd_seconds=90)
    loop = npa.FleetReplanLoop(npa.BatchPlanner(), maps[0][0], goals, scene_ids=sids, **kw)
    out = loop.run(start)
    print(f"{mode}: success {out['success'].mean():.2f}, plans {out['replans'].mean():.1f}, failed attempts "
          f"{out['failed_attempts'].sum()} in {int((out['failed_attempts'] > 0).sum())} missions, abandoned "
          f"{int(out['abandoned'].sum())}")
    assert (out["failed_attempts"] > 0).any(), "no mission re-targeted: the jitter and retry paths were not exercised"
    for i in range(64):
        one = npa.FleetReplanLoop(npa.BatchPlanner(), maps[0][0], goals[i:i + 1], scene_ids=sids[i:i + 1], mission_ids=[i], **kw)
        o1 = one.run(start[i:i + 1])
        for k in out:
            assert np.array_equal(np.asarray(o1[k])[0], np.asarray(out[k])[i], equal_nan=True), (i, k, o1[k][0], out[k][i])
        assert np.array_equal(one.commands(0), loop.commands(i)), i


# ------------------------------------------------------------------ 7. invariants over a fleet of 512
def test_invariants_over_a_fleet_of_512(maps):
    start, goals, sids = draw_missions([m for m, _ in maps], 64, seed=1)
    assert len(goals) == 512
    dist = np.linalg.norm(goals - start, axis=1)
    assert dist.min() >= 25.0 and dist.max() <= 30.0
    for (m, grid), k in zip(maps, range(0, 512, 64)):
        assert grid.get_edt_dis(start[k]) >= 0.7 and all(grid.get_edt_dis(g) >= 0.7 for g in goals[k:k + 64])
    max_replans = 60
    loop = npa.FleetReplanLoop(npa.BatchPlanner(), maps[0][0], goals, scene_ids=sids, seed=2)
    out = loop.run(start, max_replans=max_replans)
    ok = out["success"]
    print(f"fleet of 512: success {ok.mean():.3f}, plans a mission {out['replans'].mean():.1f}, failed attempts a mission "
          f"{out['failed_attempts'].mean():.2f}, abandoned {int(out['abandoned'].sum())}, metric_fail "
          f"{int(out['metric_fail'].sum())}, cmd_full {int(((out['flags'] & _lib.NEO_FLEET_FLAG_CMD_FULL) != 0).sum())}, "
          f"median weighted metric {np.nanmedian(out['weighted']):.2f}, min clearance of the successful "
          f"{out['min_clearance'][ok].min() if ok.any() else float('nan'):.3f}")
    assert ok.any()
    assert np.all(out["final_dist"][ok] < 0.2)
    assert not np.any(out["audit_flags"][ok] & _lib.NEO_AUDIT_FLAG_METRIC_FAIL)
    reason = (out["abandoned"] | ((out["flags"] & _lib.NEO_FLEET_FLAG_CMD_FULL) != 0) | out["metric_fail"]
              | ~(out["final_dist"] < 0.2))
    assert np.all(reason[~ok])
    assert np.all(out["replans"] <= max_replans)
    assert np.all(out["n_flown"] <= out["n_cmd"]) and np.all(out["n_cmd"] <= loop.cap)
    assert np.array_equal(out["count"], (out["n_flown"] + 5) // 6)
    for i in np.flatnonzero(ok)[:8]:
        assert np.linalg.norm(loop.commands(i)[-1, 0] - goals[i]) < 0.2
