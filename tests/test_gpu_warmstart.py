"""Fleet mode "warmstart" on the GPU: neo_fleet_warm_guess_dev and neo_fleet_warm_carry_dev against the NumPy model
(tests/warm_oracle_np.py), a non-finite first guess re-seeded by plan_dev, a fleet of one against the CPU oracle's
warm-started flight, the fleet's independence of its composition, and the mode with a recorder and counter jitter."""
import ctypes

import numpy as np
import pytest

import neo_planner_amd as npa
import warm_oracle_np as won
from neo_planner_amd import _lib, synth
from neo_planner_amd.replan import ReplanLoop
from oracle import minco_np as onp
from test_gpu_init import SENT64, _p, _torch, ctx_T, same, sub_args, subsets_of, tau_gap_ulp, up
from test_gpu_record import _fleet_setup, _fly

pytestmark = pytest.mark.gpu

NEO_ERR_INVALID = 1
ORIGIN = (0.0, -15.0)
COLLISION = 0x100
TAUS = (0.0, 1.0, -1.0, 36.0, -36.0, 40.0, -40.0, 800.0, -800.0, np.nan)
# (solved, status, attempts): solved twice; unsolved with an answer and the collision flag; raised, re-seeded and not
OUTCOMES = ((1, 0, 1), (1, 1, 3), (0, 1 | COLLISION, 5), (0, 4, 5), (0, 5, 5), (0, 4, 1), (0, 5, 1), (0, 3 | COLLISION, 5))


@pytest.fixture(scope="module")
def maps():
    out = []
    for s in range(8):
        m = npa.ESDF()
        m.occupancy_map_cb(synth.OccupancyGridMsg(synth.occupancy_2d(s)))
        out.append(m)
    return out


# ------------------------------------------------------------------ 1. the two kernels against the model
def case(B, count):
    """B missions' plans and outcomes: every outcome of OUTCOMES in turn (a fleet of one takes the one its count picks),
    every tau of TAUS among random ones"""
    rng = np.random.default_rng([91, B, count])
    M, n = count + 1, 3 * count + 1
    x = np.concatenate([rng.uniform(-30.0, 30.0, (B, 2 * count)), rng.uniform(-3.0, 3.0, (B, M))], 1)
    flat = x[:, 2 * count:].reshape(-1)
    at = np.arange(0, flat.size, 2)
    flat[at] = np.resize(TAUS, at.size)
    x[:, 2 * count:] = flat.reshape(B, M)
    pick = [OUTCOMES[(b + count) % len(OUTCOMES)] for b in range(B)]
    solved, status, attempts = (np.array([p[k] for p in pick], np.int32) for k in range(3))
    return dict(x=x, head=rng.uniform(-30.0, 30.0, (B, 3, 2)), solved=solved, status=status, attempts=attempts), M, n


@pytest.mark.parametrize("count", [1, 2, 20])
@pytest.mark.parametrize("B", [1, 64, 65, 257])
def test_kernels_equal_the_model(B, count):
    """Carry, then guess from the device's own carry, under the three launch lists.  Waypoints and every copied value bit
    for bit, NaNs in the same places; rows outside the list and the guard row keep their sentinel.
    Durations within 8 ulp of the model's: exp(-tau) is within 1 ulp of the truth on the device and in libm, so the two
    differ by at most 2 ulp; in s = 1 + e that error weighs e / (1 + e) < 1 and each side rounds once (half an ulp
    each): < 3 ulp; the quotient (T_max - T_min) / s carries it on and rounds once a side: < 4 ulp; so does the sum with
    T_min (T_min >= 0: the quotient's share is at most 1): < 5 ulp.  An ulp halves where a result crosses a power of two
    between two steps, which is what the allowance to 8 is for.
    tau within 4 ulp of the model fed the device's durations: log's argument is then the same bits, the device's fp64
    log and libm's are each good to 1 ulp -- 2 ulp derived, 4 allowed, as for neo_init_guess_dev.
    Largest gaps seen on the MI355X: durations 2 ulp, tau 1 ulp."""
    torch, dev = _torch()
    c, T_min, T_max = ctx_T()
    bp = npa.BatchPlanner(ctx=c)
    h, M, n = case(B, count)
    init_ts = bp._batch_ts_tau(M - 1)[0]
    assert init_ts[0] == init_ts[-1] == 1.5 * bp.cfg.init_T and (M == 2 or init_ts[1] == bp.cfg.init_T)
    t = {k: up(v) for k, v in h.items()}
    worst_T = worst_tau = 0.0
    for subset in subsets_of(B):
        keep, sp, ns = sub_args(subset)
        wl0, tc0 = np.full((B + 1, 2, count), SENT64), np.full((B + 1, M), SENT64)
        d_wl, d_tc = up(wl0), up(tc0)
        torch.cuda.synchronize(dev)
        c.check(c.lib.neo_fleet_warm_carry_dev(c.h, B, sp, ns, M, _p(t["x"]), _p(t["head"]), _p(t["solved"]), _p(t["status"]),
                                               _p(t["attempts"]), _lib.ptr(init_ts), _p(d_wl), _p(d_tc)))
        c.synchronize()
        want_wl, want_tc = wl0.copy(), tc0.copy()
        want_wl[:B], want_tc[:B] = won.carry(h["x"], h["head"], h["solved"], h["status"], h["attempts"], init_ts, wl0[:B],
                                             tc0[:B], T_min, T_max, subset)
        got_wl, got_tc = d_wl.cpu().numpy(), d_tc.cpu().numpy()
        assert same(got_wl, want_wl), subset
        gap = tau_gap_ulp(got_tc, want_tc)
        worst_T = max(worst_T, gap)
        assert gap <= 8.0, (subset, gap)
        rows = won.launched(B, subset)
        computed = np.zeros(B + 1, bool)
        computed[rows] = ((h["solved"][rows] != 0) | ((h["status"][rows] & 0xff) <= 3))
        assert same(got_tc[~computed], want_tc[~computed]), subset        # copied, kept, not launched, the guard
        if subset is None and B >= 8:
            assert (got_tc[:B][(h["solved"] == 0) & (h["attempts"] == 1)] == SENT64).all()
            assert (got_tc[:B][(h["status"] == 4) & (h["attempts"] == 5)] == init_ts).all()
            assert (got_tc[:B][h["solved"] != 0] != SENT64).all() and np.isnan(got_tc[:B]).any()
        # the guess from what the device carries; on the whole list some durations are set to the edges by hand
        ts_in = got_tc.copy()
        if subset is None:
            ts_in[0, 0], ts_in[B - 1, M - 1] = T_min, T_max
            if B > 2:
                ts_in[1, 0], ts_in[2, 0] = np.nan, np.inf
        x00 = np.full((B + 1, n), SENT64)
        d_x0, d_ts = up(x00), up(ts_in)
        torch.cuda.synchronize(dev)
        c.check(c.lib.neo_fleet_warm_guess_dev(c.h, B, sp, ns, M, _p(t["head"]), _p(d_wl), _p(d_ts), _p(d_x0)))
        c.synchronize()
        want = x00.copy()
        want[:B] = won.guess(h["head"], got_wl[:B], ts_in[:B], T_min, T_max, subset, x00[:B])
        got = d_x0.cpu().numpy()
        assert same(got[:, :2 * count], want[:, :2 * count]), subset
        gap = tau_gap_ulp(got[:, 2 * count:], want[:, 2 * count:])
        worst_tau = max(worst_tau, gap)
        assert gap <= 4.0, (subset, gap)
        assert (got[B] == SENT64).all()
        outside = np.setdiff1d(np.arange(B), rows)
        assert (got[outside] == SENT64).all() and (got_wl[outside] == SENT64).all()
        if subset is None:
            assert np.isnan(got[0, 2 * count]) and np.isnan(got[B - 1, n - 1])      # exactly T_min, exactly T_max
            assert B <= 2 or (np.isnan(got[1, 2 * count]) and np.isnan(got[2, 2 * count]))
    print(f"B = {B}, count = {count}: largest gap of the device's durations {worst_T:.2f} ulp, of its tau {worst_tau:.2f} ulp")


def test_argument_errors():
    torch, dev = _torch()
    c, T_min, T_max = ctx_T()
    B, count = 3, 2
    h, M, n = case(B, count)
    t = {k: up(v) for k, v in h.items()}
    wl, tc, x0 = up(np.full((B, 2, count), SENT64)), up(np.full((B, M), SENT64)), up(np.full((B, n), SENT64))
    init_ts = npa.BatchPlanner(ctx=c)._batch_ts_tau(M - 1)[0]
    four = up(np.array([0, 1, 2, 0], dtype=np.int32))
    torch.cuda.synchronize(dev)
    calls = {
        "neo_fleet_warm_guess_dev": [_p(t["head"]), _p(wl), _p(tc), _p(x0)],
        "neo_fleet_warm_carry_dev": [_p(t["x"]), _p(t["head"]), _p(t["solved"]), _p(t["status"]), _p(t["attempts"]),
                                     _lib.ptr(init_ts), _p(wl), _p(tc)],
    }
    for name, args in calls.items():
        fn = getattr(c.lib, name)
        for b_bad in (0, -1):
            assert fn(c.h, b_bad, None, 0, M, *args) == NEO_ERR_INVALID, name
            assert b"B must be >= 1" in c.lib.neo_last_error(c.h)
        assert fn(c.h, B, _p(four), 4, M, *args) == NEO_ERR_INVALID, name
        assert b"bad subset size" in c.lib.neo_last_error(c.h)
        assert fn(c.h, B, _p(four), -1, M, *args) == NEO_ERR_INVALID, name
        for m_bad in (1, 0, -3, _lib.NEO_MAX_PIECES + 1):
            assert fn(c.h, B, None, 0, m_bad, *args) == NEO_ERR_INVALID, (name, m_bad)
            assert b"M must be in 2 .. 64" in c.lib.neo_last_error(c.h)
        for k in range(len(args)):
            bad = list(args)
            bad[k] = None
            assert fn(c.h, B, None, 0, M, *bad) == NEO_ERR_INVALID, (name, k)
            assert b"null buffer" in c.lib.neo_last_error(c.h)
    c.synchronize()
    assert (wl.cpu().numpy() == SENT64).all() and (tc.cpu().numpy() == SENT64).all() and (x0.cpu().numpy() == SENT64).all()


# ------------------------------------------------------------------ 2. a non-finite first guess re-seeds
def test_a_non_finite_first_guess_is_re_seeded(maps):
    """a carried duration of exactly T_max gives a NaN tau: that request's first attempt ends NEO_TRAJ_NONFINITE at its
    first evaluation and counts no iteration; with attempts left plan_dev re-seeds it from the straight line"""
    torch, dev = _torch()
    c, T_min, T_max = ctx_T()
    bp = npa.BatchPlanner(ctx=c)
    B, count = 4, int(bp.cfg.init_wpts_num)
    M = count + 1
    head = np.zeros((B, 3, 2)); tail = np.zeros((B, 3, 2))
    head[:, 0, 1] = tail[:, 0, 1] = np.linspace(-1.0, 1.0, B)
    tail[:, 0, 0], tail[:, 1, 0] = 5.0, 0.8
    ts = np.tile(bp._batch_ts_tau(M - 1)[0], (B, 1))
    ts[1, 1] = T_max
    wl = np.stack([np.linspace(0.0, 5.0, count + 2)[1:-1], np.zeros(count)])[None].repeat(B, 0)
    d_head, d_tail, d_wl, d_ts = up(head), up(tail), up(wl), up(ts)
    d_x0 = up(np.zeros((B, 3 * count + 1)))
    torch.cuda.synchronize(dev)
    bp.warm_guess_dev(d_head, d_wl, d_ts, d_x0)
    c.synchronize()
    x0 = d_x0.cpu().numpy()
    assert np.isnan(x0[1, 2 * count + 1]) and np.isnan(x0).sum() == 1
    one = bp.plan_dev(maps[0], d_head, d_tail, x0=d_x0, seed=5, max_attempts=1)
    st, att, nit_total = (one[k].cpu().numpy() for k in ("status", "attempts", "nit_total"))
    assert (st[1] & 0xff) == _lib.NEO_TRAJ_NONFINITE and att[1] == 1 and nit_total[1] == 0 and one["nfev"][1].item() == 1
    assert one["solved"][1].item() == 0
    bufs = bp.plan_dev(maps[0], d_head, d_tail, x0=d_x0, seed=5)
    att, nit, nit_total, solved = (bufs[k].cpu().numpy() for k in ("attempts", "nit", "nit_total", "solved"))
    print(f"attempts {att}, nit_total {nit_total}, solved {solved}")
    assert att[1] >= 2 and bufs["launch_sizes"][0] == B
    if att[1] == 2:      # its first attempt added nothing: the total is the second attempt's
        assert nit_total[1] == nit[1]


# ------------------------------------------------------------------ 3. a fleet of one against the oracle
@pytest.mark.parametrize("scene", [0, 3])
def test_fleet_of_one_flies_the_cpu_oracles_warm_started_flight(maps, scene):
    loop = npa.FleetReplanLoop(npa.BatchPlanner(), maps[scene], [[30.0, 0.0]], mode="warmstart")
    out = loop.run([[0.0, 0.0]])
    basic = npa.FleetReplanLoop(npa.BatchPlanner(), maps[scene], [[30.0, 0.0]], resident=True).run([[0.0, 0.0]])
    np.random.seed(503)
    state = np.random.get_state()
    grid = onp.GridESDF(synth.occupancy_2d(scene), synth.RES, 300, 300, ORIGIN)
    ref = ReplanLoop(onp.OraclePlanner(onp.PlannerParams()), grid, mode="warmstart").run()
    after = np.random.get_state()
    assert np.array_equal(after[1], state[1]) and after[2:] == state[2:], "the oracle flight drew random numbers: not comparable"
    path = loop.commands(0)[:, 0, :]
    n = min(len(path), len(ref["path"]))
    print(f"scene {scene}: fleet {out['replans'][0]} plans, {out['failed_attempts'][0]} failed, {out['n_cmd'][0]} commands, "
          f"iterations {out['iter_num'][0]} (mode basic: {basic['iter_num'][0]}), runs {out['opt_runs'][0]}, clearance "
          f"{out['min_clearance'][0]:.3f}; oracle {ref['replans']} plans, {ref['failed_attempts']} failed, "
          f"{len(ref['path'])} commands, iterations {ref['iter_num']}, clearance {ref['min_clearance']:.3f}; max position "
          f"difference {np.max(np.linalg.norm(path[:n] - ref['path'][:n], axis=1)):.4f} m")
    assert ref["success"] and bool(out["success"][0])
    assert out["replans"][0] == ref["replans"] and out["failed_attempts"][0] == ref["failed_attempts"]
    assert out["n_cmd"][0] == len(path) and abs(len(path) - len(ref["path"])) <= 60
    assert np.max(np.linalg.norm(path[:n] - ref["path"][:n], axis=1)) < 0.25
    assert abs(out["iter_num"][0] - ref["iter_num"]) <= 0.2 * ref["iter_num"] + 5
    assert out["iter_num"][0] < basic["iter_num"][0]


# ------------------------------------------------------------------ 4. independence of the fleet's composition
def test_a_mission_flies_the_same_alone_and_in_a_fleet(maps):
    """scenes 0 - 7 with the goals (30, 0) and (30, -7) on each; missions 2 and 4 (scenes 1 and 2, goal (30, 0)) are the
    ones whose CPU-oracle flights re-target"""
    goals = np.tile(np.array([[30.0, 0.0], [30.0, -7.0]]), (8, 1))
    sids = np.repeat([m.scene_id for m in maps], 2).astype(np.int32)
    start = np.zeros((16, 2))
    kw = dict(mode="warmstart", seed=41, max_cmd_seconds=90)
    loop = npa.FleetReplanLoop(npa.BatchPlanner(), maps[0], goals, scene_ids=sids, **kw)
    out = loop.run(start)
    print(f"warmstart: success {out['success'].mean():.2f}, plans {out['replans']}, failed attempts {out['failed_attempts']}, "
          f"abandoned {int(out['abandoned'].sum())}, iterations {out['iter_num']}")
    assert (out["failed_attempts"] > 0).any(), "no mission re-targeted: the carry after a failed round was not flown"
    assert (out["replans"] >= 2).any()
    for i in (2, 4, 9, 15):
        one = npa.FleetReplanLoop(npa.BatchPlanner(), maps[0], goals[i:i + 1], scene_ids=sids[i:i + 1], mission_ids=[i], **kw)
        o1 = one.run(start[i:i + 1])
        for k in out:
            assert np.array_equal(np.asarray(o1[k])[0], np.asarray(out[k])[i], equal_nan=True), (i, k, o1[k][0], out[k][i])
        assert np.array_equal(one.commands(0), loop.commands(i)), i
        assert same(one.x[0], loop.x[i]), i


# ------------------------------------------------------------------ 5. with a recorder and counter jitter
def test_the_mode_flies_with_counter_jitter_and_a_recorder():
    fs = _fleet_setup()
    try:
        pick = [0, 1, 2, 3]
        loop, rec, out = _fly(fs, pick=pick, record=True, mode="warmstart", jitter="counter")
        plain, _, out0 = _fly(fs, pick=pick, record=False, mode="warmstart", jitter="counter")
        print(f"warmstart, counter jitter, recorder: success {out['success']}, plans {out['replans']}, failed attempts "
              f"{out['failed_attempts']}, rows {rec.n_rows}")
        assert loop.resident and (out["replans"] >= 2).all() and out["success"].any()
        for k in out:
            assert np.array_equal(np.asarray(out[k]), np.asarray(out0[k]), equal_nan=True), k
        for i in range(len(pick)):
            assert np.array_equal(loop.commands(i), plain.commands(i)), i
        assert rec.n_rows == int(out["replans"].sum())
    finally:
        c = _lib.default_context()
        for m in fs["maps"]:
            c.check(c.lib.neo_esdf_drop(c.h, m.scene_id))
