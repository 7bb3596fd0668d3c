"""The `batch` planner mode for B requests on the GPU (neo_batch_*, BatchPlanner.batch_plan / batch_plan_dev,
FleetReplanLoop(mode="batch")): the two kernels against NumPy restatements of the reference lines they replace
(traj_planner/expert_planner.py:103-168), batch_plan request by request against MinJerkPlanner.batch_plan and, for the
requests without a feasible candidate, against BatchPlanner.plan; the fleet's batch mode against itself (alone / in a
fleet), against batch_plan, and one flight next to the CPU oracle's."""
import ctypes

import numpy as np
import pytest

import neo_planner_amd as npa
from neo_planner_amd import _lib, synth
from neo_planner_amd.fleet import draw_missions, plan_seed
from neo_planner_amd.replan import ReplanLoop
from oracle import minco_np as onp

pytestmark = pytest.mark.gpu

ORIGIN = (0.0, -15.0)
SENTINEL = 777.0
INVALID = 1          # NEO_ERR_INVALID


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope="module")
def scenes():
    """scene -> (device map, the oracle's host grid) for the scenes the tests fly on"""
    out = {}
    for s in (1, 2, 7):
        occ = synth.occupancy_2d(s)
        m = npa.ESDF()
        m.occupancy_map_cb(synth.OccupancyGridMsg(occ))
        out[s] = (m, onp.GridESDF(occ, synth.RES, 300, 300, ORIGIN))
    return out


@pytest.fixture(scope="module")
def requests(scenes):
    """the request set R: 24 requests on each of scenes 1 and 2 -- head (48, 3, 2), tail, scene ids, scene of each"""
    head = np.zeros((48, 3, 2)); tail = np.zeros((48, 3, 2)); which = np.zeros(48, int)
    k = 0
    for s in (1, 2):
        grid = scenes[s][1]
        rng = np.random.default_rng([2024, s])
        for _ in range(24):
            while True:
                x = rng.uniform(1.0, 24.0); y = rng.uniform(-9.0, 9.0); th = rng.uniform(-np.pi, np.pi)
                if grid.get_edt_dis(np.array([x, y])) >= 0.7:
                    break
            p, d = np.array([x, y]), np.array([np.cos(th), np.sin(th)])
            head[k, 0], head[k, 1] = p, 0.5 * d
            tail[k, 0], tail[k, 1] = p + 5.0 * d, 0.8 * d
            which[k] = s
            k += 1
    sids = np.array([scenes[s][0].scene_id for s in which], np.int32)
    return head, tail, sids, which


def _edge_requests(rng, B):
    """random requests plus the cases where NumPy takes another path: axis-parallel (linspace's zero step), start == target"""
    start = np.stack([rng.uniform(0.0, 25.0, B), rng.uniform(-10.0, 10.0, B)], 1)
    th = rng.uniform(-np.pi, np.pi, B)
    d = np.stack([np.cos(th), np.sin(th)], 1)
    head = np.zeros((B, 3, 2)); tail = np.zeros((B, 3, 2))
    head[:, 0], head[:, 1], head[:, 2] = start, 0.5 * d, rng.normal(0, 0.1, (B, 2))
    tail[:, 0], tail[:, 1] = start + rng.uniform(0.5, 9.0, B)[:, None] * d, 0.8 * d
    tail[1, 0] = head[1, 0] + [4.0, 0.0]
    tail[2, 0] = head[2, 0] + [0.0, -3.5]
    tail[3, 0] = head[3, 0]
    return head, tail


# ------------------------------------------------------------------ 1. candidates
@pytest.mark.parametrize("count,K,offsets", [(2, 3, None), (3, 5, [0.0, 0.4, -0.4, 1.1, -0.25]), (5, 1, None), (2, 8, None)])
def test_candidates_equal_the_numpy_restatement(count, K, offsets):
    torch, dev = _torch()
    bp = npa.BatchPlanner(npa.PlannerConfig(init_wpts_num=count))
    ctx = bp.ctx
    rng = np.random.default_rng(100 + count)
    B, M = 301, count + 1                            # more than one workgroup of 256 rows, no multiple of it
    n = 2 * count + M
    head, tail = _edge_requests(rng, B)
    slots = rng.integers(0, 5, B).astype(np.int32)
    wp, _ = bp.batch_init_guess(head, tail, K=K, lateral_offsets=offsets)
    _, tau = bp._batch_ts_tau(count)
    ref_x = np.concatenate([wp.reshape(B, K, 2 * count), np.broadcast_to(tau, (B, K, M))], axis=2)
    off = None if offsets is None else _lib.as_f64(offsets)
    keep = rng.permutation(B)[:200]
    sub = np.concatenate([keep[:77], [-1], keep[77:], [B]]).astype(np.int32)      # shuffled, with two indices to skip
    P = len(sub)
    valid = (sub >= 0) & (sub < B)

    def check(x0, hk, tk, sk):
        x0, hk, tk = x0.reshape(P, K, n), hk.reshape(P, K, 3, 2), tk.reshape(P, K, 3, 2)
        sk = sk.reshape(P, K)
        assert np.array_equal(x0[valid], ref_x[sub[valid]], equal_nan=True)
        assert np.array_equal(hk[valid], np.repeat(head[sub[valid]][:, None], K, 1))
        assert np.array_equal(tk[valid], np.repeat(tail[sub[valid]][:, None], K, 1))
        assert np.array_equal(sk[valid], np.repeat(slots[sub[valid]][:, None], K, 1))
        assert np.all(x0[~valid] == SENTINEL) and np.all(hk[~valid] == SENTINEL) and np.all(tk[~valid] == SENTINEL)
        assert np.all(sk[~valid] == -5)

    x0 = np.full((P * K, n), SENTINEL); hk = np.full((P * K, 3, 2), SENTINEL); tk = hk.copy()
    sk = np.full(P * K, -5, np.int32)
    ctx.check(ctx.lib.neo_batch_candidates(ctx.h, B, _lib.ptr(sub), P, M, 2, K, _lib.ptr(head), _lib.ptr(tail), _lib.ptr(slots),
                                           _lib.ptr(tau), _lib.ptr(off), _lib.ptr(x0), _lib.ptr(hk), _lib.ptr(tk), _lib.ptr(sk)))
    check(x0, hk, tk, sk)
    assert np.isfinite(ref_x[3, 0]).all() and np.isnan(ref_x[3, 1:, :2 * count]).all()      # start == target
    d_x0 = torch.full((P * K, n), SENTINEL, dtype=torch.float64, device=dev)
    d_hk = torch.full((P * K, 3, 2), SENTINEL, dtype=torch.float64, device=dev); d_tk = d_hk.clone()
    d_sk = torch.full((P * K,), -5, dtype=torch.int32, device=dev)
    args = [_dev(sub), _dev(head), _dev(tail), _dev(slots)]
    torch.cuda.synchronize(dev)
    ctx.check(ctx.lib.neo_batch_candidates_dev(ctx.h, B, _p(args[0]), P, M, 2, K, _p(args[1]), _p(args[2]), _p(args[3]),
                                               _lib.ptr(tau), _lib.ptr(off), _p(d_x0), _p(d_hk), _p(d_tk), _p(d_sk)))
    ctx.synchronize()
    check(d_x0.cpu().numpy(), d_hk.cpu().numpy(), d_tk.cpu().numpy(), d_sk.cpu().numpy())
    # without a subset and without slots: every request, slots_k not written
    x1 = np.zeros((B * K, n)); h1 = np.zeros((B * K, 3, 2)); t1 = np.zeros((B * K, 3, 2))
    ctx.check(ctx.lib.neo_batch_candidates(ctx.h, B, None, 0, M, 2, K, _lib.ptr(head), _lib.ptr(tail), None, _lib.ptr(tau),
                                           _lib.ptr(off), _lib.ptr(x1), _lib.ptr(h1), _lib.ptr(t1), None))
    assert np.array_equal(x1.reshape(B, K, n), ref_x, equal_nan=True)


# ------------------------------------------------------------------ 2. select
def _select_restated(B, sub, K, n, xk, ck, lk, nit, nfev, st, w, init):
    """the choice of MinJerkPlanner.batch_plan (:160-165) over packed results, with NumPy"""
    out = {k: v.copy() for k, v in init.items()}
    fb = []
    for p, b in enumerate(sub):
        if not 0 <= b < B:
            continue
        rows = slice(p * K, p * K + K)
        code = st[rows] & 0xff
        feasible = (code <= _lib.NEO_TRAJ_MAXITER) & ((st[rows] & _lib.NEO_TRAJ_FLAG_COLLISION) == 0)
        cost = np.where(feasible, (lk[rows] * w).sum(axis=1), np.inf)
        k = int(np.argmin(cost)) if np.min(cost) < np.inf else -1
        counted = code < _lib.NEO_TRAJ_NUMERIC_RANGE
        out["chosen"][b], out["cand_cost"][b], out["solved"][b] = k, cost, k >= 0
        out["nit_total"][b], out["opt_runs"][b] = nit[rows][counted].sum(), counted.sum()
        if k < 0:
            fb.append(b)
            continue
        r = p * K + k
        out["x"][b], out["costs4"][b], out["costs4_last"][b] = xk[r], ck[r], lk[r]
        out["nit"][b], out["nfev"][b], out["status"][b] = nit[r], nfev[r], st[r]
    return out, np.array(fb, np.int32)


@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("shuffled", [False, True])
def test_select_equals_the_numpy_restatement_on_synthetic_results(K, shuffled):
    torch, dev = _torch()
    ctx = _lib.default_context()
    rng = np.random.default_rng(50 + K)
    B, n, M = 2300, 7, 3                              # the compaction's workgroup walks more than two chunks of 1024
    P0 = 2100
    sub = (rng.permutation(B)[:P0] if shuffled else np.sort(rng.permutation(B)[:P0])).astype(np.int32)
    if shuffled:
        sub = np.concatenate([sub[:500], [-1, B], sub[500:], [B + 9]]).astype(np.int32)
    P = len(sub)
    R = P * K
    xk = rng.normal(0, 1, (R, n)); ck = rng.random((R, 4))
    lk = rng.random((R, 4)) * rng.choice([1e-3, 1.0, 1e3], (R, 4))
    nit = rng.integers(0, 15000, R).astype(np.int32); nfev = rng.integers(0, 15000, R).astype(np.int32)
    # every status code 0 .. 7, a third of the rows with the collision flag; a quarter of the requests all-infeasible
    st = rng.choice([0, 1, 2, 3, 4, 5, 6, 7], R, p=[.3, .2, .1, .1, .1, .1, .05, .05]).astype(np.int32)
    st |= np.where(rng.random(R) < 0.33, _lib.NEO_TRAJ_FLAG_COLLISION, 0).astype(np.int32)
    allbad = rng.random(P) < 0.25
    st.reshape(P, K)[allbad] = rng.choice([4, 5, 6, 7, 0x100, 0x103], (int(allbad.sum()), K))
    lk3 = lk.reshape(P, K, 4)
    if K > 1:
        tie = np.flatnonzero(rng.random(P) < 0.3)     # exact ties: the first index wins
        lk3[tie, K - 1] = lk3[tie, 0]
        lk3[tie[::2], K // 2] = lk3[tie[::2], 0]
    lk3[rng.random(P) < 0.05, rng.integers(0, K)] = np.inf                  # a cost of +inf ...
    some = np.flatnonzero(rng.random(P) < 0.03)
    lk3[some] = np.inf                                                      # ... in every candidate: no choice
    st.reshape(P, K)[some[::2]] = 0
    lk3[rng.random(P) < 0.05, rng.integers(0, K), 2] = np.nan               # a NaN cost: the reference falls back
    w = np.array([1.0, 1.0, 1.0, 10000.0]) * rng.uniform(0.5, 1.5, 4)
    init = dict(chosen=np.full(B, -9, np.int32), cand_cost=np.full((B, K), SENTINEL), solved=np.full(B, -9, np.int32),
                x=np.full((B, n), SENTINEL), costs4=np.full((B, 4), SENTINEL), costs4_last=np.full((B, 4), SENTINEL),
                nit=np.full(B, -9, np.int32), nfev=np.full(B, -9, np.int32), status=np.full(B, -9, np.int32),
                nit_total=np.full(B, -9, np.int32), opt_runs=np.full(B, -9, np.int32))
    ref, ref_fb = _select_restated(B, sub, K, n, xk, ck, lk, nit, nfev, st, w, init)
    on = np.isin(np.arange(B), sub[(sub >= 0) & (sub < B)])
    assert (ref["chosen"][on] == -1).sum() > 100 and all((ref["chosen"][on] == k).sum() > 20 for k in range(K))
    assert np.isnan(ref["cand_cost"][on]).any() and np.all(ref["chosen"][np.isnan(ref["cand_cost"]).any(axis=1) & on] == -1)
    names = ("chosen", "cand_cost", "solved", "x", "costs4", "costs4_last", "nit", "nfev", "status", "nit_total", "opt_runs")

    def compare(got, fb, nfb):
        for k in names:
            assert np.array_equal(got[k], ref[k], equal_nan=True), k       # bit for bit, the untouched rows included
        assert nfb == len(ref_fb) and np.array_equal(fb[:nfb], ref_fb)
        if not shuffled:
            assert np.all(np.diff(fb[:nfb]) > 0)                          # ascending

    h = {k: v.copy() for k, v in init.items()}
    fb = np.full(P, -3, np.int32); nfb = np.full(1, -3, np.int32)
    ctx.check(ctx.lib.neo_batch_select(ctx.h, B, _lib.ptr(sub), P, M, 2, K, _lib.ptr(xk), _lib.ptr(ck), _lib.ptr(lk),
                                       _lib.ptr(nit), _lib.ptr(nfev), _lib.ptr(st), _lib.ptr(w),
                                       *[_lib.ptr(h[k]) for k in names], _lib.ptr(fb), _lib.ptr(nfb)))
    compare(h, fb, int(nfb[0]))
    d = {k: _dev(v) for k, v in init.items()}
    d_fb = torch.full((P,), -3, dtype=torch.int32, device=dev); d_nfb = torch.full((1,), -3, dtype=torch.int32, device=dev)
    ins = [_dev(a) for a in (sub, xk, ck, lk, nit, nfev, st)]
    torch.cuda.synchronize(dev)
    ctx.check(ctx.lib.neo_batch_select_dev(ctx.h, B, _p(ins[0]), P, M, 2, K, *[_p(t) for t in ins[1:]], _lib.ptr(w),
                                           *[_p(d[k]) for k in names], _p(d_fb), _p(d_nfb)))
    ctx.synchronize()
    compare({k: v.cpu().numpy() for k, v in d.items()}, d_fb.cpu().numpy(), int(d_nfb.item()))


def test_select_without_weights_uses_the_contexts_weights_at_set_b():
    """weights4 == NULL: the context's weights -- at parameter set B (tests/param_sets.py: [2, 0.25, 40, 300]) the candidate
    costs and the choice are the restatement's with the set's weights, and differ from the default weights' choice"""
    import param_sets as ps
    ctx = _lib.default_context()
    rng = np.random.default_rng(77)
    B, K, n, M = 16, 3, 7, 3
    sub = rng.permutation(B).astype(np.int32)
    R = B * K
    xk = rng.normal(0, 1, (R, n)); ck = rng.random((R, 4))
    lk = rng.random((R, 4)) * np.array([1.0, 1.0, 1e-1, 1e-3])      # (a collision term that decides at 10000, not at 300)
    nit = rng.integers(0, 200, R).astype(np.int32); nfev = rng.integers(0, 400, R).astype(np.int32)
    st = rng.choice([0, 1, 2, 3, 4, 0x100], R, p=[.4, .2, .1, .1, .1, .1]).astype(np.int32)
    names = ("chosen", "cand_cost", "solved", "x", "costs4", "costs4_last", "nit", "nfev", "status", "nit_total", "opt_runs")
    init = dict(chosen=np.full(B, -9, np.int32), cand_cost=np.full((B, K), SENTINEL), solved=np.full(B, -9, np.int32),
                x=np.full((B, n), SENTINEL), costs4=np.full((B, 4), SENTINEL), costs4_last=np.full((B, 4), SENTINEL),
                nit=np.full(B, -9, np.int32), nfev=np.full(B, -9, np.int32), status=np.full(B, -9, np.int32),
                nit_total=np.full(B, -9, np.int32), opt_runs=np.full(B, -9, np.int32))
    chosen = {}
    for name in ("B", None):
        bp = npa.BatchPlanner(config=ps.planner_config(name))
        bp._sync()
        w = np.asarray(bp.cfg.weights, dtype=np.float64)
        ref, ref_fb = _select_restated(B, sub, K, n, xk, ck, lk, nit, nfev, st, w, init)
        h = {k: v.copy() for k, v in init.items()}
        fb = np.full(B, -3, np.int32); nfb = np.full(1, -3, np.int32)
        ctx.check(ctx.lib.neo_batch_select(ctx.h, B, _lib.ptr(sub), B, M, 2, K, _lib.ptr(xk), _lib.ptr(ck), _lib.ptr(lk),
                                           _lib.ptr(nit), _lib.ptr(nfev), _lib.ptr(st), None,
                                           *[_lib.ptr(h[k]) for k in names], _lib.ptr(fb), _lib.ptr(nfb)))
        for k in names:
            assert np.array_equal(h[k], ref[k], equal_nan=True), (name, k)
        assert int(nfb[0]) == len(ref_fb) and np.array_equal(fb[:len(ref_fb)], ref_fb)
        chosen[name] = h["chosen"].copy()
    assert (chosen["B"] >= 0).sum() >= B // 2 and not np.array_equal(chosen["B"], chosen[None])


# ------------------------------------------------------------------ 3. batch_plan on R
class _Recording(npa.MinJerkPlanner):
    """MinJerkPlanner that keeps the tau the optimiser returned for every candidate (batch_plan keeps int_wpts and ts only)"""

    def _finish_plan_once(self, x, *rest):
        self.taus = getattr(self, "taus", []) + [x[0][-self.M:].copy()]
        return super()._finish_plan_once(x, *rest)


@pytest.fixture(scope="module")
def planned(scenes, requests):
    """BatchPlanner.batch_plan over R in both modes, once"""
    head, tail, sids, _ = requests
    out = {}
    for mode in ("f64", "f32x"):
        bp = npa.BatchPlanner(sample_dtype=mode)
        out[mode] = (bp, bp.batch_plan(scenes[1][0], head, tail, scene_ids=sids, seed=11, stream_ids=np.arange(48) + 500))
    return out


@pytest.mark.parametrize("mode", ["f64", "f32x"])
def test_batch_plan_is_the_single_request_planner_or_the_fallback_plan(scenes, requests, planned, mode, capsys):
    head, tail, sids, which = requests
    bp, out = planned[mode]
    feasible = np.isfinite(out["candidate_cost"]).sum(axis=1)
    none, some, every = int((feasible == 0).sum()), int(((feasible > 0) & (feasible < 3)).sum()), int((feasible == 3).sum())
    with capsys.disabled():
        print(f"\n{mode}: requests without a feasible candidate {none}, with some {some}, with all three {every}; "
              f"chosen {np.bincount(out['chosen'] + 1, minlength=4).tolist()} (fallback, 0, 1, 2)")
    assert none >= 4 and some >= 1 and every >= 24
    assert np.array_equal(out["chosen"] == -1, feasible == 0)
    w = np.asarray(bp.cfg.weights, dtype=np.float64)
    for b in np.flatnonzero(out["chosen"] >= 0):
        mj = _Recording(npa.PlannerConfig(), sample_dtype=mode)
        mj.batch_plan(scenes[which[b]][0], head[b, :2], tail[b, :2])
        k = int(out["chosen"][b])
        assert np.array_equal(mj.int_wpts, out["x"][b, :4].reshape(2, 2)), b
        assert len(mj.taus) == 3 and np.array_equal(mj.taus[k], out["x"][b, 4:]), b      # the tau of the kept candidate
        assert np.array_equal(mj.ts, mj.map_tau2T(out["x"][b, 4:])), b
        assert mj.final_cost == out["final_cost"][b] == out["candidate_cost"][b, k], b
        assert mj.iter_num == out["nit_total"][b] and mj.opt_running_times == out["attempts"][b], b
        assert bool(out["solved"][b]) and out["final_cost"][b] == (out["costs_last"][b] * w).sum()
    # the requests without a feasible candidate: plan(int_wpts=candidate 0) over those alone, same seed and streams
    f = np.flatnonzero(out["chosen"] == -1)
    cand, ts = bp.batch_init_guess(head[f], tail[f])
    ref = bp.plan(scenes[1][0], head[f], tail[f], int_wpts=cand[:, 0], ts=np.tile(ts, (len(f), 1)), seed=11,
                  stream_ids=(np.arange(48) + 500)[f], scene_ids=sids[f])
    for k in ("x", "costs", "costs_last", "nit", "nfev", "status", "collision", "solved"):
        assert np.array_equal(out[k][f], ref[k], equal_nan=True), k
    # ... after the three candidates of the main path, run here as a plain launch of 3 |f| trajectories
    _, tau = bp._batch_ts_tau(2)
    x0 = np.concatenate([cand.reshape(len(f) * 3, 4), np.broadcast_to(tau, (len(f) * 3, 3))], axis=1)
    main = bp.optimize(scenes[1][0], x0, np.repeat(head[f], 3, 0), np.repeat(tail[f], 3, 0), scene_ids=np.repeat(sids[f], 3))
    counted = (main["status"] < _lib.NEO_TRAJ_NUMERIC_RANGE).reshape(len(f), 3)
    assert np.array_equal(out["attempts"][f], counted.sum(axis=1) + ref["attempts"])
    assert np.array_equal(out["nit_total"][f], np.where(counted, main["nit"].reshape(len(f), 3), 0).sum(axis=1) + ref["nit_total"])
    assert np.array_equal(out["final_cost"][f], (ref["costs_last"] * w).sum(axis=1))


def test_a_degenerate_request_changes_no_other_row_and_dev_equals_host(scenes, requests, planned):
    torch, dev = _torch()
    head, tail, sids, _ = requests
    bp, out = planned["f64"]
    h2 = np.concatenate([head, head[:1]]); t2 = np.concatenate([tail, tail[:1]])
    t2[48, 0] = h2[48, 0]                                  # start == target: candidates 1 and 2 are NaN
    more = bp.batch_plan(scenes[1][0], h2, t2, scene_ids=np.concatenate([sids, sids[:1]]), seed=11,
                         stream_ids=np.arange(49) + 500)
    assert np.isinf(more["candidate_cost"][48, 1:]).all()
    for k in out:
        assert np.array_equal(more[k][:48], out[k], equal_nan=True), k
    # the resident form: same bits for the requests with a choice, the same fallback list
    c = bp.ctx
    slots = _dev(np.array([c.lib.neo_scene_slot(c.h, int(s)) for s in sids], np.int32))
    d_head, d_tail = _dev(head), _dev(tail)
    torch.cuda.synchronize(dev)
    bufs = bp.batch_plan_dev(scenes[1][0], d_head, d_tail, slots=slots)
    fb = bp.batch_fallback(bufs)
    assert np.array_equal(fb, np.flatnonzero(out["chosen"] == -1))
    ok = out["chosen"] >= 0
    assert np.array_equal(bufs["chosen"].cpu().numpy(), out["chosen"])
    assert np.array_equal(bufs["candidate_cost"].cpu().numpy(), out["candidate_cost"])
    for k in ("x", "costs", "costs_last", "nit", "nfev"):
        assert np.array_equal(bufs[k].cpu().numpy()[ok], out[k][ok]), k
    assert np.array_equal(bufs["status"].cpu().numpy()[ok] & 0xff, out["status"][ok])
    assert np.array_equal(bufs["nit_total"].cpu().numpy()[ok], out["nit_total"][ok])


# ------------------------------------------------------------------ 4. fleet
def test_a_mission_flies_the_same_alone_and_in_a_batch_fleet(scenes, capsys):
    ys = np.array([0.0, -7.0, -4.5, -2.0, 2.5, 4.0, 6.5, 9.0])
    goals = np.tile(np.stack([np.full(8, 30.0), ys], 1), (2, 1))
    sids = np.repeat([scenes[1][0].scene_id, scenes[2][0].scene_id], 8).astype(np.int32)
    start = np.zeros((16, 2))
    kw = dict(mode="batch", seed=41, max_cmd_seconds=90)
    loop = npa.FleetReplanLoop(npa.BatchPlanner(), scenes[1][0], goals, scene_ids=sids, **kw)
    out = loop.run(start)
    with capsys.disabled():
        print(f"\nbatch fleet of 16: success {out['success'].mean():.2f}, plans {out['replans'].mean():.1f}, failed attempts "
              f"{out['failed_attempts'].sum()}, runs a plan {out['opt_runs'].sum() / max(out['replans'].sum(), 1):.2f}")
    assert out["success"].any() and np.all(out["opt_runs"] >= 3 * out["replans"] - loop.uncounted_candidates)
    for i in range(16):
        one = npa.FleetReplanLoop(npa.BatchPlanner(), scenes[1][0], goals[i:i + 1], scene_ids=sids[i:i + 1], mission_ids=[i], **kw)
        o1 = one.run(start[i:i + 1])
        for k in out:
            assert np.array_equal(np.asarray(o1[k])[0], np.asarray(out[k])[i], equal_nan=True), (i, k, o1[k][0], out[k][i])
        assert np.array_equal(one.commands(0), loop.commands(i)), i


def test_first_plans_of_a_batch_fleet_are_batch_plans(scenes, capsys):
    maps = [scenes[1][0], scenes[2][0]]
    start, goals, sids = draw_missions(maps, 32, seed=3)
    bp = npa.BatchPlanner()
    loop = npa.FleetReplanLoop(bp, maps[0], goals, mode="batch", scene_ids=sids, seed=5)
    out = loop.run(start, max_replans=0)
    kind = (out["replans"] == 1) & (out["failed_attempts"] == 0)
    with capsys.disabled():
        print(f"\nfirst plans: {int(kind.sum())} of 64 missions planned at the first target")
    assert kind.mean() >= 0.75
    head = np.zeros((64, 3, 2))
    head[:, 0] = start
    tail = loop._dev["tail"].cpu().numpy()               # the target kernel's; round 0's for the missions of this kind
    ref = bp.batch_plan(maps[0], head, tail, scene_ids=sids, seed=plan_seed(5, 0, 0), stream_ids=np.arange(64))
    assert ref["solved"][kind].all()
    c = bp.ctx
    bp._sync()
    K = 1400
    rows = np.zeros((64, K, 3, 2)); cnt = np.zeros(64, np.int32)
    c.check(c.lib.neo_eval_traj_batch(c.h, 64, 3, 2, _lib.ptr(_lib.as_f64(ref["x"])), _lib.ptr(head), _lib.ptr(_lib.as_f64(tail)),
                                      60.0, K, _lib.ptr(rows), _lib.ptr(cnt)))
    for i in np.flatnonzero(kind):
        assert 0 < cnt[i] < K and out["n_cmd"][i] == cnt[i]
        assert np.array_equal(loop.commands(i), rows[i, :cnt[i]]), i
        assert out["iter_num"][i] == ref["nit_total"][i] and out["opt_runs"][i] == ref["attempts"][i]


def test_a_batch_fleet_of_one_flies_next_to_the_cpu_oracle(scenes, capsys):
    m, grid = scenes[7]
    loop = npa.FleetReplanLoop(npa.BatchPlanner(), m, [[30.0, 0.0]], mode="batch")
    out = loop.run([[0.0, 0.0]])
    np.random.seed(503)
    ref = ReplanLoop(onp.OraclePlanner(onp.PlannerParams()), grid, mode="batch").run()
    path = loop.commands(0)[:, 0, :]
    n = min(len(path), len(ref["path"]))
    with capsys.disabled():
        print(f"\nbatch fleet of one, scene 7: {out['replans'][0]} plans, {out['opt_runs'][0]} runs, {out['n_cmd'][0]} commands, "
              f"iterations {out['iter_num'][0]}, failed {out['failed_attempts'][0]}, clearance {out['min_clearance'][0]:.3f}; "
              f"oracle: {ref['replans']} plans, {len(ref['path'])} commands, iterations {ref['iter_num']}, failed "
              f"{ref['failed_attempts']}, clearance {ref['min_clearance']:.3f}; max position difference "
              f"{np.max(np.linalg.norm(path[:n] - ref['path'][:n], axis=1)):.4f} m")
    assert ref["success"] and bool(out["success"][0])
    assert out["opt_runs"][0] >= 3 * out["replans"][0] - loop.uncounted_candidates[0]


# ------------------------------------------------------------------ 5. argument errors
def test_batch_argument_errors(scenes):
    ctx = _lib.default_context()
    L = ctx.lib
    h = np.zeros((4, 3, 2)); x = np.zeros((4 * 8, 7)); i = np.zeros(4 * 8, np.int32); tau = np.zeros(3)
    cand = lambda D=2, K=3, head=_lib.ptr(h): L.neo_batch_candidates(ctx.h, 4, None, 0, 3, D, K, head, _lib.ptr(h), None,
                                                                      _lib.ptr(tau), None, _lib.ptr(x), _lib.ptr(np.zeros((32, 3, 2))),
                                                                      _lib.ptr(np.zeros((32, 3, 2))), None)
    assert cand() == 0
    for bad in (dict(D=3), dict(K=0), dict(K=9), dict(head=None)):
        assert cand(**bad) == INVALID and L.neo_last_error(ctx.h)
    c4 = np.zeros((32, 4)); o = np.zeros((4, 8)); oi = np.zeros(4, np.int32)
    sel = lambda D=2, K=3, fb=_lib.ptr(i): L.neo_batch_select(
        ctx.h, 4, None, 0, 3, D, K, _lib.ptr(x), _lib.ptr(c4), _lib.ptr(c4), _lib.ptr(i), _lib.ptr(i), _lib.ptr(i), None,
        _lib.ptr(oi), _lib.ptr(o), _lib.ptr(oi), _lib.ptr(o), _lib.ptr(o), _lib.ptr(o), None, None, _lib.ptr(oi), _lib.ptr(oi),
        _lib.ptr(oi), fb, _lib.ptr(oi))
    assert sel() == 0
    for bad in (dict(D=3), dict(K=0), dict(K=9), dict(fb=None)):
        assert sel(**bad) == INVALID and L.neo_last_error(ctx.h)
    bp = npa.BatchPlanner()
    m = scenes[1][0]
    head = np.zeros((4, 3, 2)); tail = np.ones((4, 3, 2))
    for kw in (dict(K=0), dict(K=9), dict(K=3, lateral_offsets=[0.0, 0.6]), dict(stream_ids=np.arange(3))):
        with pytest.raises(ValueError):
            bp.batch_plan(m, head, tail, **kw)
    with pytest.raises(ValueError):
        bp.batch_plan(m, np.zeros((4, 3, 3)), np.ones((4, 3, 3)))
