"""BatchPlanner.plan on resident arrays (neo_plan_*, BatchPlanner.plan_dev, FleetReplanLoop(resident=True)) on the GPU:
the two kernels against NumPy (init_guess / pack_x, and the merge restatement tests/test_plan_dev_cpu.py pins to plan's
own bookkeeping), plan_dev against plan -- every returned array bit for bit, the launch sizes too -- a request alone
against its row in the batch, and the fleet's resident form against its host form, flight by flight."""
import ctypes
import functools

import numpy as np
import pytest

import neo_planner_amd as npa
from neo_planner_amd import _lib, synth
from neo_planner_amd.fleet import draw_missions
from oracle import minco_np as onp
from test_plan_dev_cpu import MERGED, merge_restated

pytestmark = pytest.mark.gpu

ORIGIN = (0.0, -15.0)
SENTINEL = 777.0
INVALID = 1          # NEO_ERR_INVALID
IDS = np.arange(48) * 3 + 500          # the requests' stream ids: not their positions


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
    """the request set R: 24 requests on each of scenes 1 (14 m long) and 7 (11 m) -- head (48, 3, 2), tail, scene ids,
    map-table slots.  Long requests from a free start to anywhere inside the map: some targets lie in an obstacle (no
    attempt can succeed), some straight lines end in a collision that a jittered retry gets out of."""
    head = np.zeros((48, 3, 2)); tail = np.zeros((48, 3, 2)); which = np.zeros(48, int)
    k = 0
    for s, dist in ((1, 14.0), (7, 11.0)):
        grid = scenes[s][1]
        rng = np.random.default_rng([2024, s])
        for _ in range(24):
            while True:
                x = rng.uniform(1.0, 24.0); y = rng.uniform(-9.0, 9.0); th = rng.uniform(-np.pi, np.pi)
                p, d = np.array([x, y]), np.array([np.cos(th), np.sin(th)])
                if grid.get_edt_dis(p) >= 0.7 and grid.get_edt_dis(p + dist * d) >= 0.0:
                    break
            head[k, 0], head[k, 1] = p, 0.5 * d
            tail[k, 0], tail[k, 1] = p + dist * d, 0.8 * d
            which[k] = s
            k += 1
    sids = np.array([scenes[s][0].scene_id for s in which], np.int32)
    c = _lib.default_context()
    slots = np.array([c.lib.neo_scene_slot(c.h, int(s)) for s in sids], np.int32)
    return head, tail, sids, slots


# ------------------------------------------------------------------ 1. guess
def _guess_requests(rng, B, D):
    head = rng.normal(0.0, 8.0, (B, 3, D)); tail = rng.normal(0.0, 8.0, (B, 3, D))
    tail[3, 0] = head[3, 0]                                     # start == target
    tail[4, 0, 0] = head[4, 0, 0]                               # no way to go in one dimension
    return head, tail


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("count", [2, 3, 5])
def test_guess_equals_init_guess_and_pack_x(count, D):
    torch, dev = _torch()
    bp = npa.BatchPlanner(npa.PlannerConfig(init_wpts_num=count))
    ctx = bp.ctx
    rng = np.random.default_rng(10 * count + D)
    B, M = 301, count + 1                            # more than one workgroup of 256 requests, no multiple of it
    n = D * count + M
    head, tail = _guess_requests(rng, B, D)
    slots = rng.integers(0, 5, B).astype(np.int32)
    frac, tau = bp._plan_frac_tau(count)
    keep = rng.permutation(B)[:270]
    keep[0] = 3
    keep = np.unique(keep)
    rng.shuffle(keep)
    sub = np.concatenate([keep[:77], [B], keep[77:]]).astype(np.int32)      # shuffled, with one index to skip
    P = len(sub)
    valid = (sub >= 0) & (sub < B)
    noise = rng.normal(0.0, 0.5, (P, D, count))
    wp, ts = bp.init_guess(head[sub[valid]], tail[sub[valid]], count)
    x_init = rng.normal(0.0, 3.0, (B, n))
    refs = {"line": bp.pack_x(wp, ts), "noise": bp.pack_x(wp + noise[valid], ts), "x_init": x_init[sub[valid]]}
    assert not np.array_equal(refs["line"], refs["noise"]) and np.isfinite(refs["noise"]).all()

    def check(kind, x0, hk, tk, sk):
        assert np.array_equal(x0[valid], refs[kind]), kind
        assert np.array_equal(hk[valid], head[sub[valid]]) and np.array_equal(tk[valid], tail[sub[valid]])
        assert np.array_equal(sk[valid], slots[sub[valid]])
        assert np.all(x0[~valid] == SENTINEL) and np.all(hk[~valid] == SENTINEL) and np.all(tk[~valid] == SENTINEL)
        assert np.all(sk[~valid] == -5)

    d_in = [_dev(a) for a in (sub, head, tail, slots, x_init, noise)]
    for kind in ("line", "noise", "x_init"):
        xi, no = (x_init if kind == "x_init" else None), (noise if kind == "noise" else None)
        x0 = np.full((P, n), SENTINEL); hk = np.full((P, 3, D), SENTINEL); tk = hk.copy(); sk = np.full(P, -5, np.int32)
        ctx.check(ctx.lib.neo_plan_guess(ctx.h, B, _lib.ptr(sub), P, M, D, _lib.ptr(head), _lib.ptr(tail), _lib.ptr(slots),
                                         _lib.ptr(xi), _lib.ptr(no), _lib.ptr(frac), _lib.ptr(tau), _lib.ptr(x0), _lib.ptr(hk),
                                         _lib.ptr(tk), _lib.ptr(sk)))
        check(kind, x0, hk, tk, sk)
        d_x0 = torch.full((P, n), SENTINEL, dtype=torch.float64, device=dev)
        d_hk = torch.full((P, 3, D), SENTINEL, dtype=torch.float64, device=dev); d_tk = d_hk.clone()
        d_sk = torch.full((P,), -5, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        ctx.check(ctx.lib.neo_plan_guess_dev(ctx.h, B, _p(d_in[0]), P, M, D, _p(d_in[1]), _p(d_in[2]), _p(d_in[3]),
                                             _p(d_in[4]) if xi is not None else None, _p(d_in[5]) if no is not None else None,
                                             _lib.ptr(frac), _lib.ptr(tau), _p(d_x0), _p(d_hk), _p(d_tk), _p(d_sk)))
        ctx.synchronize()
        check(kind, d_x0.cpu().numpy(), d_hk.cpu().numpy(), d_tk.cpu().numpy(), d_sk.cpu().numpy())
    # without a subset and without slots: every request, slots_k not written
    x1 = np.zeros((B, n)); h1 = np.zeros((B, 3, D)); t1 = np.zeros((B, 3, D))
    ctx.check(ctx.lib.neo_plan_guess(ctx.h, B, None, 0, M, D, _lib.ptr(head), _lib.ptr(tail), None, None, None, _lib.ptr(frac),
                                     _lib.ptr(tau), _lib.ptr(x1), _lib.ptr(h1), _lib.ptr(t1), None))
    wp_all, ts_all = bp.init_guess(head, tail, count)
    assert np.array_equal(x1, bp.pack_x(wp_all, ts_all)) and np.array_equal(h1, head) and np.array_equal(t1, tail)
    assert np.array_equal(x1[3, :D * count], np.repeat(head[3, 0], count))          # start == target: the start, count times


# ------------------------------------------------------------------ 2. merge
def _packed_results(rng, P, n, with_bad_scene):
    codes = [0, 1, 2, 3, 4, 5, 7] + ([6] if with_bad_scene else [])
    st = rng.choice(codes, P).astype(np.int32)
    if with_bad_scene and P:
        st[0] = 6                                               # (position 0 is never one of the skipped ones)
    st |= np.where(rng.random(P) < 0.33, _lib.NEO_TRAJ_FLAG_COLLISION, 0).astype(np.int32)
    return (rng.normal(0, 1, (P, n)), rng.random((P, 4)), rng.random((P, 4)), rng.integers(0, 15000, P).astype(np.int32),
            rng.integers(0, 15000, P).astype(np.int32), st)


@pytest.mark.parametrize("P0", [0, 1, 63, 64, 65, 1500])
def test_merge_equals_the_numpy_restatement_on_synthetic_results(P0):
    """P across the wavefront width and across the compaction's workgroup width (1024); two merges in a row: the first
    starts a chain (reset), the second accumulates onto it, over another shuffled subset and with a bad scene among its
    statuses"""
    torch, dev = _torch()
    ctx = _lib.default_context()
    rng = np.random.default_rng(70 + P0)
    B, n, M, D = 1700, 7, 3, 2
    init = dict(x=np.full((B, n), SENTINEL), costs4=np.full((B, 4), SENTINEL), costs4_last=np.full((B, 4), SENTINEL),
                nit=np.full(B, -9, np.int32), nfev=np.full(B, -9, np.int32), status=np.full(B, -9, np.int32),
                attempts=np.full(B, 40, np.int32), nit_total=np.full(B, 5_000_000_000, np.int64),
                solved=np.full(B, -9, np.int32))
    steps = []
    for reset in (1, 0):
        sub = rng.permutation(B)[:P0].astype(np.int32)
        if P0 >= 63:
            sub[[5, P0 - 2]] = [-1, B]                          # two indices to skip, the count stays P0
        steps.append((reset, sub) + _packed_results(rng, P0, n, with_bad_scene=(reset == 0)))
    h = {k: v.copy() for k, v in init.items()}
    d = {k: _dev(v) for k, v in init.items()}
    ref = init
    for reset, sub, xk, ck, lk, nit, nfev, st in steps:
        P = len(sub)
        ref, ref_list, ref_bad = merge_restated(B, sub, reset, xk, ck, lk, nit, nfev, st, ref)
        assert ref_bad == int(reset == 0 and P > 0)

        def compare(got, lst, nl, bad):
            for k in MERGED:
                assert np.array_equal(got[k], ref[k]), k            # bit for bit, the rows not launched included
            assert nl == len(ref_list) and np.array_equal(lst[:nl], ref_list) and bad == ref_bad   # in position order

        lst = np.full(max(P, 1), -3, np.int32); nl = np.full(1, -3, np.int32); bad = np.full(1, -3, np.int32)
        ctx.check(ctx.lib.neo_plan_merge(ctx.h, B, _lib.ptr(sub), P, M, D, reset, _lib.ptr(xk), _lib.ptr(ck), _lib.ptr(lk),
                                         _lib.ptr(nit), _lib.ptr(nfev), _lib.ptr(st), *[_lib.ptr(h[k]) for k in MERGED],
                                         _lib.ptr(lst), _lib.ptr(nl), _lib.ptr(bad)))
        compare(h, lst, int(nl[0]), int(bad[0]))
        d_lst = torch.full((max(P, 1),), -3, dtype=torch.int32, device=dev)
        d_cnt = torch.full((2,), -3, dtype=torch.int32, device=dev)
        ins = [_dev(a) if a.size else torch.zeros(8, dtype=torch.from_numpy(a).dtype, device=dev)
               for a in (sub, xk, ck, lk, nit, nfev, st)]
        torch.cuda.synchronize(dev)
        ctx.check(ctx.lib.neo_plan_merge_dev(ctx.h, B, _p(ins[0]), P, M, D, reset, *[_p(t) for t in ins[1:]],
                                             *[_p(d[k]) for k in MERGED], _p(d_lst), _p(d_cnt[0:]), _p(d_cnt[1:])))
        ctx.synchronize()
        cnt = d_cnt.cpu().numpy()
        compare({k: v.cpu().numpy() for k, v in d.items()}, d_lst.cpu().numpy(), int(cnt[0]), int(cnt[1]))
    on = np.zeros(B, bool)
    for _, sub, *_rest in steps:
        on[sub[(sub >= 0) & (sub < B)]] = True
    for k in MERGED:
        assert np.array_equal(ref[k][~on], init[k][~on]), k          # (the restatement itself leaves them alone)
    if P0 == 1500:
        both = np.intersect1d(steps[0][1], steps[1][1])
        both = both[(both >= 0) & (both < B)]
        assert both.size > 1000 and np.all(ref["attempts"][both] == 2)


# ------------------------------------------------------------------ 2b. one merge kernel behind both entry points
MERGE_B, MERGE_P = 1300, 1100          # more than one chunk of the compactions' 1024 and 256 lanes


@functools.lru_cache(maxsize=None)
def _merge_case(M, D):
    """one merge's inputs, made once: a shuffled subset of MERGE_P of MERGE_B requests with one index to skip, packed
    results whose status column walks the codes 0 .. 7 without and with the collision flag, sentinel request-indexed
    arrays -- and for reset = 1 and 0 what merge_restated makes of them"""
    n = D * (M - 1) + M
    rng = np.random.default_rng(1000 * M + D)
    B, P = MERGE_B, MERGE_P
    sub = rng.permutation(B)[:P].astype(np.int32)
    sub[700] = B                                                # an index outside 0 .. B - 1
    st = (np.arange(P) % 8 + np.where(np.arange(P) // 8 % 2 == 1, _lib.NEO_TRAJ_FLAG_COLLISION, 0)).astype(np.int32)
    packed = (rng.normal(0, 1, (P, n)), rng.random((P, 4)), rng.random((P, 4)), rng.integers(0, 15000, P).astype(np.int32),
              rng.integers(0, 15000, P).astype(np.int32), st)
    init = dict(x=np.full((B, n), SENTINEL), costs4=np.full((B, 4), SENTINEL), costs4_last=np.full((B, 4), SENTINEL),
                nit=np.full(B, -9, np.int32), nfev=np.full(B, -9, np.int32), status=np.full(B, -9, np.int32),
                attempts=np.full(B, 40, np.int32), nit_total=np.full(B, 5_000_000_000, np.int64),
                solved=np.full(B, -9, np.int32))
    refs = {reset: merge_restated(B, sub, reset, *packed, init) for reset in (1, 0)}
    assert all(0 < len(lst) < P - 1 and bad == 1 for _, lst, bad in refs.values())
    return n, sub, packed, init, refs


def _grouped_merge(ctx, M, D, stride, reset, sub, packed, init):
    """neo_adaptive_merge_dev (clear_bad = 1) over the case as the one group of M - 1 waypoints, then
    neo_adaptive_compact_dev with the one segment [0, P): (request-indexed arrays, failed list, its length, bad word)"""
    torch, dev = _torch()
    B, P, G = MERGE_B, MERGE_P, _lib.NEO_MAX_PIECES
    d = {k: _dev(v) for k, v in init.items()}
    if stride != init["x"].shape[1]:
        d["x"] = torch.full((B, stride), SENTINEL, dtype=torch.float64, device=dev)
    ins = [_dev(a) for a in (sub,) + packed]
    d_lst = torch.full((P,), -3, dtype=torch.int32, device=dev)
    d_nf = torch.full((G,), -3, dtype=torch.int32, device=dev)
    d_bad = torch.full((1,), -3, dtype=torch.int32, device=dev)
    begin, lens = np.zeros(G, np.int32), np.zeros(G, np.int32)
    lens[M - 1] = P
    torch.cuda.synchronize(dev)
    ctx.check(ctx.lib.neo_adaptive_merge_dev(ctx.h, B, _p(ins[0]), P, M, D, stride, reset, 1, *[_p(t) for t in ins[1:]],
                                             *[_p(d[k]) for k in MERGED], _p(d_lst), _p(d_bad)))
    ctx.check(ctx.lib.neo_adaptive_compact_dev(ctx.h, _lib.ptr(begin), _lib.ptr(lens), _p(d_lst), _p(d_nf)))
    ctx.synchronize()
    nf = d_nf.cpu().numpy()
    assert np.all(np.delete(nf, M - 1) == 0)                    # (an empty segment: 0)
    return {k: v.cpu().numpy() for k, v in d.items()}, d_lst.cpu().numpy(), int(nf[M - 1]), int(d_bad.item())


@pytest.mark.parametrize("M, D", [(3, 2), (33, 3)])
def test_the_grouped_merge_is_the_fixed_merge(M, D):
    """neo_plan_merge_dev, and on copies of the same inputs neo_adaptive_merge_dev with x_stride = n and
    neo_adaptive_compact_dev over one segment: equal request-indexed arrays, failed list and count, bad-scene word --
    both the NumPy restatement's.  n = 7 and n = 129 (the x copy takes more than two strides of 64 lanes)"""
    torch, dev = _torch()
    ctx = _lib.default_context()
    n, sub, packed, init, refs = _merge_case(M, D)
    assert n == {3: 7, 33: 129}[M]
    B, P = MERGE_B, MERGE_P
    for reset in (1, 0):
        ref, ref_list, ref_bad = refs[reset]
        d = {k: _dev(v) for k, v in init.items()}
        ins = [_dev(a) for a in (sub,) + packed]
        d_lst = torch.full((P,), -3, dtype=torch.int32, device=dev)
        d_cnt = torch.full((2,), -3, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        ctx.check(ctx.lib.neo_plan_merge_dev(ctx.h, B, _p(ins[0]), P, M, D, reset, *[_p(t) for t in ins[1:]],
                                             *[_p(d[k]) for k in MERGED], _p(d_lst), _p(d_cnt[0:]), _p(d_cnt[1:])))
        ctx.synchronize()
        fixed = ({k: v.cpu().numpy() for k, v in d.items()}, d_lst.cpu().numpy()) + tuple(d_cnt.tolist())
        grouped = _grouped_merge(ctx, M, D, n, reset, sub, packed, init)
        for got, lst, nl, bad in (fixed, grouped):
            for k in MERGED:
                assert np.array_equal(got[k], ref[k]), (reset, k)       # bit for bit, the rows not launched included
            assert nl == len(ref_list) and np.array_equal(lst[:nl], ref_list) and bad == ref_bad, reset
        assert np.array_equal(fixed[1][:fixed[2]], grouped[1][:grouped[2]])


def test_the_merge_writes_x_in_rows_of_its_stride():
    """the (3, 2) case with x_stride = 10 over a sentinel x: columns 0 .. 6 of a launched request's row are its packed
    row, columns 7 .. 9 NaN; the rows of the skipped index and of the requests not listed keep the sentinel"""
    ctx = _lib.default_context()
    n, sub, packed, init, refs = _merge_case(3, 2)
    ref, ref_list, ref_bad = refs[1]
    got, lst, nl, bad = _grouped_merge(ctx, 3, 2, 10, 1, sub, packed, init)
    valid = (sub >= 0) & (sub < MERGE_B)
    on = np.zeros(MERGE_B, bool)
    on[sub[valid]] = True
    assert on.sum() == MERGE_P - 1
    assert np.array_equal(got["x"][sub[valid], :n], packed[0][valid]) and np.isnan(got["x"][on, n:]).all()
    assert np.all(got["x"][~on] == SENTINEL)
    for k in MERGED[1:]:
        assert np.array_equal(got[k], ref[k]), k
    assert nl == len(ref_list) and np.array_equal(lst[:nl], ref_list) and bad == ref_bad


# ------------------------------------------------------------------ 3. plan_dev against plan
PLAN_KEYS = ("x", "costs", "costs_last", "nit", "nfev", "status", "collision", "attempts", "nit_total", "solved")


def _as_plan(bufs, rows=None):
    """plan_dev's resident results in the form of plan's dict"""
    h = {k: bufs[k].cpu().numpy() for k in ("x", "costs", "costs_last", "nit", "nfev", "status", "attempts", "nit_total",
                                             "solved")}
    st = h["status"]
    out = dict(h, status=st & 0xff, collision=(st & _lib.NEO_TRAJ_FLAG_COLLISION) != 0, solved=h["solved"] != 0)
    return out if rows is None else {k: v[rows] for k, v in out.items()}


def _equal(got, ref):
    for k in PLAN_KEYS:
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k], equal_nan=True), k


@pytest.fixture(scope="module")
def planned(scenes, requests):
    """BatchPlanner.plan over R in both modes, once, and plan_dev over the same"""
    torch, dev = _torch()
    head, tail, sids, slots = requests
    out = {}
    for mode in ("f64", "f32x"):
        bp = npa.BatchPlanner(sample_dtype=mode)
        ref = bp.plan(scenes[1][0], head, tail, scene_ids=sids, seed=11, stream_ids=IDS, return_launch_sizes=True)
        d_head, d_tail, d_slots = _dev(head), _dev(tail), _dev(slots)
        torch.cuda.synchronize(dev)
        bufs = bp.plan_dev(scenes[1][0], d_head, d_tail, slots=d_slots, seed=11, stream_ids=IDS)
        out[mode] = (bp, ref, bufs, (d_head, d_tail, d_slots))
    return out


@pytest.mark.parametrize("mode", ["f64", "f32x"])
def test_plan_dev_is_plan_bit_for_bit(planned, mode, capsys):
    bp, ref, bufs, _ = planned[mode]
    hist = np.bincount(ref["attempts"], minlength=6).tolist()
    spent = int(((ref["attempts"] == 5) & ~ref["solved"]).sum())
    first = int(((ref["attempts"] == 1) & ref["solved"]).sum())
    with capsys.disabled():
        print(f"\n{mode}: requests by attempts {hist[1:]}, unsolved after all five {spent}, solved at the first {first}; "
              f"launch sizes {ref['launch_sizes']}")
    # the inputs exercise the chain: retries, a request that uses every attempt, and a majority that needs none
    assert (ref["attempts"] >= 2).sum() >= 3 and spent >= 1 and first >= 24
    assert ((ref["attempts"] >= 2) & ref["solved"]).sum() >= 2          # ... and retries that got somewhere
    _equal(_as_plan(bufs), ref)
    assert bufs["launch_sizes"] == ref["launch_sizes"] and len(ref["launch_sizes"]) == 5
    assert len(set(ref["launch_sizes"])) >= 3                            # the launch list shrinks from attempt to attempt


def test_plan_dev_over_a_subset_is_plan_over_those_requests(scenes, requests, planned):
    torch, dev = _torch()
    head, tail, sids, _ = requests
    bp, full, _, (d_head, d_tail, d_slots) = planned["f32x"]
    rng = np.random.default_rng(5)
    sub = rng.permutation(48)[:31]
    assert (full["attempts"][sub] >= 2).sum() >= 2
    ref = bp.plan(scenes[1][0], head[sub], tail[sub], scene_ids=sids[sub], seed=23, stream_ids=IDS[sub], return_launch_sizes=True)
    bufs = bp.plan_buffers(48, dev)
    for k in ("x", "costs", "costs_last"):
        bufs[k].fill_(SENTINEL)
    for k in ("nit", "nfev", "status", "attempts", "nit_total", "solved"):
        bufs[k].fill_(-9)
    d_sub = _dev(sub.astype(np.int32))
    torch.cuda.synchronize(dev)
    assert bp.plan_dev(scenes[1][0], d_head, d_tail, bufs=bufs, slots=d_slots, subset=d_sub, seed=23, stream_ids=IDS) is bufs
    _equal(_as_plan(bufs, sub), ref)
    assert bufs["launch_sizes"] == ref["launch_sizes"]
    rest = np.setdiff1d(np.arange(48), sub)
    assert np.all(bufs["x"].cpu().numpy()[rest] == SENTINEL) and np.all(bufs["costs_last"].cpu().numpy()[rest] == SENTINEL)
    for k in ("nit", "nfev", "status", "attempts", "nit_total", "solved"):
        assert np.all(bufs[k].cpu().numpy()[rest] == -9), k
    # the caller's own x and solved are written instead of the ones in bufs
    own_x = torch.full((48, 7), SENTINEL, dtype=torch.float64, device=dev)
    own_s = torch.full((48,), -9, dtype=torch.int32, device=dev)
    before = bufs["x"].clone()
    torch.cuda.synchronize(dev)
    bp.plan_dev(scenes[1][0], d_head, d_tail, bufs=bufs, slots=d_slots, subset=d_sub, x=own_x, solved=own_s, seed=23, stream_ids=IDS)
    assert torch.equal(bufs["x"], before) and np.array_equal(own_x.cpu().numpy()[sub], ref["x"])
    assert np.array_equal(own_s.cpu().numpy()[sub] != 0, ref["solved"]) and np.all(own_s.cpu().numpy()[rest] == -9)


def test_plan_dev_over_an_empty_subset_plans_nothing(scenes, planned):
    """the fixed form with a subset of no entries: the same bufs come back, every result as it was, and one launch of
    size 0 on record (the guess and the merge are called for the empty list, the optimiser is not)"""
    torch, dev = _torch()
    bp, _, _, (d_head, d_tail, d_slots) = planned["f32x"]
    bufs = bp.plan_buffers(48, dev)
    keys = ("x", "costs", "costs_last", "nit", "nfev", "status", "attempts", "nit_total", "solved")
    for k in keys:
        bufs[k].fill_(SENTINEL if bufs[k].dtype == torch.float64 else -9)
    for k in ("x_k", "costs_k", "last_k"):
        bufs[k].fill_(-SENTINEL)            # (what a merge of rows that were never launched would bring over)
    before = {k: bufs[k].clone() for k in keys}
    empty = torch.zeros((0,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    assert bp.plan_dev(scenes[1][0], d_head, d_tail, bufs=bufs, slots=d_slots, subset=empty, seed=23, stream_ids=IDS) is bufs
    for k in keys:
        assert torch.equal(bufs[k], before[k]), k
    assert bufs["launch_sizes"] == [0]


def test_plan_dev_from_a_callers_first_guess_is_plan_with_int_wpts(scenes, requests, planned):
    torch, dev = _torch()
    head, tail, sids, _ = requests
    bp, _, _, (d_head, d_tail, d_slots) = planned["f64"]
    cand, ts = bp.batch_init_guess(head, tail, K=2)               # the guess shifted sideways by 0.6 m
    ts = np.tile(ts, (48, 1))
    ref = bp.plan(scenes[1][0], head, tail, int_wpts=cand[:, 1], ts=ts, scene_ids=sids, seed=31, stream_ids=IDS,
                  return_launch_sizes=True)
    assert (ref["attempts"] >= 2).sum() >= 3
    d_x0 = _dev(bp.pack_x(cand[:, 1], ts))
    torch.cuda.synchronize(dev)
    bufs = bp.plan_dev(scenes[1][0], d_head, d_tail, x0=d_x0, slots=d_slots, seed=31, stream_ids=IDS)
    _equal(_as_plan(bufs), ref)
    assert bufs["launch_sizes"] == ref["launch_sizes"]
    assert torch.equal(d_x0, _dev(bp.pack_x(cand[:, 1], ts)))      # x0 is only read


# ------------------------------------------------------------------ 4. independence
def test_a_request_planned_alone_equals_its_row_in_the_batch(scenes, requests, planned):
    torch, dev = _torch()
    bp, ref, _, (d_head, d_tail, d_slots) = planned["f64"]
    spent = np.flatnonzero((ref["attempts"] == 5) & ~ref["solved"])
    retried = np.flatnonzero((ref["attempts"] >= 2) & ref["solved"])
    first = np.flatnonzero(ref["attempts"] == 1)
    assert retried.size >= 2
    picks = [int(spent[0]), int(first[0]), int(retried[0]), int(retried[-1])]
    for i in picks:
        one = bp.plan_dev(scenes[1][0], d_head[i:i + 1].clone(), d_tail[i:i + 1].clone(), slots=d_slots[i:i + 1].clone(),
                          seed=11, stream_ids=IDS[i:i + 1])
        _equal(_as_plan(one), {k: ref[k][i:i + 1] for k in PLAN_KEYS})
        assert one["launch_sizes"] == [1] * int(ref["attempts"][i])


# ------------------------------------------------------------------ 5. fleet
@pytest.mark.parametrize("mode", ["basic", "batch"])
def test_the_resident_fleet_flies_the_host_fleets_flights(scenes, mode, capsys):
    maps = [scenes[1][0], scenes[2][0]]
    start, goals, sids = draw_missions(maps, 12, seed=3)
    runs = {}
    for resident in (False, True):
        loop = npa.FleetReplanLoop(npa.BatchPlanner(), maps[0], goals, mode=mode, scene_ids=sids, seed=5,
                                   mission_ids=np.arange(24) + 100, resident=resident)
        runs[resident] = (loop, loop.run(start, max_replans=6))
    (host_loop, host), (res_loop, res) = runs[False], runs[True]
    retries = int((host["opt_runs"] - (3 if mode == "batch" else 1) * (host["replans"] + host["failed_attempts"])).sum())
    with capsys.disabled():
        print(f"\n{mode}: plans {int(host['replans'].sum())}, failed attempts {int(host['failed_attempts'].sum())}, optimiser "
              f"runs beyond the first of a plan {retries + int(host_loop.uncounted_candidates.sum())}")
    assert host["replans"].sum() >= 24 * 4
    assert res_loop._plan is not None and host_loop._plan is None        # the resident chain ran, and only there
    assert set(res) == set(host)
    for k in host:
        assert np.array_equal(np.asarray(res[k]), np.asarray(host[k]), equal_nan=True), k
    for i in range(24):
        assert np.array_equal(res_loop.commands(i), host_loop.commands(i)), i
    assert np.array_equal(res_loop.uncounted_candidates, host_loop.uncounted_candidates)


# ------------------------------------------------------------------ 6. argument errors
def test_plan_dev_argument_errors(scenes, requests, planned):
    torch, dev = _torch()
    bp, _, _, (d_head, d_tail, d_slots) = planned["f64"]
    m = scenes[1][0]
    with pytest.raises(ValueError):
        bp.plan_dev(m, d_head, d_tail, bufs=bp.plan_buffers(47, dev))
    with pytest.raises(ValueError):
        bp.plan_dev(m, d_head, d_tail, bufs=bp.plan_buffers(48, dev, waypoints=3))
    with pytest.raises(ValueError):
        bp.plan_dev(m, d_head, d_tail, stream_ids=np.arange(47))
    bad = d_slots.clone()
    bad[7] = 99                                                   # a map-table slot without a map
    torch.cuda.synchronize(dev)
    with pytest.raises(_lib.NeoError):
        bp.plan_dev(m, d_head, d_tail, slots=bad, seed=11, stream_ids=IDS)
    bp.plan_dev(m, d_head[:4].clone(), d_tail[:4].clone(), slots=d_slots[:4].clone(), seed=11)   # the context stays usable
    ctx = bp.ctx
    L = ctx.lib
    h = np.zeros((4, 3, 2)); x = np.zeros((4, 7)); i4 = np.zeros(4, np.int32); c4 = np.zeros((4, 4)); f = np.zeros(2); tau = np.zeros(3)
    guess = lambda M=3, D=2, head=_lib.ptr(h), frac=_lib.ptr(f), n_sub=0, sub=None: L.neo_plan_guess(
        ctx.h, 4, sub, n_sub, M, D, head, _lib.ptr(h), None, None, None, frac, _lib.ptr(tau), _lib.ptr(x), _lib.ptr(h.copy()),
        _lib.ptr(h.copy()), None)
    assert guess() == 0
    for kw in (dict(D=4), dict(D=1), dict(M=1), dict(head=None), dict(frac=None), dict(n_sub=5, sub=_lib.ptr(np.zeros(5, np.int32)))):
        assert guess(**kw) == INVALID and L.neo_last_error(ctx.h)
    i8 = np.zeros(4, np.int64)
    merge = lambda M=3, D=2, lst=_lib.ptr(i4.copy()), bad_word=_lib.ptr(np.zeros(1, np.int32)): L.neo_plan_merge(
        ctx.h, 4, None, 0, M, D, 1, _lib.ptr(x), _lib.ptr(c4), _lib.ptr(c4), _lib.ptr(i4), _lib.ptr(i4), _lib.ptr(i4),
        _lib.ptr(x.copy()), _lib.ptr(c4.copy()), _lib.ptr(c4.copy()), _lib.ptr(i4.copy()), _lib.ptr(i4.copy()),
        _lib.ptr(i4.copy()), _lib.ptr(i4.copy()), _lib.ptr(i8), _lib.ptr(i4.copy()), lst, _lib.ptr(np.zeros(1, np.int32)), bad_word)
    assert merge() == 0
    for kw in (dict(D=4), dict(M=1), dict(lst=None), dict(bad_word=None)):
        assert merge(**kw) == INVALID and L.neo_last_error(ctx.h)
