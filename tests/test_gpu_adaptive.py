"""Adaptive waypoint counts on the GPU (neo_adaptive_*, BatchPlanner.plan / plan_dev with waypoints="adaptive"): the count
kernel against BatchPlanner.adaptive_counts bit for bit, the bucket kernel against NumPy's stable argsort, the segmented
compaction against NumPy, plan_dev against plan in every returned array (NaN padding included), a request alone against
its row of the batch, subsets, the number of host waits, the clamp and the C ABI's errors."""
import numpy as np
import pytest

import neo_planner_amd as npa
from neo_planner_amd import _lib, synth

pytestmark = pytest.mark.gpu

SENTINEL = 777.0
INVALID = 1          # NEO_ERR_INVALID
G = _lib.NEO_MAX_PIECES
SCENES = (1, 7)      # the two maps of the plan tests
REQ_SEED = 5         # the requests' draw (synth.replan_requests)
SEED = 11            # the retries' streams
IDS = np.arange(48) * 3 + 500          # the requests' stream ids: not their positions


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _dev(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope="module")
def ctx():
    """a context of this module's own: its maps do not shift the map-table slots other modules' tests count on"""
    c = _lib.Context(0)
    yield c
    c.close()


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


# ------------------------------------------------------------------ 1. the count kernel
def _count_requests(rng, B, D):
    """random requests 0 .. 40 m long with the edge cases in front: lengths on the lattice and one double above, zero
    length, NaN, infinity, a square that overflows, a length that clamps"""
    head = np.zeros((B, 3, D)); tail = np.zeros((B, 3, D))
    head[:, 0] = rng.uniform(-10.0, 10.0, (B, D))
    u = rng.normal(size=(B, D)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    tail[:, 0] = head[:, 0] + u * rng.uniform(0.0, 40.0, (B, 1))
    head[:12, 0] = 0.0
    tail[:12, 0] = 0.0
    up = np.nextafter(4.0, 5.0)
    for k, (a, b) in enumerate([(4, 0), (up, 0), (0, up), (3, 4), (6, 8), (0, 0), (np.nan, 1), (np.inf, 0), (1e200, 1e200),
                                (130, 0), (1e150, 0), (128, 0)]):
        tail[k, 0, 0], tail[k, 0, 1] = a, b
    head[:, 1:] = rng.normal(size=(B, 2, D)); tail[:, 1:] = rng.normal(size=(B, 2, D))      # (velocities are not read)
    return head, tail


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("seg,max_w", [(2.0, 63), (0.5, 63), (3.0, 5)])
def test_count_kernel_equals_the_model_bit_for_bit(ctx, D, seg, max_w):
    torch, dev = _torch()
    B = 4099
    bp = npa.BatchPlanner(npa.PlannerConfig(init_seg_len=seg))
    head, tail = _count_requests(np.random.default_rng([21, D]), B, D)
    ref, ref_cl = bp.adaptive_counts(head, tail, max_w)
    assert ref[:12].tolist() == bp.adaptive_counts(head[:12], tail[:12], max_w)[0].tolist()
    if (seg, max_w) == (2.0, 63):
        assert ref[:12].tolist() == [1, 2, 2, 2, 4, 1, 1, 1, 1, 63, 63, 63] and ref_cl[:12].tolist() == [False] * 9 + [True, True, False]
        assert len(set(ref.tolist())) >= 15
    assert ref_cl.any() and not ref_cl.all()
    counts = np.full(B, -7, np.int32); clamped = np.full(B, -7, np.int32)
    ctx.check(ctx.lib.neo_adaptive_count(ctx.h, B, None, 0, D, _lib.ptr(head), _lib.ptr(tail), seg, max_w, _lib.ptr(counts), _lib.ptr(clamped)))
    assert np.array_equal(counts, ref) and np.array_equal(clamped, ref_cl.astype(np.int32))
    # the device form over a subset with -1, B and a repeated valid index: listed rows are written, the others stay
    sub = np.concatenate([[-1, B, 5, 5, 0, B - 1], np.random.default_rng(3).permutation(B)[:700]]).astype(np.int32)
    listed = np.unique(sub[(sub >= 0) & (sub < B)])
    rest = np.setdiff1d(np.arange(B), listed)
    d_counts = torch.full((B,), -7, dtype=torch.int32, device=dev); d_cl = torch.full((B,), -7, dtype=torch.int32, device=dev)
    d_head, d_tail, d_sub = _dev(head), _dev(tail), _dev(sub)
    torch.cuda.synchronize(dev)
    p = _lib.dev_ptr
    ctx.check(ctx.lib.neo_adaptive_count_dev(ctx.h, B, p(d_sub), sub.size, D, p(d_head), p(d_tail), seg, max_w, p(d_counts), p(d_cl)))
    ctx.check(ctx.lib.neo_adaptive_count_dev(ctx.h, B, p(d_sub), 0, D, p(d_head), p(d_tail), seg, max_w, p(d_counts), p(d_cl)))   # empty: no-op
    ctx.synchronize()
    got, got_cl = d_counts.cpu().numpy(), d_cl.cpu().numpy()
    assert np.array_equal(got[listed], ref[listed]) and np.array_equal(got_cl[listed], ref_cl[listed].astype(np.int32))
    assert np.all(got[rest] == -7) and np.all(got_cl[rest] == -7)
    # the host form with an empty subset writes nothing either
    counts[:] = -7
    ctx.check(ctx.lib.neo_adaptive_count(ctx.h, B, _lib.ptr(sub), 0, D, _lib.ptr(head), _lib.ptr(tail), seg, max_w, _lib.ptr(counts), _lib.ptr(clamped)))
    assert np.all(counts == -7)


# ------------------------------------------------------------------ 2. the bucket kernel
def _bucket_ref(counts, lst, B):
    """np.argsort(counts[list], kind="stable") restricted to the valid indices with a count the table has a group for"""
    lst = np.asarray(lst)
    valid = lst[(lst >= 0) & (lst < B)]
    valid = valid[(counts[valid] >= 0) & (counts[valid] < G)]
    order = valid[np.argsort(counts[valid], kind="stable")]
    begin = np.concatenate([[0], np.cumsum(np.bincount(counts[valid], minlength=G))])
    return order.astype(np.int32), begin.astype(np.int32)


def _bucket(c, B, sub, n_sub, counts, rows):
    order = np.full(rows, -5, np.int32); begin = np.full(G + 1, -5, np.int32); total = np.full(1, -5, np.int32)
    c.check(c.lib.neo_adaptive_bucket(c.h, B, _lib.ptr(sub), n_sub, _lib.ptr(counts), _lib.ptr(order), _lib.ptr(begin), _lib.ptr(total)))
    return order, begin, int(total[0])


@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, 1023, 1024, 1025, 4099])
def test_bucket_kernel_is_the_stable_argsort(ctx, P):
    rng = np.random.default_rng([8, P])
    B = P + 9
    patterns = dict(one=np.full(B, 17), each=1 + np.arange(B) % 63, random=rng.integers(1, 64, B), descending=63 - np.arange(B) % 63,
                    two_runs=np.repeat([40, 3], [B // 2, B - B // 2]))
    for name, counts in patterns.items():
        counts = _i32(counts)
        for skipped in (False, True):
            sub = rng.permutation(B)[:max(P, 1)].astype(np.int32)     # the list's order is not the requests'; P of it count
            cnt = counts.copy()
            if skipped and P > 0:
                sub[rng.integers(0, P, max(P // 7, 1))] = rng.choice([-1, B, B + 100, -2 ** 31], max(P // 7, 1))
                sub[P // 2] = sub[0]                                  # a repeated index keeps both places
                cnt[rng.integers(0, B, max(B // 9, 1))] = rng.choice([0, 64, -3, 1000], max(B // 9, 1))   # 0: a group; the others: dropped
            ref_order, ref_begin = _bucket_ref(cnt, sub[:P], B)
            order, begin, total = _bucket(ctx, B, sub, P, cnt, max(P, 1))
            kept = ref_order.size
            assert total == kept == begin[G] and np.array_equal(begin, ref_begin), (name, skipped)
            assert np.array_equal(order[:kept], ref_order) and np.all(order[kept:] == -5), (name, skipped)
            again = _bucket(ctx, B, sub, P, cnt, max(P, 1))             # the same input: the same output
            assert np.array_equal(again[0], order) and np.array_equal(again[1], begin) and again[2] == total
    if P > 0:       # without a subset: position p is request p; at P = 63 every count 1 .. 63 exactly once
        counts = _i32(rng.permutation(63) + 1 if P == 63 else rng.integers(1, 64, P))
        order, begin, total = _bucket(ctx, P, None, 0, counts, P)
        assert total == P and np.array_equal(order, np.argsort(counts, kind="stable")) and np.array_equal(begin, _bucket_ref(counts, np.arange(P), P)[1])


def test_bucket_kernel_on_resident_arrays(ctx):
    torch, dev = _torch()
    p = _lib.dev_ptr
    rng = np.random.default_rng(17)
    B, P = 3000, 2100
    counts = _i32(rng.integers(1, 64, B)); sub = rng.permutation(B)[:P].astype(np.int32)
    d_counts, d_sub = _dev(counts), _dev(sub)
    d_order = torch.full((P,), -5, dtype=torch.int32, device=dev); d_table = torch.full((G + 2,), -5, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.check(ctx.lib.neo_adaptive_bucket_dev(ctx.h, B, p(d_sub), P, p(d_counts), p(d_order), p(d_table), p(d_table[G + 1:])))
    ctx.synchronize()
    ref_order, ref_begin = _bucket_ref(counts, sub, B)
    assert np.array_equal(d_order.cpu().numpy(), ref_order) and np.array_equal(d_table.cpu().numpy(), np.append(ref_begin, P))
    ctx.check(ctx.lib.neo_adaptive_bucket_dev(ctx.h, B, p(d_sub), 0, p(d_counts), p(d_order), p(d_table), p(d_table[G + 1:])))   # an empty list
    ctx.synchronize()
    assert not d_table.cpu().numpy().any() and np.array_equal(d_order.cpu().numpy(), ref_order)


# ------------------------------------------------------------------ 3. the segmented compaction
def test_compact_kernel_packs_every_segment_in_place(ctx):
    rng = np.random.default_rng(4)
    lens = np.zeros(G, np.int32)
    lens[[1, 2, 5, 6, 9, 20, 40, 63]] = [1, 255, 256, 257, 1000, 0, 513, 3]
    begin = np.zeros(G, np.int32)
    begin[1:] = np.cumsum(lens + 2)[:-1]                              # two rows between the segments: they must stay
    rows = int(begin[-1] + lens[-1] + 2)
    pending = np.full(rows, -1, np.int32)
    want = pending.copy(); n_want = np.zeros(G, np.int32)
    for g in range(G):
        seg = np.where(rng.random(lens[g]) < 0.4, rng.integers(0, 10 ** 6, lens[g]), -1).astype(np.int32)
        pending[begin[g]:begin[g] + lens[g]] = seg
        pending[begin[g] + lens[g]:begin[g] + lens[g] + 2] = -77
        n_want[g] = (seg >= 0).sum()
        want[begin[g]:begin[g] + n_want[g]] = seg[seg >= 0]
    gaps = pending == -77
    n_failed = np.full(G, -5, np.int32)
    ctx.check(ctx.lib.neo_adaptive_compact(ctx.h, _lib.ptr(begin), _lib.ptr(lens), rows, _lib.ptr(pending), _lib.ptr(n_failed)))
    assert np.array_equal(n_failed, n_want) and n_want[9] > 300 and n_want[20] == 0
    for g in range(G):
        assert np.array_equal(pending[begin[g]:begin[g] + n_want[g]], want[begin[g]:begin[g] + n_want[g]]), g
    assert np.all(pending[gaps] == -77)


# ------------------------------------------------------------------ 4. plan_dev against plan
PLAN_KEYS = ("x", "costs", "costs_last", "nit", "nfev", "status", "collision", "attempts", "nit_total", "solved", "counts", "clamped")
RESIDENT = ("x", "costs", "costs_last", "nit", "nfev", "status", "attempts", "nit_total", "solved", "counts", "clamped")


def _as_plan(bufs, rows=None):
    """plan_dev's resident results in the form of plan's dict"""
    h = {k: bufs[k].cpu().numpy() for k in RESIDENT}
    st = h["status"]
    out = dict(h, status=st & 0xff, collision=(st & _lib.NEO_TRAJ_FLAG_COLLISION) != 0, solved=h["solved"] != 0, clamped=h["clamped"] != 0)
    return out if rows is None else {k: v[rows] for k, v in out.items()}


def _same(a, b):
    """two resident arrays hold the same values (a ragged x holds NaN)"""
    return np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)


def _equal(got, ref, rows=None):
    for k in PLAN_KEYS:
        r = ref[k] if rows is None else ref[k][rows]
        assert got[k].dtype == r.dtype and got[k].shape == r.shape and np.array_equal(got[k], r, equal_nan=True), k


def _ragged(res):
    """the NaN padding is where the counts say, and nowhere else"""
    n = res["x"].shape[1]
    D = 2
    own = (D + 1) * res["counts"] + 1
    assert np.array_equal(np.isnan(res["x"]), np.arange(n)[None, :] >= own[:, None])


@pytest.fixture(scope="module")
def scenes(ctx):
    out = {}
    for s in SCENES:
        m = npa.ESDF(ctx=ctx)
        m.occupancy_map_cb(synth.OccupancyGridMsg(synth.occupancy_2d(s)))
        out[s] = m
    return out


@pytest.fixture(scope="module")
def requests(ctx, scenes):
    """48 requests 1 to 13 m long (counts 1 to 6), 24 on each map, drawn as synth draws them: goals anywhere, also
    inside an inflated obstacle -- some fail by design"""
    parts = [synth.replan_requests(REQ_SEED + k, 24, 1, D=2, length_range=(1.0, 13.0), y_range=(-5.0, 5.0)) for k in range(2)]
    head = np.concatenate([q[0] for q in parts]); tail = np.concatenate([q[1] for q in parts])
    head[:, 0, 0] += np.repeat([4.0, 9.0], 24)                 # into the forest
    tail[:, 0, 0] += np.repeat([4.0, 9.0], 24)
    sids = np.array([scenes[s].scene_id for s in np.repeat(SCENES, 24)], np.int32)
    slots = np.array([ctx.lib.neo_scene_slot(ctx.h, int(s)) for s in sids], np.int32)
    return head, tail, sids, slots


@pytest.fixture(scope="module")
def planned(ctx, scenes, requests):
    """plan and plan_dev with waypoints="adaptive" over the 48 requests: both jitters, on the two maps (slots) and on
    one map (no slots)"""
    torch, dev = _torch()
    head, tail, sids, slots = requests
    bp = npa.BatchPlanner(ctx=ctx)
    dv = (_dev(head), _dev(tail), _dev(slots))
    torch.cuda.synchronize(dev)
    out = dict(bp=bp, dev=dv)
    for jitter in ("numpy", "counter"):
        for two_maps in (True, False):
            ref = bp.plan(scenes[SCENES[0]], head, tail, waypoints="adaptive", scene_ids=sids if two_maps else None, seed=SEED,
                          stream_ids=IDS, jitter=jitter, return_launch_sizes=True)
            bufs = bp.plan_dev(scenes[SCENES[0]], dv[0], dv[1], waypoints="adaptive", slots=dv[2] if two_maps else None, seed=SEED,
                               stream_ids=IDS, jitter=jitter)
            out[jitter, two_maps] = (ref, bufs)
    return out


@pytest.mark.parametrize("two_maps", [True, False])
@pytest.mark.parametrize("jitter", ["numpy", "counter"])
def test_plan_dev_is_plan_bit_for_bit(planned, requests, jitter, two_maps, capsys):
    ref, bufs = planned[jitter, two_maps]
    retried = sorted(set(ref["counts"][ref["attempts"] >= 2].tolist()))
    with capsys.disabled():
        print(f"\n{jitter}, two maps {two_maps}: counts {np.bincount(ref['counts']).tolist()}, counts with a retry {retried}, solved "
              f"{int(ref['solved'].sum())} of 48, attempts {np.bincount(ref['attempts'], minlength=6)[1:].tolist()}, launch sizes "
              f"{ref['launch_sizes']}, by group {ref['group_launch_sizes']}")
    assert np.array_equal(ref["counts"], npa.BatchPlanner().adaptive_counts(requests[0], requests[1])[0])
    assert ref["counts"].min() == 1 and ref["counts"].max() == 6 and not ref["clamped"].any()
    # the inputs exercise the chain: retries in at least two groups, a request that ends solved and one that does not
    assert len(retried) >= 2 and ref["solved"].any() and not ref["solved"].all()
    _ragged(ref)
    _equal(_as_plan(bufs), ref)
    assert bufs["launch_sizes"] == ref["launch_sizes"] and bufs["group_launch_sizes"] == ref["group_launch_sizes"]
    assert bufs["max_waypoints"] == ref["max_waypoints"] == 63 and ref["x"].shape == (48, 2 * 63 + 63 + 1)
    # group by group, a uniform-M consumer gets the same dense rows from either form
    for a, b in zip(npa.BatchPlanner.adaptive_groups(ref), npa.BatchPlanner.adaptive_groups(bufs)):
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.isfinite(a[2]).all()


def test_an_adaptive_group_is_the_fixed_plan_of_its_requests(planned, scenes, requests):
    """what a user had before: plan(waypoints=c) over the requests of one count gives their rows"""
    head, tail, sids, _ = requests
    ref, _ = planned["numpy", True]
    bp = planned["bp"]
    c = int(np.bincount(ref["counts"]).argmax())
    g = np.flatnonzero(ref["counts"] == c)
    one = bp.plan(scenes[SCENES[0]], head[g], tail[g], waypoints=c, scene_ids=sids[g], seed=SEED, stream_ids=IDS[g])
    n = 3 * c + 1
    assert np.array_equal(one["x"], ref["x"][g, :n]) and np.array_equal(one["attempts"], ref["attempts"][g])
    assert np.array_equal(one["costs"], ref["costs"][g])


def test_the_host_waits_once_per_attempt(planned):
    for key in (("numpy", True), ("counter", True), ("counter", False)):
        ref, bufs = planned[key]
        attempts_run = len(bufs["launch_sizes"])
        issued = sum(len(v) for v in bufs["group_launch_sizes"].values())
        assert attempts_run >= 2 and len(bufs["group_launch_sizes"]) >= 4 and issued > attempts_run
        assert bufs["host_waits"] == dict(grouping=1, attempts=attempts_run)       # not groups x attempts
        assert attempts_run == int(ref["attempts"].max())


def test_a_group_beyond_1024_rows_is_dispatched_by_effort_and_equals_the_host_form(ctx, scenes):
    """1100 requests of one count and 40 of another: the large group takes plan_dev's effort-order path (more than 1024
    rows), its retries do not; two attempts"""
    torch, dev = _torch()
    a = synth.replan_requests(31, 1100, 1, D=2, length_range=(4.1, 5.9), y_range=(-5.0, 5.0))
    b = synth.replan_requests(32, 40, 1, D=2, length_range=(8.1, 9.9), y_range=(-5.0, 5.0))
    head = np.concatenate([a[0], b[0]]); tail = np.concatenate([a[1], b[1]])
    head[:, 0, 0] += 4.0; tail[:, 0, 0] += 4.0
    order = np.random.default_rng(2).permutation(1140)               # the groups interleaved in the batch
    head, tail = np.ascontiguousarray(head[order]), np.ascontiguousarray(tail[order])
    bp = npa.BatchPlanner(ctx=ctx)
    m = scenes[SCENES[0]]
    ref = bp.plan(m, head, tail, waypoints="adaptive", max_attempts=2, seed=SEED, jitter="counter", return_launch_sizes=True)
    assert np.bincount(ref["counts"]).tolist() == [0, 0, 1100, 0, 40]
    sizes = ref["group_launch_sizes"]
    assert sizes[2][0] == 1100 and 0 < sizes[2][1] <= 1024 and len(sizes[4]) == 2 and ref["solved"].any()
    d_head, d_tail = _dev(head), _dev(tail)
    torch.cuda.synchronize(dev)
    bufs = bp.plan_dev(m, d_head, d_tail, waypoints="adaptive", max_waypoints=6, max_attempts=2, seed=SEED, jitter="counter")
    got = _as_plan(bufs)
    assert got["x"].shape == (1140, 19) and np.array_equal(got["x"], ref["x"][:, :19], equal_nan=True) and np.isnan(ref["x"][:, 19:]).all()
    for k in PLAN_KEYS[1:]:
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), k
    assert bufs["launch_sizes"] == ref["launch_sizes"] and bufs["group_launch_sizes"] == sizes
    assert bufs["host_waits"] == dict(grouping=1, attempts=2)


# ------------------------------------------------------------------ 5. independence
@pytest.mark.parametrize("jitter", ["numpy", "counter"])
def test_a_request_planned_alone_equals_its_row_in_the_batch(planned, scenes, jitter):
    bp, (d_head, d_tail, d_slots) = planned["bp"], planned["dev"]
    ref, _ = planned[jitter, True]
    retried = np.flatnonzero(ref["attempts"] >= 2)
    first = np.flatnonzero(ref["attempts"] == 1)
    picks = list(dict.fromkeys(retried[np.argsort(ref["counts"][retried], kind="stable")][[0, -1, len(retried) // 2]].tolist()
                               + first[np.argsort(ref["counts"][first], kind="stable")][[0, -1]].tolist() + [0, 24, 47, 13, 30]))[:8]
    assert len(picks) == 8 and len(set(ref["counts"][picks].tolist())) >= 3
    for i in picks:
        one = bp.plan_dev(scenes[SCENES[0]], d_head[i:i + 1].clone(), d_tail[i:i + 1].clone(), slots=d_slots[i:i + 1].clone(),
                          waypoints="adaptive", seed=SEED, stream_ids=IDS[i:i + 1], jitter=jitter)
        _equal(_as_plan(one), ref, rows=slice(i, i + 1))
        assert one["launch_sizes"] == [1] * int(ref["attempts"][i])


# ------------------------------------------------------------------ 6. subsets, the caller's own arrays
def test_plan_dev_over_a_subset_leaves_the_other_requests_alone(planned, scenes, requests):
    torch, dev = _torch()
    head, tail, sids, _ = requests
    bp, (d_head, d_tail, d_slots) = planned["bp"], planned["dev"]
    full, _ = planned["counter", True]
    sub = np.random.default_rng(5).permutation(48)[:24]
    assert len(set(full["counts"][sub][full["attempts"][sub] >= 2].tolist())) >= 2
    ref = bp.plan(scenes[SCENES[0]], head[sub], tail[sub], waypoints="adaptive", scene_ids=sids[sub], seed=23, stream_ids=IDS[sub],
                  jitter="counter", return_launch_sizes=True)
    bufs = bp.plan_buffers(48, dev, waypoints="adaptive")
    for k in ("x", "costs", "costs_last"):
        bufs[k].fill_(SENTINEL)
    for k in ("nit", "nfev", "status", "attempts", "nit_total", "solved", "counts", "clamped"):
        bufs[k].fill_(-9)
    d_sub = _dev(sub.astype(np.int32))
    torch.cuda.synchronize(dev)
    kw = dict(bufs=bufs, slots=d_slots, subset=d_sub, waypoints="adaptive", seed=23, stream_ids=IDS, jitter="counter")
    assert bp.plan_dev(scenes[SCENES[0]], d_head, d_tail, **kw) is bufs
    _equal(_as_plan(bufs, sub), ref)
    assert bufs["launch_sizes"] == ref["launch_sizes"] and bufs["group_launch_sizes"] == ref["group_launch_sizes"]
    rest = np.setdiff1d(np.arange(48), sub)
    for k in ("x", "costs", "costs_last"):
        assert np.all(bufs[k].cpu().numpy()[rest] == SENTINEL), k
    for k in ("nit", "nfev", "status", "attempts", "nit_total", "solved", "counts", "clamped"):
        assert np.all(bufs[k].cpu().numpy()[rest] == -9), k
    dense = {int(c): (idx, xd) for c, idx, xd in npa.BatchPlanner.adaptive_groups(bufs, rows=sub)}
    assert sorted(np.concatenate([v[0] for v in dense.values()]).tolist()) == sorted(sub.tolist())
    # the caller's own x and solved are written instead of the ones in bufs
    own_x = torch.full((48, 190), SENTINEL, dtype=torch.float64, device=dev)
    own_s = torch.full((48,), -9, dtype=torch.int32, device=dev)
    before = bufs["x"].clone()
    torch.cuda.synchronize(dev)
    bp.plan_dev(scenes[SCENES[0]], d_head, d_tail, x=own_x, solved=own_s, **kw)
    assert _same(bufs["x"], before)
    assert np.array_equal(own_x.cpu().numpy()[sub], ref["x"], equal_nan=True) and np.all(own_x.cpu().numpy()[rest] == SENTINEL)
    assert np.array_equal(own_s.cpu().numpy()[sub] != 0, ref["solved"]) and np.all(own_s.cpu().numpy()[rest] == -9)
    # an empty subset plans nothing
    empty = torch.zeros((0,), dtype=torch.int32, device=dev)
    snapshot = {k: bufs[k].clone() for k in RESIDENT}
    torch.cuda.synchronize(dev)
    bp.plan_dev(scenes[SCENES[0]], d_head, d_tail, **dict(kw, subset=empty))
    assert bufs["launch_sizes"] == [] and bufs["host_waits"] == dict(grouping=0, attempts=0)
    assert all(_same(bufs[k], snapshot[k]) for k in RESIDENT)


# ------------------------------------------------------------------ 7. the clamp
def test_a_clamped_batch_equals_the_host_form(planned, scenes, requests):
    head, tail, sids, _ = requests
    bp, (d_head, d_tail, d_slots) = planned["bp"], planned["dev"]
    free, _ = planned["counter", True]
    ref = bp.plan(scenes[SCENES[0]], head, tail, waypoints="adaptive", max_waypoints=3, scene_ids=sids, seed=SEED, stream_ids=IDS,
                  jitter="counter", return_launch_sizes=True)
    assert np.array_equal(ref["clamped"], free["counts"] > 3) and 5 <= ref["clamped"].sum() <= 43
    assert np.array_equal(ref["counts"], np.minimum(free["counts"], 3)) and ref["x"].shape == (48, 10)
    _ragged(ref)
    bufs = bp.plan_dev(scenes[SCENES[0]], d_head, d_tail, slots=d_slots, waypoints="adaptive", max_waypoints=3, seed=SEED,
                       stream_ids=IDS, jitter="counter")
    _equal(_as_plan(bufs), ref)
    assert bufs["launch_sizes"] == ref["launch_sizes"] and sorted(bufs["group_launch_sizes"]) == [1, 2, 3]
    same = free["counts"] <= 3                                      # a request the clamp does not touch plans as before
    assert np.array_equal(ref["x"][same, :10], free["x"][same, :10], equal_nan=True) and np.isnan(free["x"][same, 10:]).all()


# ------------------------------------------------------------------ 8. the C ABI's errors
def test_c_abi_errors_come_back_before_any_launch(ctx):
    torch, dev = _torch()
    L, p, q = ctx.lib, _lib.dev_ptr, _lib.ptr
    B = 6
    head = np.zeros((B, 3, 2)); tail = np.ones((B, 3, 2))
    counts = np.full(B, -7, np.int32); clamped = np.full(B, -7, np.int32); sub = np.arange(B, dtype=np.int32)
    count = lambda B=B, sub=None, n_sub=0, D=2, head=q(head), tail=q(tail), seg=2.0, w=63, counts=q(counts), clamped=q(clamped): \
        L.neo_adaptive_count(ctx.h, B, sub, n_sub, D, head, tail, seg, w, counts, clamped)
    for kw in (dict(B=0), dict(B=-1), dict(D=1), dict(D=4), dict(w=0), dict(w=64), dict(seg=0.0), dict(seg=-1.0), dict(seg=float("inf")),
               dict(seg=float("nan")), dict(head=None), dict(tail=None), dict(counts=None), dict(clamped=None),
               dict(sub=q(sub), n_sub=B + 1), dict(sub=q(sub), n_sub=-1)):
        assert count(**kw) == INVALID and L.neo_last_error(ctx.h), kw
    assert np.all(counts == -7) and np.all(clamped == -7)
    assert count() == 0 and np.all(counts == 1) and not clamped.any()
    d_head, d_tail = _dev(head), _dev(tail)
    d_counts = torch.full((B,), -7, dtype=torch.int32, device=dev); d_order = torch.full((B,), -7, dtype=torch.int32, device=dev)
    d_table = torch.full((G + 2,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    for args in ((0, None, 0, 2, p(d_head), p(d_tail), 2.0, 63), (B, None, 0, 5, p(d_head), p(d_tail), 2.0, 63),
                 (B, None, 0, 2, p(d_head), p(d_tail), 2.0, 64), (B, None, 0, 2, p(d_head), p(d_tail), float("nan"), 63),
                 (B, None, 0, 2, None, p(d_tail), 2.0, 63)):
        assert L.neo_adaptive_count_dev(ctx.h, *args, p(d_counts), p(d_order)) == INVALID and L.neo_last_error(ctx.h), args
    bucket = lambda B=B, sub=None, n_sub=0, counts=p(d_counts), order=p(d_order), begin=p(d_table), total=p(d_table[G + 1:]): \
        L.neo_adaptive_bucket_dev(ctx.h, B, sub, n_sub, counts, order, begin, total)
    for kw in (dict(B=0), dict(counts=None), dict(order=None), dict(begin=None), dict(total=None), dict(sub=p(d_order), n_sub=B + 1),
               dict(sub=p(d_order), n_sub=3)):
        assert bucket(**kw) == INVALID and L.neo_last_error(ctx.h), kw
    x_k = torch.zeros((B, 7), dtype=torch.float64, device=dev); c4 = torch.zeros((B, 4), dtype=torch.float64, device=dev)
    i4 = torch.zeros((B,), dtype=torch.int32, device=dev); i8 = torch.zeros((B,), dtype=torch.int64, device=dev)
    d_x = torch.full((B, 10), SENTINEL, dtype=torch.float64, device=dev); d_pending = torch.full((B,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    merge = lambda B=B, M=3, D=2, stride=10, x_k=p(x_k), x=p(d_x), pending=p(d_pending), bad=p(d_table): L.neo_adaptive_merge_dev(
        ctx.h, B, None, 0, M, D, stride, 1, 1, x_k, p(c4), p(c4), p(i4), p(i4), p(i4), x, p(c4), p(c4), p(i4), p(i4), p(i4), p(i4), p(i8),
        p(i4), pending, bad)
    for kw in (dict(B=0), dict(M=1), dict(M=65), dict(D=4), dict(stride=6), dict(x_k=None), dict(x=None), dict(pending=None), dict(bad=None)):
        assert merge(**kw) == INVALID and L.neo_last_error(ctx.h), kw
    begin = np.zeros(G, np.int32); lens = np.zeros(G, np.int32)
    lens[2] = B
    neg = lens.copy(); neg[5] = -1
    far = begin.copy(); far[2] = 1
    host_pending = np.full(B, -7, np.int32); host_failed = np.full(G, -7, np.int32)
    for args in ((None, q(lens), B, q(host_pending), q(host_failed)), (q(begin), None, B, q(host_pending), q(host_failed)),
                 (q(begin), q(neg), B, q(host_pending), q(host_failed)), (q(far), q(lens), B, q(host_pending), q(host_failed)),
                 (q(begin), q(lens), -1, q(host_pending), q(host_failed)), (q(begin), q(lens), B, None, q(host_failed)),
                 (q(begin), q(lens), B, q(host_pending), None)):
        assert L.neo_adaptive_compact(ctx.h, *args) == INVALID and L.neo_last_error(ctx.h)
    assert L.neo_adaptive_compact_dev(ctx.h, q(begin), q(neg), p(d_pending), p(d_order)) == INVALID
    assert L.neo_adaptive_compact_dev(ctx.h, q(begin), q(lens), None, p(d_order)) == INVALID
    ctx.synchronize()
    # nothing was launched: every output is what it was
    assert np.all(host_pending == -7) and np.all(host_failed == -7)
    for t, v in ((d_counts, -7), (d_order, -7), (d_table, -7), (d_pending, -7), (d_x, SENTINEL)):
        assert bool((t == v).all())
