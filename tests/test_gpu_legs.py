"""Fleet campaigns on the GPU (csrc/neo_legs.hpp, neo_fleet_leg_close_dev / neo_fleet_leg_open_dev / neo_fleet_leg_goal,
FleetReplanLoop(goal_sequences=...)): the two kernels against NumPy restatements bit for bit, their argument errors, a
campaign of one goal against the single-goal flight, a fleet of one against three chained replan.ReplanLoop legs of the
CPU oracle, a mission's independence of the fleet it flies in, the batch staying full, the leg time limit, and onboard
maps (and a recorder) that last from leg to leg."""
import ctypes
import functools

import numpy as np
import pytest

import depth_oracle_np as don
import neo_planner_amd as npa
from neo_planner_amd import _lib, synth
from neo_planner_amd.depth import DepthCamera
from neo_planner_amd.goal_sequences import GoalSequences
from neo_planner_amd.onboard import OnboardMapper
from neo_planner_amd.record import DemoRecorder
from neo_planner_amd.replan import ReplanLoop
from oracle import minco_np as onp

import fleet_flight_cases as ffc

pytestmark = pytest.mark.gpu

ORIGIN = (0.0, -15.0)
SENTINEL = 777.0
F = {name: k for k, name in enumerate(_lib.LEG_FIELDS)}
LANDED, ABANDONED, TIMEOUT, STUCK, OPEN = (_lib.NEO_LEG_LANDED, _lib.NEO_LEG_ABANDONED, _lib.NEO_LEG_TIMEOUT, _lib.NEO_LEG_STUCK,
                                           _lib.NEO_LEG_OPEN)
OCCUPIED = [6.0, 4.5]      # a cell of scene 3 inside an obstacle


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run(ctx, fn, *args):
    """a `_dev` call between torch's stream and the context's"""
    torch, dev = _torch()
    torch.cuda.synchronize(dev)
    ctx.check(fn(ctx.h, *args))
    ctx.synchronize()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _dist(p, g):
    d = np.asarray(p) - np.asarray(g, dtype=np.float64)
    return np.sqrt(d[0] * d[0] + d[1] * d[1])


@pytest.fixture(scope="module")
def map3():
    m = npa.ESDF()
    m.occupancy_map_cb(synth.OccupancyGridMsg(synth.occupancy_2d(3)))
    return m


# ------------------------------------------------------------------ 1. the kernels against NumPy
def _kernel_state(B, max_legs, kind):
    """B missions in every state a leg can end in: the five outcomes in turn, n_flown 0 (nothing planned), 1 and cap, legs
    0 .. max_legs - 1 and, where B allows, a mission whose leg index is outside the log"""
    rng = np.random.default_rng(1000 * B + 10 * max_legs + kind)
    cap = 12
    s = dict(B=B, cap=cap, max_legs=max_legs, threshold=0.2)
    s["outcome"] = (np.arange(B) % 5 + 1).astype(np.int32)
    s["cmd"] = rng.normal(0.0, 3.0, (B, cap, 3, 2))
    shape = np.arange(B) % 7      # 0: nothing planned; 1: on row 0; 2: a full array flown to its end or stopped on its last row
    s["cmd_len"] = np.where(shape == 0, 0, np.where(shape == 2, cap, rng.integers(1, cap + 1, B))).astype(np.int32)
    s["cmd_index"] = np.where(shape == 1, 0, np.where(shape == 2, cap - 1, rng.integers(0, cap + 3, B))).astype(np.int32)
    s["head"] = rng.normal(0.0, 3.0, (B, 3, 2))
    s["goal"] = rng.normal(0.0, 3.0, (B, 2))
    near = np.flatnonzero(np.arange(B) % 5 == 0)      # LANDED rows that end within the threshold of their goal: successes
    for b in near:
        if s["cmd_len"][b] > 0:
            s["goal"][b] = s["cmd"][b, s["cmd_len"][b] - 1, 0] + [0.05, -0.1]
    s["flags"] = np.where(np.arange(B) % 3 == 1, rng.choice([1, 2, 8], B), 0).astype(np.int32)
    s["count"] = rng.integers(0, 40, B).astype(np.int32)
    s["audit_flags"] = np.where(np.arange(B) % 4 == 3, rng.choice([1, 2, 4, 8], B), 0).astype(np.int32)
    s["audit"] = rng.normal(0.0, 1.0, (B, _lib.NEO_AUDIT_FIELDS))
    s["leg"] = (np.arange(B) // 5 % max_legs).astype(np.int32)      # (every outcome meets every leg index, B allowing)
    if B > 2:
        s["leg"][B - 1] = max_legs            # outside the log: skipped
    if B > 40:
        s["leg"][B - 2] = -1
        s["leg"][7] = max_legs - 1            # a mission at max_legs with goals to spare
    s["leg_start"] = rng.normal(0.0, 3.0, (B, 2))
    s["future_index"] = rng.integers(0, cap, B).astype(np.int32)
    s["cur_pos"] = rng.normal(0.0, 3.0, (B, 2))
    if kind == _lib.NEO_LEGS_TABLE:      # counts 1 .. max_legs + 2: missions on their last goal, and missions the log cuts short
        s["seq"] = GoalSequences.from_lists([rng.uniform(-5.0, 30.0, (1 + (b * 5) % (max_legs + 2), 2)) for b in range(B)])
    else:
        ids = rng.permutation(2 ** 20)[:B]
        ids[0] = 2 ** 31 - 1
        s["seq"] = GoalSequences.flap(B, max(1, max_legs - 1), 2 ** 40 + 17, mission_ids=ids)      # the last goal comes before the log ends
    return s


def _close_np(s):
    B, cap = s["B"], s["cap"]
    ln = np.clip(s["cmd_len"], 0, cap)
    nf = np.where(s["outcome"] == LANDED, ln, np.clip(np.minimum(s["cmd_index"].astype(np.int64) + 1, ln), 0, cap)).astype(np.int32)
    end = np.stack([s["cmd"][b, nf[b] - 1, :2] if nf[b] > 0 else s["head"][b, :2] for b in range(B)])
    d = end[:, 0] - s["goal"]
    dist = np.where(nf > 0, np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]), np.inf)
    assert np.array_equal(dist[nf > 0], np.linalg.norm(d, axis=1)[nf > 0])      # np.linalg.norm's bits, as _finish takes them
    return nf, end, dist


def _open_np(s, nf, end, dist, on):
    """the rows after neo_fleet_leg_open_dev over the missions `on`"""
    L, seq = s["max_legs"], s["seq"]
    o = {k: s[k].copy() for k in ("leg", "leg_start", "goal", "cur_pos", "head", "cmd_len", "cmd_index", "future_index", "flags")}
    o["leg_log"] = np.full((s["B"], L, _lib.NEO_LEG_FIELDS), SENTINEL)
    opened = []
    for b in np.flatnonzero(on):
        k = int(s["leg"][b])
        if not 0 <= k < L:
            continue
        oc = int(s["outcome"][b])
        fl = int(s["flags"][b]) | (_lib.NEO_FLEET_FLAG_ABANDONED if oc == ABANDONED else 0)
        afl = int(s["audit_flags"][b])
        ok = oc == LANDED and dist[b] < s["threshold"] and not afl & (_lib.NEO_AUDIT_FLAG_METRIC_FAIL | _lib.NEO_AUDIT_FLAG_NONFINITE) \
            and fl == 0
        o["leg_log"][b, k] = np.concatenate([s["goal"][b], s["leg_start"][b], [oc, nf[b], dist[b], fl, s["count"][b], afl],
                                             s["audit"][b], [float(ok)]])
        o["leg"][b] = k + 1
        g = seq.goal(b, k + 1)
        if oc == OPEN or k + 1 >= L or g is None:
            continue
        opened.append(b)
        o["goal"][b] = g
        o["cur_pos"][b] = o["leg_start"][b] = end[b, 0]
        o["head"][b] = [end[b, 0], end[b, 1], [0.0, 0.0]]
        o["cmd_len"][b] = o["cmd_index"][b] = o["future_index"][b] = 0
        o["flags"][b] = 0
    return o, np.array(opened, np.int64)


def _seq_struct(seq):
    """the sequence's arrays on the device and the struct that names them (the arrays are returned to keep them alive)"""
    keep = (_dev(seq.goals if len(seq.goals) else np.zeros((1, 2))), _dev(seq.seq_begin),
            None if seq.mission_ids is None else _dev(seq.mission_ids))
    return seq.struct(_p, *keep), keep


@pytest.mark.parametrize("kind", [_lib.NEO_LEGS_TABLE, _lib.NEO_LEGS_FLAP])
@pytest.mark.parametrize("max_legs", [1, 2, 5])
@pytest.mark.parametrize("B", [1, 3, 70])
def test_close_and_open_equal_numpy_bit_for_bit(B, max_legs, kind):
    torch, dev = _torch()
    ctx = _lib.default_context()
    s = _kernel_state(B, max_legs, kind)
    cap, L = s["cap"], max_legs
    nf, end, dist = _close_np(s)
    if B == 70:
        assert {0, 1, cap} <= set(nf.tolist()) and set(s["outcome"].tolist()) == {1, 2, 3, 4, 5}
    seq_c, keep = _seq_struct(s["seq"])
    pick = np.flatnonzero(np.arange(B) % 4 != 2)[:max(B - 2, 1)]
    subsets = [None, (np.concatenate([[B + 3], pick[::-1], [-1]]) if B > 2 else pick).astype(np.int32)]      # (at most B entries)
    seen_open = seen_last = seen_cut = 0
    for sub in subsets:
        on = np.ones(B, bool) if sub is None else np.isin(np.arange(B), sub)
        d_sub = None if sub is None else _dev(sub)
        sub_args = (_p(d_sub), 0 if sub is None else len(sub))
        rows = (B,) + sub_args
        # ---- close
        d = {k: _dev(s[k]) for k in ("outcome", "cmd", "cmd_len", "cmd_index", "head", "goal", "count", "audit_flags", "audit", "leg",
                                     "leg_start", "cur_pos", "future_index", "flags")}
        d_nf = torch.full((B,), -7, dtype=torch.int32, device=dev)
        d_end = torch.full((B, 2, 2), SENTINEL, dtype=torch.float64, device=dev)
        d_dist = torch.full((B,), SENTINEL, dtype=torch.float64, device=dev)
        _run(ctx, ctx.lib.neo_fleet_leg_close_dev, B, _p(d["outcome"]), *sub_args, _p(d["cmd"]), cap, _p(d["cmd_len"]), _p(d["cmd_index"]),
             _p(d["head"]), _p(d["goal"]), _p(d_nf), _p(d_end), _p(d_dist))
        g_nf, g_end, g_dist = d_nf.cpu().numpy(), d_end.cpu().numpy(), d_dist.cpu().numpy()
        assert np.array_equal(g_nf[on], nf[on]) and np.all(g_nf[~on] == -7)
        assert np.array_equal(_bits(g_end[on]), _bits(end[on])) and np.all(g_end[~on] == SENTINEL)
        assert np.array_equal(_bits(g_dist[on]), _bits(dist[on])) and np.all(g_dist[~on] == SENTINEL)
        # ---- open, on close's outputs
        d_log = torch.full((B, L, _lib.NEO_LEG_FIELDS), SENTINEL, dtype=torch.float64, device=dev)
        _run(ctx, ctx.lib.neo_fleet_leg_open_dev, B, _p(d["outcome"]), *sub_args, ctypes.byref(seq_c), L, s["threshold"], _p(d_nf), _p(d_end),
             _p(d_dist), _p(d["count"]), _p(d["audit_flags"]), _p(d["audit"]), _p(d["leg"]), _p(d_log), _p(d["leg_start"]),
             _p(d["goal"]), _p(d["cur_pos"]), _p(d["head"]), _p(d["cmd_len"]), _p(d["cmd_index"]), _p(d["future_index"]),
             _p(d["flags"]))
        want, opened = _open_np(s, nf, end, dist, on)
        assert np.array_equal(_bits(d_log.cpu().numpy()), _bits(want["leg_log"])), "the log"
        for k in ("leg", "leg_start", "goal", "cur_pos", "head", "cmd_len", "cmd_index", "future_index", "flags"):
            assert np.array_equal(_bits(d[k].cpu().numpy()), _bits(want[k])), k      # untouched rows keep every byte
        assert np.array_equal(d["cmd"].cpu().numpy(), s["cmd"])
        logged = on & (s["leg"] >= 0) & (s["leg"] < L)
        seen_open += len(opened)
        seen_last += int(np.sum(logged & (s["outcome"] != OPEN) & (s["leg"] + 1 >= s["seq"].count)))
        seen_cut += int(np.sum(logged & (s["outcome"] != OPEN) & (s["leg"] + 1 < s["seq"].count) & (s["leg"] + 1 >= L)))
        # ---- the tick's kernels on a freshly opened leg: the advance leaves it alone, the pose looks at the new goal, the
        # splice starts at row 0
        if len(opened):
            before = {k: d[k].cpu().numpy() for k in ("cur_pos", "head", "cmd_index", "future_index")}
            _run(ctx, ctx.lib.neo_fleet_advance_dev, *rows, _p(d["cmd"]), cap, _p(d["cmd_len"]), _p(d["cmd_index"]),
                 _p(d["future_index"]), 60, 60, _p(d["cur_pos"]), _p(d["head"]))
            for k, v in before.items():
                assert np.array_equal(_bits(d[k].cpu().numpy()[opened]), _bits(v[opened])), k
            pose = torch.full((B, 5), SENTINEL, dtype=torch.float64, device=dev)
            _run(ctx, ctx.lib.neo_fleet_pose_dev, *rows, _p(d["cmd"]), cap, _p(d["cmd_len"]), _p(d["cmd_index"]), _p(d["cur_pos"]),
                 _p(d["goal"]), 2.0, _p(pose))
            got = pose.cpu().numpy()[opened]
            dg = want["goal"][opened] - want["cur_pos"][opened]
            n = np.sqrt(dg[:, 0] * dg[:, 0] + dg[:, 1] * dg[:, 1])
            assert np.array_equal(got[:, :2], want["cur_pos"][opened]) and np.array_equal(got[:, 3:], dg / n[:, None])
            # the splice with first = 0 starts at the future_index = 0 that open left (it was anything before): the rows,
            # lengths and indices of a first = 1 splice, which starts at row 0 by definition; row 0 is the opened head
            M, hz = 3, 1.0      # (three pieces of a few seconds at one row a second fit the 12 rows)
            x = np.zeros((B, 7))
            for q in (0, 1):
                x[:, q] = want["cur_pos"][:, 0] + (q + 1) / 3.0 * (want["goal"][:, 0] - want["cur_pos"][:, 0])
                x[:, 2 + q] = want["cur_pos"][:, 1] + (q + 1) / 3.0 * (want["goal"][:, 1] - want["cur_pos"][:, 1])
            tail = np.zeros((B, 3, 2))
            tail[:, 0] = want["goal"]
            d_x, d_tail, d_opened = _dev(x), _dev(tail), _dev(opened.astype(np.int32))
            spliced = []
            for first in (0, 1):
                c = {k: d[k].clone() for k in ("cmd", "cmd_len", "cmd_index", "future_index", "flags")}
                _run(ctx, ctx.lib.neo_fleet_splice_dev, B, _p(d_opened), len(opened), M, _p(d_x), _p(d["head"]), _p(d_tail), None, hz,
                     first, _p(c["cmd"]), cap, _p(c["cmd_len"]), _p(c["cmd_index"]), _p(c["future_index"]), _p(c["flags"]))
                spliced.append({k: v.cpu().numpy() for k, v in c.items()})
            at0, at1 = spliced
            for k in at0:
                assert np.array_equal(_bits(at0[k]), _bits(at1[k])), k
            assert np.all(at0["cmd_len"][opened] >= 2) and np.all(at0["cmd_len"][opened] <= cap) and np.all(at0["flags"][opened] == 0)
            assert np.all(at0["cmd_index"][opened] == 0) and np.all(at0["future_index"][opened] == 0)
            assert np.allclose(at0["cmd"][opened, 0, :2], want["head"][opened, :2], rtol=0.0, atol=1e-9)
            rest = np.setdiff1d(np.arange(B), opened)
            assert np.array_equal(at0["cmd"][rest], d["cmd"].cpu().numpy()[rest])
    if B == 70 and max_legs > 2:
        assert seen_open >= 10 and seen_last >= 2 and (seen_cut >= 1 or kind == _lib.NEO_LEGS_FLAP), (seen_open, seen_last, seen_cut)
        ok = want["leg_log"][:, :, F["success"]]
        assert np.any(ok == 1.0) and np.any(ok == 0.0)
    if max_legs == 1:
        assert seen_open == 0      # a log of one leg opens nothing


@pytest.mark.parametrize("kind", [_lib.NEO_LEGS_TABLE, _lib.NEO_LEGS_FLAP])
def test_leg_goal_equals_the_model_bit_for_bit(kind):
    ctx = _lib.default_context()
    B = 70
    seq = _kernel_state(B, 5, kind)["seq"]
    rng = np.random.default_rng(5)
    mission = np.concatenate([np.repeat(np.arange(B), 8), [-1, B, B + 5]]).astype(np.int32)
    leg_of = np.concatenate([np.tile(np.arange(-1, 7), B), [0, 0, 0]]).astype(np.int32)
    order = rng.permutation(len(mission))
    mission, leg_of = mission[order], leg_of[order]
    goal = np.full((len(mission), 2), SENTINEL)
    exists = np.full(len(mission), -1, np.int32)
    c = seq.struct(_lib.ptr)
    ctx.check(ctx.lib.neo_fleet_leg_goal(ctx.h, ctypes.byref(c), B, len(mission), _lib.ptr(mission), _lib.ptr(leg_of), _lib.ptr(goal),
                                         _lib.ptr(exists)))
    want = [seq.goal(b, k) if 0 <= b < B else None for b, k in zip(mission, leg_of)]
    assert np.array_equal(exists, [w is not None for w in want]) and 0 < exists.sum() < len(exists)
    have = exists == 1
    assert np.array_equal(_bits(goal[have]), _bits(np.stack([w for w in want if w is not None]))) and np.isnan(goal[~have]).all()


# ------------------------------------------------------------------ 2. argument errors
def test_leg_argument_errors():
    torch, dev = _torch()
    ctx = _lib.default_context()
    L = ctx.lib
    z = torch.zeros(4096, dtype=torch.float64, device=dev)      # (a log of 2 x 64 rows fits)
    zi = torch.zeros(16, dtype=torch.int32, device=dev)
    names = ("outcome", "cmd", "cmd_len", "cmd_index", "head", "goal", "n_flown", "leg_end", "final_dist")

    def close(B=2, sub=None, n_sub=0, cap=4, **null):
        a = {k: _p(zi if k in ("outcome", "cmd_len", "cmd_index", "n_flown") else z) for k in names}
        a.update({k: None for k in null})
        return L.neo_fleet_leg_close_dev(ctx.h, B, a["outcome"], sub, n_sub, a["cmd"], cap, a["cmd_len"], a["cmd_index"], a["head"],
                                         a["goal"], a["n_flown"], a["leg_end"], a["final_dist"])
    assert close() == 0
    for k in names:
        assert close(**{k: True}) == 1 and b"null" in L.neo_last_error(ctx.h), k
    assert close(B=-1) == 1 and close(sub=_p(zi), n_sub=3) == 1 and close(sub=_p(zi), n_sub=-1) == 1
    assert close(cap=0) == 1 and b"cap" in L.neo_last_error(ctx.h)

    table = GoalSequences.from_lists([[[1.0, 2.0]], [[3.0, 4.0], [5.0, 6.0]]])
    flap = GoalSequences.flap(2, 3, 9)
    tc, keep_t = _seq_struct(table)
    fc, keep_f = _seq_struct(flap)
    onames = ("outcome", "n_flown", "leg_end", "final_dist", "count", "audit_flags", "audit", "leg", "leg_log", "leg_start", "goal",
              "cur_pos", "head", "cmd_len", "cmd_index", "future_index", "flags")
    ints = ("outcome", "n_flown", "count", "audit_flags", "leg", "cmd_len", "cmd_index", "future_index", "flags")

    def changed(c, **kw):
        out = _lib.NeoLegSequences.from_buffer_copy(c)
        for k, v in kw.items():
            setattr(out, k, v)
        return out

    def open_(B=2, sub=None, n_sub=0, seq=tc, max_legs=2, thr=0.2, **null):
        a = {k: _p(zi if k in ints else z) for k in onames}
        a.update({k: None for k in null})
        return L.neo_fleet_leg_open_dev(ctx.h, B, a["outcome"], sub, n_sub, None if seq is None else ctypes.byref(seq), max_legs, thr,
                                        *[a[k] for k in onames[1:]])
    assert open_() == 0 and open_(seq=fc) == 0
    for k in onames:
        assert open_(**{k: True}) == 1 and b"null" in L.neo_last_error(ctx.h), k
    assert open_(seq=None) == 1 and open_(B=-1) == 1 and open_(sub=_p(zi), n_sub=3) == 1
    assert open_(max_legs=0) == 1 and open_(max_legs=65) == 1 and b"max_legs" in L.neo_last_error(ctx.h)
    assert open_(max_legs=64) == 0
    for thr in (-0.1, float("nan"), float("inf")):
        assert open_(thr=thr) == 1 and b"threshold" in L.neo_last_error(ctx.h)
    assert open_(thr=0.0) == 0
    # the four cases test_gpu_abi_refusals.py records for the older list entry points: list_check's two, then an empty list and a
    # subset of none, each with a NULL buffer -- nothing may pass as a launch
    for call, who in ((close, b"fleet leg close"), (open_, b"fleet leg open")):
        assert call(B=-1) == 1 and L.neo_last_error(ctx.h) == who + b": B must be >= 0"
        assert call(B=1, sub=_p(zi), n_sub=2) == 1 and L.neo_last_error(ctx.h) == who + b": bad subset size"
        for kw in (dict(B=0), dict(B=1, sub=_p(zi), n_sub=0)):
            assert call(cmd_len=True, **kw) == 1 and L.neo_last_error(ctx.h) == who + b": null buffer"
    assert open_(seq=changed(tc, n_goals=1)) == 1 and b"fewer goals" in L.neo_last_error(ctx.h)      # two missions, one goal
    assert open_(seq=changed(tc, goals=None)) == 1 and open_(seq=changed(tc, seq_begin=None)) == 1
    assert open_(seq=changed(tc, kind=2)) == 1 and b"kind" in L.neo_last_error(ctx.h)
    assert open_(seq=changed(fc, legs=0)) == 1 and open_(seq=changed(fc, legs=65)) == 1
    assert open_(seq=changed(fc, y_scale=float("nan"))) == 1
    ctx.synchronize()
    # the host form reads the table: a mission without a goal is refused by name
    g, ex = np.zeros((1, 2)), np.zeros(1, np.int32)
    m = np.zeros(1, np.int32)
    bad = changed(table.struct(_lib.ptr))
    begin = np.array([0, 0, 3], np.int32)      # mission 0 has no goal
    goals3 = np.zeros((3, 2))
    bad.seq_begin, bad.goals, bad.n_goals = begin.ctypes.data, goals3.ctypes.data, 3
    call = lambda c, n=1, mm=m: L.neo_fleet_leg_goal(ctx.h, ctypes.byref(c), 2, n, _lib.ptr(mm), _lib.ptr(m), _lib.ptr(g), _lib.ptr(ex))
    assert call(bad) == 1 and b"every mission needs" in L.neo_last_error(ctx.h)
    good = table.struct(_lib.ptr)
    assert call(good) == 0 and ex[0] == 1 and np.array_equal(g[0], [1.0, 2.0])
    assert call(good, n=-1) == 1 and call(good, mm=None) == 1 and call(good, n=0) == 0


# ------------------------------------------------------------------ 3. a campaign of one goal is the single-goal flight
START8 = np.array([[0.0, 0.0], [0.5, -2.0], [0.5, 3.0], [1.0, -6.0], [0.5, 1.0], [0.5, 0.5], [0.0, -1.0], [1.0, 5.0]])
# mission 3 does not arrive in the ticks it gets (OPEN), 4 flies at an obstacle (ABANDONED), 5 lands after its first plan
GOALS8 = np.array([[7.1, 2.5], [9.6, -2.5], [8.8, 8.9], [14.3, -7.1], OCCUPIED, [3.0, 0.5], [12.0, 6.0], [4.5, 6.5]])


def _recorded(loop, *args, **kw):
    ctx = loop.bp.ctx
    lib, proxy = ctx.lib, ffc.RecordingLib(ctx.lib)
    ctx.lib = proxy
    try:
        out = loop.run(*args, **kw)
    finally:
        ctx.lib = lib
    return out, proxy


@pytest.mark.parametrize("mode,resident", [("basic", False), ("basic", True), ("batch", False)])
def test_a_campaign_of_one_goal_is_the_single_goal_flight(map3, mode, resident):
    kw = dict(mode=mode, resident=resident, seed=41, max_cmd_seconds=60)
    plain = npa.FleetReplanLoop(npa.BatchPlanner(), map3, GOALS8, **kw)
    ref, ref_calls = _recorded(plain, START8, max_replans=7)
    camp = npa.FleetReplanLoop(npa.BatchPlanner(), map3, None, goal_sequences=GoalSequences.from_lists(GOALS8[:, None, :]), **kw)
    out, calls = _recorded(camp, START8, max_replans=7)
    print(f"{mode} resident={resident}: success {ref['success'].tolist()}, abandoned {ref['abandoned'].tolist()}, replans "
          f"{ref['replans'].tolist()}, outcomes {out['leg_outcome'][:, 0].tolist()}, synchronizes {ref_calls.syncs} -> {calls.syncs} "
          f"over {len(camp.timings)} ticks")
    assert ref["success"].any() and ref["abandoned"][4] and not ref["success"].all()
    for k in ref:
        assert np.array_equal(np.asarray(out[k]), np.asarray(ref[k]), equal_nan=True), (k, out[k], ref[k])
    for i in range(8):
        assert np.array_equal(camp.commands(i), plain.commands(i)), i
    assert np.array_equal(camp.x, plain.x)
    assert [t["active"] for t in camp.timings] == [t["active"] for t in plain.timings]
    assert calls.syncs <= ref_calls.syncs + len(camp.timings)
    assert {LANDED, ABANDONED, OPEN} <= set(out["leg_outcome"][:, 0].tolist()) and np.all(out["n_legs"] == 1)
    assert np.array_equal(out["leg_success"][:, 0] == 1, ref["success"]) and np.array_equal(out["leg_replans"][:, 0], ref["replans"])
    assert np.array_equal(out["leg_start_x"][:, 0], START8[:, 0]) and np.array_equal(out["leg_goal_y"][:, 0], GOALS8[:, 1])
    assert np.array_equal(out["leg_n_flown"][:, 0], ref["n_flown"]) and np.array_equal(out["leg_final_dist"][:, 0], ref["final_dist"])


# ------------------------------------------------------------------ 4. a fleet of one against the CPU oracle's campaign
ORACLE_GOALS = [[7.1, 2.5], [3.5, -3.1], [9.6, -2.5]]


@functools.lru_cache(maxsize=None)
def _oracle_campaign():
    grid = onp.GridESDF(synth.occupancy_2d(3), synth.RES, 300, 300, ORIGIN)
    np.random.seed(503)
    state = np.random.get_state()
    pos, vel, legs = np.zeros(2), np.zeros(2), []
    for g in ORACLE_GOALS:
        loop = ReplanLoop(onp.OraclePlanner(onp.PlannerParams()), grid, goal=g)
        out = loop.run(pos, vel)
        out["commands"] = loop.des_state_array
        legs.append(out)
        pos, vel = loop.des_state_array[-1, 0].copy(), loop.des_state_array[-1, 1].copy()
    after = np.random.get_state()
    assert np.array_equal(after[1], state[1]) and after[2:] == state[2:], "an oracle leg drew random numbers: not comparable"
    return legs


def test_fleet_of_one_flies_the_oracle_campaign(map3):
    ref = _oracle_campaign()
    assert [r["replans"] for r in ref] == [5, 4, 4] and [len(r["commands"]) for r in ref] == [582, 535, 510]
    assert all(r["success"] and r["failed_attempts"] == 0 for r in ref)
    seq = GoalSequences.from_lists([ORACLE_GOALS])
    cmds, outs = [], []
    for L in (1, 2, 3):      # the last leg's command array stays: the campaign cut after leg L shows leg L's
        loop = npa.FleetReplanLoop(npa.BatchPlanner(), map3, None, goal_sequences=seq, max_legs=L)
        outs.append(loop.run([[0.0, 0.0]]))
        cmds.append(loop.commands(0))
    out = outs[2]
    assert out["n_legs"][0] == 3 and bool(out["success"][0]) and out["leg_outcome"][0].tolist() == [LANDED] * 3
    assert not outs[0]["success"][0] and outs[0]["leg_success"][0, 0] == 1      # one of three goals is not the campaign
    for k in range(3):
        r, cmd = ref[k], cmds[k]
        n = min(len(cmd), len(r["commands"]))
        diff = np.max(np.linalg.norm(cmd[:n, 0] - r["commands"][:n, 0], axis=1))
        print(f"leg {k}: fleet {out['leg_replans'][0, k]} plans, {out['leg_failed_attempts'][0, k]} failed, iterations "
              f"{out['leg_iter_num'][0, k]}, {out['leg_n_flown'][0, k]} flown; oracle {r['replans']} plans, {r['failed_attempts']} "
              f"failed, iterations {r['iter_num']}, {len(r['commands'])} rows; max position difference {diff:.4f} m; clearance "
              f"{out['leg_min_clearance'][0, k]:.3f}")
        assert out["leg_replans"][0, k] == r["replans"] and out["leg_failed_attempts"][0, k] == r["failed_attempts"]
        assert out["leg_n_flown"][0, k] == len(r["commands"]) == len(cmd)
        assert diff < 0.25
        assert abs(out["leg_iter_num"][0, k] - r["iter_num"]) <= 0.2 * r["iter_num"] + 5
        assert out["leg_ticks"][0, k] == r["replans"] and out["leg_success"][0, k] == 1 and out["leg_flags"][0, k] == 0
        assert np.array_equal([out["leg_goal_x"][0, k], out["leg_goal_y"][0, k]], ORACLE_GOALS[k])
        assert out["leg_final_dist"][0, k] == _dist(cmd[-1, 0], ORACLE_GOALS[k])
        if k < 2:      # the shorter campaigns flew the same legs, and the next leg starts on this one's last row, exactly
            for key in out:
                if key.startswith("leg_"):
                    assert np.array_equal(outs[k][key][0, :k + 1], out[key][0, :k + 1], equal_nan=True), (k, key)
            assert out["leg_start_x"][0, k + 1] == cmd[-1, 0, 0] and out["leg_start_y"][0, k + 1] == cmd[-1, 0, 1]
            assert np.array_equal(cmds[k + 1][0, 0], cmd[-1, 0])      # and its first plan was spliced at row 0, from there
            assert np.allclose(cmds[k + 1][0, 1], cmd[-1, 1], atol=1e-9)
    assert np.array_equal(out["leg_first_tick"][0], np.concatenate([[0], np.cumsum(out["leg_ticks"][0])[:2]]))
    assert out["replans"][0] == 13 and out["iter_num"][0] == out["leg_iter_num"][0].sum() and out["n_cmd"][0] == len(cmds[2])
    assert out["leg_start_x"][0, 0] == 0.0 and out["leg_start_y"][0, 0] == 0.0


# ------------------------------------------------------------------ 5. / 6. alone and in a fleet; the batch stays full
SEQ8 = [[[7.1, 2.5], [3.5, -3.1], [9.6, -2.5]],
        [[9.0, -4.0], [3.5, -3.1]],
        [[4.5, 6.5], [2.0, 2.0], [5.0, 0.0], [3.0, 0.5]],
        [[14.3, -7.1]],
        [OCCUPIED, [2.0, 2.0]],                # every plan of the first leg's last tick fails; the second leg flies
        [[3.0, 0.5], [9.6, -2.5], [3.5, -3.1]],      # (a goal closer than longitu_step_dis is a leg of one tick)
        [[10.0, 3.0], [5.0, 0.0]],
        [[4.5, 6.5], [8.8, 8.9], [2.0, 2.0], [12.0, 6.0]]]
CAMPAIGN_MODES = {"basic_resident": dict(mode="basic", resident=True),
                  "basic_resident_counter": dict(mode="basic", resident=True, jitter="counter"),
                  "batch_counter": dict(mode="batch", jitter="counter")}


@functools.lru_cache(maxsize=None)
def _fleet_campaign(name, pick=None):
    m = npa.ESDF()
    m.occupancy_map_cb(synth.OccupancyGridMsg(synth.occupancy_2d(3)))
    idx = np.arange(8) if pick is None else np.array(pick)
    seq = GoalSequences.from_lists(SEQ8).take(idx)
    loop = npa.FleetReplanLoop(npa.BatchPlanner(), m, None, goal_sequences=seq, mission_ids=idx, seed=41, max_cmd_seconds=60, max_legs=4,
                               **CAMPAIGN_MODES[name])
    out = loop.run(START8[idx], max_replans=40)
    c = _lib.default_context()
    cmds = [loop.commands(i) for i in range(len(idx))]
    active = [t["active"] for t in loop.timings]
    c.check(c.lib.neo_esdf_drop(c.h, m.scene_id))
    return out, cmds, active


@pytest.mark.parametrize("name", list(CAMPAIGN_MODES))
def test_a_mission_flies_its_campaign_the_same_alone_and_in_a_fleet(name):
    out, cmds, _ = _fleet_campaign(name)
    print(f"{name}: legs {out['n_legs'].tolist()}, outcomes {out['leg_outcome'].tolist()}, success {out['success'].tolist()}, replans "
          f"{out['replans'].tolist()}")
    assert np.array_equal(out["n_legs"], [len(s) for s in SEQ8])
    for i in (0, 2, 5):
        o1, c1, _ = _fleet_campaign(name, (i,))
        assert set(o1) == set(out)
        for k in out:
            assert np.array_equal(np.asarray(o1[k])[0], np.asarray(out[k])[i], equal_nan=True), (i, k, o1[k][0], out[k][i])
        assert np.array_equal(c1[0], cmds[i]), i


@pytest.mark.parametrize("name", list(CAMPAIGN_MODES))
def test_the_batch_stays_full(name):
    out, _, active = _fleet_campaign(name)
    last = out["n_legs"] - 1
    ends = out["leg_first_tick"][np.arange(8), last] + out["leg_ticks"][np.arange(8), last]      # the tick after a campaign's last
    first_out = int(ends.min())
    assert active[:first_out] == [8] * first_out and active[first_out] < 8
    later = out["leg_first_tick"][:, 1]
    assert first_out >= 3 and np.sum((later > 0) & (later < first_out)) >= 2      # legs were closed and opened while the batch was full
    # the abandoned leg is followed by a leg that flies
    assert out["leg_outcome"][4].tolist()[:2] == [ABANDONED, LANDED] and out["leg_flags"][4, 0] == _lib.NEO_FLEET_FLAG_ABANDONED
    assert out["leg_failed_attempts"][4, 0] >= 11 and out["leg_success"][4].tolist()[:2] == [0, 1] and not out["success"][4]
    assert out["leg_first_tick"][4, 1] == out["leg_first_tick"][4, 0] + out["leg_ticks"][4, 0]
    assert out["leg_replans"][4, 1] >= 1 and out["leg_final_dist"][4, 1] < 0.2 and out["flags"][4] == 0 and not out["abandoned"][4]
    # totals are sums over the legs; padding beyond n_legs
    flown = np.arange(out["leg_ticks"].shape[1])[None, :] < out["n_legs"][:, None]
    for total, per in (("replans", "leg_replans"), ("failed_attempts", "leg_failed_attempts"), ("iter_num", "leg_iter_num"),
                       ("opt_runs", "leg_opt_runs")):
        assert np.array_equal(out[total], np.where(flown, out[per], 0).sum(axis=1)), total
    assert np.all(out["leg_outcome"][~flown] == -1) and np.isnan(out["leg_final_dist"][~flown]).all()
    assert np.all(out["leg_ticks"][~flown] == -1) and np.all(out["leg_first_tick"][~flown] == -1)
    ok = np.array([all(out["leg_success"][b, :out["n_legs"][b]] == 1) for b in range(8)])
    assert np.array_equal(out["success"], ok) and ok.sum() >= 3


# ------------------------------------------------------------------ 7. the leg time limit
def test_leg_timeout_closes_a_leg_and_the_next_starts_from_the_row_being_flown(map3):
    seq = GoalSequences.from_lists([[[24.4, 7.6], [14.3, -7.1]], [[3.0, 0.5], [15.6, 8.6]]])
    start = np.array([[0.0, 0.0], [0.5, 0.5]])
    kw = dict(goal_sequences=seq, leg_timeout=3.0, resident=True)
    # step / cmd_hz = 1 s: (j + 1) > 3 first holds for j = 3, the leg's tick 3 counted from 0 -- four ticks, three periods flown
    loop1 = npa.FleetReplanLoop(npa.BatchPlanner(), map3, None, max_legs=1, **kw)
    o1 = loop1.run(start, max_replans=12)
    cmd1 = loop1.commands(0)
    loop = npa.FleetReplanLoop(npa.BatchPlanner(), map3, None, **kw)
    out = loop.run(start, max_replans=12)
    print(f"outcomes {out['leg_outcome'].tolist()}, ticks {out['leg_ticks'].tolist()}, n_flown {out['leg_n_flown'].tolist()}")
    assert out["leg_outcome"].tolist() == [[TIMEOUT, TIMEOUT], [LANDED, TIMEOUT]] and o1["leg_outcome"].tolist() == [[TIMEOUT], [LANDED]]
    assert out["leg_ticks"].tolist() == [[4, 4], [1, 4]] and out["leg_first_tick"].tolist() == [[0, 4], [0, 1]]
    assert out["leg_n_flown"][0].tolist() == [181, 181] and out["leg_n_flown"][1, 1] == 181
    assert len(loop.timings) == 8 and [t["active"] for t in loop.timings] == [2, 2, 2, 2, 2, 1, 1, 1]
    assert not out["success"].any() and out["leg_success"].tolist() == [[0, 0], [1, 0]] and np.all(out["leg_flags"] == 0)
    # the second leg starts on the row being flown when the first was closed, with its velocity
    assert out["leg_start_x"][0, 1] == cmd1[180, 0, 0] and out["leg_start_y"][0, 1] == cmd1[180, 0, 1]
    assert np.linalg.norm(cmd1[180, 1]) > 0.3
    cmd2 = loop.commands(0)
    assert np.array_equal(cmd2[0, 0], cmd1[180, 0]) and np.allclose(cmd2[0, 1], cmd1[180, 1], atol=1e-9)
    assert out["leg_final_dist"][0, 0] == _dist(cmd1[180, 0], [24.4, 7.6]) == o1["final_dist"][0]
    assert out["n_flown"][0] == 181 and out["n_cmd"][0] == len(cmd2) and out["final_dist"][0] == out["leg_final_dist"][0, 1]


def test_a_leg_opened_at_the_end_of_the_last_tick_is_logged_open_and_empty(map3):
    """max_replans = 0: mission 0 lands its first goal (2.5 m away) at tick 0, its second leg is opened and the run is over;
    mission 1 is still on its first leg.  Both legs are logged NEO_LEG_OPEN, the never-planned one empty."""
    seq = GoalSequences.from_lists([[[3.0, 0.5], [15.6, 8.6]], [[24.4, 7.6], [14.3, -7.1]]])
    loop = npa.FleetReplanLoop(npa.BatchPlanner(), map3, None, goal_sequences=seq, resident=True)
    out = loop.run(np.array([[0.5, 0.5], [0.0, 0.0]]), max_replans=0)
    assert len(loop.timings) == 1 and out["n_legs"].tolist() == [2, 1] and out["leg_outcome"].tolist() == [[LANDED, OPEN], [OPEN, -1]]
    assert out["leg_ticks"].tolist() == [[1, 0], [1, -1]] and out["leg_first_tick"].tolist() == [[0, -1], [0, -1]]
    assert out["leg_replans"].tolist() == [[1, 0], [1, -1]] and out["leg_success"].tolist() == [[1, 0], [0, -1]]
    # the never-planned leg: nothing flown from where the first leg ended, towards the second goal
    assert out["leg_n_flown"][0, 1] == 0 and np.isinf(out["leg_final_dist"][0, 1]) and out["leg_count"][0, 1] == 0
    assert [out["leg_goal_x"][0, 1], out["leg_goal_y"][0, 1]] == [15.6, 8.6]
    assert _dist([out["leg_start_x"][0, 1], out["leg_start_y"][0, 1]], [3.0, 0.5]) < 0.2
    # the old keys describe it, as the device does: its command array is the empty one
    assert out["n_flown"][0] == 0 and out["n_cmd"][0] == 0 and np.isinf(out["final_dist"][0]) and len(loop.commands(0)) == 0
    assert not out["success"].any() and not out["abandoned"].any() and out["replans"].tolist() == [1, 1]
    # mission 1 stopped on row 0 of its only plan
    assert out["leg_n_flown"][1, 0] == 1 and out["n_cmd"][1] > 1 and out["final_dist"][1] == _dist([0.0, 0.0], [24.4, 7.6])


# ------------------------------------------------------------------ 8. onboard maps last from leg to leg
def test_onboard_maps_and_the_recorder_last_from_leg_to_leg(map3):
    scenes = DepthCamera.pack_scenes([don.boxes_of(synth.forest_boxes(3))])
    seq = GoalSequences.from_lists([[[9.6, -2.5], [0.5, 0.5]]])
    ctx = _lib.default_context()
    cam = DepthCamera(width=64, height=48)
    occ = []
    try:
        for L in (1, 2):
            mapper = OnboardMapper(ctx, cam, 1)
            rec = DemoRecorder(DepthCamera(width=64, height=48), capacity=64)
            loop = npa.FleetReplanLoop(npa.BatchPlanner(), map3, None, goal_sequences=seq, max_legs=L, onboard=mapper, scenes=scenes,
                                       record=rec, resident=True, max_cmd_seconds=60)
            out = loop.run([[0.5, 0.5]], max_replans=30)
            occ.append(mapper.occupancy[0].cpu().numpy().copy())
            rows = rec.rows()
            mapper.close()
            mapper = None
    finally:
        if mapper is not None:
            mapper.close()
    print(f"legs {out['n_legs'].tolist()}, outcomes {out['leg_outcome'].tolist()}, ticks {out['leg_ticks'].tolist()}, known cells "
          f"{int((occ[0] >= 0).sum())} -> {int((occ[1] >= 0).sum())}, occupied {int((occ[0] == 100).sum())} -> {int((occ[1] == 100).sum())}, "
          f"recorded rows {len(rows['meta'])}")
    assert out["n_legs"][0] == 2 and out["leg_replans"][0, 0] >= 1 and out["leg_replans"][0, 1] >= 1
    # what leg 1 saw is still there after leg 2: no cell went back to unknown at the leg change, and leg 2 added to it
    known1, known2 = occ[0] >= 0, occ[1] >= 0
    assert (occ[0] == 100).sum() > 0 and np.all(known2[known1]) and known2.sum() > known1.sum()
    # the recorder holds rows of both legs: ticks before and from the second leg's first tick
    ticks = rows["meta"][:, 1]
    t1 = out["leg_first_tick"][0, 1]
    assert len(ticks) == out["replans"][0] and np.sum(ticks < t1) == out["leg_replans"][0, 0] and np.sum(ticks >= t1) == out["leg_replans"][0, 1]
