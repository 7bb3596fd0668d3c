"""The learned warm start on resident arrays, on the GPU: neo_init_motion_dev, neo_init_head_dev and neo_init_guess_dev
against the NumPy models (tests/init_oracle_np.py), their argument errors, BatchNeoPlanner.plan_dev against
BatchPlanner.plan_dev from the same guess, and FleetReplanLoop's modes "neo" and "nn"."""
import ctypes

import numpy as np
import pytest

import init_oracle_np as ion
import neo_planner_amd as npa
from neo_planner_amd import _lib
from neo_planner_amd.record import DemoRecorder
from test_gpu_record import MAX_REPLANS, _fleet_setup, _fly

pytestmark = pytest.mark.gpu

NEO_ERR_INVALID = 1
SENT32, SENT64 = np.float32(-7.25), -7.25


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _ini():
    from neo_planner_amd import initializer as ini
    return ini


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def up(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------ kernels against the oracle
_BLOB = []


def blob():
    """the head's weights of a seeded PlannerNet(24, 32), packed on the CPU"""
    if not _BLOB:
        torch, _ = _torch()
        torch.manual_seed(5)
        _BLOB.append(_ini().pack_head_weights(_ini().PlannerNet(24, 32)).numpy().copy())
    return _BLOB[0]


def case(B):
    """B requests' states, features and network outputs; request 0's durations lie below T_min, above T_max and exactly
    in the middle (tau = 0), request 1's outputs are NaN"""
    rng = np.random.default_rng([77, B])
    yaw = rng.uniform(-np.pi, np.pi, B)
    pose = np.stack([rng.uniform(0.0, 30.0, B), rng.uniform(-15.0, 15.0, B), rng.uniform(0.5, 3.0, B), np.cos(yaw), np.sin(yaw)], 1)
    out9 = np.concatenate([rng.uniform(-12.0, 12.0, (B, 6)), rng.uniform(0.3, 5.5, (B, 3))], 1).astype(np.float32)
    out9[0, 6:] = (0.1, 7.0, 2.75)
    if B > 1:
        out9[1] = np.nan
    return dict(pose=pose, cur_vel=rng.uniform(-3.0, 3.0, (B, 2)), head=rng.uniform(-30.0, 30.0, (B, 3, 2)),
                tail=rng.uniform(-30.0, 30.0, (B, 3, 2)), feature=rng.normal(0.0, 1.0, (B, 24)).astype(np.float32), out9=out9)


def subsets_of(B):
    """none; a permuted subset with -1 and B among its entries (a subset has at most B entries: two requests give way to
    them, and with B = 1 there is room for -1 alone); an empty one"""
    if B == 1:
        return [None, [-1], []]
    order = [int(b) for b in np.random.default_rng(B).permutation(B)]
    order[1], order[-2] = -1, B
    return [None, order, []]


def sub_args(subset):
    """(device tensor kept alive, pointer, n_subset): an empty subset still hands over a valid pointer"""
    if subset is None:
        return None, None, 0
    t = up(np.asarray(subset if len(subset) else [0], dtype=np.int32))
    return t, _p(t), len(subset)


def guarded(rows, cols, dtype):
    """(rows + 1, cols) of sentinels: the last row is the guard behind the array"""
    return np.full((rows + 1, cols), SENT32 if dtype == np.float32 else SENT64, dtype)


def ctx_T():
    c = _lib.default_context()
    npa.BatchPlanner(ctx=c)._sync()           # the default parameters, whatever an earlier test set
    return c, float(c.params.T_min), float(c.params.T_max)


def tau_gap_ulp(got, want):
    """largest |got - want| in units of spacing(|want|) over the finite entries; NaNs must sit in the same places"""
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    return float((np.abs(got[ok] - want[ok]) / np.spacing(np.abs(want[ok]))).max()) if ok.any() else 0.0


@pytest.mark.parametrize("B", [1, 3, 70])
def test_kernels_equal_the_oracle(B):
    """1, 3 and 70 requests (70 crosses a wavefront and the head's tile of 32, with a ragged tail) under the three
    subsets: motion and head bit for bit (one feature row per request, and one shared row), the guess's waypoints bit
    for bit and its tau within 4 ulp of NumPy's -- log's argument is computed identically, the device's fp64 log and
    NumPy's are each good to 1 ulp, so 2 ulp is the derived bound and 4 the allowance.  Largest gap seen on the MI355X:
    1 ulp.  Rows outside the launch and the guard row keep their sentinels."""
    torch, dev = _torch()
    c, T_min, T_max = ctx_T()
    h = case(B)
    t = {k: up(v) for k, v in h.items()}
    w = up(blob())
    worst = 0.0
    for subset in subsets_of(B):
        keep, sp, ns = sub_args(subset)
        motion, out, out1, x0 = guarded(B, 24, np.float32), guarded(B, 9, np.float32), guarded(B, 9, np.float32), guarded(B, 7, np.float64)
        want_motion = motion.copy()
        want_motion[:B] = ion.motion(h["pose"], h["cur_vel"], h["head"], h["tail"], subset, motion[:B])
        # the head reads the oracle's motion rows, the guess its own crafted outputs: each kernel is compared alone
        full_motion = ion.motion(h["pose"], h["cur_vel"], h["head"], h["tail"])
        d_motion, d_out, d_out1, d_x0, d_full = up(motion), up(out), up(out1), up(x0), up(full_motion)
        torch.cuda.synchronize(dev)
        c.check(c.lib.neo_init_motion_dev(c.h, B, sp, ns, _p(t["pose"]), _p(t["cur_vel"]), _p(t["head"]), _p(t["tail"]), _p(d_motion)))
        c.check(c.lib.neo_init_head_dev(c.h, B, sp, ns, _p(w), w.numel(), _p(t["feature"]), B, _p(d_full), _p(d_out)))
        c.check(c.lib.neo_init_head_dev(c.h, B, sp, ns, _p(w), w.numel(), _p(t["feature"][B - 1:]), 1, _p(d_full), _p(d_out1)))
        c.check(c.lib.neo_init_guess_dev(c.h, B, sp, ns, _p(t["out9"]), _p(t["pose"]), _p(d_x0)))
        c.synchronize()
        assert same(d_motion.cpu().numpy(), want_motion), subset
        for got, feat in ((d_out, h["feature"]), (d_out1, h["feature"][B - 1:])):
            want = out.copy()
            want[:B] = ion.head(blob(), feat, full_motion, subset, out[:B])
            assert same(got.cpu().numpy(), want), subset
        want = x0.copy()
        want[:B] = ion.guess(h["out9"], h["pose"], T_min, T_max, subset, x0[:B])
        got = d_x0.cpu().numpy()
        assert same(got[:, :4], want[:, :4]), subset
        gap = tau_gap_ulp(got[:, 4:], want[:, 4:])
        worst = max(worst, gap)
        assert gap <= 4.0, (subset, gap)
        assert (got[B] == SENT64).all()
        if subset is None:
            assert got[0, 6] == 0.0 and got[0, 4] < -6.0 and got[0, 5] > 6.0
            assert B == 1 or np.isnan(got[1]).all()
            assert np.isfinite(d_out.cpu().numpy()[:B]).all()
    print(f"B = {B}: largest gap of the device's tau from NumPy's: {worst:.2f} ulp")


def test_argument_errors():
    torch, dev = _torch()
    c, T_min, T_max = ctx_T()
    B = 3
    h = case(B)
    t = {k: up(v) for k, v in h.items()}
    w = up(blob())
    motion, out, x0 = up(guarded(B, 24, np.float32)), up(guarded(B, 9, np.float32)), up(guarded(B, 7, np.float64))
    four = up(np.array([0, 1, 2, 0], dtype=np.int32))
    torch.cuda.synchronize(dev)
    calls = {
        "neo_init_motion_dev": [_p(t["pose"]), _p(t["cur_vel"]), _p(t["head"]), _p(t["tail"]), _p(motion)],
        "neo_init_head_dev": [_p(w), w.numel(), _p(t["feature"]), B, _p(motion), _p(out)],
        "neo_init_guess_dev": [_p(t["out9"]), _p(t["pose"]), _p(x0)],
    }
    for name, args in calls.items():
        fn = getattr(c.lib, name)
        for b_bad in (0, -1):
            assert fn(c.h, b_bad, None, 0, *args) == NEO_ERR_INVALID, name
            assert b"B must be >= 1" in c.lib.neo_last_error(c.h)
        assert fn(c.h, B, _p(four), 4, *args) == NEO_ERR_INVALID, name
        assert b"bad subset size" in c.lib.neo_last_error(c.h)
        assert fn(c.h, B, _p(four), -1, *args) == NEO_ERR_INVALID, name
        for k, a in enumerate(args):
            if isinstance(a, ctypes.c_void_p):
                bad = list(args)
                bad[k] = None
                assert fn(c.h, B, None, 0, *bad) == NEO_ERR_INVALID, (name, k)
                assert b"null buffer" in c.lib.neo_last_error(c.h)
    head = calls["neo_init_head_dev"]
    for n_weights in (0, w.numel() - 1, w.numel() + 1):
        assert c.lib.neo_init_head_dev(c.h, B, None, 0, head[0], n_weights, *head[2:]) == NEO_ERR_INVALID
        assert b"n_weights" in c.lib.neo_last_error(c.h)
    for rows in (0, 2, B + 1, -1):
        assert c.lib.neo_init_head_dev(c.h, B, None, 0, *head[:3], rows, *head[4:]) == NEO_ERR_INVALID
        assert b"feature_rows" in c.lib.neo_last_error(c.h)
    c.synchronize()
    assert (motion.cpu().numpy() == SENT32).all() and (out.cpu().numpy() == SENT32).all() and (x0.cpu().numpy() == SENT64).all()


# ------------------------------------------------------------------ BatchNeoPlanner and the fleet
def strip_features(img):
    """stands in for the backbone: 24 strip sums of the image in exact integer arithmetic, divided once -- a mission's
    features cannot depend on who shares the batch (a GEMM's may)"""
    torch, _ = _torch()
    n = img.shape[0]
    sums = img.reshape(n, 24, -1).to(torch.int64).sum(dim=2)
    return (sums.to(torch.float64) / (255.0 * (img[0].numel() // 24))).to(torch.float32)


def make_neo(fs, bp, stub):
    torch, dev = _torch()
    ini = _ini()
    torch.manual_seed(11)
    net = ini.PlannerNet(48, 64)
    if stub:
        net.image_features = strip_features
    return ini.BatchNeoPlanner(bp, ini.BatchInitializer(net, device=dev), fs["cam"])


def fly(fs, neo, mode, pick=None, record=False, max_replans=MAX_REPLANS):
    idx = np.arange(fs["B"]) if pick is None else np.asarray(pick)
    rec = DemoRecorder(fs["cam"], capacity=40 * len(idx)) if record else None
    loop = npa.FleetReplanLoop(neo.bp, fs["maps"][0], fs["goals"][idx], scene_ids=fs["sids"][idx], mission_ids=idx, mode=mode,
                               neo=neo, scenes=fs["packed"], scene_index=fs["scene_index"][idx], record=rec)
    out = loop.run(fs["start"][idx], max_replans=max_replans)
    return loop, rec, out


@pytest.fixture(scope="module")
def fleet():
    fs = _fleet_setup()
    bp = npa.BatchPlanner()
    neo = make_neo(fs, bp, stub=True)
    loop, _, out = fly(fs, neo, "neo")
    print(f"neo fleet of {fs['B']}: {len(loop.timings)} ticks, success {out['success'].mean():.2f}, "
          f"{out['iter_num'].sum() / max(out['opt_runs'].sum(), 1):.1f} iterations a run")
    yield fs, neo, loop, out
    c = _lib.default_context()
    for m in fs["maps"]:
        c.check(c.lib.neo_esdf_drop(c.h, m.scene_id))


def assert_same_flights(a_loop, a, b_loop, b, a_rows=None):
    """b's missions are a's missions a_rows (None: all): every result array and every command array bit for bit"""
    rows = np.arange(len(b["success"])) if a_rows is None else np.asarray(a_rows)
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k])[rows], np.asarray(b[k]), equal_nan=True), k
    for j, i in enumerate(rows):
        assert same(a_loop.commands(int(i)), b_loop.commands(j)), i


def test_plan_dev_is_plan_dev_from_the_networks_guess(fleet):
    """12 requests of the three scenes: BatchNeoPlanner.plan_dev's results are BatchPlanner.plan_dev's from x0 = neo.x0
    with the same seed, bit for bit; neo.motion and neo.x0 are the oracle's for the downloaded states"""
    torch, dev = _torch()
    fs, neo = fleet[0], fleet[1]
    c, T_min, T_max = ctx_T()
    n = 12
    rng = np.random.default_rng(8)
    head, tail = np.zeros((n, 3, 2)), np.zeros((n, 3, 2))
    head[:, 0], tail[:, 0] = fs["start"][:n], fs["goals"][:n]
    head[:, 1] = rng.uniform(-0.5, 0.5, (n, 2))
    d = fs["goals"][:n] - fs["start"][:n]
    pose = npa.DepthCamera.poses(np.concatenate([fs["start"][:n], np.full((n, 1), 2.0)], 1), np.arctan2(d[:, 1], d[:, 0]))
    vel = rng.uniform(-0.5, 0.5, (n, 2))
    slots = up(np.array([c.lib.neo_scene_slot(c.h, int(s)) for s in fs["sids"][:n]], dtype=np.int32))
    boxes, begin = (up(a) for a in fs["packed"])
    t = dict(pose=up(pose), vel=up(vel), head=up(head), tail=up(tail))
    feat = neo.features_dev(boxes, begin, t["pose"], up(fs["scene_index"][:n]))
    assert tuple(feat.shape) == (n, 24) and feat.dtype == torch.float32 and len({r.tobytes() for r in feat.cpu().numpy()}) >= 3
    a = neo.plan_dev(fs["maps"][0], t["pose"], t["vel"], t["head"], t["tail"], feat, slots=slots, seed=7)
    x0 = neo.x0.clone()
    b = neo.bp.plan_dev(fs["maps"][0], t["head"], t["tail"], x0=x0, slots=slots, seed=7)
    for k in ("x", "costs", "costs_last", "nit", "nfev", "status", "attempts", "nit_total", "solved"):
        assert same(a[k].cpu().numpy(), b[k].cpu().numpy()), k
    assert a["launch_sizes"] == b["launch_sizes"] and a["launch_sizes"][0] == n
    motion = ion.motion(pose, vel, head, tail)
    assert same(neo.motion.cpu().numpy(), motion)
    w = _ini().pack_head_weights(neo.init.net).cpu().numpy()
    out9 = ion.head(w, feat.cpu().numpy(), motion)
    assert same(neo.out.cpu().numpy(), out9)
    want = ion.guess(out9, pose, T_min, T_max)
    got = x0.cpu().numpy()
    assert same(got[:, :4], want[:, :4]) and tau_gap_ulp(got[:, 4:], want[:, 4:]) <= 4.0
    # the torch head is the other route to the same guess, within fp32 rounding of the network's outputs
    x0_t = neo.warm_start_dev(t["pose"], t["vel"], t["head"], t["tail"], feat, head_impl="torch")
    c.synchronize()
    assert x0_t is neo.x0 and np.abs(neo.out.cpu().numpy() - out9).max() <= 1e-5
    with pytest.raises(ValueError):
        neo.warm_start_dev(t["pose"], t["vel"], t["head"], t["tail"], feat, head_impl="mfma")


def test_mission_3_alone_flies_as_in_the_fleet(fleet):
    fs, neo, loop, out = fleet
    one, _, o1 = fly(fs, neo, "neo", pick=[3])
    assert int(out["replans"][3]) > 1
    assert_same_flights(loop, out, one, o1, a_rows=[3])


def test_recording_changes_no_neo_flight(fleet):
    fs, neo, loop, out = fleet
    rec_loop, rec, o = fly(fs, neo, "neo", record=True)
    assert_same_flights(loop, out, rec_loop, o)
    assert rec.n_rows == int(o["replans"].sum()) > fs["B"]
    assert all("neo_s" in t and "record_s" in t for t in rec_loop.timings) and all("record_s" not in t for t in loop.timings)


def test_nn_mode_flies_the_networks_guess(fleet):
    """max_replans = 0: the first plan alone, unoptimised -- no optimiser run is counted, the resident plan is the
    network's guess (the oracle's, for the loop's downloaded states) and every command array starts at its start"""
    fs, neo = fleet[0], fleet[1]
    c, T_min, T_max = ctx_T()
    loop, _, out = fly(fs, neo, "nn", max_replans=0)
    assert (out["iter_num"] == 0).all() and (out["opt_runs"] == 0).all()
    x = loop.x
    assert x.shape == (fs["B"], 7) and same(x, neo.x0.cpu().numpy()) and not x.flags.writeable
    d = {k: loop._dev[k].cpu().numpy() for k in ("pose", "cur_vel", "head", "tail", "feature")}
    w = _ini().pack_head_weights(neo.init.net).cpu().numpy()
    want = ion.guess(ion.head(w, d["feature"], ion.motion(d["pose"], d["cur_vel"], d["head"], d["tail"])), d["pose"], T_min, T_max)
    assert same(x[:, :4], want[:, :4]) and tau_gap_ulp(x[:, 4:], want[:, 4:]) <= 4.0
    assert (out["replans"] + out["failed_attempts"] >= 1).all() and (out["replans"] == 1).any()
    for i in np.flatnonzero(out["replans"] == 1):
        assert np.array_equal(loop.commands(int(i))[0, 0], fs["start"][i]), i


def test_neo_mode_with_the_real_backbone_runs_to_the_end(fleet):
    fs = fleet[0]
    neo = make_neo(fs, npa.BatchPlanner(), stub=False)
    loop, _, out = fly(fs, neo, "neo")
    for i in range(fs["B"]):
        assert np.isfinite(loop.commands(i)).all(), i
    assert (out["opt_runs"] >= out["replans"]).all() and (out["replans"] >= 1).any()
    print(f"neo fleet with the ResNet backbone (untrained): {out['success'].mean():.2f} reach the goal, "
          f"{out['iter_num'].sum() / max(out['opt_runs'].sum(), 1):.1f} iterations a run")


def test_basic_resident_flies_as_before(fleet):
    """the new code stays off the old paths: mode "basic" with resident=True gives the result arrays of the host-array
    loop of test_gpu_record.py, bit for bit"""
    fs = fleet[0]
    a_loop, _, a = _fly(fs, record=False)
    b_loop, _, b = _fly(fs, record=False, resident=True)
    assert_same_flights(a_loop, a, b_loop, b)
    assert all("neo_s" not in t for t in b_loop.timings)
