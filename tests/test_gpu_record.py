"""The fleet's record mode on the GPU: neo_record_state_dev and neo_record_commit_dev against the NumPy model
(tests/record_oracle_np.py) bit for bit, the capacity of the dataset, a row's independence of the launch, the argument
errors, FleetReplanLoop(record=...) against the same fleet without it, and the trainer on the recorded rows."""
import ctypes

import numpy as np
import pytest

import depth_oracle_np as don
import record_oracle_np as ron
import neo_planner_amd as npa
from neo_planner_amd import _lib, synth
from neo_planner_amd.depth import DepthCamera
from neo_planner_amd.record import DemoRecorder, FIELDS

pytestmark = pytest.mark.gpu

NEO_ERR_INVALID = 1
CAP = 8                                                     # rows of a mission's command array in the kernel tests
SENTINEL = dict(motion=-7.25, wpts_local=-7.25, tau=-7.25, pose=-7.25, meta=-77, images=0xAB)


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------ kernels against the oracle
_CASES = {}


def mission_case(b, M, W, H):
    """everything the kernels read of mission b; it depends on b (and the shape) alone, so a fleet of 3 is the head of a
    fleet of 70.  cmd_len is 0 for every third mission (the first plan), cmd_index lies beyond the array for some (the
    kernel clamps), a quarter of the missions did not solve."""
    key = (b, M, W, H)
    if key not in _CASES:
        rng = np.random.default_rng([1000 + b, M, W, H])
        yaw = rng.uniform(-np.pi, np.pi)
        cmd_len = 0 if b % 3 == 1 else int(rng.integers(1, CAP + 1))
        _CASES[key] = dict(
            pose=np.array([rng.uniform(0.0, 30.0), rng.uniform(-15.0, 15.0), 2.0, np.cos(yaw), np.sin(yaw)]),
            head=rng.uniform(-30.0, 30.0, (3, 2)), tail=rng.uniform(-30.0, 30.0, (3, 2)),
            x=np.concatenate([rng.uniform(-30.0, 30.0, 2 * (M - 1)), rng.uniform(-4.0, 4.0, M)]),
            cmd=rng.uniform(-5.0, 5.0, (CAP, 3, 2)), cmd_len=cmd_len,
            cmd_index=cmd_len + 2 if b % 7 == 5 else int(rng.integers(0, max(cmd_len, 1))),
            solved=int(b % 4 != 2), image=rng.integers(0, 256, (H, W), dtype=np.uint8))
    return _CASES[key]


def fleet_case(missions, M, W, H):
    cs = [mission_case(b, M, W, H) for b in missions]
    host = {k: np.ascontiguousarray(np.stack([np.asarray(c[k]) for c in cs])) for k in cs[0]}
    for k in ("cmd_len", "cmd_index", "solved"):
        host[k] = host[k].astype(np.int32)
    host["mission_ids"] = np.asarray(missions, dtype=np.int32)
    return host


class Device:
    """a fleet case and a dataset of capacity + 1 rows (the last one a guard) on the GPU"""

    def __init__(self, host, capacity, M, W, H):
        torch, dev = _torch()
        self.host, self.capacity, self.M, self.W, self.H = host, capacity, M, W, H
        self.B = host["x"].shape[0]
        self.t = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
        self.t["cur_vel"] = torch.full((self.B, 2), -3.5, dtype=torch.float64, device=dev)
        self.t["row_of"] = torch.full((self.B,), -9, dtype=torch.int32, device=dev)
        self.t["n_rows"] = torch.zeros(1, dtype=torch.int32, device=dev)
        self.t["dropped"] = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ref = ron.empty_dataset(capacity + 1, M, H, W, SENTINEL)
        self.data = {k: torch.from_numpy(v.copy()).to(dev) for k, v in self.ref.items()}
        self.ref_n = self.ref_dropped = 0
        self.ref_vel = np.full((self.B, 2), -3.5)
        torch.cuda.synchronize(dev)

    def sub(self, subset):
        torch, dev = _torch()
        return None if subset is None else torch.from_numpy(np.asarray(subset, dtype=np.int32)).to(dev)

    def state(self, subset=None):
        torch, dev = _torch()
        c, t, s = _lib.default_context(), self.t, self.sub(subset)
        torch.cuda.synchronize(dev)
        c.check(c.lib.neo_record_state_dev(c.h, self.B, _p(s), 0 if s is None else len(subset), _p(t["cmd"]), CAP,
                                           _p(t["cmd_len"]), _p(t["cmd_index"]), _p(t["head"]), _p(t["cur_vel"])))
        c.synchronize()
        h = self.host
        self.ref_vel = ron.state(h["cmd"], h["cmd_len"], h["cmd_index"], h["head"], subset, self.ref_vel)
        return t["cur_vel"].cpu().numpy()

    def commit_rc(self, subset=None, tick=0, round_=0, **over):
        torch, dev = _torch()
        c, t, d, s = _lib.default_context(), self.t, self.data, self.sub(subset)
        a = dict(B=self.B, M=self.M, W=self.W, H=self.H, capacity=self.capacity)
        ptr = {k: _p(v) for k, v in list(t.items()) + [("data_" + k, v) for k, v in d.items()]}
        for k, v in over.items():
            if k in a:
                a[k] = v
            else:
                assert k in ptr and v is None
                ptr[k] = None
        torch.cuda.synchronize(dev)
        rc = c.lib.neo_record_commit_dev(
            c.h, a["B"], _p(s), 0 if s is None else len(subset), a["M"], ptr["x"], ptr["head"], ptr["tail"], ptr["solved"],
            ptr["pose"], ptr["cur_vel"], ptr["image"], a["W"], a["H"], ptr["mission_ids"], tick, round_, a["capacity"],
            ptr["data_motion"], ptr["data_wpts_local"], ptr["data_tau"], ptr["data_pose"], ptr["data_meta"], ptr["data_images"],
            ptr["row_of"], ptr["n_rows"], ptr["dropped"])
        c.synchronize()
        return rc

    def commit(self, subset=None, tick=0, round_=0):
        """the call on the GPU and in the oracle; returns the two row_of"""
        assert self.commit_rc(subset, tick, round_) == 0
        h = self.host
        row_of, self.ref_n, self.ref_dropped = ron.commit(
            self.ref, self.capacity, self.ref_n, self.ref_dropped, self.M, h["x"], h["head"], h["tail"], h["solved"], h["pose"],
            self.ref_vel, h["image"], subset, h["mission_ids"], tick, round_)
        n = self.B if subset is None else len(subset)
        return self.t["row_of"].cpu().numpy()[:n], row_of

    def check(self):
        """every array, guard row included, bit for bit; the counters"""
        for k in FIELDS:
            got = self.data[k].cpu().numpy()
            assert same(got, self.ref[k]), k
            assert (got[self.capacity] == SENTINEL[k]).all(), f"guard row of {k}"
        assert int(self.t["n_rows"].item()) == self.ref_n and int(self.t["dropped"].item()) == self.ref_dropped


def subsets_of(B):
    """two launches: most missions in a shuffled order (with an index outside the fleet among them), then all of them"""
    if B == 1:
        return None, [0]
    order = np.random.default_rng(B).permutation(B)
    first = [int(b) for b in order if b % 5 != 3]
    first = first[:-1]                                      # (a subset has at most B entries)
    return first[:len(first) // 2] + [B + 4] + first[len(first) // 2:], None


@pytest.mark.parametrize("M", [3, 5])
@pytest.mark.parametrize("B", [1, 3, 70])
@pytest.mark.parametrize("size", [(64, 48), (61, 37), (5, 3)])
def test_state_and_commit_equal_the_oracle(size, B, M):
    """1, 3 and 70 missions, images whose size is a multiple of 16 bytes and two that are not (rows then start anywhere
    inside 16 bytes), M = 3 and 5: the velocities, then two commits one after the other"""
    W, H = size
    dv = Device(fleet_case(range(B), M, W, H), capacity=2 * B + 3, M=M, W=W, H=H)
    s0, s1 = subsets_of(B)
    # missions outside the state launch keep what the buffer held; then the rest
    assert same(dv.state(s0), dv.ref_vel)
    assert same(dv.state(None), dv.ref_vel)
    h = dv.host
    for b in range(B):
        want = h["head"][b, 1] if h["cmd_len"][b] == 0 else h["cmd"][b, min(h["cmd_index"][b], h["cmd_len"][b] - 1), 1]
        assert np.array_equal(dv.ref_vel[b], want)
    for tick, (r, s) in enumerate([(0, s0), (1, s1)]):
        got, want = dv.commit(s, tick=3 + tick, round_=r)
        assert np.array_equal(got, want)
        dv.check()
    if B >= 3:
        assert 0 < dv.ref_n < 2 * B and (h["solved"] == 0).any() and (h["cmd_len"] == 0).any() and (h["cmd_len"] >= 1).any()
        assert dv.ref_dropped == 0


@pytest.mark.parametrize("B", [70, 2500])
def test_capacity(B):
    """fewer rows than missions that solved -- 2500 missions take the rank kernel through three chunks --: the first
    `capacity` of them in order, the others counted, the guard row of every array untouched; a commit into the full
    dataset changes nothing but the count"""
    W, H, M = (61, 37, 3) if B == 70 else (5, 3, 3)
    capacity = 20 if B == 70 else 1100
    dv = Device(fleet_case(range(B), M, W, H), capacity=capacity, M=M, W=W, H=H)
    dv.state(None)
    got, want = dv.commit(None, tick=1)
    assert np.array_equal(got, want)
    dv.check()
    solved = np.flatnonzero(dv.host["solved"])
    assert solved.size > capacity and dv.ref_n == capacity and dv.ref_dropped == solved.size - capacity
    assert np.array_equal(np.flatnonzero(got >= 0), solved[:capacity]) and np.array_equal(got[solved[:capacity]], np.arange(capacity))
    assert np.array_equal(dv.data["meta"].cpu().numpy()[:capacity, 0], solved[:capacity])
    got, want = dv.commit(None, tick=2)
    assert (got == -1).all() and np.array_equal(got, want)
    dv.check()
    assert dv.ref_dropped == 2 * solved.size - capacity


def test_a_row_does_not_depend_on_the_launch():
    """a mission alone, and among 70 at another position, with another row number and so another place inside 16 bytes"""
    W, H, M = 61, 37, 5
    among = Device(fleet_case(range(70), M, W, H), capacity=80, M=M, W=W, H=H)
    among.state(None)
    s0, _ = subsets_of(70)
    got, _ = among.commit(s0, tick=4, round_=2)
    among.check()
    k = next(k for k, b in enumerate(s0) if got[k] > 0 and (int(got[k]) * W * H) % 16 != 0 and b != k and b >= 20)
    m, row = s0[k], int(got[k])
    alone = Device(fleet_case([m], M, W, H), capacity=2, M=M, W=W, H=H)
    alone.state(None)
    assert alone.commit(None, tick=4, round_=2)[0].tolist() == [0]
    alone.check()
    for f in FIELDS:
        assert same(among.data[f][row].cpu().numpy(), alone.data[f][0].cpu().numpy()), f
    assert int(alone.data["meta"][0, 0].item()) == m


def test_argument_errors():
    W, H, M = 5, 3, 3
    dv = Device(fleet_case(range(3), M, W, H), capacity=4, M=M, W=W, H=H)
    bad = [dict(B=0), dict(B=-1), dict(M=1), dict(M=65), dict(capacity=0), dict(W=0), dict(W=4097), dict(H=0), dict(H=4097)]
    bad += [{k: None} for k in ("x", "head", "tail", "pose", "cur_vel", "image", "row_of", "n_rows", "dropped", "data_motion",
                                "data_wpts_local", "data_tau", "data_pose", "data_meta", "data_images")]
    for over in bad:
        assert dv.commit_rc(None, **over) == NEO_ERR_INVALID, over
    assert dv.commit_rc([0, 1, 2, 0]) == NEO_ERR_INVALID           # more entries than missions
    c, t = _lib.default_context(), dv.t
    args = [_p(t["cmd"]), CAP, _p(t["cmd_len"]), _p(t["cmd_index"]), _p(t["head"]), _p(t["cur_vel"])]
    assert c.lib.neo_record_state_dev(c.h, 0, None, 0, *args) == NEO_ERR_INVALID
    assert b"B must be >= 1" in c.lib.neo_last_error(c.h)
    for k in (0, 2, 3, 4, 5):
        a = list(args)
        a[k] = None
        assert c.lib.neo_record_state_dev(c.h, 3, None, 0, *a) == NEO_ERR_INVALID, k
    a = list(args)
    a[1] = 0
    assert c.lib.neo_record_state_dev(c.h, 3, None, 0, *a) == NEO_ERR_INVALID
    c.synchronize()
    dv.check()                                                      # nothing was launched: sentinels and zero counters
    assert (t["cur_vel"].cpu().numpy() == -3.5).all() and (t["row_of"].cpu().numpy() == -9).all()
    # optional pointers: without solved every launched mission gets a row, without mission_ids its index
    assert dv.commit_rc(None, solved=None, mission_ids=None) == 0
    assert int(t["n_rows"].item()) == 3 and dv.data["meta"].cpu().numpy()[:3, 0].tolist() == [0, 1, 2]


# ------------------------------------------------------------------ the fleet
FLEET_CAM = dict(width=64, height=48)
MAX_REPLANS = 25


def _fleet_setup():
    scenes = [don.boxes_of(synth.forest_boxes(s)) for s in (0, 1, 2)]
    maps = []
    for s in (0, 1, 2):
        m = npa.ESDF()
        m.occupancy_map_cb(synth.OccupancyGridMsg(synth.occupancy_2d(s)))
        maps.append(m)
    B = 24
    scene_index = (np.arange(B) % 3).astype(np.int32)
    rng = np.random.default_rng(42)
    start = np.stack([np.full(B, 0.5), np.linspace(-3.0, 3.0, B)], 1)
    th = rng.uniform(-0.3, 0.3, B)
    goals = start + rng.uniform(10.0, 12.0, B)[:, None] * np.stack([np.cos(th), np.sin(th)], 1)
    sids = np.array([maps[s].scene_id for s in scene_index], dtype=np.int32)
    return dict(scenes=scenes, packed=DepthCamera.pack_scenes(scenes), maps=maps, B=B, scene_index=scene_index, start=start,
                goals=goals, sids=sids, cam=DepthCamera(**FLEET_CAM))


def _fly(fs, pick=None, record=True, **kw):
    idx = np.arange(fs["B"]) if pick is None else np.asarray(pick)
    rec = DemoRecorder(fs["cam"], capacity=40 * len(idx)) if record else None
    extra = dict(record=rec, scenes=fs["packed"], scene_index=fs["scene_index"][idx]) if record else {}
    loop = npa.FleetReplanLoop(npa.BatchPlanner(), fs["maps"][0], fs["goals"][idx], scene_ids=fs["sids"][idx], mission_ids=idx,
                               **extra, **kw)
    out = loop.run(fs["start"][idx], max_replans=MAX_REPLANS)
    return loop, rec, out


@pytest.fixture(scope="module")
def fleet():
    fs = _fleet_setup()
    loop, rec, out = _fly(fs)
    rows = rec.rows()
    print(f"recorded fleet of {fs['B']}: {rec.n_rows} rows in {len(loop.timings)} ticks, success {out['success'].mean():.2f}")
    yield fs, loop, rec, out, rows
    c = _lib.default_context()
    for m in fs["maps"]:
        c.check(c.lib.neo_esdf_drop(c.h, m.scene_id))


def rows_of_missions(rows, ids):
    keep = np.isin(rows["meta"][:, 0], ids)
    return {k: v[keep] for k, v in rows.items()}


def assert_same_rows(a, b):
    assert set(a) == set(b)
    for k in a:
        assert same(a[k], b[k]), k


def test_recording_changes_no_flight(fleet):
    fs, loop, rec, out, rows = fleet
    plain, none, ref = _fly(fs, record=False)
    assert none is None and set(ref) == set(out)
    for k in ref:
        assert np.array_equal(np.asarray(ref[k]), np.asarray(out[k]), equal_nan=True), k
    for i in range(fs["B"]):
        assert np.array_equal(plain.commands(i), loop.commands(i)), i
    assert all("record_s" not in t for t in plain.timings) and all("record_s" in t for t in loop.timings)


def test_rows_counters_and_order(fleet):
    fs, loop, rec, out, rows = fleet
    n = rec.n_rows
    assert n == int(out["replans"].sum()) > fs["B"] and rec.dropped == 0
    assert all(rows[k].shape[0] == n for k in rows)
    meta = rows["meta"]
    order = np.lexsort((meta[:, 0], meta[:, 2], meta[:, 1]))            # by tick, then round, then mission
    assert np.array_equal(order, np.arange(n))
    assert len({tuple(m) for m in meta.tolist()}) == n
    assert np.array_equal(np.bincount(meta[:, 0], minlength=fs["B"]), out["replans"])
    # the first plan: at rest at the start, looking at the goal, the plan starts where the vehicle is
    first = meta[:, 1] == 0
    assert first.any() and not first.all()
    assert np.array_equal(rows["pose"][first][:, :2], fs["start"][meta[first, 0]])
    assert (rows["motion"][first][:, :3] == 0.0).all() and (rows["motion"][first][:, 12:18] == 0.0).all()
    assert (rows["motion"][~first][:, 0] > 0.0).any()                    # later the vehicle moves, forward in its own frame
    assert (rows["ts"] > 0.5).all() and (rows["ts"] < 5.0).all()
    assert (rows["motion"][:, 14] == 0.0).all() and (rows["wpts_local"][:, 2::3] == 0.0).all()


def test_images_are_what_the_camera_sees_from_the_stored_poses(fleet):
    fs, loop, rec, out, rows = fleet
    torch, dev = _torch()
    boxes, begin = fs["packed"]
    sidx = fs["scene_index"][rows["meta"][:, 0]]
    img = fs["cam"].render_dev(torch.from_numpy(boxes).to(dev), torch.from_numpy(begin).to(dev),
                               torch.from_numpy(rows["pose"]).to(dev), torch.from_numpy(sidx).to(dev), want_m=False)["depth_u8"]
    assert np.array_equal(img.cpu().numpy(), rows["images"])
    assert len({r.tobytes() for r in rows["images"]}) >= 10


def test_a_second_run_after_reset_stores_the_same_bytes(fleet):
    fs, loop, rec, out, rows = fleet
    rec.reset()
    assert rec.n_rows == 0 and rec.dropped == 0
    loop.run(fs["start"], max_replans=MAX_REPLANS)
    assert_same_rows(rec.rows(), rows)


def test_mission_3_alone_records_the_fleets_rows(fleet):
    fs, loop, rec, out, rows = fleet
    one, rec1, o1 = _fly(fs, pick=[3])
    assert np.array_equal(one.commands(0), loop.commands(3))
    want = rows_of_missions(rows, [3])
    assert want["meta"].shape[0] == int(out["replans"][3]) > 1
    assert_same_rows(rec1.rows(), want)


def test_resident_records_the_same_rows(fleet):
    fs, loop, rec, out, rows = fleet
    pick = list(range(8))
    res_loop, res_rec, res = _fly(fs, pick=pick, resident=True)
    assert_same_rows(res_rec.rows(), rows_of_missions(rows, pick))


def test_batch_mode_records_the_same_rows_resident_or_not(fleet):
    fs = fleet[0]
    pick = list(range(8))
    a_loop, a_rec, a = _fly(fs, pick=pick, mode="batch", resident=False)
    b_loop, b_rec, b = _fly(fs, pick=pick, mode="batch", resident=True)
    assert a_rec.n_rows == int(a["replans"].sum()) > len(pick)
    assert_same_rows(a_rec.rows(), b_rec.rows())


def test_recording_on_onboard_maps(fleet):
    """with onboard= as well the recorder takes the poses the mapper sensed from: the flights are those of the onboard
    fleet without a recorder, and every image is what the camera sees from its row's pose"""
    from neo_planner_amd.onboard import OnboardMapper
    fs = fleet[0]
    torch, dev = _torch()
    pick = np.arange(4)
    runs = []
    for record in (False, True):
        mapper = OnboardMapper(_lib.default_context(), fs["cam"], len(pick))
        rec = DemoRecorder(fs["cam"], capacity=40 * len(pick)) if record else None
        loop = npa.FleetReplanLoop(npa.BatchPlanner(), fs["maps"][0], fs["goals"][pick], scene_ids=fs["sids"][pick],
                                   mission_ids=pick, onboard=mapper, scenes=fs["packed"], scene_index=fs["scene_index"][pick],
                                   record_poses=True, record=rec)
        out = loop.run(fs["start"][pick], max_replans=MAX_REPLANS)
        runs.append((out, [loop.commands(i) for i in range(len(pick))], mapper.occupancy.cpu().numpy(), rec))
        mapper.close()
    (a, a_cmd, a_occ, _), (b, b_cmd, b_occ, rec) = runs
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k
    assert all(np.array_equal(x, y) for x, y in zip(a_cmd, b_cmd)) and np.array_equal(a_occ, b_occ)
    rows = rec.rows()
    assert rec.n_rows == int(b["replans"].sum()) > len(pick) and rec.dropped == 0
    for pose, (mission, tick, _) in zip(rows["pose"], rows["meta"]):
        assert np.array_equal(pose, b["poses"][tick, mission])
    boxes, begin = fs["packed"]
    img = fs["cam"].render_dev(torch.from_numpy(boxes).to(dev), torch.from_numpy(begin).to(dev), torch.from_numpy(rows["pose"]).to(dev),
                               torch.from_numpy(fs["scene_index"][rows["meta"][:, 0]]).to(dev), want_m=False)["depth_u8"]
    assert np.array_equal(img.cpu().numpy(), rows["images"])


def test_record_needs_scenes(fleet):
    fs = fleet[0]
    with pytest.raises(ValueError):
        npa.FleetReplanLoop(npa.BatchPlanner(), fs["maps"][0], fs["goals"], record=fleet[2])
    with pytest.raises(ValueError):
        npa.FleetReplanLoop(npa.BatchPlanner(), fs["maps"][0], fs["goals"], scenes=fs["packed"],
                            record=DemoRecorder(fs["cam"], capacity=4, M=5))


def test_training_on_the_gpu(fleet):
    """two epochs on the fleet's first 96 rows in batches of 8 (24 steps): the losses are finite and the network came
    back on the GPU"""
    fs, loop, rec, out, rows = fleet
    from neo_planner_amd import initializer as ini
    torch, dev = _torch()
    inputs, labels = rec.training_tensors(rows)
    assert inputs.shape == (rows["meta"].shape[0], 48 * 64 + 24) and labels.shape[1] == 9 and inputs.shape[0] >= 96
    net, losses, held_out = npa.train_initializer(inputs[:96], labels[:96], net=ini.PlannerNet(48, 64), epochs=2, batch_size=8,
                                                  device=dev)
    print(f"training loss per epoch {losses}, held out {held_out:.4f}")
    assert len(losses) == 2 and np.isfinite(losses).all() and np.isfinite(held_out)
    assert next(net.parameters()).is_cuda
