"""The geo warm start on the GPU (neo_geo_search_batch[_dev], neo_geo_prune_batch, BatchPlanner.geo_init / geo_plan,
GeoPlanner, ReplanLoop(mode="geo")) against the reference's own results (tests/golden/g7_geo_*.npz) and against the CPU
restatement (tests/geo_oracle_np.py): paths, costs and key nodes equal, not close."""
import ctypes
import os

import numpy as np
import pytest

import geo_oracle_np as geo
import neo_planner_amd as npa
from neo_planner_amd import _lib, synth
from neo_planner_amd.replan import ReplanLoop

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENES = ("scene0", "scene1", "scene2", "res025", "pocket")
NEO_ERR_INVALID, NEO_ERR_NO_MAP, NEO_ERR_UNSUPPORTED = 1, 3, 4
F = _lib


def fixture(name):
    return np.load(os.path.join(GOLDEN, f"g7_geo_{name}.npz"))


def gpu_map(occ, res=synth.RES, origin=(0.0, -15.0)):
    m = npa.ESDF()
    m.occupancy_map_cb(synth.OccupancyGridMsg(np.asarray(occ), res, tuple(float(v) for v in origin)))
    return m


def cpu_map(gm):
    return geo.Map(gm.esdf_map, gm.map_resolution, (gm.map_origin.x, gm.map_origin.y))


_MAPS = {}


def scene(name):
    """(GPU map, oracle map) of a fixture's map, built once"""
    if name not in _MAPS:
        d = fixture(name)
        gm = gpu_map(d["occ"], float(d["res"]), d["origin"])
        _MAPS[name] = (gm, cpu_map(gm))
    return _MAPS[name]


def check_equal(out, ref, idx=None):
    idx = range(len(ref)) if idx is None else idx
    for k, i in enumerate(idx):
        path, cost, nexp, flags = ref[i][:4]
        n = len(path)
        assert out["path_len"][k] == n, (i, out["path_len"][k], n)
        assert out["path_cost"][k] == cost, i
        assert out["expansions"][k] == nexp, (i, out["expansions"][k], nexp)
        assert out["flags"][k] & 7 == flags, (i, out["flags"][k], flags)
        if "paths" in out and n <= out["paths"].shape[1]:
            assert np.array_equal(out["paths"][k, :n], np.array(path)), i


def oracle(cm, starts, targets, max_expansions=0):
    g = geo.Grid(cm)
    res = []
    for s, t in zip(starts, targets):
        path, cost, nexp, flags = geo.astar(g, s, t, max_expansions)
        res.append((path, cost, nexp, flags, geo.prune(cm, path)[0]))
    return res


def test_gpu_equals_reference_fixtures():
    bp = npa.BatchPlanner()
    for name in SCENES:
        d = fixture(name)
        gm, _ = scene(name)
        cap = int(d["path_len"].max())
        out = bp.geo_init(gm, d["start"], d["target"], path_cap=cap)
        assert np.array_equal(out["path_len"], d["path_len"]), name
        assert np.array_equal(out["path_cost"], d["path_cost"]), name
        assert np.array_equal(out["key_pts"], d["pruned"]), name
        for i, n in enumerate(d["path_len"]):
            assert np.array_equal(out["paths"][i, :n], d["paths"][i, :n]), (name, i)
            assert np.isnan(out["paths"][i, n:]).all(), (name, i)
        assert np.array_equal(out["int_wpts"], d["pruned"][:, 1:3].transpose(0, 2, 1))
        assert np.allclose(out["ts"], 2.5 * np.array([1.5, 1.0, 1.5]))
        assert not np.any(out["flags"] & (F.NEO_GEO_FLAG_CAPPED | F.NEO_GEO_FLAG_PATH_TRUNCATED))


def test_prune_batch_on_reference_paths():
    bp = npa.BatchPlanner()
    for name in SCENES:
        d = fixture(name)
        gm, _ = scene(name)
        paths = np.nan_to_num(d["paths"])
        kp = bp.geo_prune(gm, paths, d["path_len"])
        assert np.array_equal(kp, d["pruned"]), name


def random_requests(cm, n, rng, reach=8.0):
    """starts anywhere on the expanded grid (some in collision, some just outside), targets near them, on and beyond the
    expanded border, some blocked"""
    g = geo.Grid(cm)
    x0, x1 = g.oxe - 0.3, g.oxe + g.We * cm.res + 0.3
    y0, y1 = g.oye - 0.3, g.oye + g.He * cm.res + 0.3
    starts = np.column_stack([rng.uniform(x0, x1, n), rng.uniform(y0, y1, n)])
    targets = starts + rng.uniform(-reach, reach, (n, 2))
    k = n // 8
    targets[:k, 0] = rng.choice([x0 - 0.05, x1 + 0.05, g.oxe + 0.01, g.oxe + (g.We - 1) * cm.res + 0.02], k)
    return starts, targets


def test_gpu_equals_restatement_on_random_requests():
    bp = npa.BatchPlanner()
    rng = np.random.default_rng(3)
    seen = 0
    for name, n in (("scene0", 80), ("scene1", 80), ("scene2", 60), ("res025", 60), ("pocket", 40)):
        gm, cm = scene(name)
        starts, targets = random_requests(cm, n, rng, reach=8.0 if name.startswith("scene") else 3.0)
        ref = oracle(cm, starts, targets)
        out = bp.geo_init(gm, starts, targets, path_cap=max(len(r[0]) for r in ref))
        check_equal(out, ref)
        assert np.array_equal(out["key_pts"], np.array([r[4] for r in ref])), name
        seen |= np.bitwise_or.reduce(out["flags"])
    assert seen & F.NEO_GEO_FLAG_NO_PATH and seen & F.NEO_GEO_FLAG_START_OUTSIDE


def test_multi_scene_batches():
    bp = npa.BatchPlanner()
    rng = np.random.default_rng(5)
    names = ("scene0", "scene1", "res025", "pocket")
    starts, targets, sids, refs = [], [], [], []
    for name in names:
        gm, cm = scene(name)
        s, t = random_requests(cm, 12, rng, reach=4.0)
        r = oracle(cm, s, t)
        starts.append(s); targets.append(t); sids += [gm.scene_id] * 12; refs += r
    perm = rng.permutation(len(sids))
    S, T = np.concatenate(starts)[perm], np.concatenate(targets)[perm]
    out = bp.geo_init(scene("scene2")[0], S, T, scene_ids=np.array(sids, np.int32)[perm], path_cap=2048)
    check_equal(out, [refs[i] for i in perm])
    assert np.array_equal(out["key_pts"], np.array([refs[i][4] for i in perm]))


def _local_requests(B, rng):
    """cfg2-style 2-D requests on scene 0: starts in free space, 5 m local targets toward random goals"""
    gm, cm = scene("scene0")
    starts, targets = [], []
    while len(starts) < B:
        s = np.array([rng.uniform(0.5, 29.5), rng.uniform(-14.5, 14.5)])
        if cm.dist(*s) < 0.6:
            continue
        a = rng.uniform(-np.pi, np.pi)
        starts.append(s)
        targets.append(s + 5.0 * np.array([np.cos(a), np.sin(a)]))
    return gm, np.array(starts), np.array(targets)


def test_results_do_not_depend_on_the_batch():
    bp = npa.BatchPlanner()
    gm, S, T = _local_requests(4096, np.random.default_rng(11))
    full = bp.geo_init(gm, S, T, path_cap=512)
    perm = np.random.default_rng(12).permutation(4096)
    pm = bp.geo_init(gm, S[perm], T[perm], path_cap=512)
    for k in ("key_pts", "path_len", "path_cost", "expansions", "flags", "paths"):
        assert np.array_equal(pm[k], full[k][perm], equal_nan=True), k
    for i in (0, 17, 4095):
        one = bp.geo_init(gm, S[i:i + 1], T[i:i + 1], path_cap=512)
        for k in ("key_pts", "path_len", "path_cost", "expansions", "flags", "paths"):
            assert np.array_equal(one[k][0], full[k][i], equal_nan=True), (k, i)
    # and a sample of them against the restatement
    cm = scene("scene0")[1]
    idx = np.arange(0, 4096, 97)
    check_equal({k: full[k][idx] for k in full}, oracle(cm, S[idx], T[idx]))


def test_dev_form_equals_host_form():
    torch = pytest.importorskip("torch")
    bp = npa.BatchPlanner()
    gm, S, T = _local_requests(300, np.random.default_rng(13))
    host = bp.geo_init(gm, S, T, path_cap=64)
    dev = torch.device("cuda:0")
    B = len(S)
    kp = torch.zeros((B, 4, 2), dtype=torch.float64, device=dev)
    cost = torch.zeros(B, dtype=torch.float64, device=dev)
    plen, nexp, flags = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3))
    paths = torch.zeros((B, 64, 2), dtype=torch.float64, device=dev)
    st = torch.tensor(S, device=dev); tg = torch.tensor(T, device=dev)
    bp.geo_init_dev(gm, st, tg, kp, plen, cost, nexp, flags, paths=paths)
    bp.ctx.synchronize()
    assert np.array_equal(kp.cpu().numpy(), host["key_pts"])
    assert np.array_equal(cost.cpu().numpy(), host["path_cost"])
    assert np.array_equal(plen.cpu().numpy(), host["path_len"])
    assert np.array_equal(nexp.cpu().numpy(), host["expansions"])
    assert np.array_equal(flags.cpu().numpy(), host["flags"])
    assert np.array_equal(paths.cpu().numpy(), host["paths"], equal_nan=True)
    # slots: two scenes, and a slot outside the table
    g1 = scene("scene1")[0]
    slots = torch.tensor([npa.default_context().lib.neo_scene_slot(bp.ctx.h, s) for s in
                          ([gm.scene_id, g1.scene_id] * (B // 2))], dtype=torch.int32, device=dev)
    slots[5] = 1000
    bp.geo_init_dev(gm, st, tg, kp, plen, cost, nexp, flags, slots=slots)
    bp.ctx.synchronize()
    ref = bp.geo_init(gm, S, T, scene_ids=np.array([gm.scene_id, g1.scene_id] * (B // 2), np.int32))
    f = flags.cpu().numpy()
    assert f[5] == F.NEO_GEO_FLAG_BAD_SCENE
    ok = np.arange(B) != 5
    assert np.array_equal(kp.cpu().numpy()[ok], ref["key_pts"][ok])
    assert np.array_equal(f[ok], ref["flags"][ok])


def test_max_expansions_and_path_cap():
    bp = npa.BatchPlanner()
    gm, cm = scene("scene0")
    S = np.array([[1.0, 0.0], [1.0, 0.0], [2.0, 3.0]])
    T = np.array([[9.0, 1.0], [1.05, 0.02], [6.0, -3.0]])
    ref = oracle(cm, S, T)
    full = bp.geo_init(gm, S, T, path_cap=1024)
    cap = int(ref[0][2]) // 2
    capped = bp.geo_init(gm, S, T, max_expansions=cap, path_cap=1024)
    check_equal(capped, oracle(cm, S, T, max_expansions=cap))
    assert capped["flags"][0] == F.NEO_GEO_FLAG_CAPPED and capped["expansions"][0] == cap
    assert capped["path_len"][0] == 1
    # enough expansions: the reference's result
    loose = bp.geo_init(gm, S, T, max_expansions=max(int(r[2]) for r in ref), path_cap=1024)
    for k in ("key_pts", "path_len", "path_cost", "expansions", "flags", "paths"):
        assert np.array_equal(loose[k], full[k], equal_nan=True), k
    # a short copy: only the copied path is cut
    short = bp.geo_init(gm, S, T, path_cap=5)
    assert short["flags"][0] == F.NEO_GEO_FLAG_PATH_TRUNCATED and short["flags"][1] == 0
    for k in ("key_pts", "path_len", "path_cost", "expansions"):
        assert np.array_equal(short[k], full[k]), k
    assert np.array_equal(short["paths"][0], full["paths"][0, :5])


def test_argument_rejection():
    c = npa.default_context()
    gm, _ = scene("scene0")
    B = 2
    st = np.zeros((B, 2)); tg = np.ones((B, 2))
    kp = np.zeros((B, 4, 2)); cost = np.zeros(B)
    plen, nexp, flags = (np.zeros(B, np.int32) for _ in range(3))
    P = _lib.ptr

    def call(scene_id, B=B, start=st, target=tg, kp=kp, max_exp=0, cap=0, path=None, sid=None):
        return c.lib.neo_geo_search_batch(c.h, scene_id, P(sid), B, P(start), P(target), max_exp, cap, P(kp), P(path),
                                          P(plen), P(cost), P(nexp), P(flags))

    assert call(gm.scene_id) == 0
    assert call(gm.scene_id, B=0) == NEO_ERR_INVALID
    assert call(gm.scene_id, start=None) == NEO_ERR_INVALID
    assert call(gm.scene_id, kp=None) == NEO_ERR_INVALID
    assert call(gm.scene_id, max_exp=-1) == NEO_ERR_INVALID
    assert call(gm.scene_id, path=np.zeros((B, 1, 2)), cap=0) == NEO_ERR_INVALID
    assert call(987654) == NEO_ERR_NO_MAP
    assert call(gm.scene_id, sid=np.array([gm.scene_id, 987654], np.int32)) == NEO_ERR_NO_MAP
    m3 = npa.ESDF3D(np.full((8, 8, 8), 2.0, np.float32), 0.1, (0.0, 0.0, 0.0))
    assert call(m3.scene_id) == NEO_ERR_UNSUPPORTED
    assert call(gm.scene_id, sid=np.array([gm.scene_id, m3.scene_id], np.int32)) == NEO_ERR_UNSUPPORTED
    paths = np.zeros((B, 3, 2)); pl = np.array([3, 4], np.int32)
    assert c.lib.neo_geo_prune_batch(c.h, gm.scene_id, None, B, P(paths), P(pl), 3, P(kp)) == NEO_ERR_INVALID
    assert c.lib.neo_geo_prune_batch(c.h, m3.scene_id, None, B, P(paths), P(pl * 0 + 1), 3, P(kp)) == NEO_ERR_UNSUPPORTED
    # a budget without room for one slot
    assert c.lib.neo_geo_workspace_budget(c.h, ctypes.c_size_t(1000)) == 0
    try:
        assert call(gm.scene_id) == 2
        assert "budget" in c.lib.neo_last_error(c.h).decode()
    finally:
        c.lib.neo_geo_workspace_budget(c.h, ctypes.c_size_t(2 << 30))
    assert call(gm.scene_id) == 0


def test_geo_planner_reference_interface():
    d = fixture("scene0")
    gm, _ = scene("scene0")
    gp = npa.GeoPlanner(npa.PlannerConfig())
    for i in range(len(d["start"])):
        n = int(d["path_len"][i])
        path = gp.astar_planner.plan(gm, d["start"][i], d["target"][i])
        assert np.array_equal(np.array(path), d["paths"][i, :n]), i
        assert gp.astar_planner.target_cost == d["path_cost"][i]
        assert np.array_equal(np.array(gp.prune_path_nodes(gm, path)), d["pruned"][i]), i


def test_geo_traj_plan_reproduces_reference_runs():
    """GeoPlanner.geo_traj_plan in the fp64 mode against the reference's geo_traj_plan: the same exception, final
    int_wpts / ts within 1e-4 (the criteria of test_gpu_parity's g3 / g5 replays)"""
    import types
    d = fixture("plan")
    gm = gpu_map(d["occ"], float(d["res"]), d["origin"])
    for i in range(len(d["seed"])):
        gp = npa.GeoPlanner(npa.PlannerConfig())
        st = types.SimpleNamespace(global_pos=d["start"][i], global_vel=d["vel"][i])
        np.random.seed(int(d["seed"][i]))
        err = ""
        try:
            gp.geo_traj_plan(gm, st, d["tail"][i])
        except Exception as ex:
            err = f"{type(ex).__name__}:{ex}"
        assert err.split(":")[0] == str(d["error"][i]).split(":")[0], i
        rel = lambda a, b: np.abs(np.asarray(a) - b).max() / max(np.abs(b).max(), 1e-300)
        assert rel(gp.int_wpts, d["final_int_wpts"][i]) < 1e-4, i
        assert rel(gp.ts, d["final_ts"][i]) < 1e-4, i


def test_geo_plan_batch():
    bp = npa.BatchPlanner()
    gm, S, T = _local_requests(64, np.random.default_rng(17))
    head = np.zeros((64, 3, 2)); head[:, 0] = S
    tail = np.zeros((64, 3, 2)); tail[:, 0] = T
    out = bp.geo_plan(gm, head, tail, seed=1)
    g = out["geo"]
    assert np.array_equal(g["key_pts"], bp.geo_init(gm, S, T)["key_pts"])
    ref = bp.plan(gm, head, tail, int_wpts=g["int_wpts"], ts=g["ts"], seed=1)
    assert np.array_equal(out["x"], ref["x"]) and np.array_equal(out["attempts"], ref["attempts"])
    assert out["solved"].mean() > 0.5


def test_replan_loop_geo_reaches_goal():
    occ = synth.occupancy_2d(3)
    m = gpu_map(occ)
    np.random.seed(503)
    out = ReplanLoop(npa.GeoPlanner(npa.PlannerConfig()), m, mode="geo").run()
    assert out["success"]
    assert np.linalg.norm(out["path"][-1] - np.array([30.0, 0.0])) < 0.2
    assert out["min_clearance"] > 0.3
