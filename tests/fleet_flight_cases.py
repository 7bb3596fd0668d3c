"""What tools/gen_golden_fleet.py and test_gpu_fleet_flights.py share: sixteen short fleet flights that between them go
through every mode and option of FleetReplanLoop, flown through its public surface only, and what is kept of each -- a
SHA-256 over everything the flight produced, the run-length-encoded sequence of library entry points called during run(),
and the number of context synchronisations.

Six missions, two on each of the three synth scenes, four replans.  The missions are chosen for the branches they take:

  0, 1, 2   fly ~11 m through the thickest rows of their forests
  3, 5      a goal inside an obstacle, a little further than longitu_step_dis: the first plan is an ordinary one, then the
            local target is the goal itself, all eleven targets of that tick fail (rounds r > 0, jitter, plan retries, the
            batch mode's fallback) and the mission is abandoned -- from then on the active missions are a true subset
  4         a goal 3 m away in the open: it lands after its first plan

With goal routes missions 1, 3 and 5 chase a short open route whose last vertex lies inside an obstacle (the goal stops
there: every target of the later ticks fails, failed_ticks counts them) and missions 0, 2 and 4 a short closed one."""
import hashlib

import numpy as np

B = 6
CAM = dict(width=64, height=48)
MAX_REPLANS = 4
MAX_CMD_SECONDS = 30
SEED = 41
SCENES = (0, 1, 2)
START = [[0.5, -1.0], [0.5, -2.0], [0.5, 0.0], [0.5, 2.0], [0.5, 5.5], [0.5, -3.0]]
GOALS = [[11.5, -3.0], [12.0, -2.5], [12.0, 0.5], [6.5, 2.0], [3.5, 6.0], [6.5, -2.5]]
# (vertices, speed, closed) per mission
ROUTES = [([[8.0, -0.5], [10.0, 0.5], [9.0, -1.5]], 0.8, True),
          ([[3.0, -1.0], [3.5, 0.5]], 1.5, False),
          ([[7.0, 0.5], [8.5, 1.5], [8.5, -0.5]], 0.8, True),
          ([[4.0, 2.0], [6.5, 2.0]], 1.5, False),
          ([[4.0, 6.0], [6.0, 7.0], [6.0, 5.5]], 0.8, True),
          ([[5.0, -4.5], [6.5, -2.5]], 1.5, False)]
OCCUPIED = dict(goals=(3, 5), routes=(1, 3, 5))      # whose goal / whose route's end lies inside an obstacle

# name -> (FleetReplanLoop keywords, onboard, record, goal routes); the order is the issue's table
CONFIGS = {
    "basic_host": (dict(mode="basic"), False, False, False),
    "basic_resident": (dict(mode="basic", resident=True), False, False, False),
    "basic_host_counter": (dict(mode="basic", jitter="counter"), False, False, False),
    "basic_resident_counter_record": (dict(mode="basic", resident=True, jitter="counter"), False, True, False),
    "geo": (dict(mode="geo"), False, False, False),
    "batch_host": (dict(mode="batch"), False, False, False),
    "batch_resident_counter": (dict(mode="batch", resident=True, jitter="counter"), False, False, False),
    "warmstart": (dict(mode="warmstart"), False, False, False),
    "warmstart_onboard_record": (dict(mode="warmstart"), True, True, False),
    "neo": (dict(mode="neo"), False, False, False),
    "neo_record": (dict(mode="neo"), False, True, False),
    "nn_onboard": (dict(mode="nn"), True, False, False),
    "basic_resident_onboard_poses": (dict(mode="basic", resident=True, record_poses=True), True, False, False),
    "batch_routes_counter_record": (dict(mode="batch", jitter="counter"), False, True, True),
    "warmstart_routes": (dict(mode="warmstart"), False, False, True),
    "basic_host_routes": (dict(mode="basic"), False, False, True),
}
NETWORK = ("neo", "neo_record", "nn_onboard")      # the configurations that run torch's network
BATCH = ("batch_host", "batch_resident_counter", "batch_routes_counter_record")
ROUTED = tuple(k for k, v in CONFIGS.items() if v[3])

# left out of the recorded sequence: bookkeeping that launches nothing
SKIPPED_PREFIXES = ("neo_ctx_", "neo_params_")
SKIPPED_NAMES = ("neo_last_error", "neo_scene_slot")


def setup():
    """the three scenes and their 2-D maps, the camera, the missions (as test_gpu_record.py's _fleet_setup, for six)"""
    import depth_oracle_np as don
    import neo_planner_amd as npa
    from neo_planner_amd import synth
    from neo_planner_amd.depth import DepthCamera
    scenes = [don.boxes_of(synth.forest_boxes(s)) for s in SCENES]
    maps = []
    for s in SCENES:
        m = npa.ESDF()
        m.occupancy_map_cb(synth.OccupancyGridMsg(synth.occupancy_2d(s)))
        maps.append(m)
    scene_index = (np.arange(B) % 3).astype(np.int32)
    return dict(scenes=scenes, packed=DepthCamera.pack_scenes(scenes), maps=maps, B=B, scene_index=scene_index,
                start=np.array(START), goals=np.array(GOALS), cam=DepthCamera(**CAM),
                sids=np.array([maps[s].scene_id for s in scene_index], dtype=np.int32))


def drop(fs):
    from neo_planner_amd import _lib
    c = _lib.default_context()
    for m in fs["maps"]:
        c.check(c.lib.neo_esdf_drop(c.h, m.scene_id))


def routes():
    from neo_planner_amd.goal_routes import GoalRoutes
    return GoalRoutes.from_lists([r for r, _, _ in ROUTES], [s for _, s, _ in ROUTES], [c for _, _, c in ROUTES])


def strip_features(img):
    """stands in for the backbone (test_gpu_init.py): 24 strip sums of the image in exact integer arithmetic"""
    import torch
    n = img.shape[0]
    sums = img.reshape(n, 24, -1).to(torch.int64).sum(dim=2)
    return (sums.to(torch.float64) / (255.0 * (img[0].numel() // 24))).to(torch.float32)


def make_neo(fs, bp):
    """test_gpu_init.py's make_neo(stub=True)"""
    import torch
    from neo_planner_amd import initializer as ini
    torch.manual_seed(11)
    net = ini.PlannerNet(48, 64)
    net.image_features = strip_features
    return ini.BatchNeoPlanner(bp, ini.BatchInitializer(net, device=torch.device("cuda", 0)), fs["cam"])


def weights_digest(neo):
    from neo_planner_amd import initializer as ini
    return hashlib.sha256(ini.pack_head_weights(neo.init.net).cpu().numpy().tobytes()).hexdigest()


class RecordingLib:
    """stands in for ctx.lib during a flight: hands every entry point through and keeps the names called"""

    def __init__(self, lib):
        self._lib, self.names, self.syncs = lib, [], 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("neo_") or not callable(fn):
            return fn

        def call(*args):
            if name == "neo_ctx_synchronize":
                self.syncs += 1
            if not name.startswith(SKIPPED_PREFIXES) and name not in SKIPPED_NAMES:
                self.names.append(name)
            return fn(*args)
        return call


def run_length(names, widest=48):
    """the names in order as one string, run-length encoded: a name or a phrase of up to `widest` names that comes k times
    in a row is written once, as name*k or (a b c)*k (the phrase encoded the same way); `neo_` is left off"""
    names = [n[4:] if n.startswith("neo_") else n for n in names]
    out, i = [], 0
    while i < len(names):
        covered, width, times = 0, 1, 1
        for w in range(1, min(widest, (len(names) - i) // 2) + 1):
            k = 1
            while names[i + k * w:i + (k + 1) * w] == names[i:i + w]:
                k += 1
            if k > 1 and k * w > covered:
                covered, width, times = k * w, w, k
        if covered == 0:
            out.append(names[i])
            i += 1
        else:
            unit = names[i:i + width]
            out.append((unit[0] if width == 1 else "(" + run_length(unit, widest) + ")") + "*%d" % times)
            i += covered
    return " ".join(out)


def _feed(h, a):
    a = np.ascontiguousarray(a)
    h.update(str(a.dtype).encode() + b"|" + repr(tuple(a.shape)).encode() + b"|")
    h.update(a.tobytes())


def digest(loop, out, rec):
    """SHA-256 over every array of the result dict in sorted key order (dtype, shape, bytes), every mission's commands,
    loop.x, and the recorder's rows"""
    h = hashlib.sha256()
    for k in sorted(out):
        h.update(k.encode() + b"=")
        _feed(h, out[k])
    for i in range(B):
        _feed(h, loop.commands(i))
    _feed(h, loop.x)
    if rec is not None:
        rows = rec.rows()
        for k in sorted(rows):
            h.update(k.encode() + b"=")
            _feed(h, rows[k])
    return h.hexdigest()


def fly(fs, name, neo=None):
    """one configuration's flight with the recording proxy in place of ctx.lib.  Returns what the fixture keeps of it."""
    import neo_planner_amd as npa
    from neo_planner_amd import _lib
    from neo_planner_amd.onboard import OnboardMapper
    from neo_planner_amd.record import DemoRecorder
    kw, onboard, record, routed = CONFIGS[name]
    kw = dict(kw)
    bp = neo.bp if neo is not None else npa.BatchPlanner()
    ctx = bp.ctx
    cams = name in NETWORK or onboard or record
    if cams:
        kw.update(scenes=fs["packed"], scene_index=fs["scene_index"])
    mapper = OnboardMapper(ctx, fs["cam"], B) if onboard else None
    rec = DemoRecorder(fs["cam"], capacity=12 * B * (MAX_REPLANS + 1)) if record else None
    if name in NETWORK:
        kw.update(neo=neo)
    loop = npa.FleetReplanLoop(bp, fs["maps"][0], None if routed else fs["goals"], scene_ids=fs["sids"],
                               mission_ids=np.arange(B), seed=SEED, max_cmd_seconds=MAX_CMD_SECONDS, onboard=mapper,
                               record=rec, goal_routes=routes() if routed else None, **kw)
    lib, proxy = ctx.lib, RecordingLib(ctx.lib)
    ctx.lib = proxy
    try:
        out = loop.run(fs["start"], max_replans=MAX_REPLANS)
    finally:
        ctx.lib = lib
    got = dict(digest=digest(loop, out, rec), calls=run_length(proxy.names), synchronizes=proxy.syncs,
               replans=int(out["replans"].sum()), failed_attempts=int(out["failed_attempts"].sum()),
               replans_max=int(out["replans"].max()), ticks=len(loop.timings))
    if name in BATCH:      # a mission went to the fallback if it ran more than its rounds' three candidates
        rounds = out["replans"].astype(np.int64) + out["failed_attempts"]
        got["fallback_missions"] = int((out["opt_runs"] + loop.uncounted_candidates > 3 * rounds).sum())
    if routed:
        got["failed_ticks"] = int(out["failed_ticks"].sum())
    if mapper is not None:
        mapper.close()
    return got
