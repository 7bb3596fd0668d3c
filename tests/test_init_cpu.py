"""The learned warm start on resident arrays, off the GPU: the NumPy models of the neo_init_* kernels
(tests/init_oracle_np.py) against the network, the recorder's motion vector and the host route
(BatchInitializer.warm_start + pack_x), the weight blob, the C ABI's new names and FleetReplanLoop's argument errors."""
import copy
import inspect
import os
import re

import numpy as np
import pytest

import init_oracle_np as ion
import record_oracle_np as ron
import neo_planner_amd as npa
from neo_planner_amd import _lib, build

torch = pytest.importorskip("torch")
from neo_planner_amd import initializer as ini  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def seeded_net(cls=ini.PlannerNet, seed=5):
    torch.manual_seed(seed)
    return cls(24, 32).eval()


def random_states(rng, n, reach=30.0):
    """n poses, velocities, look-ahead states and targets: positions up to `reach` metres"""
    yaw = rng.uniform(-np.pi, np.pi, n)
    pose = np.stack([rng.uniform(0.0, reach, n), rng.uniform(-reach / 2, reach / 2, n), rng.uniform(0.5, 3.0, n),
                     np.cos(yaw), np.sin(yaw)], 1)
    return pose, rng.uniform(-3.0, 3.0, (n, 2)), rng.uniform(-reach, reach, (n, 3, 2)), rng.uniform(-reach, reach, (n, 3, 2))


def test_head_model_is_the_network_within_fp32_rounding():
    """256 rows of N(0, 1) features and N(0, 3) motion, and 256 rows whose motion comes from positions up to 30 m: the
    sequential fp32 model is as close to the fp64 network as torch's own fp32 head, within a factor 4 (the yardstick is
    torch's error on the same rows; the factor allows for another summation order)"""
    net = seeded_net()
    blob = ini.pack_head_weights(net).numpy()
    net64 = copy.deepcopy(net).double()
    rng = np.random.default_rng(17)
    far = ion.motion(*random_states(rng, 256))
    for name, feat, mot in [("random rows", rng.normal(0.0, 1.0, (256, 24)), rng.normal(0.0, 3.0, (256, 24))),
                            ("positions up to 30 m", rng.normal(0.0, 1.0, (256, 24)), far)]:
        feat, mot = feat.astype(np.float32), mot.astype(np.float32)
        with torch.no_grad():
            ref = net64.head(torch.from_numpy(feat).double(), torch.from_numpy(mot).double()).numpy()
            t32 = net.head(torch.from_numpy(feat), torch.from_numpy(mot)).numpy()
        model = ion.head_rows(blob, feat, mot)
        assert model.dtype == np.float32 and model.shape == (256, 9)
        e_model, e_torch = np.abs(model - ref).max(), np.abs(t32.astype(np.float64) - ref).max()
        print(f"{name}: model {e_model:.2e}, torch fp32 {e_torch:.2e}, ratio {e_model / e_torch:.2f}, "
              f"output scale {np.abs(ref).max():.2f}")
        assert e_torch > 0 and e_model <= 4 * e_torch
    # one shared feature row is the same row for every request
    shared = ion.head_rows(blob, feat[:1], mot)
    assert np.array_equal(shared.view(np.uint32), ion.head_rows(blob, np.repeat(feat[:1], 256, 0), mot).view(np.uint32))


def test_motion_model_is_the_recorders_motion():
    pose, vel, head, tail = random_states(np.random.default_rng(3), 40)
    m64 = ion.motion64(pose, vel, head, tail)
    for b in range(40):
        assert np.array_equal(m64[b].view(np.uint64), ron.motion_vector(pose[b], vel[b], head[b], tail[b]).view(np.uint64))
    m32 = ion.motion(pose, vel, head, tail)
    assert m32.dtype == np.float32 and np.array_equal(m32.view(np.uint32), m64.astype(np.float32).view(np.uint32))
    kept = ion.motion(pose, vel, head, tail, subset=[5, -1, 40, 2], out=np.full((40, 24), -7.25, np.float32))
    assert np.array_equal(kept[[2, 5]], m32[[2, 5]]) and (np.delete(kept, [2, 5], 0) == -7.25).all()


class FixedHead(torch.nn.Module):
    """a network whose head answers with given rows: the host route's arithmetic after the network, alone"""

    def __init__(self, out9):
        super().__init__()
        self.rows = torch.from_numpy(np.asarray(out9, dtype=np.float32))

    def head(self, img_feature, motion):
        return self.rows


def test_guess_model_is_the_host_route():
    """BatchInitializer.warm_start's waypoints (an einsum with the 3 x 3 attitude) within 1e-12 of the model's -- the
    bound of two rounding routes in test_record_cpu.py -- and pack_x's tau bit for bit where the clamped durations are
    equal; durations below T_min, above T_max and NaN included"""
    rng = np.random.default_rng(23)
    n = 64
    pose = random_states(rng, n)[0]
    out9 = np.concatenate([rng.uniform(-12.0, 12.0, (n, 6)), rng.uniform(0.0, 6.0, (n, 3))], 1).astype(np.float32)
    out9[0, 6:] = (0.1, 7.0, 2.75)
    bp = npa.BatchPlanner()
    T_min, T_max = float(bp.cfg.T_min), float(bp.cfg.T_max)
    init = ini.BatchInitializer(FixedHead(out9), device="cpu", T_min=T_min, T_max=T_max)
    R = np.zeros((n, 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1], R[:, 2, 2] = pose[:, 3], -pose[:, 4], pose[:, 4], pose[:, 3], 1.0
    wp, ts = init.warm_start(torch.zeros(1, 24), np.zeros((n, 24), np.float32), R, pose[:, :3])
    host = bp.pack_x(wp.numpy(), ts.numpy())
    model = ion.guess(out9, pose, T_min, T_max)
    assert host.shape == model.shape == (n, 7)
    worst = np.abs(host[:, :4] - model[:, :4]).max()
    print(f"waypoints, host route against the model: {worst:.2e}")
    assert worst <= 1e-12
    assert np.array_equal(ion.clamp(out9[:, 6:].astype(np.float64), T_min, T_max), ts.numpy())
    assert np.array_equal(host[:, 4:].view(np.uint64), model[:, 4:].view(np.uint64))
    assert model[0, 6] == 0.0 and model[0, 4] < -6.0 and model[0, 5] > 6.0 and np.isfinite(model).all()
    nan = ion.guess(np.full((1, 9), np.nan, np.float32), pose[:1], T_min, T_max)
    assert np.isnan(nan).all()
    kept = ion.guess(out9, pose, T_min, T_max, subset=[3, n, 1], x0=np.full((n, 7), -7.25))
    assert np.array_equal(kept[[1, 3]], model[[1, 3]]) and (np.delete(kept, [1, 3], 0) == -7.25).all()


def test_pack_head_weights():
    net = seeded_net()
    blob = ini.pack_head_weights(net)
    assert blob.dtype == torch.float32 and blob.shape == (20817,) == (_lib.NEO_INIT_HEAD_FLOATS,) and ion.HEAD_FLOATS == 20817
    assert blob.device == next(net.parameters()).device and not blob.requires_grad
    # the order: unpacked into a fresh network, the head's parameters are the packed network's
    fresh = seeded_net(seed=99)
    layers = ini.head_layers(fresh)
    assert [(l.in_features, l.out_features) for l in layers] == [(i, o) for i, o, _ in ion.LAYERS]
    with torch.no_grad():
        for layer, (W, b, _) in zip(layers, ion.unpack(blob.numpy())):
            layer.weight.copy_(torch.from_numpy(W.copy()))
            layer.bias.copy_(torch.from_numpy(b.copy()))
    a, b = net.state_dict(), fresh.state_dict()
    keys = [k for k in a if k.startswith(("motion_backbone.", "mlp."))]
    assert len(keys) == 16 and all(torch.equal(a[k], b[k]) for k in keys)
    assert not torch.equal(a["img_backbone.fc.weight"], b["img_backbone.fc.weight"])
    with pytest.raises(ValueError):
        ini.pack_head_weights(seeded_net(ini.PlannerNetConv))
    with pytest.raises(ValueError):
        ini.pack_head_weights(net.mlp)


def test_init_entry_points_in_the_abi():
    assert "neo_disp_init.hip" in build.SOURCES
    # the family's header recompiles this unit alone, the recorder's helpers this unit and the recorder
    assert [s for s in build.SOURCES if "neo_init.hpp" in build.headers_of(s)] == ["neo_disp_init.hip"]
    assert [s for s in build.SOURCES if "neo_record.hpp" in build.headers_of(s)] == ["neo_disp_record.hip", "neo_disp_init.hip"]
    build.build()
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "neo_planner.h")).read()
    for name, count in {"neo_init_motion_dev": 9, "neo_init_head_dev": 10, "neo_init_guess_dev": 7}.items():
        assert name in _lib.EXPORTS
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header)
        assert decl, name
        assert len(getattr(lib, name).argtypes) == len(decl.group(1).split(",")) == count, name
    assert re.search(r"#define\s+NEO_INIT_HEAD_FLOATS\s+20817\b", header) and re.search(r"#define\s+NEO_ABI_VERSION\s+1\b", header)
    tool = open(os.path.join(REPO, "tools", "kernel_resource_usage.py")).read()
    assert "neo_disp_init.hip" in tool


def test_fleet_modes_and_their_argument_errors():
    params = inspect.signature(npa.FleetReplanLoop.__init__).parameters
    assert "neo" in params and isinstance(npa.FleetReplanLoop.x, property)
    bp = npa.BatchPlanner()
    cam = npa.DepthCamera(width=32, height=24)
    neo = ini.BatchNeoPlanner(bp, ini.BatchInitializer(seeded_net(), device="cpu"), cam)
    assert neo.kernel_head and callable(neo.warm_start_dev) and callable(neo.plan_dev)
    goals = np.array([[10.0, 0.0], [12.0, 1.0]])
    scenes = npa.DepthCamera.pack_scenes([np.zeros((0, 6))])
    for mode in ("neo", "nn"):
        loop = npa.FleetReplanLoop(bp, None, goals, mode=mode, neo=neo, scenes=scenes)
        assert loop.resident and loop.neo is neo and loop.mode == mode
        with pytest.raises(ValueError, match="neo=BatchNeoPlanner"):
            npa.FleetReplanLoop(bp, None, goals, mode=mode, scenes=scenes)
        with pytest.raises(ValueError, match="scenes"):
            npa.FleetReplanLoop(bp, None, goals, mode=mode, neo=neo)
        with pytest.raises(ValueError, match="batch_planner"):
            npa.FleetReplanLoop(npa.BatchPlanner(), None, goals, mode=mode, neo=neo, scenes=scenes)
        bp5 = npa.BatchPlanner(npa.PlannerConfig(init_wpts_num=4))
        neo5 = ini.BatchNeoPlanner(bp5, neo.init, cam)
        with pytest.raises(ValueError, match="init_wpts_num"):
            npa.FleetReplanLoop(bp5, None, goals, mode=mode, neo=neo5, scenes=scenes)
        other = ini.BatchNeoPlanner(bp, neo.init, cam)
        other.camera = npa.DepthCamera(width=64, height=48)
        with pytest.raises(ValueError, match="camera"):
            npa.FleetReplanLoop(bp, None, goals, mode=mode, neo=other, scenes=scenes)
        with pytest.raises(ValueError, match="scene_index"):
            npa.FleetReplanLoop(bp, None, goals, mode=mode, neo=neo, scenes=scenes, scene_index=[0])
    with pytest.raises(ValueError):
        npa.FleetReplanLoop(bp, None, goals, mode="neon")
    with pytest.raises(ValueError):
        ini.BatchNeoPlanner(bp, neo.init, npa.DepthCamera(width=64, height=48))
    # the modes that exist take no notice of a neo planner
    assert npa.FleetReplanLoop(bp, None, goals, mode="basic", neo=neo).neo is None
    with pytest.raises(_lib.NeoError):
        npa.FleetReplanLoop(bp, None, goals).x
