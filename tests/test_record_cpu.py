"""The fleet's record mode off the GPU: the NumPy model of the kernels (tests/record_oracle_np.py) against the
reference's form_nn_input / form_nn_output, the durations of a row, the dataset's file, the C ABI's new names and the
trainer on the CPU."""
import os
import re

import numpy as np
import pytest

import record_oracle_np as ron
from neo_planner_amd import _lib, build
from neo_planner_amd.record import DemoRecorder, tau_to_ts
from oracle import minco_np as onp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_case(rng, M):
    yaw = rng.uniform(-np.pi, np.pi)
    pose = np.array([rng.uniform(0.0, 30.0), rng.uniform(-15.0, 15.0), rng.uniform(0.5, 3.0), np.cos(yaw), np.sin(yaw)])
    cur_vel = rng.uniform(-3.0, 3.0, 2)
    head, tail = rng.uniform(-30.0, 30.0, (3, 2)), rng.uniform(-30.0, 30.0, (3, 2))
    x = np.concatenate([rng.uniform(-30.0, 30.0, 2 * (M - 1)), rng.uniform(-4.0, 4.0, M)])
    return pose, cur_vel, head, tail, x


def test_oracle_rows_are_the_references_rows():
    """200 random poses and states: the (c, s) route of the kernels and the reference's quaternion route differ by
    rounding only"""
    rng = np.random.default_rng(7)
    worst = 0.0
    for k in range(200):
        M = 3 if k % 2 == 0 else 5
        pose, cur_vel, head, tail, x = random_case(rng, M)
        motion = ron.motion_vector(pose, cur_vel, head, tail)
        wpts = ron.waypoints_local(pose, x, M)
        ref_motion, ref_wpts = ron.reference_row(pose, cur_vel, head, tail, x, M)
        assert motion.shape == ref_motion.shape == (24,) and wpts.shape == ref_wpts.shape == (3 * (M - 1),)
        worst = max(worst, np.abs(motion - ref_motion).max(), np.abs(wpts - ref_wpts).max())
    print(f"largest difference between the two attitude routes: {worst:.2e}")
    assert worst <= 1e-12


def test_rank_gives_rows_in_order_and_counts_what_does_not_fit():
    solved = np.array([1, 0, 1, 1, 0, 1, 1], np.int32)
    row_of, n, dropped = ron.rank(7, None, solved, 10, 4, 0)
    assert row_of.tolist() == [4, -1, 5, 6, -1, 7, 8] and (n, dropped) == (9, 0)
    row_of, n, dropped = ron.rank(7, [6, 5, 9, 0, 1], solved, 6, 4, 2)
    assert row_of.tolist() == [4, 5, -1, -1, -1] and (n, dropped) == (6, 3)
    assert ron.rank(7, None, None, 3, 3, 0)[1:] == (3, 7)


def synthetic_rows(n=9, M=3, H=5, W=7, seed=3):
    rng = np.random.default_rng(seed)
    return dict(images=rng.integers(0, 256, (n, H, W), dtype=np.uint8), motion=rng.normal(size=(n, 24)),
                wpts_local=rng.normal(size=(n, 3 * (M - 1))), tau=rng.uniform(-6.0, 6.0, (n, M)), pose=rng.normal(size=(n, 5)),
                meta=rng.integers(0, 99, (n, 3)).astype(np.int32))


def test_ts_is_map_tau2T_bit_for_bit():
    a = synthetic_rows(M=5)
    rec = DemoRecorder.from_arrays(**a, T_min=0.5, T_max=5.0)
    ts = rec.rows()["ts"]
    o = onp.OraclePlanner(onp.PlannerParams())
    assert (o.T_min, o.T_max) == (0.5, 5.0)
    o.M = 5
    for i in range(a["tau"].shape[0]):
        assert np.array_equal(ts[i].view(np.uint64), o.map_tau2T(a["tau"][i]).view(np.uint64))
    assert np.array_equal(tau_to_ts(a["tau"], 0.5, 5.0), ts)
    lab = rec.labels()
    assert lab.shape == (9, 3 * 4 + 5) and np.array_equal(lab[:, :12], a["wpts_local"]) and np.array_equal(lab[:, 12:], ts)


def test_save_and_load_round_trip(tmp_path):
    a = synthetic_rows()
    rec = DemoRecorder.from_arrays(**a, des_pos_z=1.5, T_min=0.4, T_max=6.0, dropped=2)
    path = str(tmp_path / "demo.npz")
    rec.save(path)
    back = DemoRecorder.load(path)
    r0, r1 = rec.rows(), back.rows()
    assert set(r1) == {"images", "motion", "wpts_local", "tau", "pose", "meta", "ts"}
    for k in r1:
        assert r1[k].dtype == r0[k].dtype and np.array_equal(r1[k], r0[k]) and np.array_equal(r1[k][:9], a.get(k, r0[k])), k
    assert (back.M, back.n_rows, back.dropped, back.des_pos_z, back.T_min, back.T_max) == (3, 9, 2, 1.5, 0.4, 6.0)
    assert (back.height, back.width) == (5, 7)
    inputs, labels = back.training_tensors()
    assert inputs.dtype == labels.dtype == np.float32 and inputs.shape == (9, 5 * 7 + 24) and labels.shape == (9, 9)
    assert np.array_equal(inputs[:, :35], a["images"].reshape(9, -1).astype(np.float32))
    assert np.array_equal(inputs[:, 35:], a["motion"].astype(np.float32))


def test_record_entry_points_in_the_abi():
    # (the init unit shares the recorder's helpers)
    assert [s for s in build.SOURCES if "neo_record.hpp" in build.headers_of(s)] == ["neo_disp_record.hip", "neo_disp_init.hip"]
    build.build()
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "neo_planner.h")).read()
    for name, count in {"neo_record_state_dev": 10, "neo_record_commit_dev": 27}.items():
        assert name in _lib.EXPORTS
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header)
        assert decl, name
        assert len(getattr(lib, name).argtypes) == len(decl.group(1).split(",")) == count, name


def test_recorder_and_trainer_are_exported():
    import neo_planner_amd as npa
    assert {"DemoRecorder", "train_initializer"} <= set(npa.__all__)
    assert npa.DemoRecorder is DemoRecorder and callable(npa.train_initializer)
    import inspect
    assert "record" in inspect.signature(npa.FleetReplanLoop.__init__).parameters


def test_train_initializer_on_the_cpu(monkeypatch):
    """64 synthetic rows of 24 x 32 images whose labels are a fixed linear map of the motion vector: the split is
    51 / 13, two calls with one seed give the same losses, and five epochs bring the training loss down"""
    torch = pytest.importorskip("torch")
    from neo_planner_amd import initializer as ini
    from neo_planner_amd.training import train_initializer
    rng = np.random.default_rng(11)
    n, H, W = 64, 24, 32
    images = rng.integers(0, 256, (n, H, W)).astype(np.float32)
    motion = rng.normal(size=(n, 24)).astype(np.float32)
    labels = (motion @ rng.normal(scale=0.3, size=(24, 9)).astype(np.float32)).astype(np.float32)
    inputs = np.concatenate([images.reshape(n, -1), motion], axis=1)
    runs, splits = [], []
    split = torch.utils.data.random_split

    def watched_split(dataset, lengths, **kw):
        splits.append((len(dataset), list(lengths)))
        return split(dataset, lengths, **kw)

    monkeypatch.setattr(torch.utils.data, "random_split", watched_split)
    for _ in range(2):
        torch.manual_seed(5)
        net = ini.PlannerNet(H, W)
        frozen = net.img_backbone.layer1[0].conv1.weight.detach().clone()
        net, losses, held_out = train_initializer(inputs, labels, net=net, epochs=5, batch_size=8, seed=42, device="cpu")
        assert len(losses) == 5 and np.isfinite(losses).all() and np.isfinite(held_out)
        assert torch.equal(net.img_backbone.layer1[0].conv1.weight.detach(), frozen)       # the backbone stayed frozen
        assert all(p.requires_grad for p in net.parameters()) and not net.training
        runs.append((losses, held_out))
    assert runs[0] == runs[1]
    print(f"training loss per epoch {runs[0][0]}, held out {runs[0][1]:.4f}")
    assert runs[0][0][-1] < runs[0][0][0]
    assert splits == [(64, [51, 13])] * 2
    with pytest.raises(ValueError):
        train_initializer(inputs[:, :-1], labels, net=ini.PlannerNet(H, W), device="cpu")
