"""The image backbone of the learned warm start on the GPU: neo_backbone_features_dev against the fp64 restatement of its
weight blob (initializer.backbone_model), its independence of the batch bit for bit, what it leaves of the memory around
its buffers, and BatchNeoPlanner / FleetReplanLoop on the kernel backbone."""
import ctypes

import numpy as np
import pytest

import neo_planner_amd as npa
from neo_planner_amd import _lib
from test_backbone_cpu import randomised_net
from test_gpu_record import _fleet_setup

pytestmark = pytest.mark.gpu

# (the last four: one-pixel and even images, the pooled image that exactly fills the stem's 8 x 4 tile and the one that passes it
# by a pixel; tests/test_gpu_backbone_launches.py takes them launch by launch)
SIZES = [(9, 13), (33, 47), (120, 160), (1, 1), (2, 2), (16, 32), (17, 33)]
N_MOST = 70
GUARD = 64


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _ini():
    from neo_planner_amd import initializer as ini
    return ini


def _p(t, first=0):
    return ctypes.c_void_p(t.data_ptr() + first) if t is not None else None


def batch_images(H, W, n=N_MOST, seed=0):
    """n images of random uint8 values; image 1 is all 0 and image 2 all 255 (both are among the first three)"""
    img = np.random.default_rng([seed, H, W]).integers(0, 256, (n, H, W), dtype=np.uint8)
    if n > 2:
        img[1], img[2] = 0, 255
    return img


_REF = {}


def reference(H, W):
    """computed once a size and shared, for the 70 images of batch_images: the network, its float32 blob on the CPU, the
    fp64 values of the blob (backbone_model: the yardstick) and the float32 torch module's on the CPU (plain nn.Conv2d,
    BatchNorm unfolded: the reference arithmetic, whose error against the yardstick is e_ref)"""
    if (H, W) not in _REF:
        torch, _ = _torch()
        ini = _ini()
        net = randomised_net(H=H, W=W)
        img = batch_images(H, W)
        blob = ini.pack_backbone_weights(net)
        want = ini.backbone_model(blob, img)
        with torch.no_grad():
            f32 = net.float().eval().image_features(torch.from_numpy(img).float().reshape(-1, 1, H, W)).numpy().astype(np.float64)
        assert np.isfinite(want).all()
        _REF[(H, W)] = dict(net=net, img=img, blob=blob, want=want, f32=f32)
    return _REF[(H, W)]


def run_kernel(blob_dev, img_dev, chunk=None):
    """neo_backbone_features_dev on the default context; features as a NumPy array"""
    torch, _ = _torch()
    c = _lib.default_context()
    torch.cuda.synchronize()
    feat, _ws = _ini().backbone_features_kernel(c, blob_dev, img_dev, chunk=chunk or max(1, int(img_dev.shape[0])))
    c.synchronize()
    return feat.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("n", [1, 3, N_MOST])
@pytest.mark.parametrize("H,W", SIZES)
def test_features_equal_the_fp64_model(H, W, n):
    """The first n of the size's 70 images (n = 70: several column tiles in layer 4 and a ragged one in every layer).
    e_ref = the largest error of torch's float32 module on the CPU against the fp64 model over these n images; the kernel
    may err by 4 e_ref: both are fp32 sums of the same products in another order (plus one rounding of a folded weight),
    and 4 leaves room for the ordering.  Ratios seen on the MI355X: 1.0 - 3.6, the largest for the three
    images of 33 x 47, where the all-255 image carries the kernel's error."""
    torch, dev = _torch()
    r = reference(H, W)
    got = run_kernel(r["blob"].to(dev), torch.from_numpy(r["img"][:n]).to(dev))
    want = r["want"][:n]
    e_ref = np.abs(r["f32"][:n] - want).max()
    err = np.abs(got.astype(np.float64) - want).max()
    print(f"{H} x {W}, n = {n}: kernel {err:.3e}, e_ref {e_ref:.3e}, ratio {err / e_ref:.2f}, scale {np.abs(want).max():.3e}")
    assert got.shape == (n, 24) and got.dtype == np.float32 and np.isfinite(got).all()
    assert e_ref > 0.0 and err <= 4.0 * e_ref


@pytest.mark.parametrize("H,W", SIZES[:2])
def test_an_images_features_do_not_depend_on_the_batch(H, W):
    """image i alone, at positions 0, 37 and 69 of a batch of 70, and the batch in chunks of 32 against 128: the same bits"""
    torch, dev = _torch()
    r = reference(H, W)
    blob = r["blob"].to(dev)
    img = r["img"]
    whole = run_kernel(blob, torch.from_numpy(img).to(dev), chunk=128)
    split = run_kernel(blob, torch.from_numpy(img).to(dev), chunk=32)
    assert np.array_equal(bits(whole), bits(split))
    for i in (0, 5, 37, 69):
        alone = run_kernel(blob, torch.from_numpy(img[i:i + 1]).to(dev))
        assert np.array_equal(bits(alone[0]), bits(whole[i])), i
        for pos in (0, 37, 69):
            moved = img[::-1].copy()            # other neighbours, too
            moved[pos] = img[i]
            assert np.array_equal(bits(run_kernel(blob, torch.from_numpy(moved).to(dev))[pos]), bits(whole[i])), (i, pos)
    assert len({row.tobytes() for row in whole}) == N_MOST      # (the features do tell the images apart)


def test_a_one_pixel_images_features_do_not_depend_on_the_batch():
    """1 x 1 images, 129 of them: every convolution has one column an image, so a column tile spans 128 images and the
    129th is the one live column of a second tile.  Image i alone and at positions 0, 127 and 128: the same bits"""
    torch, dev = _torch()
    n = 129
    r = reference(1, 1)
    blob = r["blob"].to(dev)
    img = batch_images(1, 1, n=n, seed=1)
    whole = run_kernel(blob, torch.from_numpy(img).to(dev))
    for i in (0, 5, 127, 128):
        alone = run_kernel(blob, torch.from_numpy(img[i:i + 1]).to(dev))
        assert np.array_equal(bits(alone[0]), bits(whole[i])), i
        for pos in (0, 127, 128):
            moved = img[::-1].copy()
            moved[pos] = img[i]
            assert np.array_equal(bits(run_kernel(blob, torch.from_numpy(moved).to(dev))[pos]), bits(whole[i])), (i, pos)
    assert len({row.tobytes() for row in whole}) == len(np.unique(img)) > 90      # (the features tell the pixel values apart)


@pytest.mark.parametrize("H,W,n", [(33, 47, 3), (9, 13, 70)])
def test_the_call_writes_its_buffers_only(H, W, n):
    """64 guard bytes behind a workspace of exactly neo_backbone_workspace_bytes and behind feature_out stay; a second
    call with other images into the used workspace gives what a fresh one gives"""
    torch, dev = _torch()
    c = _lib.default_context()
    r = reference(H, W)
    blob = r["blob"].to(dev)
    need = int(c.lib.neo_backbone_workspace_bytes(n, H, W))
    assert need > 0 and need % 16 == 0
    ws = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    out = torch.full((n * 24 * 4 + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    first, other = torch.from_numpy(r["img"][:n]).to(dev), torch.from_numpy(r["img"][::-1][:n].copy()).to(dev)
    torch.cuda.synchronize()
    results = []
    for img in (first, other):
        c.call("neo_backbone_features_dev", _p(blob), blob.numel(), _p(img), n, H, W, _p(ws), need, _p(out))
        c.synchronize()
        assert (ws[need:].cpu().numpy() == 0xA5).all() and (out[n * 24 * 4:].cpu().numpy() == 0x5A).all()
        results.append(out[:n * 24 * 4].cpu().numpy().view(np.float32).reshape(n, 24).copy())
    assert np.array_equal(bits(results[0]), bits(run_kernel(blob, first)))
    assert np.array_equal(bits(results[1]), bits(run_kernel(blob, other)))
    assert not np.array_equal(results[0], results[1])


# ------------------------------------------------------------------ BatchNeoPlanner and the fleet
CAM = dict(width=40, height=32)


@pytest.fixture(scope="module")
def fleet():
    torch, dev = _torch()
    ini = _ini()
    fs = _fleet_setup()
    fs["cam"] = npa.DepthCamera(**CAM)
    net = randomised_net(H=CAM["height"], W=CAM["width"], seed=11)
    neos = {impl: ini.BatchNeoPlanner(npa.BatchPlanner(), ini.BatchInitializer(net, device=dev), fs["cam"], backbone_impl=impl)
            for impl in ("torch", "kernel")}
    yield fs, neos
    c = _lib.default_context()
    for m in fs["maps"]:
        c.check(c.lib.neo_esdf_drop(c.h, m.scene_id))


def test_features_dev_on_the_kernel_backbone_and_a_plan_from_it(fleet):
    """six requests' rendered 40 x 32 images: the kernel route is within 4 e_ref of the fp64 model of its blob (e_ref: the
    float32 module on the CPU, as above), hence within that plus the torch route's own error of the torch route; then
    plan_dev from the kernel's features"""
    torch, dev = _torch()
    ini = _ini()
    fs, neos = fleet
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n = 6
    d = fs["goals"][:n] - fs["start"][:n]
    pose = up(npa.DepthCamera.poses(np.concatenate([fs["start"][:n], np.full((n, 1), 2.0)], 1), np.arctan2(d[:, 1], d[:, 0])))
    boxes, begin = (up(a) for a in fs["packed"])
    sidx = up(fs["scene_index"][:n])
    img = fs["cam"].render_dev(boxes, begin, pose, sidx, want_m=False)["depth_u8"].cpu()
    k = neos["kernel"].features_dev(boxes, begin, pose, sidx)
    t = neos["torch"].features_dev(boxes, begin, pose, sidx)
    assert tuple(k.shape) == (n, 24) and k.dtype == torch.float32 and k.is_contiguous()
    # the same images in hand: BatchInitializer.image_features on the kernels gives the same bits
    assert torch.equal(neos["kernel"].init.image_features(img.to(dev), impl="kernel"), k)
    net = neos["kernel"].init.net
    want = ini.backbone_model(ini.pack_backbone_weights(net), img)
    import copy
    with torch.no_grad():
        f32 = copy.deepcopy(net).cpu().float().eval().image_features(img.float().reshape(n, 1, CAM["height"], CAM["width"])).numpy()
    e_ref = np.abs(f32 - want).max()
    e_k, e_t = np.abs(k.cpu().numpy() - want).max(), np.abs(t.cpu().numpy() - want).max()
    gap = np.abs(k.cpu().numpy().astype(np.float64) - t.cpu().numpy()).max()
    print(f"six requests: kernel {e_k:.3e}, torch route {e_t:.3e}, e_ref {e_ref:.3e}, kernel against torch {gap:.3e}")
    assert len({row.tobytes() for row in k.cpu().numpy()}) >= 3
    assert e_k <= 4.0 * e_ref and gap <= 4.0 * e_ref + e_t
    head, tail = np.zeros((n, 3, 2)), np.zeros((n, 3, 2))
    head[:, 0], tail[:, 0] = fs["start"][:n], fs["goals"][:n]
    c = _lib.default_context()
    slots = up(np.array([c.lib.neo_scene_slot(c.h, int(s)) for s in fs["sids"][:n]], dtype=np.int32))
    bufs = neos["kernel"].plan_dev(fs["maps"][0], pose, up(np.zeros((n, 2))), up(head), up(tail), k, slots=slots, seed=7)
    c.synchronize()
    assert np.isfinite(neos["kernel"].x0.cpu().numpy()).all() and np.isfinite(bufs["x"].cpu().numpy()).all()
    assert bufs["launch_sizes"][0] == n


def test_a_neo_fleet_flies_on_the_kernel_backbone(fleet):
    """eight missions, mode "neo", a 40 x 32 camera: the loop needs nothing but features_dev; it runs to its end, times the
    sensing as neo_s and returns finite results.  (Not compared with the torch route's flights: the features differ by
    rounding, and so may the flights.)"""
    fs, neos = fleet
    idx = np.arange(8)
    neo = neos["kernel"]
    loop = npa.FleetReplanLoop(neo.bp, fs["maps"][0], fs["goals"][idx], scene_ids=fs["sids"][idx], mission_ids=idx, mode="neo",
                               neo=neo, scenes=fs["packed"], scene_index=fs["scene_index"][idx])
    out = loop.run(fs["start"][idx], max_replans=25)
    assert loop.timings and all("neo_s" in t for t in loop.timings)
    for i in range(len(idx)):
        assert np.isfinite(loop.commands(i)).all(), i
    assert (out["opt_runs"] >= out["replans"]).all() and (out["replans"] >= 1).any()
    assert np.isfinite(np.asarray(out["iter_num"], dtype=np.float64)).all()
    assert neo._workspace is not None and neo.backbone_impl == "kernel"
