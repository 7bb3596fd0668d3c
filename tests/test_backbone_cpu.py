"""The image backbone of the learned warm start, off the GPU: the folded weight blob (pack_backbone_weights), its fp64
restatement (backbone_model) against the torch module in fp64, the launch table behind it (backbone_launches) against the
blob's size and the C shape query, and the entry points in the C ABI."""
import os
import re

import numpy as np
import pytest
import torch

from neo_planner_amd import _lib, build
from neo_planner_amd import initializer as ini

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(9, 13), (33, 47), (120, 160)]


def randomised_net(cls=ini.PlannerNet, H=9, W=13, seed=3):
    """a seeded network whose every BatchNorm has running_mean, running_var, weight and bias drawn at random: with the
    fresh module's gamma = 1, mean = 0, var = 1, beta = 0 a wrong fold would pass.  gamma and var around 1 and small means
    keep the 17 convolutions deep activations of uint8 images finite and away from an all-zero ReLU."""
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    net = cls(H, W).eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.num_features
                m.running_mean.copy_(torch.randn(n, generator=g) * 0.3)
                m.running_var.copy_(torch.rand(n, generator=g) + 0.5)
                m.weight.copy_(torch.rand(n, generator=g) + 0.5)
                m.bias.copy_(torch.randn(n, generator=g) * 0.2)
    return net


def images(n, H, W, seed=0):
    rng = np.random.default_rng([seed, n, H, W])
    return torch.from_numpy(rng.integers(0, 256, (n, H, W), dtype=np.uint8))


def module_features64(net, img):
    """the torch module in fp64, eval mode, on the CPU"""
    import copy
    net64 = copy.deepcopy(net).double().eval()
    with torch.no_grad():
        return net64.image_features(img.double().reshape(-1, 1, *img.shape[-2:])).numpy()


@pytest.mark.parametrize("H,W", SIZES)
def test_model_of_the_folded_blob_is_the_module(H, W):
    """backbone_model of the fold equals net.double().eval().image_features to 1e-10 relative, at odd image sizes (the
    stride-2 layers and the padding see ragged edges); one image at 120 x 160, two at the smaller sizes.

    The bound holds for the fold as computed, in fp64 (dtype=torch.float64).  The float32 blob the kernels take is that
    fold rounded once -- asserted bit for bit -- and cannot itself meet 1e-10: a relative error of 2^-24 a weight moves
    the features by about 3e-8 relative (printed; 2.9e-8 at 33 x 47)."""
    n = 1 if H >= 100 else 2
    net = randomised_net(H=H, W=W)
    img = images(n, H, W)
    want = module_features64(net, img)
    assert np.isfinite(want).all() and np.abs(want).max() > 1e-3
    if n > 1:
        assert np.abs(want[0] - want[1]).max() > 1e-3 * np.abs(want).max()      # the features differ between images
    fold64 = ini.pack_backbone_weights(net, dtype=torch.float64)
    got = ini.backbone_model(fold64, img)
    scale = np.abs(want).max()
    err = np.abs(got - want).max() / scale
    blob = ini.pack_backbone_weights(net)
    assert blob.dtype == torch.float32 and torch.equal(blob, fold64.to(torch.float32))
    err32 = np.abs(ini.backbone_model(blob, img) - want).max() / scale
    print(f"{H} x {W}: fold in fp64 {err:.2e} relative, the float32 blob {err32:.2e}")
    assert got.shape == (n, 24) and got.dtype == np.float64
    assert err <= 1e-10
    assert err32 <= 1e-5       # (sanity only: the cast is pinned bit for bit above)


def test_a_fresh_batchnorm_would_hide_the_fold():
    """the randomised statistics matter: with them, the blob differs from the unfolded convolution weights"""
    net = randomised_net()
    blob = ini.pack_backbone_weights(net).numpy()
    stem = net.img_backbone.conv1.weight.detach().permute(2, 3, 1, 0).reshape(-1).numpy()
    assert not np.allclose(blob[:stem.size], stem, rtol=1e-3)
    assert np.abs(blob[stem.size:stem.size + 64]).max() > 1e-3       # the folded bias of a bias-free convolution


def test_blob_size_layout_and_networks():
    net = randomised_net()
    blob = ini.pack_backbone_weights(net)
    assert blob.dtype == torch.float32 and tuple(blob.shape) == (_lib.NEO_BACKBONE_FLOATS,) == (ini.BACKBONE_FLOATS,) == (11177752,)
    assert blob.device == next(net.parameters()).device and not blob.requires_grad and blob.is_contiguous()
    # the tail of the blob is the fc as it stands: W [24][512] row-major, then b [24]
    fc = net.img_backbone.fc
    assert torch.equal(blob[-24:], fc.bias.detach()) and torch.equal(blob[-24 - 24 * 512:-24], fc.weight.detach().reshape(-1))
    # the stem: W [7][7][1][64], then b [64], folded
    bn = net.img_backbone.bn1
    s = (bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)).detach()
    w = (net.img_backbone.conv1.weight.detach().double() * s[:, None, None, None]).permute(2, 3, 1, 0).reshape(-1)
    assert torch.equal(blob[:49 * 64], w.float())
    assert torch.equal(blob[49 * 64:49 * 64 + 64], (bn.bias.double() - bn.running_mean.double() * s).detach().float())
    # a PlannerNetConv's backbone packs to the same layout: the same backbone parameters give the same blob
    conv = randomised_net(ini.PlannerNetConv)
    conv.img_backbone.load_state_dict(net.img_backbone.state_dict())
    assert torch.equal(ini.pack_backbone_weights(conv), blob)
    assert torch.equal(ini.pack_backbone_weights(net.img_backbone), blob)
    with pytest.raises(ValueError):
        ini.pack_backbone_weights(net.mlp)
    with pytest.raises(ValueError):
        ini.backbone_model(blob[:-1], images(1, 9, 13))


def test_backbone_impl_argument():
    class Cam:
        height, width = 9, 13
    init = ini.BatchInitializer(randomised_net(), device="cpu")
    assert ini.BatchNeoPlanner(None, init, Cam()).backbone_impl == "torch"
    neo = ini.BatchNeoPlanner(None, init, Cam(), backbone_impl="kernel")
    assert neo.backbone_impl == "kernel" and neo.backbone_chunk >= 1
    assert neo.backbone_weights() is neo.backbone_weights() and neo.backbone_weights(refresh=True).numel() == ini.BACKBONE_FLOATS
    with pytest.raises(ValueError):
        ini.BatchNeoPlanner(None, init, Cam(), backbone_impl="mfma")
    with pytest.raises(ValueError):
        init.image_features(images(1, 9, 13), impl="mfma")
    with pytest.raises(ValueError):
        init.image_features(images(1, 9, 13), impl="kernel")        # a CPU initializer: there is no CPU fallback


def test_backbone_entry_points_in_the_abi():
    assert "neo_disp_backbone.hip" in build.SOURCES
    # the family's header recompiles this unit alone
    assert [s for s in build.SOURCES if "neo_backbone.hpp" in build.headers_of(s)] == ["neo_disp_backbone.hip"]
    build.build()
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "neo_planner.h")).read()
    for kind, name, count in (("size_t", "neo_backbone_workspace_bytes", 3), ("int", "neo_backbone_features_dev", 10),
                              ("int", "neo_backbone_launch_times", 11), ("int", "neo_backbone_activation_dev", 12),
                              ("int", "neo_backbone_activation_shape", 6)):
        assert name in _lib.EXPORTS
        decl = re.search(r"\b" + kind + r"\s+" + name + r"\s*\(([^)]*)\)", header)
        assert decl, name
        assert len(getattr(lib, name).argtypes) == len(decl.group(1).split(",")) == count, name
    assert re.search(r"#define\s+NEO_BACKBONE_FLOATS\s+11177752\b", header)
    assert re.search(r"#define\s+NEO_BACKBONE_LAUNCHES\s+21\b", header) and _lib.NEO_BACKBONE_LAUNCHES == 21
    # three buffers of the pool's 64-channel output at 160 x 120; nothing for no image or no size
    assert lib.neo_backbone_workspace_bytes(64, 120, 160) == 3 * 64 * 30 * 40 * 64 * 4
    assert lib.neo_backbone_workspace_bytes(1, 1, 1) == 3 * 512 * 4
    assert lib.neo_backbone_workspace_bytes(0, 120, 160) == 0 and lib.neo_backbone_workspace_bytes(4, 0, 160) == 0
    tool = open(os.path.join(REPO, "tools", "kernel_resource_usage.py")).read()
    assert "neo_disp_backbone.hip" in tool


# the sizes the launches are tested at on the GPU (tests/test_gpu_backbone_launches.py), and the sizes above
LAUNCH_SIZES = [(1, 1), (1, 13), (9, 1), (2, 2), (16, 32), (17, 33), (33, 47)]


def test_launch_table_ends_at_the_blob_size_and_has_the_c_shapes():
    """initializer.backbone_launches: 21 launches, whose weights tile the blob without a gap (in the blob's order: a
    block's conv2 before its downsample branch, which is launched first), whose inputs are their sources' outputs, and
    whose output shapes are neo_backbone_activation_shape's at every size"""
    import ctypes
    build.build()
    lib = _lib.load()
    for H, W in LAUNCH_SIZES + SIZES + [(32, 40), (480, 640)]:
        table = ini.backbone_launches(H, W)
        assert len(table) == _lib.NEO_BACKBONE_LAUNCHES == 21
        assert [r.kind for r in table] == ["stem"] + ["conv"] * 19 + ["poolfc"]
        at = 0
        for r in sorted(table, key=lambda r: r.w_off):
            assert r.w_off == at and r.b_off == at + r.ks * r.ks * r.cin * r.cout, r
            at = r.b_off + r.cout
        assert at == ini.BACKBONE_FLOATS
        assert [k for k, r in enumerate(table) if r.ks == 1 and r.kind == "conv"] == [6, 11, 16]
        for k, r in enumerate(table):
            h, w, c = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
            assert lib.neo_backbone_activation_shape(k, H, W, ctypes.byref(h), ctypes.byref(w), ctypes.byref(c)) == _lib.NEO_OK
            assert (h.value, w.value, c.value) == (r.hout, r.wout, r.cout), (H, W, k)
            assert -1 <= r.src < k and (r.resid is None or 0 <= r.resid < k)
            if r.src >= 0:
                s = table[r.src]
                assert (s.hout, s.wout, s.cout) == (r.hin, r.win, r.cin), (H, W, k)
            if r.resid is not None:
                s = table[r.resid]
                assert (s.hout, s.wout, s.cout) == (r.hout, r.wout, r.cout), (H, W, k)
        assert (table[0].hin, table[0].win, table[0].src) == (H, W, -1) and table[-1].src == 19
    h = ctypes.c_int(-1)
    p = ctypes.byref(h)
    for bad in ((-1, 9, 13), (21, 9, 13), (0, 0, 13), (0, 9, 0)):
        assert lib.neo_backbone_activation_shape(*bad, p, p, p) == 1, bad          # NEO_ERR_INVALID
    assert lib.neo_backbone_activation_shape(0, 9, 13, None, p, p) == 1 and h.value == -1
