"""Every launch of the image backbone on the GPU, one at a time (neo_backbone_activation_dev), from the DEVICE's own
outputs of the launches it reads: errors do not accumulate and a failure names its launch.  A launch is held to

 (a) the fp64 model of that launch (initializer.backbone_launch_model) -- elementwise within the rounding bound of any fp32
     summation of its products (test_backbone_chain.launch_bound: derived, not measured), and its largest error at most 4
     e_seq, e_seq being the largest error of the chain model on the same inputs (tests/host_harness/backbone_host.cpp: a
     reference chain of the same length over the same products, which differs from the kernel in nothing but possibly the
     order; 4 is the margin test_features_equal_the_fp64_model gives two fp32 sums of the same products);
 (b) the SUMMATION RULE of csrc/neo_backbone.hpp: the device's values ARE the chain model's (np.array_equal on the
     floats: -0 and +0 agree, the sign of a ReLU's zero is not pinned by the rule);
 (c) its buffers: 64 guard bytes behind act_out stay, and launch 20's activation is neo_backbone_features_dev's bits.

The sizes are the smallest at which each index computation can go wrong (CASES)."""
import ctypes

import numpy as np
import pytest

from neo_planner_amd import _lib
from neo_planner_amd import initializer as ini
from test_backbone_chain import build_chain_lib, chain_launch, launch_bound
from test_backbone_cpu import randomised_net
from test_gpu_backbone import batch_images, bits, run_kernel

pytestmark = pytest.mark.gpu

GUARD = 64
# H, W, n: what the case reaches
CASES = [
    (1, 1, 1),        # every layer 1 x 1: one column in every conv launch; the activation buffer is sized by layer 4
    (1, 1, 128),      # ... exactly one column tile (a tile spans 128 images)
    (1, 1, 129),      # ... one live column in a second tile
    (1, 13, 3),       # a one-pixel axis: every tap of a row is padding
    (9, 1, 3),        # ... of a column
    (2, 2, 3),        # an even size: stride 2 never touches the far padding
    (16, 32, 4),      # the pooled image is exactly one 8 x 4 stem tile; 128, 32, 8 and 4 columns in layers 1 .. 4
    (17, 33, 3),      # one pooled pixel past the tile on both axes; 135 columns in layer 1: a tile ends in mid-row
    (33, 47, 3),      # the odd size of test_gpu_backbone.py, launch by launch
]


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _p(t, first=0):
    return ctypes.c_void_p(t.data_ptr() + first)


@pytest.fixture(scope="module")
def chain_lib(tmp_path_factory):
    return build_chain_lib(tmp_path_factory.mktemp("bbhost"))


@pytest.fixture(scope="module")
def net():
    """the network (its weights do not depend on the image size): the float32 blob on the CPU as NumPy, in fp64, on the GPU"""
    torch, dev = _torch()
    blob = ini.pack_backbone_weights(randomised_net())
    return dict(blob32=blob.numpy(), blob64=blob.double(), blob_dev=blob.to(dev))


def device_activations(blob_dev, img_dev, H, W):
    """the 21 activations of neo_backbone_activation_dev as float32 NumPy arrays, each fetched by a call of its own into a
    buffer with GUARD bytes of 0x5A behind it, out of a workspace of exactly neo_backbone_workspace_bytes with a guard too"""
    torch, dev = _torch()
    c = _lib.default_context()
    n = int(img_dev.shape[0])
    need = int(c.lib.neo_backbone_workspace_bytes(n, H, W))
    ws = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    table = ini.backbone_launches(H, W)
    bufs = []
    for k, rec in enumerate(table):
        floats = n * rec.hout * rec.wout * rec.cout
        bufs.append(torch.full((floats * 4 + GUARD,), 0x5A, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    for k, rec in enumerate(table):
        c.call("neo_backbone_activation_dev", _p(blob_dev), blob_dev.numel(), _p(img_dev), n, H, W, _p(ws), need, k, _p(bufs[k]),
               n * rec.hout * rec.wout * rec.cout)
    c.synchronize()
    acts = []
    for k, rec in enumerate(table):
        raw = bufs[k].cpu().numpy()
        assert (raw[-GUARD:] == 0x5A).all(), f"launch {k}: the guard behind act_out"
        shape = (n, rec.cout) if rec.kind == "poolfc" else (n, rec.hout, rec.wout, rec.cout)
        acts.append(raw[:-GUARD].view(np.float32).reshape(shape).copy())
    assert (ws[need:].cpu().numpy() == 0xA5).all(), "the guard behind the workspace"
    return table, acts


def ulps(a, b):
    """the largest distance of two float32 arrays in units of the last place (-0 and +0 are 0 apart)"""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.abs(key(a) - key(b)).max())


@pytest.mark.parametrize("H,W,n", CASES)
def test_every_launch_against_the_fp64_model_and_the_chain_model(chain_lib, net, H, W, n):
    """(a), (b) and (c) of the module's text for the 21 launches of one case; every launch's figures are printed, all
    failures of the case are reported together, each with its launch.  Seen on the MI355X: all 189
    launches 0 ulp from the chain model -- the f32 MFMA is the k-ordered fmaf chain --, hence err / e_seq = 1.00
    everywhere; the largest error 0.001 - 0.073 of the rounding bound."""
    torch, dev = _torch()
    img = batch_images(H, W, n=n)
    img_dev = torch.from_numpy(img).to(dev)
    table, acts = device_activations(net["blob_dev"], img_dev, H, W)
    dev_out = dict(enumerate(acts))
    dev_out[-1] = img
    failures = []
    for k, rec in enumerate(table):
        x, r = dev_out[rec.src], None if rec.resid is None else dev_out[rec.resid]
        got = acts[k]
        want = ini.backbone_launch_model(net["blob64"], rec, x, r)
        bound = launch_bound(net["blob64"], rec, x, r)
        seq = chain_launch(chain_lib, net["blob32"], rec, x, r)
        assert got.shape == want.shape == seq.shape and np.isfinite(got).all(), k
        err = np.abs(got.astype(np.float64) - want)
        e_seq = np.abs(seq.astype(np.float64) - want).max()
        worst = err.max()
        ratio = worst / e_seq if e_seq > 0.0 else (0.0 if worst == 0.0 else np.inf)
        print(f"{H} x {W}, n = {n}, launch {k:2d} ({rec.kind} {rec.ks} x {rec.ks}, {rec.cin} -> {rec.cout}, "
              f"{n * rec.hout * rec.wout} columns): err {worst:.3e}, e_seq {e_seq:.3e}, ratio {ratio:.2f}, "
              f"err / bound {(err / np.maximum(bound, 1e-300)).max():.4f}, {ulps(got, seq)} ulp from the chain model, "
              f"scale {np.abs(want).max():.3e}")
        if not (err <= bound).all():
            failures.append(f"launch {k}: (a) {int((err > bound).sum())} elements beyond the rounding bound of the fp64 model")
        if not worst <= 4.0 * e_seq:
            failures.append(f"launch {k}: (a) err {worst:.3e} > 4 e_seq = {4.0 * e_seq:.3e}")
        if not np.array_equal(got, seq):
            failures.append(f"launch {k}: (b) {int((got != seq).sum())} values are not the chain model's, {ulps(got, seq)} ulp")
        if rec.kind != "poolfc" and not np.abs(want).max() > 0.0:
            failures.append(f"launch {k}: the fp64 model is all zero: nothing is tested")
    assert not failures, "\n".join(failures)
    # (c) the last launch's activation is the features call's output, bit for bit
    assert np.array_equal(bits(acts[-1]), bits(run_kernel(net["blob_dev"], img_dev)))
