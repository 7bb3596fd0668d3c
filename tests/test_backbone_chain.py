"""The SUMMATION RULE of the image backbone (csrc/neo_backbone.hpp, include/neo_planner.h) as a plain host program,
tests/host_harness/backbone_host.cpp -- the "chain model": every launch as nested loops of std::fmaf in the order the rule
states, written from the rule and not from the kernels -- pinned here, without a GPU, to the fp64 model of the weight blob
(initializer.backbone_model / backbone_launch_model).  tests/test_gpu_backbone_launches.py then holds every launch of the
device to both."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from neo_planner_amd import initializer as ini
from test_backbone_cpu import images, randomised_net

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "host_harness", "backbone_host.cpp")
U = 2.0 ** -24          # the unit roundoff of fp32


def _cpu_has_fma():
    try:
        return any(" fma " in line + " " for line in open("/proc/cpuinfo") if line.startswith("flags"))
    except OSError:
        return False


def build_chain_lib(directory):
    """g++ -O2 -std=c++17 -ffp-contract=off, as lbfgs_host.cpp is built.  -mfma where the CPU has the instruction: std::fmaf
    is then one instruction instead of a call of the C library's (which is correctly rounded too: the values are the same,
    the 1.4 G steps of 129 images a second instead of several)."""
    so = os.path.join(str(directory), "backbone_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off"] +
                          (["-mfma"] if _cpu_has_fma() else []) + [SRC, "-o", so])
    L = ctypes.CDLL(so)
    c_p, c_i = ctypes.c_void_p, ctypes.c_int
    L.bb_host_stem.restype = L.bb_host_conv.restype = L.bb_host_pool_fc.restype = None
    L.bb_host_stem.argtypes = [c_p] * 4 + [c_i] * 3
    L.bb_host_conv.argtypes = [c_p] * 5 + [c_i] * 10
    L.bb_host_pool_fc.argtypes = [c_p] * 4 + [c_i] * 4
    return L


@pytest.fixture(scope="module")
def chain_lib(tmp_path_factory):
    return build_chain_lib(tmp_path_factory.mktemp("bbhost"))


def chain_launch(L, blob, rec, act_in, resid=None):
    """one launch of the chain model: blob a float32 NumPy array, rec a record of initializer.backbone_launches, act_in the
    float32 output of launch rec.src ([n][hin][win][cin]; the stem: the uint8 images), resid that of rec.resid or None.
    Returns float32 [n][hout][wout][cout] (the poolfc: [n][24])."""
    assert blob.dtype == np.float32 and blob.size == ini.BACKBONE_FLOATS and (rec.resid is None) == (resid is None)
    want_in = np.uint8 if rec.kind == "stem" else np.float32
    act_in = np.ascontiguousarray(act_in)
    assert act_in.dtype == want_in and act_in.size % (rec.hin * rec.win * rec.cin) == 0
    n = act_in.size // (rec.hin * rec.win * rec.cin)
    w, b = blob[rec.w_off:rec.b_off], blob[rec.b_off:rec.b_off + rec.cout]
    p = lambda a: a.ctypes.data
    if rec.kind == "stem":
        out = np.full((n, rec.hout, rec.wout, rec.cout), np.nan, dtype=np.float32)
        L.bb_host_stem(p(act_in), p(w), p(b), p(out), n, rec.hin, rec.win)
    elif rec.kind == "conv":
        out = np.full((n, rec.hout, rec.wout, rec.cout), np.nan, dtype=np.float32)
        if resid is not None:
            resid = np.ascontiguousarray(resid)
            assert resid.dtype == np.float32 and resid.size == out.size
        L.bb_host_conv(p(act_in), p(w), p(b), p(resid) if resid is not None else None, p(out), n, rec.hin, rec.win, rec.cin,
                       rec.hout, rec.wout, rec.cout, rec.ks, rec.stride, rec.relu)
    else:
        out = np.full((n, rec.cout), np.nan, dtype=np.float32)
        L.bb_host_pool_fc(p(act_in), p(w), p(b), p(out), n, rec.hin * rec.win, rec.cin, rec.cout)
    return out


def launch_bound(blob, rec, act_in, resid=None):
    """what ANY fp32 summation of the launch's products may err by, an element: (K + 2) 2^-24 (|b| + sum |w| |x| + |resid|)
    with K = ks ks cin products.  Derived, not measured: a sum of K + 1 terms in any order rounds at most K times, each
    rounding at most 2^-24 of a partial sum, which is at most S = |b| + sum |w| |x| to first order; the residual add
    rounds once more, on at most S + |resid|; the second-order term K^2 2^-48 S / 2 is below 2^-24 S for K <= 4608, which
    is the bound's last unit.  ReLU and the stem's max do not increase a difference.  (For the pool + fc, K = 512 counts
    the fc's chain; the P - 1 adds and the division of the mean round P more times on values of the inputs' size.  The
    two spare units cover P <= 2 by this derivation; the launches tested have P <= 4.)  S comes from running the same
    fp64 launch on the absolute values."""
    K = rec.ks * rec.ks * rec.cin
    return (K + 2) * U * ini.backbone_launch_model(blob, rec, act_in, resid, absolute=True)


def chain_images(n, H, W):
    """n random uint8 images; image 1 all 0, image 2 all 255 where n > 2"""
    img = images(n, H, W).numpy().copy()
    if n > 2:
        img[1], img[2] = 0, 255
    return img


def fp64_chain(blob, table, img):
    """the fp64 model launch by launch: {launch: float64 output in the device's layout}, -1 the images"""
    blob = blob.double()
    outs = {-1: img}
    for k, rec in enumerate(table):
        outs[k] = ini.backbone_launch_model(blob, rec, outs[rec.src], None if rec.resid is None else outs[rec.resid])
    return outs


@pytest.mark.parametrize("H,W", [(9, 13), (16, 32)])
def test_chain_model_features_equal_the_fp64_model(chain_lib, H, W):
    """all 21 launches of the chain model one after the other, three images: its features meet the criterion the kernels'
    features are held to (tests/test_gpu_backbone.py): err <= 4 e_ref against backbone_model, e_ref the error of torch's
    float32 module on the CPU over the same images.  And backbone_launch_model chained is backbone_model."""
    n = 3
    net = randomised_net(H=H, W=W)
    img = chain_images(n, H, W)
    blob = ini.pack_backbone_weights(net)
    want = ini.backbone_model(blob, img)
    with torch.no_grad():
        f32 = net.float().eval().image_features(torch.from_numpy(img).float().reshape(n, 1, H, W)).numpy().astype(np.float64)
    table = ini.backbone_launches(H, W)
    blob32 = blob.numpy()
    outs = {-1: img}
    for k, rec in enumerate(table):
        outs[k] = chain_launch(chain_lib, blob32, rec, outs[rec.src], None if rec.resid is None else outs[rec.resid])
        assert outs[k].dtype == np.float32 and np.isfinite(outs[k]).all(), k
    got = outs[len(table) - 1]
    e_ref = np.abs(f32 - want).max()
    err = np.abs(got.astype(np.float64) - want).max()
    print(f"{H} x {W}: chain model {err:.3e}, e_ref {e_ref:.3e}, ratio {err / e_ref:.2f}, scale {np.abs(want).max():.3e}")
    assert got.shape == (n, 24) and e_ref > 0.0 and err <= 4.0 * e_ref
    assert np.array_equal(fp64_chain(blob, table, img)[len(table) - 1], want)


@pytest.mark.parametrize("H,W", [(1, 1), (9, 13), (16, 32)])
def test_every_launch_of_the_chain_model_is_within_the_rounding_bound(chain_lib, H, W):
    """every launch alone, fed the fp64 model's input rounded to fp32 (both sides read the same fp32 values): every element
    within launch_bound of backbone_launch_model"""
    n = 3
    net = randomised_net(H=H, W=W)
    img = chain_images(n, H, W)
    blob = ini.pack_backbone_weights(net)
    table = ini.backbone_launches(H, W)
    blob32, blob64 = blob.numpy(), blob.double()
    outs64 = fp64_chain(blob64, table, img)
    in32 = {k: (v if k < 0 else v.astype(np.float32)) for k, v in outs64.items()}
    worst = []
    for k, rec in enumerate(table):
        x, r = in32[rec.src], None if rec.resid is None else in32[rec.resid]
        got = chain_launch(chain_lib, blob32, rec, x, r)
        want = ini.backbone_launch_model(blob64, rec, x, r)
        bound = launch_bound(blob64, rec, x, r)
        assert got.shape == want.shape == bound.shape, k
        err = np.abs(got.astype(np.float64) - want)
        worst.append(float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (k, rec.kind, worst[-1])
        if rec.kind != "poolfc":
            assert np.abs(want).max() > 0.0, k              # (no launch is dead: there is something to be wrong about)
    print(f"{H} x {W}: largest err / bound a launch: " + " ".join(f"{v:.3f}" for v in worst))
