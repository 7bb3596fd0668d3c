"""The bf16 route of the image backbone on the GPU (csrc/neo_backbone_bf16.hpp): the device's pack against its NumPy twin,
every launch one at a time from the DEVICE's own stored activations (neo_backbone_bf16_activation_dev), the features
end to end against what the format itself costs, their independence of the batch, the argument refusals, and
BatchNeoPlanner / FleetReplanLoop on backbone_impl="kernel_bf16".

A launch is held to
 (a) the fp64 model of that launch on the quantised weights and the device's own bf16 inputs, whose products are exact in
     fp32: |f32 - want| <= (K + 2) 2^-23 S + 2^-126 elementwise, S the same launch on absolute values, K = ks ks cin.  The
     bound of ANY fp32 accumulation of these terms, whether a step rounds to nearest (2^-24) or truncates (2^-23): derived,
     not measured -- how the bf16 matrix instruction sums its 16 products is not assumed;
 (b) the stored bf16 bits are bf16_bits(bf16_round(f32)) of the fp32 values the same launch handed out: the device's
     conversion is the twin's round-to-nearest-even;
 (c) 64 guard bytes behind both outputs and behind a workspace of exactly neo_backbone_bf16_workspace_bytes stay;
 (d) launch 20's values are neo_backbone_features_bf16_dev's bits;
 (e) the model is not all zero in any launch but the last."""
import ctypes
import os
import re

import numpy as np
import pytest

import neo_planner_amd as npa
from neo_planner_amd import _lib
from neo_planner_amd import initializer as ini
from test_backbone_cpu import randomised_net
from test_gpu_backbone import batch_images, bits, reference
from test_gpu_record import _fleet_setup

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
NEO_ERR_INVALID = 1
# the column tile of bb_conv_bf16_kernel, from the kernels' header
T = int(re.search(r"constexpr\s+int\s+kBhTileCols\s*=\s*(\d+)",
                  open(os.path.join(REPO, "neo-planner_amd", "csrc", "neo_backbone_bf16.hpp")).read()).group(1))
# H, W, n: the sizes of tests/test_gpu_backbone_launches.py CASES, its two tile cases at this kernel's column tile
CASES = [
    (1, 1, 1),        # every layer 1 x 1: one column in every conv launch
    (1, 1, T),        # ... exactly one column tile
    (1, 1, T + 1),    # ... one live column in a second tile
    (1, 13, 3),       # a one-pixel axis: every tap of a row is padding
    (9, 1, 3),        # ... of a column
    (2, 2, 3),        # an even size: stride 2 never touches the far padding
    (16, 32, 4),      # the pooled image is exactly one 8 x 4 stem tile
    (17, 33, 3),      # one pooled pixel past the tile on both axes; 135 columns in layer 1: a tile ends in mid-row
    (33, 47, 3),      # the odd size of the end-to-end test, launch by launch
]


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _p(t, first=0):
    return ctypes.c_void_p(t.data_ptr() + first) if t is not None else None


@pytest.fixture(scope="module")
def net():
    """the network of the fp32 launch test: its float32 blob, the twin's packed blob on the CPU and the GPU, and the
    quantised weights in fp64 (the fp32 blob's order)"""
    torch, dev = _torch()
    blob32 = ini.pack_backbone_weights(randomised_net())
    packed = ini.pack_backbone_weights_bf16(blob32)
    return dict(blob32=blob32, packed=packed, packed_dev=packed.to(dev), un64=ini.unpack_backbone_weights_bf16(packed))


def run_bf16(packed_dev, img_dev, chunk=None):
    """neo_backbone_features_bf16_dev on the default context through backbone_features_kernel; features as NumPy"""
    torch, _ = _torch()
    c = _lib.default_context()
    torch.cuda.synchronize()
    feat, _ws = ini.backbone_features_kernel(c, packed_dev, img_dev, chunk=chunk or max(1, int(img_dev.shape[0])), precision="bf16")
    c.synchronize()
    return feat.cpu().numpy()


def test_the_devices_pack_is_the_twins(net):
    torch, dev = _torch()
    c = _lib.default_context()
    n = _lib.NEO_BACKBONE_BF16_BYTES
    blob_dev = net["blob32"].to(dev)
    out = torch.full((n + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    c.call("neo_backbone_pack_bf16_dev", _p(blob_dev), blob_dev.numel(), _p(out), n)
    c.synchronize()
    got = out.cpu().numpy()
    assert (got[n:] == 0x5A).all(), "the guard behind the packed blob"
    want = net["packed"].numpy()
    assert np.array_equal(got[:n], want), f"{int((got[:n] != want).sum())} bytes differ, the first at {int(np.argmax(got[:n] != want))}"


def device_activations(packed_dev, img_dev, H, W):
    """the 21 launches of neo_backbone_bf16_activation_dev as (bf16 bits or None, float32 values), each fetched by a call of
    its own into buffers with GUARD bytes of 0x5A behind them, out of a workspace of exactly
    neo_backbone_bf16_workspace_bytes with a guard too"""
    torch, dev = _torch()
    c = _lib.default_context()
    n = int(img_dev.shape[0])
    need = int(c.lib.neo_backbone_bf16_workspace_bytes(n, H, W))
    assert need > 0 and need % 16 == 0
    ws = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    table = ini.backbone_launches(H, W)
    b16, f32 = [], []
    for k, rec in enumerate(table):
        elems = n * rec.hout * rec.wout * rec.cout
        b16.append(None if rec.kind == "poolfc" else torch.full((elems * 2 + GUARD,), 0x5A, dtype=torch.uint8, device=dev))
        f32.append(torch.full((elems * 4 + GUARD,), 0x5A, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    for k, rec in enumerate(table):
        c.call("neo_backbone_bf16_activation_dev", _p(packed_dev), packed_dev.numel(), _p(img_dev), n, H, W, _p(ws), need, k,
               _p(b16[k]), _p(f32[k]), n * rec.hout * rec.wout * rec.cout)
    c.synchronize()
    acts = []
    for k, rec in enumerate(table):
        shape = (n, rec.cout) if rec.kind == "poolfc" else (n, rec.hout, rec.wout, rec.cout)
        raw32 = f32[k].cpu().numpy()
        assert (raw32[-GUARD:] == 0x5A).all(), f"launch {k}: the guard behind act_f32_out"
        stored = None
        if b16[k] is not None:
            raw16 = b16[k].cpu().numpy()
            assert (raw16[-GUARD:] == 0x5A).all(), f"launch {k}: the guard behind act_bf16_out"
            stored = raw16[:-GUARD].view(np.uint16).reshape(shape).copy()
        acts.append((stored, raw32[:-GUARD].view(np.float32).reshape(shape).copy()))
    assert (ws[need:].cpu().numpy() == 0xA5).all(), "the guard behind the workspace"
    return table, acts


@pytest.mark.parametrize("H,W,n", CASES)
def test_every_launch_against_the_fp64_model_of_its_own_inputs(net, H, W, n):
    """(a) .. (e) of the module's text for the 21 launches of one case; every launch's err / bound is printed, all failures
    of the case are reported together, each with its launch.  Seen on the MI355X: err / bound 0.0002 - 0.011
    in the 171 convolution launches, 0.008 - 0.033 in the stem's, 0.0009 - 0.0026 in the pool + fc's; no stored value off
    the twin's rounding."""
    torch, dev = _torch()
    img = batch_images(H, W, n=n)
    img_dev = torch.from_numpy(img).to(dev)
    table, acts = device_activations(net["packed_dev"], img_dev, H, W)
    # what a later launch reads: the stored bf16 values, widened
    stored = {k: ini.bf16_from_bits(a[0]).astype(np.float64) for k, a in enumerate(acts) if a[0] is not None}
    stored[-1] = img
    failures = []
    for k, rec in enumerate(table):
        x, r = stored[rec.src], None if rec.resid is None else stored[rec.resid]
        b16, got = acts[k]
        want = ini.backbone_launch_model(net["un64"], rec, x, r)
        S = ini.backbone_launch_model(net["un64"], rec, x, r, absolute=True)
        K = rec.ks * rec.ks * rec.cin
        bound = (K + 2) * 2.0 ** -23 * S + 2.0 ** -126
        assert got.shape == want.shape and np.isfinite(got).all(), k
        err = np.abs(got.astype(np.float64) - want)
        print(f"{H} x {W}, n = {n}, launch {k:2d} ({rec.kind} {rec.ks} x {rec.ks}, {rec.cin} -> {rec.cout}, "
              f"{n * rec.hout * rec.wout} columns): err {err.max():.3e}, err / bound {(err / bound).max():.4f}, "
              f"scale {np.abs(want).max():.3e}")
        if not (err <= bound).all():
            failures.append(f"launch {k}: (a) {int((err > bound).sum())} elements beyond the bound of an fp32 accumulation, "
                            f"err / bound {(err / bound).max():.3f}")
        if b16 is not None:
            twin = ini.bf16_bits(ini.bf16_round(got))
            if not np.array_equal(b16, twin):
                failures.append(f"launch {k}: (b) {int((b16 != twin).sum())} stored values are not the twin's rounding of the fp32 value")
        if rec.kind != "poolfc" and not np.abs(want).max() > 0.0:
            failures.append(f"launch {k}: (e) the fp64 model is all zero: nothing is tested")
    assert not failures, "\n".join(failures)
    # (d) the last launch's values are the features call's output, bit for bit
    assert np.array_equal(bits(acts[-1][1]), bits(run_bf16(net["packed_dev"], img_dev)))


def test_features_end_to_end_within_what_the_format_costs():
    """70 images of 33 x 47: the device's features are within 4 e_q of backbone_model(blob32), e_q being the largest error of
    backbone_bf16_model (the quantised chain in fp64) against the same yardstick on the same images; 4 is the margin the
    project gives two roundings of the same products."""
    torch, dev = _torch()
    r = reference(33, 47)
    packed = ini.pack_backbone_weights_bf16(r["blob"])
    got = run_bf16(packed.to(dev), torch.from_numpy(r["img"]).to(dev))
    want = r["want"]
    e_q = np.abs(ini.backbone_bf16_model(packed, r["img"]) - want).max()
    err = np.abs(got.astype(np.float64) - want).max()
    scale = np.abs(want).max()
    print(f"33 x 47, n = 70: device {err:.3e} ({100 * err / scale:.3f} % of the scale), e_q {e_q:.3e} "
          f"({100 * e_q / scale:.3f} %), ratio {err / e_q:.2f}")
    assert got.shape == (70, 24) and got.dtype == np.float32 and np.isfinite(got).all()
    assert e_q > 0.0 and err <= 4.0 * e_q
    assert len({row.tobytes() for row in got}) == 70


def test_an_images_features_do_not_depend_on_the_batch(net):
    """image 5 of batch_images(17, 33) alone, in a batch of 3, at position 69 of 70 (a second column tile in every layer:
    layer 4 has two columns an image) and through backbone_features_kernel in chunks of 1, 2 and n: the same bits"""
    torch, dev = _torch()
    img = batch_images(17, 33)
    packed = net["packed_dev"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    assert 2 * 69 >= T
    alone = run_bf16(packed, up(img[5:6]))[0]
    assert np.isfinite(alone).all() and np.abs(alone).max() > 0.0
    three = img[[9, 5, 11]]
    assert np.array_equal(bits(run_bf16(packed, up(three))[1]), bits(alone))
    moved = img[::-1].copy()
    moved[69] = img[5]
    assert np.array_equal(bits(run_bf16(packed, up(moved))[69]), bits(alone))
    whole = run_bf16(packed, up(img))
    for chunk in (1, 2, len(img)):
        assert np.array_equal(bits(run_bf16(packed, up(img), chunk=chunk)), bits(whole)), chunk
    assert np.array_equal(bits(whole[5]), bits(alone))
    assert len({row.tobytes() for row in whole}) == len(img)


def test_refusals_and_the_empty_call():
    """every refusal include/neo_planner.h lists: NEO_ERR_INVALID with a message, the poisoned outputs untouched"""
    torch, dev = _torch()
    c = _lib.default_context()
    L = c.lib
    N, H, W = 2, 9, 13
    need = int(L.neo_backbone_bf16_workspace_bytes(N, H, W))
    nbytes = _lib.NEO_BACKBONE_BF16_BYTES
    packed = torch.zeros(nbytes + 16, dtype=torch.uint8, device=dev)
    blob = torch.zeros(_lib.NEO_BACKBONE_FLOATS, dtype=torch.float32, device=dev)
    img = torch.zeros((N, H, W), dtype=torch.uint8, device=dev)
    ws = torch.zeros(need + 16, dtype=torch.uint8, device=dev)
    out = torch.full((N, 24), -7.25, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    good = dict(packed=_p(packed), packed_bytes=nbytes, images=_p(img), n=N, H=H, W=W, workspace=_p(ws), workspace_bytes=need,
                out=_p(out))
    order = ("packed", "packed_bytes", "images", "n", "H", "W", "workspace", "workspace_bytes", "out")

    def call(**change):
        a = dict(good, **change)
        return L.neo_backbone_features_bf16_dev(c.h, *[a[k] for k in order])

    bad = [dict(packed=None), dict(images=None), dict(workspace=None), dict(out=None), dict(n=-1), dict(H=0), dict(W=0),
           dict(H=-3), dict(n=2 ** 20, H=2 ** 6, W=2 ** 5), dict(packed_bytes=nbytes - 1), dict(packed_bytes=nbytes + 1),
           dict(packed_bytes=0), dict(workspace_bytes=need - 1), dict(workspace_bytes=0), dict(workspace=_p(ws, 4)),
           dict(packed=_p(packed, 8))]
    for change in bad:
        assert call(**change) == NEO_ERR_INVALID, change
        assert b"backbone bf16" in L.neo_last_error(c.h), change
    assert L.neo_backbone_features_bf16_dev(None, *[good[k] for k in order]) == NEO_ERR_INVALID
    assert call(n=0) == _lib.NEO_OK and call(n=0, workspace_bytes=0) == _lib.NEO_OK
    # the pack
    pk = torch.full((nbytes + 16,), 0x5A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    for args in ((None, blob.numel(), _p(pk), nbytes), (_p(blob), blob.numel(), None, nbytes),
                 (_p(blob), blob.numel() - 1, _p(pk), nbytes), (_p(blob), blob.numel(), _p(pk), nbytes - 2),
                 (_p(blob), blob.numel(), _p(pk), nbytes + 16), (_p(blob), blob.numel(), _p(pk, 8), nbytes)):
        assert L.neo_backbone_pack_bf16_dev(c.h, *args) == NEO_ERR_INVALID, args
        assert b"backbone bf16 pack" in L.neo_last_error(c.h), args
    assert L.neo_backbone_pack_bf16_dev(None, _p(blob), blob.numel(), _p(pk), nbytes) == NEO_ERR_INVALID
    # the measuring form
    ms = (ctypes.c_float * _lib.NEO_BACKBONE_LAUNCHES)()
    args = [good[k] for k in order]
    assert L.neo_backbone_bf16_launch_times(c.h, *args, None) == NEO_ERR_INVALID
    assert L.neo_backbone_bf16_launch_times(c.h, args[0], 5, *args[2:], ms) == NEO_ERR_INVALID
    assert L.neo_backbone_bf16_launch_times(c.h, *args[:3], 0, *args[4:], ms) == NEO_ERR_INVALID
    # one launch's output
    h, w, ch = (ctypes.c_int() for _ in range(3))
    launch = 7
    assert L.neo_backbone_activation_shape(launch, H, W, ctypes.byref(h), ctypes.byref(w), ctypes.byref(ch)) == _lib.NEO_OK
    elems = N * h.value * w.value * ch.value
    a16 = torch.full((elems,), 0x5A5A, dtype=torch.int16, device=dev)
    a32 = torch.full((elems,), -7.25, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    good_act = dict(good, launch=launch, a16=_p(a16), a32=_p(a32), elems=elems)

    def call_act(**change):
        a = dict(good_act, **change)
        return L.neo_backbone_bf16_activation_dev(c.h, *[a[k] for k in order[:-1]], a["launch"], a["a16"], a["a32"], a["elems"])

    bad_act = [b for b in bad if "out" not in b] + [
        dict(a16=None, a32=None), dict(launch=-1), dict(launch=_lib.NEO_BACKBONE_LAUNCHES), dict(elems=elems - 1),
        dict(elems=elems + 1), dict(elems=0), dict(launch=0), dict(n=0),
        dict(launch=20, elems=N * 24), dict(launch=20, elems=N * 24, a32=None)]      # launch 20 has fp32 values only
    for change in bad_act:
        assert call_act(**change) == NEO_ERR_INVALID, change
        assert b"backbone bf16" in L.neo_last_error(c.h), change
    assert call_act(n=0, elems=0) == _lib.NEO_OK
    c.synchronize()
    # nothing was launched or copied by any of them
    assert (out.cpu().numpy() == np.float32(-7.25)).all() and (pk.cpu().numpy() == 0x5A).all()
    assert (a32.cpu().numpy() == np.float32(-7.25)).all() and (a16.cpu().numpy() == 0x5A5A).all()
    # ... and the good calls run: a zero blob gives zero features, zero activations, and 21 times
    assert call() == _lib.NEO_OK and call_act() == _lib.NEO_OK and call_act(a16=None) == _lib.NEO_OK
    assert call_act(a32=None) == _lib.NEO_OK and call_act(launch=20, elems=N * 24, a16=None) == _lib.NEO_OK
    assert L.neo_backbone_bf16_launch_times(c.h, *args, ms) == _lib.NEO_OK
    c.synchronize()
    assert (out.cpu().numpy() == 0.0).all() and (a16.cpu().numpy() == 0).all() and (a32.cpu().numpy() == 0.0).all()
    assert all(0.0 < t < 1e3 for t in ms)


# ------------------------------------------------------------------ BatchNeoPlanner and the fleet
CAM = dict(width=40, height=32)


@pytest.fixture(scope="module")
def fleet():
    torch, dev = _torch()
    fs = _fleet_setup()
    fs["cam"] = npa.DepthCamera(**CAM)
    net = randomised_net(H=CAM["height"], W=CAM["width"], seed=11)
    neo = ini.BatchNeoPlanner(npa.BatchPlanner(), ini.BatchInitializer(net, device=dev), fs["cam"], backbone_impl="kernel_bf16")
    yield fs, neo
    c = _lib.default_context()
    for m in fs["maps"]:
        c.check(c.lib.neo_esdf_drop(c.h, m.scene_id))


def test_features_dev_on_the_bf16_backbone(fleet):
    """six requests' rendered 40 x 32 images: features_dev is backbone_features_kernel(precision="bf16") on the same images,
    and BatchInitializer.image_features(impl="kernel_bf16"), bit for bit; the blob is packed once"""
    torch, dev = _torch()
    fs, neo = fleet
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n = 6
    d = fs["goals"][:n] - fs["start"][:n]
    pose = up(npa.DepthCamera.poses(np.concatenate([fs["start"][:n], np.full((n, 1), 2.0)], 1), np.arctan2(d[:, 1], d[:, 0])))
    boxes, begin = (up(a) for a in fs["packed"])
    sidx = up(fs["scene_index"][:n])
    img = fs["cam"].render_dev(boxes, begin, pose, sidx, want_m=False)["depth_u8"].contiguous()
    k = neo.features_dev(boxes, begin, pose, sidx)
    assert tuple(k.shape) == (n, 24) and k.dtype == torch.float32 and k.is_contiguous()
    packed = neo.backbone_weights(precision="bf16")
    assert packed is neo.backbone_weights(precision="bf16") and packed.dtype == torch.uint8 and packed.is_cuda
    assert torch.equal(packed.cpu(), ini.pack_backbone_weights_bf16(ini.pack_backbone_weights(neo.init.net).cpu()))
    direct = run_bf16(packed, img)
    assert np.array_equal(bits(k.cpu().numpy()), bits(direct))
    assert torch.equal(neo.init.image_features(img, impl="kernel_bf16"), k)
    assert np.isfinite(direct).all() and len({row.tobytes() for row in direct}) >= 3
    # (another route than the fp32 kernels: not their bits)
    assert not np.array_equal(neo.init.image_features(img, impl="kernel").cpu().numpy(), direct)


def test_a_neo_fleet_flies_on_the_bf16_backbone(fleet):
    """eight missions, mode "neo", a 40 x 32 camera: a few ticks to finite results"""
    fs, neo = fleet
    idx = np.arange(8)
    loop = npa.FleetReplanLoop(neo.bp, fs["maps"][0], fs["goals"][idx], scene_ids=fs["sids"][idx], mission_ids=idx, mode="neo",
                               neo=neo, scenes=fs["packed"], scene_index=fs["scene_index"][idx])
    out = loop.run(fs["start"][idx], max_replans=6)
    assert loop.timings and all("neo_s" in t for t in loop.timings)
    for i in range(len(idx)):
        assert np.isfinite(loop.commands(i)).all(), i
    assert (out["opt_runs"] >= out["replans"]).all() and (out["replans"] >= 1).any()
    assert np.isfinite(np.asarray(out["iter_num"], dtype=np.float64)).all()
    assert neo._workspace is not None and neo.backbone_impl == "kernel_bf16"


def test_wrong_arguments_raise(fleet):
    torch, dev = _torch()
    fs, neo = fleet
    with pytest.raises(ValueError):
        ini.BatchNeoPlanner(neo.bp, neo.init, fs["cam"], backbone_impl="kernel_fp16")
    with pytest.raises(ValueError):
        neo.init.image_features(torch.zeros((1, 32, 40), dtype=torch.uint8, device=dev), impl="bf16")
    img = torch.zeros((1, 32, 40), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        ini.backbone_features_kernel(_lib.default_context(), neo.backbone_weights(precision="bf16"), img, precision="fp16")
    with pytest.raises(ValueError):       # the float32 blob is not the packed one
        ini.backbone_features_kernel(_lib.default_context(), neo.backbone_weights(), img, precision="bf16")
