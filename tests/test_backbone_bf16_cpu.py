"""The bf16 route of the image backbone, off the GPU: the rounding twin (bf16_round, bf16_bits, bf16_from_bits), the
packed blob (pack_backbone_weights_bf16 / unpack_backbone_weights_bf16) against the layout text of
csrc/neo_backbone_bf16.hpp, what the format costs (backbone_bf16_model against backbone_model), and the entry points in
the C ABI."""
import os
import re

import numpy as np
import pytest
import torch

from neo_planner_amd import _lib, build
from neo_planner_amd import initializer as ini
from test_backbone_cpu import images, randomised_net

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def test_bf16_round_on_hand_made_vectors():
    one = 0x3F800000
    cases = [
        (one + 0x8000, one),                    # 1 + 2^-8: a tie, down to the even 1
        (one + 0x18000, one + 0x20000),         # 1 + 3 2^-8: a tie, up to the even 1 + 2^-6
        (one + 0x8001, one + 0x10000),          # just above a tie
        (one + 0x7FFF, one),                    # just below a tie
        (one + 0x18001, one + 0x20000), (one + 0x17FFF, one + 0x10000),
        (0x00000000, 0x00000000), (0x80000000, 0x80000000),           # +-0
        (0x7F800000, 0x7F800000), (0xFF800000, 0xFF800000),           # +-inf
        (0x7F7FFFFF, 0x7F800000), (0xFF7FFFFF, 0xFF800000),           # +-FLT_MAX -> +-inf
        (0x00000001, 0x00000000), (0x00008000, 0x00000000),           # fp32 denormals: below and at the first tie (to even 0)
        (0x00008001, 0x00010000), (0x00018000, 0x00020000),           # ... above it; a tie up to the even denormal
        (0x007FFFFF, 0x00800000), (0x807FFFFF, 0x80800000),           # the largest denormal rounds up to FLT_MIN
    ]
    x = f32([c[0] for c in cases])
    got = ini.bf16_round(x)
    assert got.dtype == np.float32
    assert got.view(np.uint32).tolist() == [c[1] for c in cases]
    assert ini.bf16_bits(x).tolist() == [c[1] >> 16 for c in cases]
    assert np.array_equal(ini.bf16_from_bits(ini.bf16_bits(x)).view(np.uint32), got.view(np.uint32))
    assert float(got[0]) == 1.0 and float(got[1]) == 1.0 + 2.0 ** -6
    nan = ini.bf16_round(f32([0x7FC00000, 0x7F800001, 0xFFFFFFFF, 0x7F80FFFF]))
    assert np.isnan(nan).all()


def test_bf16_round_is_idempotent_and_nearest():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.standard_normal(4096).astype(np.float32) * 300.0,
                        rng.integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    x = x[np.isfinite(x)]
    once = ini.bf16_round(x)
    assert np.array_equal(ini.bf16_round(once).view(np.uint32), once.view(np.uint32))
    assert (once.view(np.uint32) & 0xFFFF == 0).all()
    # nearest: no further than half a bf16 step of the value's binade (the normal values)
    normal = np.abs(x) >= np.float32(2.0 ** -126)
    fin = np.isfinite(once) & normal
    step = 2.0 ** (np.floor(np.log2(np.abs(x[fin].astype(np.float64)))) - 7)
    assert (np.abs(once[fin].astype(np.float64) - x[fin]) <= step / 2).all()


def header_constant(path, name):
    m = re.search(r"(?:#define\s+|constexpr\s+int\s+)" + name + r"\s*=?\s*(\d+)", open(os.path.join(REPO, path)).read())
    assert m, name
    return int(m.group(1))


@pytest.fixture(scope="module")
def blobs():
    blob32 = ini.pack_backbone_weights(randomised_net())
    return blob32, ini.pack_backbone_weights_bf16(blob32)


def test_packed_blob_size_is_the_headers(blobs):
    blob32, packed = blobs
    n = header_constant("include/neo_planner.h", "NEO_BACKBONE_BF16_BYTES")
    assert packed.dtype == torch.uint8 and packed.is_contiguous()
    assert tuple(packed.shape) == (n,) == (_lib.NEO_BACKBONE_BF16_BYTES,) == (ini.BACKBONE_BF16_BYTES,) == (22396000,)
    assert n == 2 * 11157504 + 4 * 20248
    # every part starts 16-byte aligned
    assert all(at % 16 == 0 for _, _, _, at, _ in ini._bf16_parts())
    with pytest.raises(ValueError):
        ini.pack_backbone_weights_bf16(blob32[:-1])
    with pytest.raises(ValueError):
        ini.unpack_backbone_weights_bf16(packed[:-1])


def test_unpack_is_the_rounded_blob_and_keeps_the_fp32_parts(blobs):
    blob32, packed = blobs
    src = blob32.numpy()
    un = ini.unpack_backbone_weights_bf16(packed)
    assert un.dtype == torch.float64 and tuple(un.shape) == (ini.BACKBONE_FLOATS,)
    un = un.numpy()
    table = ini.backbone_launches(9, 13)
    convs = 0
    for rec in table:
        w = slice(rec.w_off, rec.b_off)
        b = slice(rec.b_off, rec.b_off + rec.cout)
        assert np.array_equal(un[b].astype(np.float32).view(np.uint32), src[b].view(np.uint32)), rec       # a bias: the same bits
        if rec.kind == "conv":
            convs += 1
            assert np.array_equal(un[w], ini.bf16_round(src[w]).astype(np.float64)), rec
            assert not np.array_equal(un[w], src[w].astype(np.float64))            # (the rounding does something)
        else:
            assert np.array_equal(un[w].astype(np.float32).view(np.uint32), src[w].view(np.uint32)), rec   # the stem, the fc
    assert convs == 19


def test_packed_layout_is_the_headers_permutation():
    """a blob whose convolution weights are their own index in the blob mod 256 (exact in bf16): the value at
    [ky][kx][g][co][j] of a convolution's packed W is the index of W[ky][kx][8 g + j][co], read with explicit loops over a
    sample of positions from the header's layout text; parts follow each other without padding"""
    blob = (np.arange(ini.BACKBONE_FLOATS, dtype=np.int64) % 256).astype(np.float32)
    packed = ini.pack_backbone_weights_bf16(torch.from_numpy(blob)).numpy()
    assert np.array_equal(ini.unpack_backbone_weights_bf16(packed).numpy(), blob.astype(np.float64))
    rng = np.random.default_rng(1)
    at = 0
    for rec in sorted(ini.backbone_launches(9, 13), key=lambda r: r.w_off):
        nw = rec.ks * rec.ks * rec.cin * rec.cout
        if rec.kind != "conv":
            size = 4 * (nw + rec.cout)
            assert np.array_equal(packed[at:at + size].view(np.float32), blob[rec.w_off:rec.w_off + nw + rec.cout])
            at += size
            continue
        w16 = ini.bf16_from_bits(packed[at:at + 2 * nw].view(np.uint16))
        for _ in range(64):
            tap, ci, co = int(rng.integers(rec.ks * rec.ks)), int(rng.integers(rec.cin)), int(rng.integers(rec.cout))
            g, j = divmod(ci, 8)
            got = w16[((tap * (rec.cin // 8) + g) * rec.cout + co) * 8 + j]
            assert got == (rec.w_off + (tap * rec.cin + ci) * rec.cout + co) % 256, (rec, tap, ci, co)
        at += 2 * nw
        assert np.array_equal(packed[at:at + 4 * rec.cout].view(np.float32), blob[rec.b_off:rec.b_off + rec.cout])
        at += 4 * rec.cout
    assert at == ini.BACKBONE_BF16_BYTES


@pytest.mark.parametrize("H,W,n", [(1, 1, 3), (17, 33, 2), (33, 47, 2)])
def test_what_the_format_costs(blobs, H, W, n):
    """backbone_bf16_model (quantised weights, every stored activation rounded) against backbone_model of the float32
    blob: the largest error over the feature scale is printed (DESIGN.md 5 quotes it: 0.3 - 0.8 %); asserted only to be finite
    and not zero"""
    blob32, packed = blobs
    img = images(n, H, W)
    want = ini.backbone_model(blob32, img)
    got = ini.backbone_bf16_model(packed, img)
    assert got.shape == want.shape == (n, 24) and got.dtype == np.float64
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"{H} x {W}: bf16 chain against the float32 blob's fp64 model: {100.0 * err:.3f} % of the feature scale")
    assert np.isfinite(got).all() and np.isfinite(err) and err > 0.0


def test_bf16_arguments():
    class Cam:
        height, width = 9, 13
    init = ini.BatchInitializer(randomised_net(), device="cpu")
    neo = ini.BatchNeoPlanner(None, init, Cam(), backbone_impl="kernel_bf16")
    assert neo.backbone_impl == "kernel_bf16"
    packed = neo.backbone_weights(precision="bf16")
    assert packed is neo.backbone_weights(precision="bf16") and packed.dtype == torch.uint8
    assert packed.numel() == ini.BACKBONE_BF16_BYTES and neo.backbone_weights().numel() == ini.BACKBONE_FLOATS
    assert torch.equal(packed, ini.pack_backbone_weights_bf16(neo.backbone_weights()))
    assert neo.backbone_weights(refresh=True, precision="bf16") is not packed
    with pytest.raises(ValueError):
        neo.backbone_weights(precision="fp16")
    with pytest.raises(ValueError):
        init.image_features(images(1, 9, 13), impl="kernel_bf16")        # a CPU initializer: there is no CPU fallback
    with pytest.raises(ValueError):
        ini.backbone_features_kernel(None, packed, images(1, 9, 13), precision="fp16")


def test_bf16_entry_points_in_the_abi():
    assert "neo_disp_backbone_bf16.hip" in build.SOURCES
    # the family's header recompiles its unit alone, and the fp32 kernels' header is not part of it
    assert [s for s in build.SOURCES if "neo_backbone_bf16.hpp" in build.headers_of(s)] == ["neo_disp_backbone_bf16.hip"]
    assert "neo_backbone.hpp" not in build.headers_of("neo_disp_backbone_bf16.hip")
    build.build()
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "neo_planner.h")).read()
    for kind, name, count in (("int", "neo_backbone_pack_bf16_dev", 5), ("size_t", "neo_backbone_bf16_workspace_bytes", 3),
                              ("int", "neo_backbone_features_bf16_dev", 10), ("int", "neo_backbone_bf16_launch_times", 11),
                              ("int", "neo_backbone_bf16_activation_dev", 13)):
        assert name in _lib.EXPORTS
        decl = re.search(r"\b" + kind + r"\s+" + name + r"\s*\(([^)]*)\)", header)
        assert decl, name
        assert len(getattr(lib, name).argtypes) == len(decl.group(1).split(",")) == count, name
    # three bf16 buffers of the pool's 64-channel output at 160 x 120: half the fp32 route's; 0 where that one returns 0
    assert lib.neo_backbone_bf16_workspace_bytes(64, 120, 160) == 3 * 64 * 30 * 40 * 64 * 2
    assert lib.neo_backbone_bf16_workspace_bytes(1, 1, 1) == 3 * 512 * 2
    for bad in ((0, 120, 160), (-1, 9, 13), (4, 0, 160), (4, 9, 0), (2 ** 20, 2 ** 6, 2 ** 5)):
        assert lib.neo_backbone_bf16_workspace_bytes(*bad) == 0 == lib.neo_backbone_workspace_bytes(*bad), bad
    # the column tile the GPU tests take from the kernels' header
    assert header_constant("neo-planner_amd/csrc/neo_backbone_bf16.hpp", "kBhTileCols") >= 32
    tool = open(os.path.join(REPO, "tools", "kernel_resource_usage.py")).read()
    assert "neo_disp_backbone_bf16.hip" in tool
