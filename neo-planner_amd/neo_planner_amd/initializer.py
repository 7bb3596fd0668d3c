"""
Initializer network of neo-planner on PyTorch-ROCm: the learned warm start
that `NeoPlanner.enhanced_traj_plan` feeds to the optimiser.

reference                                                        here
  nn_trainer/nn_trainer.py:109-155  PlannerNet                    PlannerNet (same sub-module names, so a
                                                                  reference `planner_net.pth` state_dict loads)
  nn_trainer/nn_trainer_conv.py:107-159 PlannerNet (Conv1d heads) PlannerNetConv (same sub-module names)
  nn_trainer/nn_trainer.py:52-59    process_input_np              process_input_np
  traj_planner/record_planner.py:13-58 form_nn_input              form_nn_input (own quaternion helper)
  traj_planner/nn_planner.py:20-134 NNPlanner (onnxruntime)       NNPlanner (torch forward on the GPU)
  traj_planner/neo_planner.py:10-51 NeoPlanner                    NeoPlanner(MinJerkPlanner)

The reference runs the exported ONNX graph through onnxruntime's CUDA provider; here the same network
runs as a torch module on ROCm.  The backbone's convolutions run as im2col + GEMM (`conv_impl="gemm"`: F.unfold, then
one fp32 GEMM per layer on hipBLASLt/rocBLAS, i.e. on the matrix cores) because MIOpen picks its naive direct kernel
for these fp32 NCHW shapes on gfx950 (profiles/r01_cfg3_*: 63 % of the warm start's GPU time); `conv_impl="miopen"`
keeps nn.Conv2d.  Dense layers: hipBLASLt/rocBLAS on MFMA.  The
trained weights are not part of the reference tree (.MISSING_LARGE_BLOBS): parity of the *numbers* is
unpinned, parity of the *architecture and data flow* is tested against an fp64 NumPy forward of the
same weights (tests/test_initializer.py).  torchvision is not available in this image: the ResNet-18
below is written out with torchvision's parameter names.
"""
import collections

import numpy as np
import torch
import torch.nn as nn

from .planner import MinJerkPlanner

IMG_WIDTH = 640            # nn_trainer.py:19-22
IMG_HEIGHT = 480
MOTION_INPUT_SIZE = 24
OUTPUT_SIZE = 9
IMG_FEATURE_SIZE = 24
MOTION_FEATURE_SIZE = 24


# --------------------------------------------------------------------------- quaternion (pyquaternion subset)
class Quat:
    """unit quaternion with the members the reference uses from pyquaternion: `rotate`, `inverse`,
    `rotation_matrix` (record_planner.py:21-42, nn_planner.py:128-132)"""

    def __init__(self, w=1.0, x=0.0, y=0.0, z=0.0):
        q = np.array([w, x, y, z], dtype=np.float64)
        self.q = q / np.linalg.norm(q)

    @classmethod
    def from_yaw(cls, yaw):
        return cls(np.cos(yaw / 2), 0.0, 0.0, np.sin(yaw / 2))

    @property
    def rotation_matrix(self):
        w, x, y, z = self.q
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])

    @property
    def inverse(self):
        w, x, y, z = self.q
        return Quat(w, -x, -y, -z)

    def rotate(self, v):
        return self.rotation_matrix @ np.asarray(v, dtype=np.float64)


class DroneState:
    """ros_node/traj_planner_node.py:49-55"""

    def __init__(self):
        self.global_pos = np.zeros(3)
        self.global_vel = np.zeros(3)
        self.local_vel = np.zeros(3)
        self.attitude = Quat()
        self.yaw = 0.0


# --------------------------------------------------------------------------- input glue
def process_input_np(depth_img, motion_info):
    """nn_trainer.py:52-59: flatten the image, append the motion vector, float32"""
    return np.concatenate((depth_img.reshape(-1).astype(np.float32), motion_info.astype(np.float32)))


def form_nn_input(depth_img, drone_state, des_pos_z, plan_init_state, target_state):
    """record_planner.py:13-58: depth image scaled to uint8 by its maximum; 24-d motion vector
    [local velocity (3), attitude matrix row-major (9), plan start pos/vel and target pos/vel in the
    body frame (4 x 3)]"""
    depth_norm = (depth_img / np.max(depth_img) * 255).astype(np.uint8)
    q = drone_state.attitude
    start = np.zeros((2, 3))
    start[0, :2] = plan_init_state.global_pos[:2]
    start[0, 2] = des_pos_z
    start[1, :2] = plan_init_state.global_vel[:2]
    goal = np.zeros((2, 3))
    goal[:, :2] = target_state
    goal[0, 2] = des_pos_z
    to_body = q.inverse
    motion = np.concatenate((drone_state.local_vel,
                             q.rotation_matrix.reshape(-1),
                             to_body.rotate(start[0] - drone_state.global_pos),
                             to_body.rotate(start[1] - drone_state.global_vel),
                             to_body.rotate(goal[0] - drone_state.global_pos),
                             to_body.rotate(goal[1] - drone_state.global_vel)), axis=0)
    return depth_norm, motion


def form_nn_input_batch(drone_pos, drone_vel, local_vel, yaw, des_pos_z, start, target):
    """form_nn_input's motion vector for B requests whose attitude is Quat.from_yaw(yaw): drone_pos, drone_vel,
    local_vel (B, 3), yaw (B,), start (B, 2, 2) = the plan's initial position and velocity (x, y), target (B, 2, 2) =
    the target's.  Returns motion (B, 24), R (B, 3, 3) body -> world, global_pos (B, 3) -- what
    BatchInitializer.warm_start takes."""
    pos = np.asarray(drone_pos, dtype=np.float64).reshape(-1, 3)
    vel = np.asarray(drone_vel, dtype=np.float64).reshape(-1, 3)
    lv = np.asarray(local_vel, dtype=np.float64).reshape(-1, 3)
    yaw = np.asarray(yaw, dtype=np.float64).reshape(-1)
    start = np.asarray(start, dtype=np.float64)
    target = np.asarray(target, dtype=np.float64)
    B = pos.shape[0]
    w, z = np.cos(yaw / 2), np.sin(yaw / 2)
    nrm = np.sqrt(w * w + z * z)                                        # (Quat normalises)
    w, z = w / nrm, z / nrm
    R = np.zeros((B, 3, 3))
    R[:, 0, 0] = R[:, 1, 1] = 1 - 2 * (z * z)
    R[:, 0, 1] = -2 * z * w
    R[:, 1, 0] = 2 * z * w
    R[:, 2, 2] = 1.0

    def body(p_xy, z_value, origin):
        v3 = np.concatenate([p_xy, np.full((B, 1), float(z_value))], axis=1) - origin
        return np.einsum("bji,bj->bi", R, v3)                           # R^T v: the inverse rotation

    motion = np.concatenate([lv, R.reshape(B, 9), body(start[:, 0], des_pos_z, pos), body(start[:, 1], 0.0, vel),
                             body(target[:, 0], des_pos_z, pos), body(target[:, 1], 0.0, vel)], axis=1)
    return motion, R, pos.copy()


# --------------------------------------------------------------------------- network
CONV_IMPL = "gemm"      # "gemm": im2col + one GEMM per convolution (matrix cores); "miopen": nn.Conv2d as is


def _conv2d(conv, x):
    """nn.Conv2d forward.  With CONV_IMPL == "gemm" on a GPU tensor: F.unfold (im2col) and a [Cout, Cin*kh*kw] x
    [Cin*kh*kw, L] GEMM per image -- the same sums as the direct convolution in another order (fp32 round-off apart)."""
    if CONV_IMPL != "gemm" or not x.is_cuda or conv.groups != 1:
        return conv(x)
    kh, kw = conv.kernel_size
    N, _, H, W = x.shape
    Ho = (H + 2 * conv.padding[0] - conv.dilation[0] * (kh - 1) - 1) // conv.stride[0] + 1
    Wo = (W + 2 * conv.padding[1] - conv.dilation[1] * (kw - 1) - 1) // conv.stride[1] + 1
    if kh == 1 and kw == 1 and conv.padding == (0, 0):
        cols = x[:, :, ::conv.stride[0], ::conv.stride[1]].reshape(N, x.shape[1], -1)
    else:
        cols = torch.nn.functional.unfold(x, (kh, kw), dilation=conv.dilation, padding=conv.padding, stride=conv.stride)
    y = torch.matmul(conv.weight.reshape(conv.out_channels, -1), cols)           # [N, Cout, L]
    if conv.bias is not None:
        y = y + conv.bias[None, :, None]
    return y.reshape(N, conv.out_channels, Ho, Wo)


class _BasicBlock(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample[1](_conv2d(self.downsample[0], x))
        y = self.relu(self.bn1(_conv2d(self.conv1, x)))
        y = self.bn2(_conv2d(self.conv2, y))
        return self.relu(y + idt)


class ResNet18OneChannel(nn.Module):
    """torchvision.models.resnet18 with the reference's two edits (nn_trainer.py:119-122): a 1-channel
    stem and a `feature_size`-wide fc.  Parameter names follow torchvision."""

    def __init__(self, feature_size=IMG_FEATURE_SIZE):
        super().__init__()
        self.conv1 = nn.Conv2d(1, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = nn.Sequential(_BasicBlock(64, 64, 1), _BasicBlock(64, 64, 1))
        self.layer2 = nn.Sequential(_BasicBlock(64, 128, 2), _BasicBlock(128, 128, 1))
        self.layer3 = nn.Sequential(_BasicBlock(128, 256, 2), _BasicBlock(256, 256, 1))
        self.layer4 = nn.Sequential(_BasicBlock(256, 512, 2), _BasicBlock(512, 512, 1))
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512, feature_size)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(_conv2d(self.conv1, x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(torch.flatten(self.avgpool(x), 1))


class PlannerNet(nn.Module):
    """nn_trainer.py:109-155.  `forward(input)` is the reference's signature ([N, H*W + 24] float32 ->
    [N, 9]); `image_features` / `head` split it so that a batch of trajectories sharing one depth image
    runs the convolutional backbone once."""

    def __init__(self, img_height=IMG_HEIGHT, img_width=IMG_WIDTH):
        super().__init__()
        self.img_height, self.img_width = img_height, img_width
        self.img_backbone = ResNet18OneChannel(IMG_FEATURE_SIZE)
        self.motion_backbone = nn.Sequential(
            nn.Linear(MOTION_INPUT_SIZE, 48), nn.LeakyReLU(),
            nn.Linear(48, 24), nn.LeakyReLU(),
            nn.Linear(24, 24), nn.LeakyReLU(),
            nn.Linear(24, MOTION_FEATURE_SIZE))
        self.mlp = nn.Sequential(
            nn.Linear(IMG_FEATURE_SIZE + MOTION_FEATURE_SIZE, 48), nn.LeakyReLU(),
            nn.Linear(48, 96), nn.LeakyReLU(),
            nn.Linear(96, 96), nn.LeakyReLU(),
            nn.Linear(96, OUTPUT_SIZE))

    def image_features(self, img):
        """img [N, 1, H, W] -> [N, 24]"""
        return self.img_backbone(img)

    def head(self, img_feature, motion):
        """img_feature [N or 1, 24], motion [N, 24] -> [N, 9]: 20 448 MAC per trajectory of dense work"""
        if img_feature.shape[0] != motion.shape[0]:
            img_feature = img_feature.expand(motion.shape[0], -1)
        return self.mlp(torch.cat([img_feature, self.motion_backbone(motion)], dim=1))

    def forward(self, input):
        hw = self.img_width * self.img_height
        img = input[:, :hw].reshape(-1, 1, self.img_height, self.img_width)
        return self.head(self.image_features(img), input[:, hw:])


class PlannerNetConv(PlannerNet):
    """nn_trainer_conv.py:107-159: the variant whose motion branch and fusion head are Conv1d stacks over the feature
    vector treated as a 1-channel sequence (kernel 3, padding 1, 1 -> 16 -> 32 -> 64 channels, LeakyReLU), flattened
    into one Linear each.  Same sub-module names and Sequential indices as the reference, so its state_dict loads.
    Per trajectory: motion branch 24 * (3*16 + 48*32 + 96*64) + 1536*24 MAC, head 48 * (3*16 + 48*32 + 96*64) + 3072*9."""

    def __init__(self, img_height=IMG_HEIGHT, img_width=IMG_WIDTH):
        super().__init__(img_height, img_width)

        def stack(length, out):
            return nn.Sequential(
                nn.Conv1d(1, 16, kernel_size=3, stride=1, padding=1), nn.LeakyReLU(),
                nn.Conv1d(16, 32, kernel_size=3, stride=1, padding=1), nn.LeakyReLU(),
                nn.Conv1d(32, 64, kernel_size=3, stride=1, padding=1), nn.LeakyReLU(),
                nn.Flatten(), nn.Linear(64 * length, out))
        self.motion_backbone = stack(MOTION_INPUT_SIZE, MOTION_FEATURE_SIZE)
        self.mlp = stack(IMG_FEATURE_SIZE + MOTION_FEATURE_SIZE, OUTPUT_SIZE)

    def head(self, img_feature, motion):
        if img_feature.shape[0] != motion.shape[0]:
            img_feature = img_feature.expand(motion.shape[0], -1)
        mf = self.motion_backbone(motion.unsqueeze(1))                 # (:149-152) channel dimension added
        return self.mlp(torch.cat([img_feature, mf], dim=1).unsqueeze(1))


def head_layers(net):
    """the eight Linear layers of PlannerNet.head in forward order: the motion branch, then the fusion MLP"""
    return [m for m in list(net.motion_backbone) + list(net.mlp) if isinstance(m, nn.Linear)]


def pack_head_weights(net):
    """the weight blob of neo_init_head_dev (include/neo_planner.h): the eight Linear layers of `net`.head in forward
    order, each as W row-major [out][in] followed by b[out] -- NEO_INIT_HEAD_FLOATS = 20 817 float32 values in one
    tensor on `net`'s device.  A plain PlannerNet only: PlannerNetConv's stacks stay on the torch head."""
    if type(net) is not PlannerNet:
        raise ValueError("pack_head_weights: a plain PlannerNet (got %s; other networks use the torch head)" % type(net).__name__)
    with torch.no_grad():
        blob = torch.cat([t.detach().reshape(-1).to(torch.float32) for l in head_layers(net) for t in (l.weight, l.bias)])
    return blob.contiguous()


BACKBONE_FLOATS = 11177752      # NEO_BACKBONE_FLOATS (include/neo_planner.h)
_BACKBONE_CHANNELS = (64, 128, 256, 512)


def _fold_bn(conv, bn):
    """conv + BatchNorm in eval mode as one convolution with a bias, in fp64: w' = w g / sqrt(var + eps) as
    [ky][kx][ci][co], b' = beta - mean g / sqrt(var + eps)"""
    w = conv.weight.detach().double().cpu()
    scale = bn.weight.detach().double().cpu() / torch.sqrt(bn.running_var.detach().double().cpu() + bn.eps)
    bias = bn.bias.detach().double().cpu() - bn.running_mean.detach().double().cpu() * scale
    if conv.bias is not None:
        bias = bias + conv.bias.detach().double().cpu() * scale
    return (w * scale[:, None, None, None]).permute(2, 3, 1, 0).reshape(-1), bias


def pack_backbone_weights(net, dtype=torch.float32):
    """the weight blob of neo_backbone_features_dev (include/neo_planner.h): `net`.img_backbone (a PlannerNet's or a
    PlannerNetConv's: the backbone is the same) with every BatchNorm folded into the convolution in front of it, folded in
    fp64 and cast once -- NEO_BACKBONE_FLOATS float32 values in one tensor on `net`'s device.  Forward order: the stem,
    the eight blocks (conv1, conv2, then the downsample branch where there is one), the fc; a convolution as
    W [ky][kx][ci][co], then b [co]; the fc as W [24][512], then b [24].  dtype torch.float64 returns the fold before the
    cast (what the fp32 blob is the once-rounded image of; the kernels take float32 only)."""
    bb = net.img_backbone if hasattr(net, "img_backbone") else net
    if not isinstance(bb, ResNet18OneChannel):
        raise ValueError("pack_backbone_weights: a PlannerNet, a PlannerNetConv or their ResNet18OneChannel (got %s)"
                         % type(net).__name__)
    parts = list(_fold_bn(bb.conv1, bb.bn1))
    for layer in (bb.layer1, bb.layer2, bb.layer3, bb.layer4):
        for blk in layer:
            parts += _fold_bn(blk.conv1, blk.bn1)
            parts += _fold_bn(blk.conv2, blk.bn2)
            if blk.downsample is not None:
                parts += _fold_bn(blk.downsample[0], blk.downsample[1])
    parts += [bb.fc.weight.detach().double().cpu().reshape(-1), bb.fc.bias.detach().double().cpu()]
    blob = torch.cat(parts).to(dtype).contiguous()
    if blob.numel() != BACKBONE_FLOATS:
        raise ValueError("pack_backbone_weights: %d values, not NEO_BACKBONE_FLOATS: not the reference's ResNet-18" % blob.numel())
    return blob.to(next(bb.parameters()).device)


def backbone_model(blob, images):
    """What the blob of pack_backbone_weights MEANS: the features (n, 24) float64 of images (n, H, W) (uint8 values), from
    the blob alone, in fp64 on the CPU -- convolutions with a bias, ReLU, the 3 x 3 stride-2 max pool, the residual sums,
    the mean over the pixels and the fc: the launches of backbone_launches, one after the other.  The yardstick of the
    kernels (tests/test_gpu_backbone.py)."""
    blob = torch.as_tensor(blob).detach().cpu().double().reshape(-1)
    if blob.numel() != BACKBONE_FLOATS:
        raise ValueError("backbone_model: the blob has NEO_BACKBONE_FLOATS = %d values" % BACKBONE_FLOATS)
    x = torch.as_tensor(np.asarray(images.detach().cpu() if torch.is_tensor(images) else images)).double()
    x = x.reshape(-1, 1, *x.shape[-2:])
    table = backbone_launches(*x.shape[-2:])
    # a launch's output is kept until the last launch that reads it
    last_use = {}
    for k, rec in enumerate(table):
        last_use[rec.src] = last_use[rec.resid] = k
    outs = {-1: x}
    for k, rec in enumerate(table):
        outs[k] = _launch64(blob, rec, outs[rec.src], None if rec.resid is None else outs[rec.resid])
        for j in [j for j in outs if last_use.get(j, len(table)) <= k]:
            del outs[j]
    return outs[len(table) - 1].numpy()


BackboneLaunch = collections.namedtuple(
    "BackboneLaunch", "kind ks cin cout stride relu hin win hout wout w_off b_off src resid")


def backbone_launches(H, W):
    """The NEO_BACKBONE_LAUNCHES = 21 launches of neo_backbone_features_dev for images of H x W, in launch order (the
    order of neo_backbone_launch_times and neo_backbone_activation_dev), as BackboneLaunch records:
      kind            "stem" (7 x 7 stride-2 convolution, ReLU, 3 x 3 stride-2 max pool), "conv", or "poolfc" (the mean over
                      the pixels, then the fc)
      ks cin cout stride relu    the convolution (the fc: ks 1, cin 512, cout 24)
      hin win hout wout          the input's and the output's size (stem: the image's and the pooled one's; poolfc: 1 x 1 out)
      w_off b_off     where W [ks][ks][cin][cout] (the fc: [24][512]) and b [cout] start in the blob
      src             the launch whose output is the input (-1: the images)
      resid           the launch whose output is added before the ReLU, or None
    The blob holds a block as conv1, conv2, downsample; the launches run conv1, downsample, conv2."""
    size = lambda s, stride: (s - 1) // stride + 1
    at = [0]

    def take(ks, cin, cout):
        w_off = at[0]
        at[0] += ks * ks * cin * cout + cout
        return w_off, at[0] - cout

    h, w = size(size(H, 2), 2), size(size(W, 2), 2)
    recs = [BackboneLaunch("stem", 7, 1, 64, 2, 1, H, W, h, w, *take(7, 1, 64), -1, None)]
    cin, x = 64, 0                                  # x: the launch that wrote the block's input
    for li, cout in enumerate(_BACKBONE_CHANNELS):
        for blk in range(2):
            stride = 2 if (li > 0 and blk == 0) else 1
            ho, wo = size(h, stride), size(w, stride)
            o1, o2 = take(3, cin, cout), take(3, cout, cout)
            recs.append(BackboneLaunch("conv", 3, cin, cout, stride, 1, h, w, ho, wo, *o1, x, None))
            c1, idt = len(recs) - 1, x
            if stride != 1 or cin != cout:
                recs.append(BackboneLaunch("conv", 1, cin, cout, stride, 0, h, w, ho, wo, *take(1, cin, cout), x, None))
                idt = len(recs) - 1
            recs.append(BackboneLaunch("conv", 3, cout, cout, 1, 1, ho, wo, ho, wo, *o2, c1, idt))
            x, h, w, cin = len(recs) - 1, ho, wo, cout
    recs.append(BackboneLaunch("poolfc", 1, 512, IMG_FEATURE_SIZE, 1, 0, h, w, 1, 1, *take(1, 512, IMG_FEATURE_SIZE), x, None))
    return recs


def _launch64(blob, rec, x, resid, absolute=False):
    """one launch in fp64 on torch's layout: blob a float64 tensor, x (n, cin, hin, win) (the stem: (n, 1, H, W)), resid
    None or (n, cout, hout, wout); returns (n, cout, hout, wout), the poolfc (n, 24).  absolute: on |W| and |b|"""
    F = torch.nn.functional
    w, b = blob[rec.w_off:rec.b_off], blob[rec.b_off:rec.b_off + rec.cout]
    if absolute:
        w, b = w.abs(), b.abs()
    if rec.kind == "poolfc":
        return x.mean(dim=(2, 3)) @ w.reshape(rec.cout, rec.cin).T + b
    w = w.reshape(rec.ks, rec.ks, rec.cin, rec.cout).permute(3, 2, 0, 1)
    y = F.conv2d(x, w, b, stride=rec.stride, padding=rec.ks // 2)
    if rec.kind == "stem":
        return F.max_pool2d(F.relu(y), 3, 2, 1)
    if resid is not None:
        y = y + resid
    return F.relu(y) if rec.relu else y


def backbone_launch_model(blob, rec, act_in, resid=None, absolute=False):
    """ONE launch of the chain in fp64 from given inputs, in the device's layout: rec a record of backbone_launches,
    act_in the output of launch rec.src, [n][hin][win][cin] channels-last (the stem: the images, [n][H][W]), resid the
    output of launch rec.resid or None.  Returns float64 [n][hout][wout][cout], the poolfc [n][24].  absolute=True runs
    the same launch on the absolute values of the weights, the bias and the inputs: |b| + sum |w| |x| + |resid|, the
    scale of an fp32 summation's rounding error.  (A float64 CPU tensor as the blob is used as it is: callers of many
    launches convert once.)"""
    blob = torch.as_tensor(blob).detach().cpu().double().reshape(-1)
    if blob.numel() != BACKBONE_FLOATS:
        raise ValueError("backbone_launch_model: the blob has NEO_BACKBONE_FLOATS = %d values" % BACKBONE_FLOATS)
    if (rec.resid is None) != (resid is None):
        raise ValueError("backbone_launch_model: launches with rec.resid take a residual, the others none")
    x = torch.as_tensor(np.asarray(act_in)).double()
    x = x.reshape(-1, 1, rec.hin, rec.win) if rec.kind == "stem" else x.reshape(-1, rec.hin, rec.win, rec.cin).permute(0, 3, 1, 2)
    r = None if resid is None else torch.as_tensor(np.asarray(resid)).double().reshape(-1, rec.hout, rec.wout, rec.cout).permute(0, 3, 1, 2)
    if absolute:
        x, r = x.abs(), None if r is None else r.abs()
    y = _launch64(blob, rec, x.contiguous(), None if r is None else r.contiguous(), absolute)
    return (y if rec.kind == "poolfc" else y.permute(0, 2, 3, 1)).contiguous().numpy()


BACKBONE_BF16_BYTES = 22396000      # NEO_BACKBONE_BF16_BYTES (include/neo_planner.h)


def bf16_bits(a):
    """float32 values -> their bf16 bit patterns (uint16), round to nearest even, in integer arithmetic: the upper half of
    the word after adding 0x7FFF plus the lowest kept bit; a NaN stays a NaN (quiet bit set, payload's upper bits kept)"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    rounded = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (u >> 16) | 0x40, rounded).astype(np.uint16)


def bf16_from_bits(b):
    """bf16 bit patterns (uint16) -> the float32 values they are"""
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(a):
    """float32 -> float32 holding bf16 values: round to nearest even, as the device's conversion at a store"""
    return bf16_from_bits(bf16_bits(a))


def _bf16_parts():
    """the parts of the packed blob in order (csrc/neo_backbone_bf16.hpp, PACKED BLOB), as (kind, f32 offset, floats,
    byte offset, (taps, cin, cout) or None): kind "f32" is copied verbatim, "w" is a convolution's W"""
    parts, at32, at = [], 0, 0

    def add(kind, floats, shape=None):
        nonlocal at32, at
        parts.append((kind, at32, floats, at, shape))
        at32 += floats
        at += floats * (2 if kind == "w" else 4)

    add("f32", 49 * 64 + 64)
    cin = 64
    for cout in _BACKBONE_CHANNELS:
        for blk in range(2):
            convs = [(9, cin, cout), (9, cout, cout)] + ([(1, cin, cout)] if cin != cout else [])
            for taps, ci, co in convs:
                add("w", taps * ci * co, (taps, ci, co))
                add("f32", co)
            cin = cout
    add("f32", 24 * 512 + 24)
    assert at32 == BACKBONE_FLOATS and at == BACKBONE_BF16_BYTES
    return parts


def pack_backbone_weights_bf16(blob32):
    """the packed blob of neo_backbone_features_bf16_dev from the float32 blob of pack_backbone_weights: a uint8 tensor
    of NEO_BACKBONE_BF16_BYTES on the blob's device.  The NumPy twin of neo_backbone_pack_bf16_dev, written from the
    layout text of csrc/neo_backbone_bf16.hpp: the stem, the biases and the fc verbatim; a convolution's W
    [ky][kx][ci][co] as bf16 [ky][kx][ci / 8][co][8], ci = 8 g + j, rounded to nearest even."""
    t = torch.as_tensor(blob32)
    src = np.ascontiguousarray(t.detach().cpu().numpy()).reshape(-1)
    if src.dtype != np.float32 or src.size != BACKBONE_FLOATS:
        raise ValueError("pack_backbone_weights_bf16: the float32 blob of NEO_BACKBONE_FLOATS = %d values" % BACKBONE_FLOATS)
    out = np.empty(BACKBONE_BF16_BYTES, dtype=np.uint8)
    for kind, o32, floats, at, shape in _bf16_parts():
        part = src[o32:o32 + floats]
        if kind == "f32":
            out[at:at + 4 * floats] = part.view(np.uint8)
        else:
            taps, cin, cout = shape
            w = bf16_bits(part).reshape(taps, cin // 8, 8, cout).transpose(0, 1, 3, 2)
            out[at:at + 2 * floats] = np.ascontiguousarray(w).reshape(-1).view(np.uint8)
    return torch.from_numpy(out).to(t.device if torch.is_tensor(blob32) else "cpu")


def unpack_backbone_weights_bf16(packed):
    """the float64 blob of the quantised network, in the float32 blob's order (NEO_BACKBONE_FLOATS values): what the packed
    blob means.  backbone_launch_model, backbone_launches and backbone_model work on it unchanged."""
    raw = np.ascontiguousarray(torch.as_tensor(packed).detach().cpu().numpy()).reshape(-1)
    if raw.dtype != np.uint8 or raw.size != BACKBONE_BF16_BYTES:
        raise ValueError("unpack_backbone_weights_bf16: the uint8 blob of NEO_BACKBONE_BF16_BYTES = %d bytes" % BACKBONE_BF16_BYTES)
    out = np.empty(BACKBONE_FLOATS, dtype=np.float64)
    for kind, o32, floats, at, shape in _bf16_parts():
        if kind == "f32":
            out[o32:o32 + floats] = raw[at:at + 4 * floats].view(np.float32)
        else:
            taps, cin, cout = shape
            w = bf16_from_bits(raw[at:at + 2 * floats].view(np.uint16)).reshape(taps, cin // 8, cout, 8).transpose(0, 1, 3, 2)
            out[o32:o32 + floats] = w.reshape(-1)
    return torch.from_numpy(out)


def backbone_bf16_model(packed, images):
    """What the bf16 route COSTS, without a GPU: the features (n, 24) float64 of images (n, H, W) from the packed blob's
    quantised weights, every launch in fp64 and every STORED activation (the stem's and the convolutions' outputs) rounded
    with bf16_round behind it; the pool and fc's features stay as they are."""
    blob = unpack_backbone_weights_bf16(packed)
    x = torch.as_tensor(np.asarray(images.detach().cpu() if torch.is_tensor(images) else images)).double()
    x = x.reshape(-1, 1, *x.shape[-2:])
    table = backbone_launches(*x.shape[-2:])
    outs = {-1: x}
    for k, rec in enumerate(table):
        y = _launch64(blob, rec, outs[rec.src], None if rec.resid is None else outs[rec.resid])
        if rec.kind != "poolfc":
            y = torch.from_numpy(bf16_round(y.numpy().astype(np.float32)).astype(np.float64))
        outs[k] = y
    return outs[len(table) - 1].numpy()


def backbone_features_kernel(ctx, blob, images, out=None, chunk=512, workspace=None, precision="f32"):
    """neo_backbone_features_dev on `ctx`'s stream, `chunk` images a call: blob (pack_backbone_weights) and images (n, H, W)
    uint8 are contiguous device tensors that are READY (torch.cuda.synchronize after torch wrote them).  Returns
    (features (n, 24) float32, the workspace tensor used -- hand it back in to reuse it).  Asynchronous: ctx.synchronize()
    before torch reads the features.  precision "bf16": neo_backbone_features_bf16_dev, and the blob is the packed one
    (pack_backbone_weights_bf16 or neo_backbone_pack_bf16_dev: a uint8 tensor)."""
    from . import _lib
    if precision not in ("f32", "bf16"):
        raise ValueError("backbone_features_kernel: precision must be 'f32' or 'bf16'")
    n, H, W = (int(s) for s in images.shape)
    if precision == "bf16":
        if images.dtype != torch.uint8 or not images.is_contiguous() or blob.dtype != torch.uint8 or not blob.is_contiguous():
            raise ValueError("backbone_features_kernel: contiguous tensors, images (n, H, W) uint8 and the packed uint8 blob")
        entry, bytes_of = "neo_backbone_features_bf16_dev", ctx.backbone_bf16_workspace_bytes
    else:
        if images.dtype != torch.uint8 or not images.is_contiguous() or blob.dtype != torch.float32 or not blob.is_contiguous():
            raise ValueError("backbone_features_kernel: contiguous tensors, images (n, H, W) uint8 and a float32 blob")
        entry, bytes_of = "neo_backbone_features_dev", ctx.backbone_workspace_bytes
    chunk = max(1, min(int(chunk), max(n, 1)))
    need = bytes_of(chunk, H, W)
    fresh = out is None
    if out is None:
        out = torch.empty((n, IMG_FEATURE_SIZE), dtype=torch.float32, device=images.device)
    if workspace is None or workspace.numel() < need or workspace.device != images.device:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=images.device)
        fresh = True
    if fresh:
        torch.cuda.synchronize(images.device)      # (the allocations are torch's: ready before the context's stream starts)
    p = _lib.dev_ptr
    for b0 in range(0, n, chunk):
        k = min(chunk, n - b0)
        ctx.call(entry, p(blob), int(blob.numel()), p(images[b0:b0 + k]), k, H, W, p(workspace),
                 int(workspace.numel()), p(out[b0:b0 + k]))
    return out, workspace


def raycast_depth(pillars, canopy=(), eye=(1.5, 0.0, 2.0), yaw=0.0, hfov_deg=87.0, max_range=20.0,
                  height=IMG_HEIGHT, width=IMG_WIDTH):
    """Synthetic depth image of a forest scene ("ray-cast of the pillars, 480 x 640"): a pinhole camera
    at `eye` looking along +x rotated by `yaw`, horizontal field of view `hfov_deg` (a RealSense-like 87 deg), depth =
    distance along the optical axis to the nearest box or the ground plane z = 0, capped at `max_range`; returned as
    uint8 scaled by its maximum, exactly what form_nn_input hands to the network (record_planner.py:16-18).
    pillars: (cx, cy, sx, sy, sz) standing on the ground; canopy: (cx, cy, cz, sx, sy, sz)."""
    boxes = [((cx - sx / 2, cy - sy / 2, 0.0), (cx + sx / 2, cy + sy / 2, sz)) for (cx, cy, sx, sy, sz) in pillars]
    boxes += [((cx - sx / 2, cy - sy / 2, cz - sz / 2), (cx + sx / 2, cy + sy / 2, cz + sz / 2))
              for (cx, cy, cz, sx, sy, sz) in canopy]
    f = (width / 2) / np.tan(np.radians(hfov_deg) / 2)
    u = (np.arange(width) - (width - 1) / 2) / f
    v = (np.arange(height) - (height - 1) / 2) / f
    # camera frame: x forward, y left, z up
    d = np.stack(np.broadcast_arrays(np.ones((height, width)), -u[None, :], -v[:, None]), axis=-1)
    c, s_ = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, -s_, 0.0], [s_, c, 0.0], [0.0, 0.0, 1.0]])
    dirs = d @ R.T                                                      # world directions, forward component = 1
    eye = np.asarray(eye, dtype=np.float64)
    depth = np.full((height, width), max_range)
    with np.errstate(divide="ignore", invalid="ignore"):
        tg = np.where(dirs[..., 2] < 0, -eye[2] / dirs[..., 2], np.inf)          # ground plane
        depth = np.minimum(depth, tg)
        inv = 1.0 / dirs
        for lo, hi in boxes:
            t0 = (np.asarray(lo) - eye) * inv
            t1 = (np.asarray(hi) - eye) * inv
            tn = np.minimum(t0, t1).max(axis=-1)
            tf = np.maximum(t0, t1).min(axis=-1)
            hit = (tf >= np.maximum(tn, 0.0))
            depth = np.where(hit, np.minimum(depth, np.maximum(tn, 0.0)), depth)
    depth = np.clip(depth, 0.0, max_range)
    return (depth / max(depth.max(), 1e-9) * 255).astype(np.uint8)


def split_output(out, M=3, nn_output_D=3):
    """nn_planner.py:104-105: 9 outputs -> (M-1) body-frame 3-D waypoints (column major) and M durations"""
    out = np.asarray(out)
    wpts_local = out[:nn_output_D * (M - 1)].reshape(M - 1, nn_output_D).T
    return wpts_local, out[nn_output_D * (M - 1):]


class NNPlanner:
    """nn_planner.py:20-134 with a torch module in place of the onnxruntime session"""

    def __init__(self, des_pos_z=2.0, net=None, device=None, state_dict_path=None):
        self.device = torch.device(device) if device is not None else torch.device(
            "cuda" if torch.cuda.is_available() else "cpu")
        self.net = net if net is not None else PlannerNet()
        if state_dict_path is not None:
            self.net.load_state_dict(torch.load(state_dict_path, map_location="cpu"))
        self.net = self.net.to(self.device).eval()
        self.M, self.s, self.D, self.nn_output_D = 3, 3, 2, 3          # nn_planner.py:57-66
        self.head_state = np.zeros((self.s, self.D))
        self.tail_state = np.zeros((self.s, self.D))
        self.des_pos_z = des_pos_z

    def nn_traj_plan(self, depth_img, drone_state, plan_init_state, target_state):
        depth_norm, motion = form_nn_input(depth_img, drone_state, self.des_pos_z, plan_init_state, target_state)
        self.drone_state = drone_state
        self.head_state[0, :self.D] = plan_init_state.global_pos[:2]
        self.head_state[1, :self.D] = plan_init_state.global_vel[:2]
        self.tail_state[0, :self.D] = target_state[0, :2]
        self.tail_state[1, :self.D] = target_state[1, :2]
        self.predict(depth_norm, motion)

    def predict(self, depth_image_norm, motion_info):
        """nn_planner.py:87-108 (`onnx_predict`)"""
        inp = torch.from_numpy(np.array([process_input_np(depth_image_norm, motion_info)])).to(self.device)
        with torch.no_grad():
            out = self.net(inp)[0].float().cpu().numpy()
        wpts_local, self.ts = split_output(out, self.M, self.nn_output_D)
        self.int_wpts = self.get_wpts_world(wpts_local)[:self.D, :]

    onnx_predict = predict

    def get_wpts_world(self, int_wpts):
        """nn_planner.py:123-134: body frame -> world frame"""
        out = np.zeros((self.nn_output_D, self.M - 1))
        for i in range(self.M - 1):
            out[:, i] = self.drone_state.attitude.rotate(int_wpts[:, i]) + self.drone_state.global_pos
        return out


class NeoPlanner(MinJerkPlanner):
    """neo_planner.py:10-51: network output as the warm start of the optimiser"""

    def __init__(self, planner_config, nn_planner=None, **kw):
        super().__init__(planner_config, **kw)
        self.nn_planner = nn_planner if nn_planner is not None else NNPlanner(getattr(planner_config, "des_pos_z", 2.0))

    def enhanced_traj_plan(self, map, depth_img, drone_state, plan_init_state, target_state):
        self.nn_planner.nn_traj_plan(depth_img, drone_state, plan_init_state, target_state)
        start_2d = np.array([plan_init_state.global_pos[:2], plan_init_state.global_vel[:2]])
        self.warm_start_plan(map, start_2d, target_state, self.nn_planner.int_wpts, self.nn_planner.ts)


class BatchInitializer:
    """cfg3: warm starts for B trajectories that share one depth image.  The backbone runs once per
    scene; the dense layers run as [B, 48] x ... GEMMs."""

    def __init__(self, net=None, device=None, T_min=0.5, T_max=5.0, variant="mlp"):
        """variant: "mlp" (nn_trainer.py) or "conv" (nn_trainer_conv.py) when no `net` is given"""
        self.device = torch.device(device) if device is not None else torch.device(
            "cuda" if torch.cuda.is_available() else "cpu")
        if net is None:
            net = PlannerNet() if variant == "mlp" else PlannerNetConv()
        self.net = net.to(self.device).eval()
        self.T_min, self.T_max = T_min, T_max
        self._backbone_blob = self._workspace = None      # the kernel backbone's packed weights and its activation buffers
        self._backbone_bf16 = None                        # ... and the bf16 route's packed blob

    @torch.no_grad()
    def scene_feature(self, depth_norm):
        img = torch.as_tensor(np.asarray(depth_norm), dtype=torch.float32, device=self.device)
        return self.net.image_features(img.reshape(1, 1, *img.shape[-2:]))

    @torch.no_grad()
    def image_features(self, depth_u8, chunk=None, impl="torch", ctx=None):
        """features (B, 24) of B images (B, H, W), a device tensor or an array (DepthCamera's depth_u8): one feature per
        request for `warm_start`.  The backbone runs `chunk` images at a time (None: 64 on the torch module, 512 on the
        kernels, which fill the machine only across many images).  impl "torch" (the default): the torch
        module; "kernel": neo_backbone_features_dev (csrc/neo_backbone.hpp) on `ctx`'s stream (None: the default
        context) from uint8 images, float32 features that are complete when it returns; "kernel_bf16": the same on
        neo_backbone_features_bf16_dev (csrc/neo_backbone_bf16.hpp: bf16 weights and activations)."""
        if impl not in ("torch", "kernel", "kernel_bf16"):
            raise ValueError("BatchInitializer.image_features: impl must be 'torch', 'kernel' or 'kernel_bf16'")
        img = torch.as_tensor(depth_u8) if not torch.is_tensor(depth_u8) else depth_u8
        chunk = (64 if impl == "torch" else 512) if chunk is None else chunk
        if impl != "torch":
            from . import _lib
            if self.device.type != "cuda":
                raise ValueError("BatchInitializer.image_features: impl 'kernel' runs on the GPU (there is no CPU fallback)")
            if img.dtype != torch.uint8:
                raise ValueError("BatchInitializer.image_features: impl 'kernel' takes uint8 images")
            ctx = ctx if ctx is not None else _lib.default_context(self.device.index or 0)
            img = img.reshape(-1, *img.shape[-2:]).to(self.device).contiguous()
            torch.cuda.synchronize(self.device)
            bf16 = impl == "kernel_bf16"
            feat, self._workspace = backbone_features_kernel(ctx, self.backbone_weights(precision="bf16" if bf16 else "f32"),
                                                             img, chunk=chunk, workspace=self._workspace,
                                                             precision="bf16" if bf16 else "f32")
            ctx.synchronize()
            return feat
        img = img.reshape(-1, 1, *img.shape[-2:])
        out = [self.net.image_features(img[b0:b0 + chunk].to(self.device, dtype=torch.float32))
               for b0 in range(0, img.shape[0], max(1, int(chunk)))]
        return torch.cat(out, dim=0)

    def backbone_weights(self, refresh=False, precision="f32"):
        """the network's blob for neo_backbone_features_dev (pack_backbone_weights), packed at first use; refresh=True
        packs it again after the network's parameters changed.  precision "bf16": the packed blob of
        neo_backbone_features_bf16_dev (pack_backbone_weights_bf16 of the same float32 blob), cached likewise"""
        if precision not in ("f32", "bf16"):
            raise ValueError("BatchInitializer.backbone_weights: precision must be 'f32' or 'bf16'")
        if self._backbone_blob is None or refresh:
            self._backbone_blob = pack_backbone_weights(self.net)
            self._backbone_bf16 = None
            if self._backbone_blob.is_cuda:
                torch.cuda.synchronize(self._backbone_blob.device)
        if precision == "f32":
            return self._backbone_blob
        if self._backbone_bf16 is None:
            self._backbone_bf16 = pack_backbone_weights_bf16(self._backbone_blob)
            if self._backbone_bf16.is_cuda:
                torch.cuda.synchronize(self._backbone_bf16.device)
        return self._backbone_bf16

    @torch.no_grad()
    def warm_start(self, scene_feature, motion, attitude_R, global_pos, clamp_ts=True):
        """motion [B,24], attitude_R [B,3,3] (body->world), global_pos [B,3]  ->
        int_wpts [B,2,2] (world, z dropped), ts [B,3].  An untrained or extrapolating network can
        emit durations outside (T_min, T_max), where the reference's map_T2tau fails; `clamp_ts`
        keeps them inside."""
        motion = torch.as_tensor(motion, dtype=torch.float32, device=self.device)
        out = self.net.head(scene_feature, motion).double()
        R = torch.as_tensor(attitude_R, dtype=torch.float64, device=self.device)
        p = torch.as_tensor(global_pos, dtype=torch.float64, device=self.device)
        local = out[:, :6].reshape(-1, 2, 3)                       # [B, waypoint, xyz]
        world = torch.einsum("bij,bwj->bwi", R, local) + p[:, None, :]
        ts = out[:, 6:]
        if clamp_ts:
            eps = 1e-3 * (self.T_max - self.T_min)
            ts = ts.clamp(self.T_min + eps, self.T_max - eps)
        return world[:, :, :2].transpose(1, 2).contiguous(), ts.contiguous()


class BatchNeoPlanner:
    """NeoPlanner.enhanced_traj_plan (neo_planner.py:10-51) for B requests: every request's own depth image from the
    batched camera (depth.DepthCamera), the motion vectors, the initializer network, and the warm starts into
    BatchPlanner.plan.  batch_planner: a BatchPlanner; initializer: a BatchInitializer; camera: a DepthCamera of the
    network's image size.

    `warm_start` / `plan` take host arrays.  `warm_start_dev` / `plan_dev` work on RESIDENT torch tensors: the motion
    vector, the network's dense layers and the first guess are the neo_init_* kernels on the context's stream
    (csrc/neo_init.hpp), and the guess goes to BatchPlanner.plan_dev as `x0` without passing through the host."""

    def __init__(self, batch_planner, initializer, camera, des_pos_z=2.0, backbone_impl="torch"):
        """backbone_impl: how `features_dev` runs the image backbone -- "torch" (the default: the torch module, im2col and
        a GEMM per convolution on torch's stream) or "kernel" (neo_backbone_features_dev on the camera's context,
        `backbone_chunk` images a call) or "kernel_bf16" (the same on neo_backbone_features_bf16_dev: bf16 weights and
        activations on the bf16 matrix cores, fp32 features that differ from "kernel"'s by the format's rounding)"""
        if backbone_impl not in ("torch", "kernel", "kernel_bf16"):
            raise ValueError("BatchNeoPlanner: backbone_impl must be 'torch', 'kernel' or 'kernel_bf16'")
        net = initializer.net
        if (camera.height, camera.width) != (net.img_height, net.img_width):
            raise ValueError("BatchNeoPlanner: the camera renders %d x %d, the network takes %d x %d"
                             % (camera.height, camera.width, net.img_height, net.img_width))
        self.bp, self.init, self.camera, self.des_pos_z = batch_planner, initializer, camera, float(des_pos_z)
        self.chunk = 64          # images per render launch and backbone pass
        self.motion = self.out = self.x0 = None      # what the last warm_start_dev wrote: (B, 24) and (B, 9) float32, (B, 7) float64
        self._weights = self._own_x0 = None
        self.backbone_impl = backbone_impl
        # images per neo_backbone_features_dev call.  Measured on the MI355X (profiles/backbone.json, kernel_ms_by_chunk),
        # 512 images of 160 x 120: 41.3 ms in chunks of 32, 22.6 of 64, 13.8 of 128, 10.4 of 256, 9.07 in one call -- the
        # deeper layers fill the machine only across many images.  The workspace grows with it: 0.92 MB an image at
        # 160 x 120 (472 MB for 512), 14.7 MB an image at 640 x 480; a caller short of memory lowers it.
        self.backbone_chunk = 512
        self._workspace = None

    def warm_start(self, scenes, drone_pos, drone_vel, local_vel, yaw, head, tail, scene_index=None):
        """scenes: the camera's scenes (DepthCamera.pack_scenes), scene_index (B,) the scene each request sees (None:
        scene 0); the camera sits at drone_pos (B, 3) looking along yaw (B,); head, tail (B, >= 2, 2): the plan's initial
        and target position and velocity.  Returns int_wpts (B, 2, 2) and ts (B, 3) as float64 arrays and the images
        depth_u8 (B, H, W) (a device tensor when the initializer runs on the GPU)."""
        head = np.asarray(head, dtype=np.float64)
        tail = np.asarray(tail, dtype=np.float64)
        motion, R, pos = form_nn_input_batch(drone_pos, drone_vel, local_vel, yaw, self.des_pos_z, head[:, :2], tail[:, :2])
        cam = self.camera
        if self.init.device.type == "cuda":
            dev = self.init.device
            boxes, begin = cam.pack_scenes(scenes)
            if boxes.shape[0] == 0:
                boxes = np.zeros((1, 6))
            sidx = None if scene_index is None else torch.as_tensor(np.ascontiguousarray(scene_index, dtype=np.int32), device=dev)
            depth_u8 = cam.render_dev(torch.as_tensor(boxes, device=dev), torch.as_tensor(begin, device=dev),
                                      torch.as_tensor(cam.poses(pos, yaw), device=dev), sidx, chunk=self.chunk,
                                      want_m=False)["depth_u8"]
        else:
            depth_u8 = cam.render(scenes, pos, yaw, scene_index)["depth_u8"]
        feat = self.init.image_features(depth_u8, chunk=self.chunk)
        wp, ts = self.init.warm_start(feat, motion, R, pos)
        return wp.cpu().numpy(), ts.cpu().numpy(), depth_u8

    def plan(self, map, scenes, drone_pos, drone_vel, local_vel, yaw, head, tail, scene_index=None, **plan_kw):
        """render -> motion -> network -> BatchPlanner.plan(map, head, tail, int_wpts=, ts=, **plan_kw).  Returns plan's
        dict plus the network's warm start `int_wpts0`, `ts0` and the images `depth_u8`."""
        wp, ts, depth_u8 = self.warm_start(scenes, drone_pos, drone_vel, local_vel, yaw, head, tail, scene_index)
        out = self.bp.plan(map, head, tail, int_wpts=wp, ts=ts, **plan_kw)
        out["int_wpts0"], out["ts0"], out["depth_u8"] = wp, ts, depth_u8
        return out

    # ------------------------------------------------------------ on resident arrays
    @property
    def kernel_head(self):
        """the network's dense layers can run as neo_init_head_dev: a plain PlannerNet"""
        return type(self.init.net) is PlannerNet

    def head_weights(self, refresh=False):
        """the network's blob for neo_init_head_dev (pack_head_weights), packed at first use; refresh=True packs it again
        after the network's parameters changed"""
        if self._weights is None or refresh:
            self._weights = pack_head_weights(self.init.net)
            torch.cuda.synchronize(self._weights.device)
        return self._weights

    def backbone_weights(self, refresh=False, precision="f32"):
        """the network's blob for neo_backbone_features_dev (pack_backbone_weights), packed at first use; refresh=True
        packs it again after the network's parameters changed; precision "bf16": the packed blob of the bf16 route"""
        return self.init.backbone_weights(refresh, precision)

    @torch.no_grad()
    def features_dev(self, boxes, box_begin, pose, scene_index=None):
        """the image features (n, 24) float32 of what the camera sees from pose (n, 5): DepthCamera.render_dev's uint8
        images through the backbone, `chunk` images at a time (device tensors in and out; torch's stream has finished
        when it returns).  With backbone_impl "kernel" the render launches and the backbone's are queued on the camera's
        context one after the other, `backbone_chunk` images a call out of a workspace kept here, and the context's
        stream has finished when it returns: nothing is handed over to torch's stream in between."""
        if self.backbone_impl != "torch":
            precision = "bf16" if self.backbone_impl == "kernel_bf16" else "f32"
            weights = self.backbone_weights(precision=precision)
            n, dev, ctx = int(pose.shape[0]), pose.device, self.camera.ctx
            # (everything torch allocates comes first: render_dev waits for torch once, then both stages only queue)
            feat = torch.empty((n, IMG_FEATURE_SIZE), dtype=torch.float32, device=dev)
            bytes_of = ctx.backbone_bf16_workspace_bytes if precision == "bf16" else ctx.backbone_workspace_bytes
            need = bytes_of(max(1, min(self.backbone_chunk, n)), self.camera.height, self.camera.width)
            if self._workspace is None or self._workspace.numel() < need or self._workspace.device != dev:
                self._workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            img = self.camera.render_dev(boxes, box_begin, pose, scene_index, chunk=self.chunk, want_m=False, sync=False)["depth_u8"]
            backbone_features_kernel(ctx, weights, img, out=feat, chunk=self.backbone_chunk, workspace=self._workspace,
                                     precision=precision)
            ctx.synchronize()
            return feat
        img = self.camera.render_dev(boxes, box_begin, pose, scene_index, chunk=self.chunk, want_m=False)["depth_u8"]
        feat = self.init.image_features(img, chunk=self.chunk).to(torch.float32).contiguous()
        torch.cuda.synchronize(feat.device)
        return feat

    @torch.no_grad()
    def warm_start_dev(self, pose, cur_vel, head, tail, feature, subset=None, x0=None, head_impl=None):
        """The network's first guess for the requests `subset` (an int32 device tensor; None: all B) on resident tensors
        indexed by request: pose (B, 5) float64 (eye x, y, z, cos, sin: neo_fleet_pose_dev / DepthCamera.poses), cur_vel
        (B, 2), head and tail (B, 3, 2) float64, feature (B, 24) or (1, 24) float32 (one shared image).  Three launches on
        the context's stream -- neo_init_motion_dev, neo_init_head_dev, neo_init_guess_dev -- into `self.motion` (B, 24)
        and `self.out` (B, 9) float32 and `x0` (B, 7) float64 (the caller's array, or one kept here), which is returned
        and stays readable as `self.x0`; rows of requests outside the subset stay as they are.  head_impl "kernel" (the
        default for a plain PlannerNet) or "torch" (every other network's default): net.head on torch's stream between
        the motion and the guess kernels, with the waits that takes.  The caller's tensors must be ready (as for
        plan_dev: torch.cuda.synchronize after torch wrote them); the launches are asynchronous -- ctx.synchronize()
        before torch reads the results, or plan_dev, which runs on the same stream."""
        if head_impl is None:
            head_impl = "kernel" if self.kernel_head else "torch"
        if head_impl not in ("kernel", "torch"):
            raise ValueError("BatchNeoPlanner.warm_start_dev: head_impl must be 'kernel' or 'torch'")
        if head_impl == "kernel" and not self.kernel_head:
            raise ValueError("BatchNeoPlanner.warm_start_dev: head_impl 'kernel' needs a plain PlannerNet")
        B, dev = int(pose.shape[0]), pose.device
        if tuple(pose.shape) != (B, 5) or tuple(cur_vel.shape) != (B, 2) or tuple(head.shape) != (B, 3, 2) or \
                tuple(tail.shape) != (B, 3, 2) or feature.ndim != 2 or feature.shape[1] != IMG_FEATURE_SIZE or \
                feature.shape[0] not in (1, B):
            raise ValueError("BatchNeoPlanner.warm_start_dev: pose (B, 5), cur_vel (B, 2), head and tail (B, 3, 2), "
                             "feature (B or 1, 24)")
        if any(t.dtype != torch.float64 or not t.is_contiguous() for t in (pose, cur_vel, head, tail)) or \
                feature.dtype != torch.float32 or not feature.is_contiguous():
            raise ValueError("BatchNeoPlanner.warm_start_dev: contiguous tensors, float64 but for the float32 feature")
        if x0 is not None and (tuple(x0.shape) != (B, 7) or x0.dtype != torch.float64 or not x0.is_contiguous()):
            raise ValueError("BatchNeoPlanner.warm_start_dev: x0 (B, 7) float64, contiguous")
        from . import _lib
        fresh = False
        if self.motion is None or self.motion.shape[0] != B or self.motion.device != dev:
            self.motion = torch.zeros((B, MOTION_INPUT_SIZE), dtype=torch.float32, device=dev)
            self.out = torch.zeros((B, OUTPUT_SIZE), dtype=torch.float32, device=dev)
            fresh = True
        if x0 is None:
            if self._own_x0 is None or self._own_x0.shape[0] != B or self._own_x0.device != dev:
                self._own_x0 = torch.zeros((B, 7), dtype=torch.float64, device=dev)
                fresh = True
            x0 = self._own_x0
        self.x0 = x0
        weights = self.head_weights() if head_impl == "kernel" else None
        if fresh:
            torch.cuda.synchronize(dev)      # (the context has its own stream: the buffers are ready before it starts)
        self.bp._sync()                      # the context's T_min / T_max are the planner's
        c, p = self.bp.ctx, _lib.dev_ptr
        sub, n_sub = p(subset), (0 if subset is None else int(subset.numel()))
        c.call("neo_init_motion_dev", B, sub, n_sub, p(pose), p(cur_vel), p(head), p(tail), p(self.motion))
        if head_impl == "kernel":
            c.call("neo_init_head_dev", B, sub, n_sub, p(weights), int(weights.numel()), p(feature),
                   int(feature.shape[0]), p(self.motion), p(self.out))
        else:
            c.synchronize()
            self.out.copy_(self.init.net.head(feature, self.motion).to(torch.float32))
            torch.cuda.synchronize(dev)
        c.call("neo_init_guess_dev", B, sub, n_sub, p(self.out), p(pose), p(x0))
        return x0

    def plan_dev(self, map, pose, cur_vel, head, tail, feature, subset=None, head_impl=None, **plan_dev_kw):
        """warm_start_dev, then BatchPlanner.plan_dev(map, head, tail, x0=the guess, subset=subset, **plan_dev_kw): attempt 0
        starts from the network's guess, the retries from the straight line plus noise as plan_dev draws them (the
        reference's warm_start_plan after a failed first attempt).  Returns plan_dev's bufs; the guess stays in `self.x0`."""
        x0 = self.warm_start_dev(pose, cur_vel, head, tail, feature, subset=subset, head_impl=head_impl)
        return self.bp.plan_dev(map, head, tail, x0=x0, subset=subset, **plan_dev_kw)
