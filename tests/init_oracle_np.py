"""NumPy restatement of the warm-start kernels (csrc/neo_init.hpp; include/neo_planner.h, neo_init_*): the motion vector
as fp32, PlannerNet.head in sequential fp32, and the network's output as the optimiser's first guess.  The kernels are
tested against this bit for bit but for the guess's tau, where the device's fp64 log stands against NumPy's
(tests/test_gpu_init.py); tests/test_init_cpu.py holds the models against the network and the host route."""
import numpy as np

import record_oracle_np as ron

# PlannerNet.head's Linear layers in forward order, (in, out, LeakyReLU after it): the motion branch, then the fusion MLP
LAYERS = [(24, 48, True), (48, 24, True), (24, 24, True), (24, 24, False),
          (48, 48, True), (48, 96, True), (96, 96, True), (96, 9, False)]
HEAD_FLOATS = sum(i * o + o for i, o, _ in LAYERS)            # 20 817


def launched(B, subset):
    """the requests a launch works on: in range, in the order of their positions"""
    return [int(b) for b in (range(B) if subset is None else subset) if 0 <= int(b) < B]


def motion64(pose, cur_vel, head, tail):
    """record_oracle_np's motion vector for every request: (B, 24) float64"""
    return np.stack([ron.motion_vector(pose[b], cur_vel[b], head[b], tail[b]) for b in range(pose.shape[0])])


def motion(pose, cur_vel, head, tail, subset=None, out=None):
    """neo_init_motion_dev: (B, 24) float32; rows of requests outside the launch stay as `out` has them (zeros without)"""
    B = pose.shape[0]
    res = np.zeros((B, 24), np.float32) if out is None else np.array(out, dtype=np.float32)
    for b in launched(B, subset):
        res[b] = ron.motion_vector(pose[b], cur_vel[b], head[b], tail[b]).astype(np.float32)
    return res


def unpack(weights):
    """the blob -> [(W (out, in), b (out,), leaky)] float32"""
    w = np.asarray(weights, dtype=np.float32).reshape(-1)
    assert w.shape[0] == HEAD_FLOATS
    out, at = [], 0
    for i, o, leaky in LAYERS:
        out.append((w[at:at + o * i].reshape(o, i), w[at + o * i:at + o * i + o], leaky))
        at += o * i + o
    return out


def linear(W, b, a, leaky):
    """a (N, in) float32 -> (N, out): acc = b[j], then k ascending p = W[j][k] a[k], acc = acc + p, each rounded to fp32"""
    acc = np.broadcast_to(b.astype(np.float32), (a.shape[0], W.shape[0])).copy()
    with np.errstate(all="ignore"):
        for k in range(W.shape[1]):
            p = (W[None, :, k] * a[:, k, None]).astype(np.float32)
            acc = (acc + p).astype(np.float32)
        if leaky:
            acc = np.where(acc > 0, acc, (np.float32(0.01) * acc).astype(np.float32))
    return acc.astype(np.float32)


def head_rows(weights, feature, motion_rows):
    """PlannerNet.head on rows: feature (N or 1, 24), motion_rows (N, 24) float32 -> (N, 9) float32"""
    layers = unpack(weights)
    a = np.asarray(motion_rows, dtype=np.float32)
    for W, b, leaky in layers[:4]:
        a = linear(W, b, a, leaky)
    f = np.broadcast_to(np.asarray(feature, dtype=np.float32), (a.shape[0], 24))
    a = np.concatenate([f, a], axis=1)
    for W, b, leaky in layers[4:]:
        a = linear(W, b, a, leaky)
    return a


def head(weights, feature, motion_rows, subset=None, out=None):
    """neo_init_head_dev: (B, 9) float32; rows outside the launch stay"""
    B = motion_rows.shape[0]
    res = np.zeros((B, 9), np.float32) if out is None else np.array(out, dtype=np.float32)
    idx = launched(B, subset)
    if idx:
        f = feature if feature.shape[0] == 1 else feature[idx]
        res[idx] = head_rows(weights, f, motion_rows[idx])
    return res


def clamp(ts, T_min, T_max):
    eps = 1e-3 * (T_max - T_min)
    lo, hi = T_min + eps, T_max - eps
    return np.where(ts < lo, lo, np.where(ts > hi, hi, ts))              # a NaN passes, as in np.clip


def guess(out9, pose, T_min, T_max, subset=None, x0=None):
    """neo_init_guess_dev: (B, 7) float64 [x_0, x_1, y_0, y_1, tau_0, tau_1, tau_2]; rows outside the launch stay"""
    B = pose.shape[0]
    res = np.zeros((B, 7)) if x0 is None else np.array(x0, dtype=np.float64)
    o = np.asarray(out9, dtype=np.float32).astype(np.float64)
    px, py, c, s = pose[:, 0], pose[:, 1], pose[:, 3], pose[:, 4]
    new = np.zeros((B, 7))
    with np.errstate(all="ignore"):
        for i in range(2):
            lx, ly = o[:, 3 * i], o[:, 3 * i + 1]
            new[:, i] = (c * lx - s * ly) + px
            new[:, 2 + i] = (s * lx + c * ly) + py
        ts = clamp(o[:, 6:], T_min, T_max)
        new[:, 4:] = -np.log((T_max - T_min) / (ts - T_min) - 1.0)       # pack_x's expression
    idx = launched(B, subset)
    res[idx] = new[idx]
    return res
