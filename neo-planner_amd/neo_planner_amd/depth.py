"""Batched GPU depth camera: `initializer.raycast_depth` for B requests, each with its own scene and pose, in one call
(include/neo_planner.h neo_depth_render_batch; kernels in csrc/neo_depth.hpp).  It is the sensor in front of the
initializer network: `initializer.BatchNeoPlanner` renders, forms the motion vectors, runs the network and hands the
warm starts to `BatchPlanner.plan`.

The arithmetic is raycast_depth's in float32, fixed operation by operation (tests/depth_oracle_np.py restates it in
NumPy and the kernel is tested against that bit for bit); against the float64 raycast_depth the uint8 image differs, if
at all, in a silhouette pixel whose ray passes an edge within fp32 rounding."""

import numpy as np

from . import _lib


def _boxes_rows(scene):
    """a scene is an (n, 6) array of (lo xyz, hi xyz) rows, or a (pillars, canopy) pair as raycast_depth takes them"""
    if isinstance(scene, tuple) and len(scene) == 2 and not np.isscalar(scene[0]):
        return DepthCamera.boxes_of(*scene)
    return np.asarray(scene, dtype=np.float64).reshape(-1, 6)


class DepthCamera:
    """a pinhole camera of `width` x `height` pixels and horizontal field of view `hfov_deg`, depth along the optical
    axis capped at `max_range`: raycast_depth's camera (x forward, y left, z up; ground plane z = 0)"""

    def __init__(self, ctx=None, width=640, height=480, hfov_deg=87.0, max_range=20.0):
        self._ctx = ctx
        self.width, self.height = int(width), int(height)
        self.hfov_deg, self.max_range = float(hfov_deg), float(max_range)
        # as raycast_depth computes it, in float64
        self.focal_px = float((self.width / 2) / np.tan(np.radians(self.hfov_deg) / 2))
        self._buf = None

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = _lib.default_context()
        return self._ctx

    @staticmethod
    def boxes_of(pillars, canopy=()):
        """the (lo, hi) rows exactly as raycast_depth forms them: pillars (cx, cy, sx, sy, sz) standing on the ground,
        canopy (cx, cy, cz, sx, sy, sz) -> (n, 6) float64"""
        rows = [(cx - sx / 2, cy - sy / 2, 0.0, cx + sx / 2, cy + sy / 2, sz) for (cx, cy, sx, sy, sz) in pillars]
        rows += [(cx - sx / 2, cy - sy / 2, cz - sz / 2, cx + sx / 2, cy + sy / 2, cz + sz / 2)
                 for (cx, cy, cz, sx, sy, sz) in canopy]
        return np.asarray(rows, dtype=np.float64).reshape(-1, 6)

    @staticmethod
    def pack_scenes(scenes):
        """scenes: one scene or a list of scenes (see `_boxes_rows`) -> boxes (NB, 6) float64, box_begin (S + 1,) int32"""
        if isinstance(scenes, np.ndarray) and scenes.ndim == 2:
            scenes = [scenes]
        rows = [_boxes_rows(s) for s in scenes]
        begin = np.zeros(len(rows) + 1, dtype=np.int32)
        begin[1:] = np.cumsum([r.shape[0] for r in rows])
        boxes = np.concatenate(rows, axis=0) if rows else np.zeros((0, 6))
        return np.ascontiguousarray(boxes, dtype=np.float64), begin

    @staticmethod
    def poses(eye, yaw):
        """eye (B, 3), yaw (B,) -> pose (B, 5) float64: eye, cos(yaw), sin(yaw) -- NumPy's, as raycast_depth takes them"""
        eye = np.asarray(eye, dtype=np.float64).reshape(-1, 3)
        yaw = np.asarray(yaw, dtype=np.float64).reshape(-1)
        if yaw.shape[0] != eye.shape[0]:
            raise ValueError("DepthCamera: one yaw per eye")
        return np.ascontiguousarray(np.concatenate([eye, np.cos(yaw)[:, None], np.sin(yaw)[:, None]], axis=1))

    def render(self, scenes, eye, yaw, scene_index=None, want_u8=True):
        """NumPy in, NumPy out (works without torch): scenes as in `pack_scenes`, eye (B, 3), yaw (B,), scene_index (B,)
        or None (every request sees scene 0).  Returns dict(depth_u8 (B, H, W) uint8, depth_m (B, H, W) float32 metres,
        depth_max (B,) float32)."""
        boxes, begin = self.pack_scenes(scenes)
        pose = self.poses(eye, yaw)
        B = pose.shape[0]
        sidx = None if scene_index is None else np.ascontiguousarray(scene_index, dtype=np.int32).reshape(-1)
        if sidx is not None and sidx.shape[0] != B:
            raise ValueError("DepthCamera.render: one scene_index per request")
        depth_m = np.zeros((B, self.height, self.width), dtype=np.float32)
        depth_u8 = np.zeros((B, self.height, self.width), dtype=np.uint8) if want_u8 else None
        depth_max = np.zeros(B, dtype=np.float32)
        c = self.ctx
        # (a scene list without any box still hands over a valid pointer)
        bx = boxes if boxes.shape[0] else np.zeros((1, 6))
        c.call("neo_depth_render_batch", self.width, self.height, self.focal_px, self.max_range, _lib.ptr(bx),
               _lib.ptr(begin), len(begin) - 1, _lib.ptr(sidx), B, _lib.ptr(pose),
               _lib.ptr(depth_m), _lib.ptr(depth_u8), _lib.ptr(depth_max))
        return dict(depth_u8=depth_u8, depth_m=depth_m, depth_max=depth_max)

    def render_dev(self, boxes, box_begin, pose, scene_index=None, chunk=None, want_m=True, sync=True):
        """torch device tensors in and out: boxes (NB, 6) float64, box_begin (S + 1,) int32, pose (B, 5) float64
        (`poses`), scene_index (B,) int32 or None.  `chunk`: images per launch (None: all B in one).  want_m False
        returns only depth_u8 and depth_max, and depth_m is then one float32 buffer of `chunk` images that every launch
        reuses (kept by the camera).  The launches run on the context's stream, after everything torch has queued;
        sync False returns without waiting for them (`ctx.synchronize()` before torch reads the results).  Returns
        dict(depth_u8, depth_max[, depth_m])."""
        import torch
        B = int(pose.shape[0])
        H, W = self.height, self.width
        chunk = B if chunk is None else max(1, min(int(chunk), B))
        dev = pose.device
        depth_u8 = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
        depth_max = torch.empty(B, dtype=torch.float32, device=dev)
        if want_m:
            depth_m = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        else:
            if self._buf is None or self._buf.shape[0] < chunk or self._buf.device != dev or self._buf.shape[1:] != (H, W):
                self._buf = torch.empty((chunk, H, W), dtype=torch.float32, device=dev)
            depth_m = None
        for t in (boxes, box_begin, pose, scene_index):
            if t is not None and not t.is_contiguous():
                raise ValueError("DepthCamera.render_dev: tensors must be contiguous")
        if boxes.dtype != torch.float64 or pose.dtype != torch.float64 or box_begin.dtype != torch.int32 or \
                (scene_index is not None and scene_index.dtype != torch.int32):
            raise ValueError("DepthCamera.render_dev: boxes and pose float64, box_begin and scene_index int32")
        c = self.ctx
        p = _lib.dev_ptr
        torch.cuda.synchronize(dev)        # (the context has its own stream: the tensors above are ready before it starts)
        for b0 in range(0, B, chunk):
            n = min(chunk, B - b0)
            m = depth_m[b0:b0 + n] if want_m else self._buf[:n]
            c.call("neo_depth_render_batch_dev", W, H, self.focal_px, self.max_range, p(boxes), p(box_begin),
                   int(box_begin.shape[0]) - 1, p(scene_index[b0:b0 + n]) if scene_index is not None else None, n,
                   p(pose[b0:b0 + n]), p(m), p(depth_u8[b0:b0 + n]), p(depth_max[b0:b0 + n]))
        if sync:
            c.synchronize()
        out = dict(depth_u8=depth_u8, depth_max=depth_max)
        if want_m:
            out["depth_m"] = depth_m
        return out
