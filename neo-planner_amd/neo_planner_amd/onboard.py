"""Onboard maps for a fleet: every mission plans on the map it has seen (launch/map_server_onboard.launch: octomap_server
at 0.1 m from the depth camera, its projected_map into ESDF.occupancy_map_cb), not on the global map of its scene.

`OnboardMapper` keeps, for B missions, the resident log-odds and occupancy grids, one 2-D ESDF scene per mission and the
scenes' map-table slots.  A tick of sensing is `update`: render the depth images of the missions that sense
(neo_depth_render_batch_dev), integrate them (neo_onboard_integrate_batch_dev: octomap's scan insertion projected to
2-D, include/neo_planner.h; tests/onboard_oracle_np.py is the model in NumPy) and rebuild the ESDFs whose occupied
cells changed (neo_esdf_build_2d_batch_dev, in place: slots stay valid).  Unknown cells count as free, as in
ESDF.occupancy_map_cb.  `FleetReplanLoop(..., onboard=mapper, scenes=..., scene_index=...)` flies on these maps and is
audited against the true ones."""
import time

import numpy as np

from . import _lib, synth

UNKNOWN = -128          # the log-odds byte of a cell never updated


class OnboardMapper:
    """B onboard maps of `width` x `height` cells at `resolution`, origins (B, 2) or one (2,) for all.  `camera` is the
    DepthCamera the images come from; sensor_range, z_band and logodds (hit, miss, lo, hi in units of 0.05) are the
    model's parameters (neo_onboard_integrate_batch).  chunk: images rendered and integrated at a time by `update`
    (their float32 buffer is the mapper's largest: chunk * H * W * 4 bytes).

    The mapper owns B scenes of the context until `close()` drops them (dropping a scene rebuilds the map table: do it
    when no loop with resident slots is running).

    Device memory at 300 x 300: 2.9 MB of ESDF records and 0.18 MB of log-odds and occupancy a mission, about 12.5 GB for
    4096 missions."""

    def __init__(self, ctx, camera, B, width=synth.DOMAIN_CELLS, height=synth.DOMAIN_CELLS, resolution=synth.RES,
                 origins=(synth.DOMAIN_ORIGIN[0], synth.DOMAIN_ORIGIN[1]), sensor_range=6.0, z_band=synth.PROJECT_Z_RANGE,
                 logodds=(17, -8, -40, 70), chunk=512):
        import torch
        self.ctx = ctx if ctx is not None else _lib.default_context()
        self.camera = camera
        self.B, self.width, self.height = int(B), int(width), int(height)
        self.resolution, self.sensor_range = float(resolution), float(sensor_range)
        self.z_band = (float(z_band[0]), float(z_band[1]))
        self.lodds = tuple(int(v) for v in logodds)
        if self.B < 1:
            raise ValueError("OnboardMapper: B must be >= 1")
        if camera.max_range < self.sensor_range:
            raise ValueError("OnboardMapper: the camera's max_range must reach sensor_range")
        l_hit, l_miss, l_lo, l_hi = self.lodds
        if not (-127 <= l_lo <= l_hi <= 127 and 0 <= l_hit <= 127 and -127 <= l_miss <= 0):
            raise ValueError("OnboardMapper: logodds need -127 <= lo <= hi <= 127, 0 <= hit <= 127, -127 <= miss <= 0")
        org = np.asarray(origins, dtype=np.float64)
        self.origins = np.array(np.broadcast_to(org.reshape(-1, 2), (self.B, 2)), dtype=np.float64, order="C")
        self.chunk = max(1, int(chunk))
        self._device = dev = torch.device("cuda", self.ctx.device)
        self._p = _lib.dev_ptr
        self.logodds = torch.empty((self.B, self.height, self.width), dtype=torch.int8, device=dev)
        self.occupancy = torch.empty((self.B, self.height, self.width), dtype=torch.int8, device=dev)
        self.changed = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self._origins_dev = torch.from_numpy(self.origins).to(dev)
        self.scene_ids = np.array([self.ctx.new_scene_id() for _ in range(self.B)], dtype=np.int32)
        self.scene_id = int(self.scene_ids[0])      # any of the maps: what a planner call takes next to scene_ids / slots
        self.version = 0
        self.slots = None
        self._depth = None
        self.last = None
        self.reset()

    # ------------------------------------------------------------ state
    def reset(self):
        """every cell unknown again; the ESDFs are those of empty maps; the slots are read again"""
        import torch
        self.logodds.fill_(UNKNOWN)
        self.occupancy.fill_(-1)
        self.changed.zero_()
        torch.cuda.synchronize(self._device)
        self.rebuild(np.arange(self.B))
        self.refresh_slots()

    def refresh_slots(self):
        """reads the scenes' map-table slots again, into the same resident tensor.  The table is renumbered whenever a scene
        of the context is created or dropped (the mapper's own rebuilds are in place and move nothing): call this before
        the slots are used after such a change -- FleetReplanLoop.run does."""
        import torch
        c = self.ctx
        slots = np.array([c.lib.neo_scene_slot(c.h, int(s)) for s in self.scene_ids], dtype=np.int32)
        if slots.size != self.B or slots.min() < 0:
            raise _lib.NeoError("OnboardMapper: a scene without a map-table slot (closed?)")
        if self.slots is None:
            self.slots = torch.from_numpy(slots).to(self._device)
        else:
            self.slots.copy_(torch.from_numpy(slots))
        torch.cuda.synchronize(self._device)
        return self.slots

    def close(self):
        """drops the missions' scenes (their record buffers are freed, the map table is rebuilt at its next use)"""
        c, ids = self.ctx, self.scene_ids
        self.scene_ids = np.zeros(0, dtype=np.int32)
        if c is not None and getattr(c, "h", None):
            for s in ids:
                c.lib.neo_esdf_drop(c.h, int(s))

    def _host_subset(self, subset):
        if subset is None:
            return None
        if hasattr(subset, "cpu"):
            subset = subset.cpu().numpy()
        return np.ascontiguousarray(subset, dtype=np.int32).reshape(-1)

    # ------------------------------------------------------------ the three steps
    def integrate(self, depth_m, pose, subset=None):
        """one scan per launched mission: depth_m (n, H, W) float32 and pose (n, 5) float64 device tensors, row i the image
        and pose of mission subset[i] (of mission i, n = B, without a subset; subset: int32 indices, host or device).
        Returns `changed`, the resident (B,) int32 tensor: 1 where the mission's occupied cells changed in this scan."""
        import torch
        cam, c, p = self.camera, self.ctx, self._p
        sub = None
        if subset is not None:
            sub = subset if hasattr(subset, "data_ptr") else torch.from_numpy(self._host_subset(subset)).to(self._device)
            if sub.dtype != torch.int32 or not sub.is_contiguous():
                raise ValueError("OnboardMapper.integrate: subset must be a contiguous int32 array")
        n = _lib.launch_count(sub, self.B)
        if tuple(depth_m.shape) != (n, cam.height, cam.width) or depth_m.dtype != torch.float32 or not depth_m.is_contiguous():
            raise ValueError("OnboardMapper.integrate: depth_m must be a contiguous (n, H, W) float32 tensor")
        if tuple(pose.shape) != (n, 5) or pose.dtype != torch.float64 or not pose.is_contiguous():
            raise ValueError("OnboardMapper.integrate: pose must be a contiguous (n, 5) float64 tensor")
        torch.cuda.synchronize(self._device)     # (the context has its own stream: torch's tensors are ready before it starts)
        l_hit, l_miss, l_lo, l_hi = self.lodds
        c.call("neo_onboard_integrate_batch_dev", self.B, p(sub), n, p(depth_m), p(pose), cam.width, cam.height,
               cam.focal_px, cam.max_range, self.width, self.height, self.resolution, p(self._origins_dev),
               self.sensor_range, self.z_band[0], self.z_band[1], l_hit, l_miss, l_lo, l_hi, p(self.logodds),
               p(self.occupancy), p(self.changed))
        c.synchronize()
        return self.changed

    def rebuild(self, subset=None):
        """the ESDFs of the listed missions from their resident occupancy (None: those whose `changed` is set), in one
        neo_esdf_build_2d_batch_dev call.  Returns the missions rebuilt (host int32 array)."""
        import torch
        c, p = self.ctx, self._p
        if subset is None:
            idx = np.flatnonzero(self.changed.cpu().numpy() != 0).astype(np.int32)
        else:
            idx = self._host_subset(subset)
        if idx.size == 0:
            return idx
        whole = idx.size == self.B and np.array_equal(idx, np.arange(self.B))
        if whole or (idx[-1] - idx[0] + 1 == idx.size and np.all(np.diff(idx) == 1)):
            occ = self.occupancy[int(idx[0]):int(idx[-1]) + 1]           # a run of missions: no copy
        else:
            occ = self.occupancy.index_select(0, torch.from_numpy(idx.astype(np.int64)).to(self._device))
        torch.cuda.synchronize(self._device)
        c.call("neo_esdf_build_2d_batch_dev", _lib.ptr(np.ascontiguousarray(self.scene_ids[idx])), int(idx.size),
               p(occ), self.width, self.height, self.resolution,
               _lib.ptr(np.ascontiguousarray(self.origins[idx])))
        self.version += 1
        return idx

    def update(self, boxes, box_begin, pose, scene_index, subset=None):
        """render, integrate and rebuild for the listed missions (None: all).  boxes (NB, 6) float64, box_begin (S + 1,)
        int32 as DepthCamera.render_dev takes them; pose (B, 5) float64 and scene_index (B,) int32 (or None: scene 0) by
        MISSION, all device tensors.  Returns the missions whose ESDF was rebuilt; `last` holds the wall time of the three
        steps (render_s, integrate_s, rebuild_s) and the number of missions sensed and rebuilt."""
        import torch
        cam, c, p = self.camera, self.ctx, self._p
        idx = np.arange(self.B, dtype=np.int32) if subset is None else self._host_subset(subset)
        if idx.size == 0:
            return idx
        H, W = cam.height, cam.width
        chunk = min(self.chunk, idx.size)
        if self._depth is None or self._depth.shape[0] < chunk:
            self._depth = torch.empty((chunk, H, W), dtype=torch.float32, device=self._device)
        idx_dev = torch.from_numpy(idx).to(self._device)
        idx64 = idx_dev.long()
        pose_k = pose.index_select(0, idx64).contiguous()
        sidx_k = None if scene_index is None else scene_index.index_select(0, idx64).contiguous()
        n_scenes = int(box_begin.shape[0]) - 1
        tm = dict(render_s=0.0, integrate_s=0.0, rebuild_s=0.0, sensed=int(idx.size), rebuilt=0)
        for k0 in range(0, idx.size, chunk):
            n = min(chunk, idx.size - k0)
            torch.cuda.synchronize(self._device)
            t0 = time.perf_counter()
            c.call("neo_depth_render_batch_dev", W, H, cam.focal_px, cam.max_range, p(boxes), p(box_begin), n_scenes,
                   p(sidx_k[k0:k0 + n]) if sidx_k is not None else None, n,
                   p(pose_k[k0:k0 + n]), p(self._depth), None, None)
            c.synchronize()
            t1 = time.perf_counter()
            self.integrate(self._depth[:n], pose_k[k0:k0 + n], idx_dev[k0:k0 + n])
            tm["render_s"] += t1 - t0
            tm["integrate_s"] += time.perf_counter() - t1
        t0 = time.perf_counter()
        ch = self.changed.index_select(0, idx64).cpu().numpy() != 0
        rebuilt = self.rebuild(idx[ch])
        tm["rebuild_s"] = time.perf_counter() - t0
        tm["rebuilt"] = int(rebuilt.size)
        self.last = tm
        return rebuilt

    # ------------------------------------------------------------ lookups
    def query(self, i, pts):
        """nearest-cell lookups on mission i's ESDF: pts (n, 2) -> dist (n,), grad (n, 2)"""
        pts = np.ascontiguousarray(np.asarray(pts, dtype=np.float64).reshape(-1, 2))
        d = np.empty(len(pts))
        g = np.empty((len(pts), 2))
        c = self.ctx
        c.call("neo_esdf_query", int(self.scene_ids[i]), len(pts), _lib.ptr(pts), _lib.ptr(d), _lib.ptr(g))
        return d, g
