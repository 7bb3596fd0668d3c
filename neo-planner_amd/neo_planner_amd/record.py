"""Expert demonstrations of a fleet, kept on the GPU: the reference's `selected_planner:=record`
(traj_planner/record_planner.py:75-185) for B closed-loop missions.

Every successful plan of a flight becomes one row of a resident dataset -- the depth image the mission saw, the 24-d
motion vector of form_nn_input (:13-58), the body-frame waypoints of form_nn_output (:61-72) and the durations --
written by neo_record_commit_dev (include/neo_planner.h; kernels in csrc/neo_record.hpp, tests/record_oracle_np.py is
the model in NumPy).  `FleetReplanLoop(..., record=recorder, scenes=..., scene_index=...)` fills it; rows come in the
order (tick, target round, ascending mission) whatever the timing.  `training.train_initializer` fits the initializer
network to `training_tensors()`.

The reference writes one CSV line and one PNG per plan; here the rows stay in HBM until `rows()` or `save()` asks for
them, and the loop reads nothing back on their account."""
import math

import numpy as np

from . import _lib

FIELDS = ("images", "motion", "wpts_local", "tau", "pose", "meta")


def tau_to_ts(tau, T_min, T_max):
    """map_tau2T (expert_planner.py:477-483), element by element with math.exp as the reference computes it"""
    tau = np.asarray(tau, dtype=np.float64)
    ts = np.zeros(tau.shape)
    for i, t in np.ndenumerate(tau):
        try:
            e = math.exp(-t)
        except OverflowError:       # (no plan that solved has such a tau; the duration's limit is T_min)
            e = math.inf
        ts[i] = (T_max - T_min) / (1 + e) + T_min
    return ts


class DemoRecorder:
    """The resident dataset of `capacity` rows and the tick's staging buffer of images.  camera: the DepthCamera the
    missions look through (its width and height are the images'); M: pieces of a plan (init_wpts_num + 1 of the planner
    that flies); des_pos_z: the eye's height.  Rows beyond `capacity` are counted in `dropped` and not kept.

    Device memory: capacity * (H * W + 8 * (24 + 3 (M - 1) + M + 5) + 12) bytes of dataset, and B * H * W of staging once
    a fleet of B missions flies with it (160 x 120: 19 kB a row, 640 x 480: 307 kB a row)."""

    def __init__(self, camera, capacity, M=3, des_pos_z=2.0, ctx=None):
        self.camera = camera
        self.capacity, self.M, self.des_pos_z = int(capacity), int(M), float(des_pos_z)
        if self.capacity < 1 or self.M < 2:
            raise ValueError("DemoRecorder: capacity >= 1 and M >= 2")
        self.height, self.width = int(camera.height), int(camera.width)
        self._ctx = ctx
        self.T_min = self.T_max = None
        self._dev = None        # the resident arrays, made at first use
        self._host = None       # the rows of a loaded file
        self.staging = None     # (B, H, W) uint8: the tick's images by mission
        self.cur_vel = self.row_of = None
        self.chunk = 512        # images a render launch

    # ------------------------------------------------------------ device state
    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = _lib.default_context()
        return self._ctx

    def _alloc(self):
        if self._host is not None:
            raise _lib.NeoError("DemoRecorder: a loaded dataset is read-only")
        if self._dev is None:
            import torch
            c = self.ctx
            self.device = dev = torch.device("cuda", c.device)
            cap, M = self.capacity, self.M
            f = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
            self._dev = dict(images=torch.zeros((cap, self.height, self.width), dtype=torch.uint8, device=dev),
                             motion=f(cap, 24), wpts_local=f(cap, 3 * (M - 1)), tau=f(cap, M), pose=f(cap, 5),
                             meta=torch.zeros((cap, 3), dtype=torch.int32, device=dev),
                             n_rows=torch.zeros(1, dtype=torch.int32, device=dev),
                             dropped=torch.zeros(1, dtype=torch.int32, device=dev))
            self.T_min, self.T_max = float(c.params.T_min), float(c.params.T_max)
            torch.cuda.synchronize(dev)
        return self._dev

    def bind(self, B):
        """the per-mission buffers of a fleet of B missions: staging images, velocities, the round's rows"""
        import torch
        self._alloc()
        if self.staging is None or self.staging.shape[0] != B:
            self.staging = torch.zeros((B, self.height, self.width), dtype=torch.uint8, device=self.device)
            self.cur_vel = torch.zeros((B, 2), dtype=torch.float64, device=self.device)
            self.row_of = torch.full((B,), -1, dtype=torch.int32, device=self.device)
            torch.cuda.synchronize(self.device)

    def reset(self):
        """forget every row: the counters go back to zero (the arrays keep their bytes until rows overwrite them)"""
        import torch
        d = self._alloc()
        d["n_rows"].zero_()
        d["dropped"].zero_()
        torch.cuda.synchronize(self.device)

    def commit(self, B, sub, x, head, tail, solved, pose, mission_ids, tick, round_):
        """one neo_record_commit_dev over the missions `sub` (device int32, or None: all B) -- asynchronous on the context's
        stream; every argument a device tensor indexed by mission"""
        d, c = self._alloc(), self.ctx
        p = _lib.dev_ptr
        c.call("neo_record_commit_dev", int(B), p(sub), int(sub.numel()) if sub is not None else 0, self.M, p(x), p(head),
               p(tail), p(solved), p(pose), p(self.cur_vel), p(self.staging), self.width, self.height, p(mission_ids),
               int(tick), int(round_), self.capacity, p(d["motion"]), p(d["wpts_local"]), p(d["tau"]), p(d["pose"]),
               p(d["meta"]), p(d["images"]), p(self.row_of), p(d["n_rows"]), p(d["dropped"]))

    # ------------------------------------------------------------ what was recorded
    @property
    def n_rows(self):
        if self._host is not None:
            return int(self._host["motion"].shape[0])
        return 0 if self._dev is None else int(self._dev["n_rows"].item())

    @property
    def dropped(self):
        if self._host is not None:
            return int(self._host_dropped)
        return 0 if self._dev is None else int(self._dev["dropped"].item())

    def rows(self):
        """host arrays of the filled rows: images (n, H, W) uint8, motion (n, 24), wpts_local (n, 3 (M - 1)), tau (n, M),
        pose (n, 5), meta (n, 3) int32 (mission id, tick, target round), and ts (n, M) = map_tau2T(tau)"""
        if self._host is not None:
            out = {k: self._host[k] for k in FIELDS}
        else:
            n = self.n_rows
            if self._dev is None:
                M = self.M
                out = dict(images=np.zeros((0, self.height, self.width), np.uint8), motion=np.zeros((0, 24)),
                           wpts_local=np.zeros((0, 3 * (M - 1))), tau=np.zeros((0, M)), pose=np.zeros((0, 5)),
                           meta=np.zeros((0, 3), np.int32))
            else:
                out = {k: self._dev[k][:n].cpu().numpy() for k in FIELDS}
        T_min, T_max = (0.5, 5.0) if self.T_min is None else (self.T_min, self.T_max)
        out["ts"] = tau_to_ts(out["tau"], T_min, T_max)
        return out

    def labels(self, rows=None):
        """(n, 3 (M - 1) + M): the columns the reference's CSV ends with -- wpts1_x .. wpts2_z, ts1 .. ts3 for M = 3"""
        r = self.rows() if rows is None else rows
        return np.concatenate([r["wpts_local"], r["ts"]], axis=1)

    def training_tensors(self, rows=None):
        """the network's flattened inputs (n, H * W + 24) float32 -- process_input_np's layout (nn_trainer.py:52-59): the
        image row-major, then the motion vector -- and the labels (n, 3 (M - 1) + M) float32"""
        r = self.rows() if rows is None else rows
        n = r["motion"].shape[0]
        inputs = np.concatenate([r["images"].reshape(n, -1).astype(np.float32), r["motion"].astype(np.float32)], axis=1)
        return inputs, self.labels(r).astype(np.float32)

    # ------------------------------------------------------------ files
    def save(self, path):
        """the filled rows and the recorder's parameters as one .npz"""
        r = self.rows()
        T_min, T_max = (0.5, 5.0) if self.T_min is None else (self.T_min, self.T_max)
        np.savez_compressed(path, **{k: r[k] for k in FIELDS}, M=np.int32(self.M), des_pos_z=np.float64(self.des_pos_z),
                            T_min=np.float64(T_min), T_max=np.float64(T_max), dropped=np.int64(self.dropped))

    @classmethod
    def from_arrays(cls, images, motion, wpts_local, tau, pose, meta, des_pos_z=2.0, T_min=0.5, T_max=5.0, dropped=0):
        """a read-only recorder over host rows (what `load` returns): rows(), labels(), training_tensors() and save()
        work without a GPU"""
        self = cls.__new__(cls)
        self._host = dict(images=np.ascontiguousarray(images, dtype=np.uint8), motion=_lib.as_f64(motion),
                          wpts_local=_lib.as_f64(wpts_local), tau=_lib.as_f64(tau), pose=_lib.as_f64(pose),
                          meta=np.ascontiguousarray(meta, dtype=np.int32))
        n = self._host["motion"].shape[0]
        if self._host["images"].ndim != 3 or any(self._host[k].shape[0] != n for k in FIELDS) or self._host["tau"].ndim != 2:
            raise ValueError("DemoRecorder.from_arrays: one row of every array per plan, images (n, H, W)")
        self.camera, self._ctx, self._dev = None, None, None
        self.staging = self.cur_vel = self.row_of = None
        self.M, self.capacity, self.des_pos_z = int(self._host["tau"].shape[1]), max(n, 1), float(des_pos_z)
        self.height, self.width = (int(v) for v in self._host["images"].shape[1:])
        self.T_min, self.T_max, self._host_dropped = float(T_min), float(T_max), int(dropped)
        self.chunk = 512
        return self

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls.from_arrays(*(z[k] for k in FIELDS), des_pos_z=float(z["des_pos_z"]), T_min=float(z["T_min"]),
                                   T_max=float(z["T_max"]), dropped=int(z["dropped"]))
