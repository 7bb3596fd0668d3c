"""
BatchGeoPlanner: the resident twin of BatchPlanner.geo_plan (the reference's geo_traj_plan, geo_planner.py:19-35, for a
batch), shaped like initializer.BatchNeoPlanner.  ONE launch on the context's stream -- neo_geo_guess_dev: the A* search,
the prune to four key nodes and the pack of the optimiser's first guess, over a launch list, reading the start and the
target of a request from head / tail (B, 3, 2) where they lie -- then BatchPlanner.plan_dev from that guess.  Nothing
passes through the host; every returned array is bit for bit geo_plan's.

Two forms of the search (include/neo_planner.h).  The masked form reads one bit per expanded cell from a mask built per
scene and rebuilt whenever the scene's map changes: right for maps that stay.  The direct form evaluates the mask's own
expression on the map's records where the search needs a cell, and builds nothing: right for onboard maps, which change
every tick.  Their results are equal.
"""
import ctypes

import numpy as np

from . import _lib
from .onboard import OnboardMapper


def pack_guess(key_pts, tau):
    """the NumPy statement of the kernel's pack: key_pts (B, 4, 2) and the three start tau -> x0 (B, 7) =
    [k1.x, k2.x, k1.y, k2.y, tau0, tau1, tau2], k1 and k2 the inner key nodes -- BatchPlanner.pack_x of geo_init's
    int_wpts = key_pts[:, 1:3].T and ts = init_T * [1.5, 1, 1.5], copies only"""
    key_pts = np.asarray(key_pts, dtype=np.float64).reshape(-1, 4, 2)
    x0 = np.empty((key_pts.shape[0], 7))
    x0[:, 0:2] = key_pts[:, 1:3, 0]
    x0[:, 2:4] = key_pts[:, 1:3, 1]
    x0[:, 4:] = np.asarray(tau, dtype=np.float64).reshape(3)
    return x0


class BatchGeoPlanner:
    """geo_plan on RESIDENT torch tensors.  batch_planner: a BatchPlanner.  direct: True / False, the form of the search
    (module docstring); None: direct when the map handed to a call is an OnboardMapper, masked otherwise.
    max_expansions > 0 caps every search (NEO_GEO_FLAG_CAPPED: not the reference's result).

    What the last warm_start_dev wrote stays readable, by request: x0 (B, 7) float64, key_pts (B, 4, 2), path_cost (B,)
    float64, path_len, expansions, flags (B,) int32."""

    def __init__(self, batch_planner, direct=None, max_expansions=0):
        if int(max_expansions) < 0:
            raise ValueError("BatchGeoPlanner: max_expansions must be >= 0")
        self.bp, self.direct, self.max_expansions = batch_planner, (None if direct is None else bool(direct)), int(max_expansions)
        self.x0 = self.key_pts = self.path_cost = self.path_len = self.expansions = self.flags = None
        self._own_x0 = None

    def _check(self, map, head, tail, slots, subset, x0):
        """the refusals, before any device use; returns B"""
        who = "BatchGeoPlanner.warm_start_dev: "
        if head.ndim != 3 or tuple(head.shape[1:]) != (3, 2) or tuple(tail.shape) != tuple(head.shape):
            raise ValueError(who + "head and tail (B, 3, 2): the A* warm start is 2-D (D = 2) only")
        ctx = getattr(map, "ctx", None)
        if ctx is not None and ctx is not self.bp.ctx:
            raise ValueError(who + "the map lives in another context than the planner's")
        import torch
        B = int(head.shape[0])
        if any(t.dtype != torch.float64 or not t.is_contiguous() for t in (head, tail)):
            raise ValueError(who + "head and tail: contiguous float64 tensors")
        for name, t, n in (("slots", slots, B), ("subset", subset, None)):
            if t is not None and (t.dtype != torch.int32 or t.ndim != 1 or not t.is_contiguous() or
                                  (n is not None and t.numel() != n) or t.numel() > B):
                raise ValueError(who + name + ": a contiguous int32 tensor, " + ("one slot per request" if n else "at most B indices"))
        if x0 is not None and (tuple(x0.shape) != (B, 7) or x0.dtype != torch.float64 or not x0.is_contiguous()):
            raise ValueError(who + "x0 (B, 7) float64, contiguous")
        return B

    def warm_start_dev(self, map, head, tail, slots=None, subset=None, x0=None):
        """The geo first guess of the requests `subset` (an int32 device tensor of request indices; None: all B; an index
        outside 0 .. B - 1 is skipped) on resident tensors indexed by request: head and tail (B, 3, 2) float64 -- the
        search goes from head[:, 0] to tail[:, 0] --, `slots` (B,) int32 map-table slots or None (every request on `map`).
        One launch, asynchronous on the context's stream (ctx.synchronize() before torch reads the results; plan_dev runs
        on the same stream), into `x0` (B, 7) (the caller's, or one kept here) and the result arrays of the class
        docstring; rows of requests outside the subset stay as they are.  The caller's tensors must be ready
        (torch.cuda.synchronize after torch wrote them).  Returns x0."""
        B = self._check(map, head, tail, slots, subset, x0)
        import torch
        dev = head.device
        fresh = False
        if self.key_pts is None or self.key_pts.shape[0] != B or self.key_pts.device != dev:
            i = lambda: torch.zeros(B, dtype=torch.int32, device=dev)
            self.key_pts = torch.zeros((B, 4, 2), dtype=torch.float64, device=dev)
            self.path_cost = torch.zeros(B, dtype=torch.float64, device=dev)
            self.path_len, self.expansions, self.flags = i(), i(), i()
            fresh = True
        if x0 is None:
            if self._own_x0 is None or self._own_x0.shape[0] != B or self._own_x0.device != dev:
                self._own_x0 = torch.zeros((B, 7), dtype=torch.float64, device=dev)
                fresh = True
            x0 = self._own_x0
        self.x0 = x0
        if fresh:
            torch.cuda.synchronize(dev)      # (the context has its own stream: the buffers are ready before it starts)
        if subset is not None and subset.numel() == 0:
            return x0       # (an empty tensor may own no memory, and a NULL list would mean all B requests)
        self.bp._sync()                      # the context's T_min / T_max are the planner's
        direct = isinstance(map, OnboardMapper) if self.direct is None else self.direct
        p = _lib.dev_ptr
        self.bp.ctx.call("neo_geo_guess_dev", map.scene_id, p(slots), B, p(subset), _lib.launch_count(subset, B), p(head), p(tail),
                         _lib.ptr(self.bp._plan_frac_tau(2)[1]), self.max_expansions, int(direct), p(x0), p(self.key_pts),
                         p(self.path_len), p(self.path_cost), p(self.expansions), p(self.flags))
        return x0

    def plan_dev(self, map, head, tail, slots=None, subset=None, **plan_dev_kw):
        """warm_start_dev, then BatchPlanner.plan_dev(map, head, tail, x0=the guess, slots=slots, subset=subset,
        **plan_dev_kw): attempt 0 starts from the two inner key nodes, the retries from the straight line plus noise as
        plan_dev draws them (geo_plan's `plan` after a failed first attempt).  Returns plan_dev's bufs; the guess and the
        search's results stay in this object."""
        x0 = self.warm_start_dev(map, head, tail, slots=slots, subset=subset)
        return self.bp.plan_dev(map, head, tail, x0=x0, slots=slots, subset=subset, **plan_dev_kw)

    def mask_builds(self):
        """blocked masks the context has built so far (neo_geo_mask_builds): the direct form builds none"""
        n = ctypes.c_int64(0)
        self.bp.ctx.call("neo_geo_mask_builds", ctypes.byref(n))
        return int(n.value)


__all__ = ["BatchGeoPlanner", "pack_guess"]
