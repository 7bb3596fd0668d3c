"""
Host side of the MI355X planner: the reference's Python interface on top of the C ABI.

`MinJerkPlanner` keeps the names, argument meaning, side effects and exceptions of
traj_planner/expert_planner.py:28-585 (+ traj_utils.py evaluation helpers), so that
ros_node/traj_planner_node.py-style callers can switch without edits:

    planner = MinJerkPlanner(config)            # PlannerConfig-like object
    planner.plan(map, head_state, tail_state)   # or warm_start_plan / batch_plan / plan_once
    planner.int_wpts, planner.ts, planner.iter_num, planner.get_full_state_cmd(hz) ...

All arithmetic of the replan loop (coefficient solve, cost, gradient, L-BFGS-B) runs on the
GPU through libneo_planner_hip.so; this file only packs arguments, keeps the reference's
retry/exception control flow, and unpacks results.  `BatchPlanner` is the batched entry the
reference does not have: B independent replans in one launch.
"""
import math

import numpy as np

from . import _lib, counter_rng
from .esdf import ESDF, ESDF3D


class PlannerConfig:
    """parameter bag with the attribute names MinJerkPlanner reads (expert_planner.py:33-56,
    ros_node/traj_planner_node.py:32-46); defaults = launch/config/planner_config.yaml:2-13."""

    def __init__(self, **kw):
        self.v_max = 1.0
        self.T_min = 0.5
        self.T_max = 5.0
        self.safe_dis = 0.7
        self.delta_t = 0.1
        self.weights = [1.0, 1.0, 1.0, 10000.0]
        self.init_wpts_mode = 'fixed'
        self.init_seg_len = 2.0
        self.init_wpts_num = 2
        self.init_T = 2.5
        self.collision_cost_tol = 5
        self.opt_tol = 1e-2
        self.des_pos_z = 2.0
        for k, v in kw.items():
            setattr(self, k, v)


def _push_params(ctx, p, sample_dtype, stale_T=True, flags=0):
    """the optimiser options ftol / gtol / maxls / maxiter / maxfun are read from `p` where it has them; without them
    the reference's (expert_planner.py:213-225)"""
    ctx.set_params(v_max=float(p.v_max), T_min=float(p.T_min), T_max=float(p.T_max), safe_dis=float(p.safe_dis),
                   delta_t=float(p.delta_t), weights=[float(w) for w in p.weights],
                   collision_cost_tol=float(p.collision_cost_tol), ftol=float(getattr(p, "ftol", 1e-4)),
                   gtol=float(getattr(p, "gtol", 1e-4)), maxls=int(getattr(p, "maxls", 20)),
                   maxiter=int(getattr(p, "maxiter", 15000)), maxfun=int(getattr(p, "maxfun", 15000)),
                   bugcompat_stale_T=int(bool(stale_T)),
                   sample_dtype={"f64": _lib.NEO_F64, "f32": _lib.NEO_F32}[sample_dtype], flags=int(flags))


def _map_scene(ctx, map, cache):
    """scene id of `map` on the device.  Our own ESDF classes are already resident; a foreign
    object with the reference's attribute protocol (esdf.py:17-33) is snapshotted."""
    if isinstance(map, (ESDF, ESDF3D)):
        if map.ctx is not ctx:
            raise ValueError("map and planner live on different contexts")
        return map.scene_id
    snap = ESDF.from_arrays(map.esdf_map, map.esdf_grad_x, map.esdf_grad_y, map.map_resolution,
                            (map.map_origin.x, map.map_origin.y), ctx=ctx)
    old = cache.get("foreign")
    if old is not None:
        ctx.lib.neo_esdf_drop(ctx.h, old.scene_id)
    cache["foreign"] = snap
    return snap.scene_id


def _audit_result(audit, count, flags):
    """neo_audit_traj_batch's record as a dict: the ten fields by name (_lib.AUDIT_FIELDS), count, flags and the masks"""
    out = {name: audit[:, i] for i, name in enumerate(_lib.AUDIT_FIELDS)}
    out.update(count=count, flags=flags, unsafe=(flags & _lib.NEO_AUDIT_FLAG_UNSAFE) != 0,
               metric_fail=(flags & _lib.NEO_AUDIT_FLAG_METRIC_FAIL) != 0)
    return out


def _audit_weights(weights):
    return None if weights is None else _lib.as_f64(weights).reshape(3)


def _f64(*arrays):
    """the arrays as C-contiguous float64, what the host entry points read"""
    return [_lib.as_f64(a) for a in arrays]


def _ptrs(*arrays):
    """host pointers of NumPy arrays, in order (None -> NULL)"""
    return [_lib.ptr(a) for a in arrays]


def _dev_ptrs(*tensors):
    """device pointers of torch tensors, in order (None -> NULL)"""
    return [_lib.dev_ptr(t) for t in tensors]


def _eval_arrays(B, n, M, D, want_coeffs=True):
    """what neo_cost_grad_batch fills, in the order it takes them: cost (B,), costs (B, 4), grad (B, n), coeffs (B, 6 M, D)
    or None, status"""
    return np.zeros(B), np.zeros((B, 4)), np.zeros((B, n)), np.zeros((B, 6 * M, D)) if want_coeffs else None, np.zeros(B, np.int32)


def _audit_arrays(B):
    """what neo_audit_traj_batch fills, in the order it takes them: audit (B, NEO_AUDIT_FIELDS), count, flags"""
    return np.zeros((B, _lib.NEO_AUDIT_FIELDS)), np.zeros(B, np.int32), np.zeros(B, np.int32)


# ---------------------------------------------------------------- what BatchPlanner's methods share (host layer)
def _shape(x, head):
    """(B, M, D, n) of the packed rows x (B, n) = [D * (M - 1) waypoint values ; M tau] with head (B, 3, D)"""
    B, n = x.shape
    D = head.shape[2]
    return B, (n + D) // (D + 1), D, n


def _host_results(B):
    """the optimiser's five result arrays on the host, as ONE tuple in the order every entry point takes them:
    costs (B, 4), costs_last (B, 4), nit, nfev, status (B,) int32"""
    return np.zeros((B, 4)), np.zeros((B, 4)), np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)


def _dev_results(B, dev):
    """`_host_results` as zeroed torch tensors on `dev`"""
    import torch
    f = lambda: torch.zeros(B, 4, dtype=torch.float64, device=dev)
    i = lambda: torch.zeros(B, dtype=torch.int32, device=dev)
    return f(), f(), i(), i(), i()


def _result_dict(x, results, weights=None):
    """the optimiser's result dict from x and the five arrays: status split into its code and the collision flag;
    with `weights`, final_cost = (costs * weights).sum() -- the costs at x (batch_plan takes costs_last: it adds its own)"""
    costs, last, nit, nfev, st = results
    out = dict(x=x, costs=costs, costs_last=last, nit=nit, nfev=nfev, status=st & 0xff,
               collision=(st & _lib.NEO_TRAJ_FLAG_COLLISION) != 0)
    if weights is not None:
        out["final_cost"] = (costs * np.asarray(weights, dtype=np.float64)).sum(axis=1)
    return out


def _upload(dev, *arrays):
    """host arrays as tensors on `dev` (blocking copies on torch's stream)"""
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _torch_done(dev):
    """THE STREAM RULE: the context launches on a stream of its own, so what torch has queued -- uploads, zeroed buffers --
    is waited for before the context's first launch on it; in the other direction Context.synchronize"""
    import torch
    torch.cuda.synchronize(dev)


def _scene_ids(scene_ids):
    """per-request scene ids as the ABI takes them: contiguous int32, or None (every request on the call's map)"""
    return None if scene_ids is None else np.ascontiguousarray(scene_ids, dtype=np.int32)


def _stream_ids(stream_ids, B, who):
    """the stream of each request's retry noise: its position in the batch unless the caller names one per request"""
    stream_ids = np.arange(B) if stream_ids is None else np.asarray(stream_ids).reshape(-1)
    if stream_ids.shape[0] != B:
        raise ValueError("%s: stream_ids needs one id per request" % who)
    return stream_ids


def _draw_seed(rng):
    """a call's seed when the caller gave none: from `rng`, or from the OS"""
    return int((rng if rng is not None else np.random.default_rng()).integers(0, 2 ** 62))


def _work_buffers(device, header, rows, B, n, D):
    """what plan_buffers and batch_buffers share (torch tensors, zeroed): the packed work arrays of a launch of `rows`
    rows and the request-indexed results, behind the sizes in `header`.  Returns (bufs, f, i): f / i make further float64 /
    int32 arrays"""
    import torch
    f = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=device)
    i = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=device)
    bufs = dict(header, x_k=f(rows, n), head_k=f(rows, 3, D), tail_k=f(rows, 3, D), slots_k=i(rows), costs_k=f(rows, 4),
                last_k=f(rows, 4), nit_k=i(rows), nfev_k=i(rows), status_k=i(rows), x=f(B, n), costs=f(B, 4),
                costs_last=f(B, 4), nit=i(B), nfev=i(B), status=i(B), solved=i(B))
    return bufs, f, i


RESULTS_K = ("costs_k", "last_k", "nit_k", "nfev_k", "status_k")      # a launch's five result arrays in the buffers, packed
RESULTS = ("costs", "costs_last", "nit", "nfev", "status")            # ... and by request


class MinJerkPlanner:
    """MI355X-backed stand-in for expert_planner.py:MinJerkPlanner"""

    def __init__(self, config=None, ctx=None, sample_dtype="f64", stale_T=True):
        config = config if config is not None else PlannerConfig()
        self._ctx = ctx             # created on first device use: host-only helpers work without a GPU
        self.s = 3
        self.v_max = config.v_max
        self.T_min = config.T_min
        self.T_max = config.T_max
        self.safe_dis = config.safe_dis
        self.collision_cost_tol = config.collision_cost_tol
        self.weights = np.array(config.weights, dtype=np.float64)
        self.delta_t = config.delta_t
        self.opt_tol = config.opt_tol
        self.init_wpts_mode = config.init_wpts_mode
        self.init_seg_len = config.init_seg_len
        self.init_wpts_num = int(config.init_wpts_num)
        self.init_T = config.init_T
        self.batch_num = 3
        self.iter_num = 0
        self.opt_running_times = 0
        self.coeffs = []
        # "f32x": everything in fp32 (NEO_FLAG_F32_SOLVE) -- the arithmetic bench.py times, here behind the reference's own
        # interface so that the recorded reference runs (tests/golden g3 / g6) can be replayed in it
        self.flags = _lib.NEO_FLAG_F32_SOLVE if sample_dtype == "f32x" else 0
        self.sample_dtype = "f32" if sample_dtype == "f32x" else sample_dtype
        self.stale_T = stale_T
        self._cache = {}
        self._scene = None

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = _lib.default_context()
        return self._ctx

    # ------------------------------------------------------------ initial guesses (:82-140)
    def generate_init_variables(self, head_state, tail_state, seed=0):
        start, target = head_state[0], tail_state[0]
        if self.init_wpts_mode == 'adaptive':
            dist = np.linalg.norm(target - start)
            count = max(math.ceil(dist / self.init_seg_len - 1), 1)
        elif self.init_wpts_mode == 'fixed':
            count = self.init_wpts_num
        stride = (target - start) / (count + 1)
        wpts = np.linspace(start + stride, target, count, endpoint=False)
        if seed != 0:
            wpts += np.random.normal(0, 0.5, wpts.shape)   # the reference's unseeded global RNG (:94)
        ts = self.init_T * np.ones((count + 1,))
        ts[0] *= 1.5
        ts[-1] *= 1.5
        return wpts.T, ts

    def batch_generate_init_variables(self, head_state, tail_state):
        if self.init_wpts_mode != 'fixed':
            print("Error! init_wpts_mode must be 'fixed'")
        start, target = head_state[0], tail_state[0]
        forward = (target - start) / np.linalg.norm(target - start)
        sideways = np.array([[forward[1], -forward[0]], [-forward[1], forward[0]]])
        count = self.init_wpts_num
        out = np.zeros((self.batch_num, count, head_state.shape[1]))
        stride = (target - start) / (count + 1)
        out[0] = np.linspace(start + stride, target, count, endpoint=False)
        which = 0
        for i in range(1, self.batch_num):
            out[i] = out[0] + 0.6 * sideways[which]
            which = 1 - which
        ts = self.init_T * np.ones((count + 1,))
        ts[0] *= 1.5
        ts[-1] *= 1.5
        return np.transpose(out, (0, 2, 1)), ts

    # ------------------------------------------------------------ entry points (:62-80, :142-237)
    def read_planning_conditions(self, map, head_state, tail_state, int_wpts, ts, _resnapshot=True):
        self.map = map
        self.D = head_state.shape[1]
        self.M = ts.shape[0]
        self.head_state = np.zeros((self.s, self.D))
        self.tail_state = np.zeros((self.s, self.D))
        for i in range(min(self.s, head_state.shape[0])):
            self.head_state[i] = head_state[i]
        for i in range(min(self.s, tail_state.shape[0])):
            self.tail_state[i] = tail_state[i]
        self.int_wpts = int_wpts
        self.ts = ts
        # snapshot the map now: the reference reads it unlocked while a subscriber thread may
        # be rewriting it
        if _resnapshot or self._scene is None:
            self._scene = _map_scene(self.ctx, map, self._cache)

    def plan(self, map, head_state, tail_state):
        int_wpts, ts = self.generate_init_variables(head_state, tail_state)
        self.warm_start_plan(map, head_state, tail_state, int_wpts, ts)

    def warm_start_plan(self, map, head_state, tail_state, int_wpts, ts):
        self.read_planning_conditions(map, head_state, tail_state, int_wpts, ts)
        seed = 0
        while seed < 5:
            try:
                self.plan_once()
                return
            except Exception as ex:
                print(f"Re-planning for {ex}, current seed: {seed}")
                seed += 1
                self.int_wpts, self.ts = self.generate_init_variables(head_state, tail_state, seed)
        raise Exception("No solution for the given target")

    def batch_plan(self, map, head_state, tail_state):
        """expert_planner.py:142-168.  The three lateral candidates are optimised in ONE launch of three trajectories
        (a trajectory's result does not depend on its batch neighbours: bit-identical to three launches of one); the
        reference's loop -- including its success check INSIDE the loop (:160-168) and the order of its side effects on
        iter_num / opt_running_times / int_wpts -- then runs on the host over the three results."""
        cands, ts = self.batch_generate_init_variables(head_state, tail_state)
        best_wpts = np.zeros(cands.shape)
        best_ts = np.zeros((self.batch_num, len(ts)))
        cost = np.zeros(self.batch_num)
        results = None
        for i in range(self.batch_num):
            try:
                self.read_planning_conditions(map, head_state, tail_state, cands[i], ts, _resnapshot=(i == 0))
                if results is None:
                    results = self._launch_plan_once([cands[k] for k in range(self.batch_num)], ts)
                self._finish_plan_once(*[r[i:i + 1] for r in results])
                best_wpts[i] = self.int_wpts
                best_ts[i] = self.ts
                cost[i] = self.weighted_cost.sum()
                print(f"batch_cost[{i}] = {cost[i]}")
            except Exception as ex:
                print(f"The {i}th attempt is deprecated for {ex}")
                cost[i] = np.inf
            # as in the reference the check sits inside the loop (:160-168)
            if np.min(cost) < np.inf:
                k = np.argmin(cost)
                self.int_wpts = best_wpts[k]
                self.ts = best_ts[k]
                self.final_cost = cost[k]
            else:
                print("All attempts are infeasible! Start re-planning from scratch...")
                self.warm_start_plan(map, head_state, tail_state, cands[0], ts)

    def _pack_x(self):
        nq = self.D * (self.M - 1)
        return np.concatenate((np.reshape(self.int_wpts, (nq,)), self.tau), axis=0)

    def _unpack_x(self, x):
        nq = self.D * (self.M - 1)
        self.int_wpts = np.reshape(x[:nq], (self.D, self.M - 1))
        self.tau = x[nq:]
        self.ts = self.map_tau2T(self.tau)

    def _sync_params(self):
        cfg = PlannerConfig(v_max=self.v_max, T_min=self.T_min, T_max=self.T_max, safe_dis=self.safe_dis,
                            delta_t=self.delta_t, weights=self.weights,
                            collision_cost_tol=self.collision_cost_tol)
        _push_params(self.ctx, cfg, self.sample_dtype, self.stale_T, self.flags)

    def _launch_plan_once(self, wpts_list, ts):
        """one launch of len(wpts_list) trajectories that share head / tail / durations: (x, costs, last, nit, nfev, st)"""
        nb = len(wpts_list)
        nq = self.D * (self.M - 1)
        tau = self.map_T2tau(ts)
        x = np.stack([np.concatenate((np.reshape(_lib.as_f64(w), (nq,)), tau), axis=0) for w in wpts_list])
        x = np.ascontiguousarray(x, dtype=np.float64)
        self._sync_params()
        head, tail = self._ends(nb)
        res = _host_results(nb)
        self.ctx.call("neo_optimize_batch", self._scene, None, nb, self.M, self.D, *_ptrs(x, head, tail, *res))
        return (x, *res)

    def _ends(self, nb=1):
        """head and tail state as the ABI takes them: (nb, 3, D) float64, every row the planner's"""
        return [np.ascontiguousarray(np.broadcast_to(_lib.as_f64(s), (nb, 3, self.D))) for s in (self.head_state, self.tail_state)]

    def _finish_plan_once(self, x, costs, last, nit, nfev, st):
        """what plan_once does with the optimiser's answer (:226-237): exceptions first, then the side effects"""
        self.tau = self.map_T2tau(self.ts)
        code = int(st[0]) & 0xff
        self.last_status, self.last_nit, self.last_nfev = code, int(nit[0]), int(nfev[0])
        if code == _lib.NEO_TRAJ_NUMERIC_RANGE:
            raise OverflowError("math range error")          # what math.exp raises at :481
        if code == _lib.NEO_TRAJ_NONFINITE:
            # the reference leaves minimize() through Python-float overflow in the same situation
            # (e.g. (jerk)**2 at :382 once a line-search trial point blows the coefficients up)
            raise OverflowError(34, "Numerical result out of range")
        self._unpack_x(x[0])
        self.iter_num += int(nit[0])
        self.opt_running_times += 1
        self.costs = last[0].copy()                           # costs of the last evaluated x (:233)
        self.costs_at_x = costs[0].copy()
        self.weighted_cost = self.costs * self.weights
        self.final_cost = self.weighted_cost.sum()
        if self.weighted_cost[3] > self.collision_cost_tol:
            raise ValueError("collision cost too large")

    def plan_once(self):
        """expert_planner.py:205-237 -- the L-BFGS-B run happens in one kernel launch"""
        self._finish_plan_once(*self._launch_plan_once([self.int_wpts], self.ts))

    optimize = plan_once

    # ------------------------------------------------------------ callbacks (:539-585)
    def _device_eval(self, x, want_coeffs=True):
        self._sync_params()
        xx = _lib.as_f64(x).reshape(1, -1)
        head, tail = self._ends()
        cost, costs, grad, coeffs, st = out = _eval_arrays(1, xx.shape[1], self.M, self.D)
        self.ctx.call("neo_cost_grad_batch", self._scene, 1, self.M, self.D, *_ptrs(xx, head, tail, *out))
        if int(st[0]) == _lib.NEO_TRAJ_NUMERIC_RANGE:
            raise OverflowError("math range error")
        return cost[0], costs[0], grad[0], coeffs[0]

    def get_cost(self, x):
        x = np.asarray(x, dtype=np.float64)
        self._unpack_x(x)
        cost, self.costs, self._grad, self.coeffs = self._device_eval(x)
        return cost

    def get_grad(self, x):
        x = np.asarray(x, dtype=np.float64)
        self._unpack_x(x)
        _, _, grad, self.coeffs = self._device_eval(x)      # get_grad leaves self.costs alone (:572)
        return grad

    def get_coeffs(self, int_wpts, ts):
        """expert_planner.py:261-336 (coefficients only; the device never forms the 6M x 6M matrix)"""
        self.int_wpts, self.ts = int_wpts, ts
        self.tau = self.map_T2tau(np.asarray(ts, dtype=np.float64))
        _, self._eval_costs, _, self.coeffs = self._device_eval(self._pack_x())

    def reset_cost(self):
        self.costs = np.zeros(len(self.weights))

    # standalone use after get_coeffs(), as all_planner_demo.py:46-51 does
    def add_energy_cost(self):
        self.costs[0] += self._eval_costs[0]

    def add_time_cost(self):
        self.costs[1] += self._eval_costs[1]

    def add_sampled_cost(self):
        self.costs[2] += self._eval_costs[2]
        self.costs[3] += self._eval_costs[3]

    # ------------------------------------------------------------ time map (:468-483)
    def map_T2tau(self, ts):
        tau = np.zeros(self.M)
        for i in range(self.M):
            tau[i] = -math.log((self.T_max - self.T_min) / (ts[i] - self.T_min) - 1)
        return tau

    def map_tau2T(self, tau):
        ts = np.zeros(self.M)
        for i in range(self.M):
            ts[i] = (self.T_max - self.T_min) / (1 + math.exp(-tau[i])) + self.T_min
        return ts

    # ------------------------------------------------------------ evaluation (traj_utils.py:85-250)
    def _states(self, hz):
        ts = np.asarray(self.ts, dtype=np.float64)
        K = len(np.arange(0, sum(ts), 1 / hz))
        self.tau = self.map_T2tau(ts)
        x = _lib.as_f64(self._pack_x()).reshape(1, -1)
        state = np.zeros((1, max(K, 1), 3, self.D))
        cnt = np.zeros(1, np.int32)
        head, tail = self._ends()
        self._sync_params()
        c = self.ctx
        if K > 0:
            c.call("neo_eval_traj_batch", 1, self.M, self.D, _lib.ptr(x), _lib.ptr(head), _lib.ptr(tail), float(hz), K,
                   _lib.ptr(state), _lib.ptr(cnt))
        return state[0, :K]

    def get_full_state_cmd(self, hz=300):
        return self._states(hz)

    def audit(self, hz=10.0):
        """the reference's flight metric (traj_planner_node.py:333-363) of the current result (int_wpts, ts, head / tail)
        on the planner's map snapshot, sampled at `hz`: BatchPlanner.audit's dict for this one trajectory"""
        self.tau = self.map_T2tau(np.asarray(self.ts, dtype=np.float64))
        x = _lib.as_f64(self._pack_x()).reshape(1, -1)
        head, tail = self._ends()
        self._sync_params()
        record = _audit_arrays(1)
        self.ctx.call("neo_audit_traj_batch", self._scene, None, 1, self.M, self.D, _lib.ptr(x), _lib.ptr(head), _lib.ptr(tail),
                      float(hz), None, *_ptrs(*record))
        return _audit_result(*record)

    def get_pos_array(self):
        return self._states(10.0)[:, 0, :]       # np.arange(0, sum(ts), 0.1): 1/10.0 == 0.1

    def get_vel_array(self):
        return self._states(10.0)[:, 1, :]

    def get_acc_array(self):
        return self._states(10.0)[:, 2, :]

    # single-time evaluators (traj_utils.py:85-179).  Not on the hot path (visualisation helpers): plain
    # polynomial evaluation of the device-computed coefficients, with the reference's piece search.
    def _at(self, t, order):
        if isinstance(self.coeffs, list) and self.coeffs == []:
            self.get_coeffs(self.int_wpts, self.ts)
        total = sum(self.ts)
        if t > total:
            t = total
        k = 0
        while sum(self.ts[:k + 1]) < t:
            k += 1
        T = t - sum(self.ts[:k])
        beta = [np.array([1, T, T**2, T**3, T**4, T**5]), np.array([0, 1, 2*T, 3*T**2, 4*T**3, 5*T**4]),
                np.array([0, 0, 2, 6*T, 12*T**2, 20*T**3]), np.array([0, 0, 0, 6, 24*T, 60*T**2])][order]
        return np.dot(np.asarray(self.coeffs)[6 * k:6 * k + 6, :].T, beta)[None, :]

    def get_pos(self, t):
        return self._at(t, 0)

    def get_vel(self, t):
        return self._at(t, 1)

    def get_acc(self, t):
        return self._at(t, 2)

    def get_jerk(self, t):
        return self._at(t, 3)

    def get_jer_array(self):
        self.get_coeffs(self.int_wpts, self.ts)
        return np.concatenate([self.get_jerk(t) for t in np.arange(0, sum(self.ts), 0.1)], axis=0)

    def print_results(self):
        print("-----------------------Final intermediate waypoints-----------------------")
        print(np.asarray(self.int_wpts).T)
        print("-----------------------Final T--------------------------------------------")
        print(self.ts)
        self.weighted_cost = self.costs * self.weights
        print("Energy cost: %f, Time cost: %f, Feasibility cost: %f, Collision cost: %f" % tuple(self.weighted_cost))


class BatchPlanner:
    """B independent replans per call (host arrays in, host arrays out).  For device-resident
    buffers use `optimize_dev` with torch tensors."""

    def __init__(self, config=None, ctx=None, sample_dtype="f64", stale_T=True, waves_per_simd=None, lane_groups=False):
        """waves_per_simd: None (the library decides by batch size), 1 (shortest evaluations) or 2 (highest
        throughput when several batches are in flight) -- include/neo_planner.h NEO_FLAG_*; same results.
        sample_dtype: "f64" (parity mode), "f32" (fp32 sampled terms, fp64 solve and optimiser) or "f32x" (everything
        in fp32, NEO_FLAG_F32_SOLVE: 3-D fields and the reference's 2-D map)"""
        self.cfg = config if config is not None else PlannerConfig()
        self._ctx = ctx
        self.all_f32 = sample_dtype == "f32x"
        if self.all_f32:
            sample_dtype = "f32"
        self.sample_dtype = sample_dtype
        self.stale_T = stale_T
        self.flags = {None: 0, 1: _lib.NEO_FLAG_ONE_WAVE_PER_SIMD, 2: _lib.NEO_FLAG_TWO_WAVES_PER_SIMD}[waves_per_simd]
        if lane_groups:     # small problems: eight trajectories per wavefront (NEO_FLAG_LANE_GROUPS; fp32-rounding-level
            self.flags |= _lib.NEO_FLAG_LANE_GROUPS   # differences to the default kernel)
        if self.all_f32:
            self.flags |= _lib.NEO_FLAG_F32_SOLVE

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = _lib.default_context()
        return self._ctx

    def _sync(self):
        _push_params(self.ctx, self.cfg, self.sample_dtype, self.stale_T, self.flags)

    def _start_ts(self, count):
        """the start durations of `count` waypoints: init_T * [1.5, 1, ..., 1, 1.5] (:97-99).  Durations only: who maps them
        to tau, and through which log, is the caller's business (pack_x / _plan_frac_tau: np.log; _batch_ts_tau: math.log)"""
        ts = float(self.cfg.init_T) * np.ones((count + 1,))
        ts[0] *= 1.5
        ts[-1] *= 1.5
        return ts

    def pack_x(self, int_wpts, ts):
        """int_wpts (B, D, M-1), ts (B, M) -> x (B, n) with tau = map_T2tau(ts) (:468-475)"""
        B = ts.shape[0]
        tau = -np.log((self.cfg.T_max - self.cfg.T_min) / (ts - self.cfg.T_min) - 1.0)
        return np.concatenate([np.asarray(int_wpts, dtype=np.float64).reshape(B, -1), tau], axis=1)

    def unpack_x(self, x, M, D):
        B = x.shape[0]
        nq = D * (M - 1)
        ts = (self.cfg.T_max - self.cfg.T_min) / (1.0 + np.exp(-x[:, nq:])) + self.cfg.T_min
        return x[:, :nq].reshape(B, D, M - 1), ts

    def cost_grad(self, map, x, head, tail, want_coeffs=False):
        self._sync()
        x, head, tail = _f64(x, head, tail)
        B, M, D, n = _shape(x, head)
        out = _eval_arrays(B, n, M, D, want_coeffs)
        self.ctx.call("neo_cost_grad_batch", map.scene_id, B, M, D, *_ptrs(x, head, tail, *out))
        return dict(zip(("cost", "costs", "grad", "coeffs", "status"), out))

    def sampled_terms(self, map, coeffs, ts, order=None, io32=False):
        """add_sampled_cost + add_sampled_grad_CT (:392-466) for B trajectories: coeffs (B, 6M, D), ts (B, M).
        `order`: optional permutation (B,) the ESDF-lookup kernel dispatches its workgroups in (`spatial_order`); the
        results stay in the caller's order, bit-identical.  `io32`: hand the coefficients over and take the partials back
        as float32 (neo_sampled_terms_batch_f32; fp32 sampling only)"""
        self._sync()
        c = self.ctx
        ts = _lib.as_f64(ts)
        B, M = ts.shape
        D = np.shape(coeffs)[2]
        perm = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
        c.call("neo_sampled_terms_dispatch_order", _lib.ptr(perm), 0, 0 if perm is None else B)
        costs2 = np.zeros((B, 2))
        io = np.float32 if io32 else np.float64
        coeffs = np.ascontiguousarray(coeffs, dtype=io)
        gC = np.zeros((B, 6 * M, D), io); gT = np.zeros((B, M), io)
        c.call("neo_sampled_terms_batch_f32" if io32 else "neo_sampled_terms_batch", map.scene_id, B, M, D,
               *_ptrs(coeffs, ts, costs2, gC, gT))
        return dict(costs2=costs2, grad_C=gC, grad_T=gT)

    def optimize(self, map, x0, head, tail, scene_ids=None, order=True):
        """map: one map for all trajectories (scene_ids None) or any map of the right kind plus
        scene_ids (B,) int32 of per-trajectory scene ids.  `order`: start the runs expected to be long
        first (`expected_effort_order`); results are in the caller's order either way."""
        self._sync()
        c = self.ctx
        x = _lib.as_f64(x0).copy()
        head, tail = _f64(head, tail)
        B, M, D, _ = _shape(x, head)
        perm = None
        if order and B > 1024:
            _, ts0 = self.unpack_x(x, M, D)
            perm = self.expected_effort_order(head, tail, ts0)
        c.call("neo_optimize_dispatch_order_host", _lib.ptr(perm), 0 if perm is None else B)
        res = _host_results(B)
        c.call("neo_optimize_batch", map.scene_id, _lib.ptr(_scene_ids(scene_ids)), B, M, D, *_ptrs(x, head, tail, *res))
        return _result_dict(x, res, self.cfg.weights)

    def audit(self, map, x, head, tail, hz=10.0, scene_ids=None, weights=None):
        """the reference's flight metric (traj_planner_node.py:333-363, get_weighted_metric) of B trajectories x (B, n)
        under perfect tracking, sampled at `hz` (10: its metric_eva_interval of 0.1 s).  scene_ids as in `optimize`;
        weights: the three metric weights (None: the reference's [1, 1, 100]).  Returns a dict of (B,) arrays: the ten
        record fields by name (path_length, feasibility, collision, weighted, min_clearance, t_min_clearance, max_speed,
        max_acc, t_first_unsafe, duration), count, flags (NEO_AUDIT_FLAG_*) and the masks unsafe / metric_fail"""
        self._sync()
        x, head, tail = _f64(x, head, tail)
        B, M, D, _ = _shape(x, head)
        record = _audit_arrays(B)
        self.ctx.call("neo_audit_traj_batch", map.scene_id, _lib.ptr(_scene_ids(scene_ids)), B, M, D, _lib.ptr(x), _lib.ptr(head),
                      _lib.ptr(tail), float(hz), _lib.ptr(_audit_weights(weights)), *_ptrs(*record))
        return _audit_result(*record)

    def audit_dev(self, map, x, head, tail, audit, count, flags, hz=10.0, slots=None, weights=None):
        """`audit` on device tensors, asynchronous on the context's stream: x (B, n), head / tail (B, 3, D) float64,
        results into audit (B, NEO_AUDIT_FIELDS) float64, count and flags (B,) int32 -- e.g. straight on optimize_dev's
        results.  `slots`: optional int32 device tensor of map-table slots, as in optimize_dev"""
        self._sync()
        B, M, D, _ = _shape(x, head)
        p = _lib.dev_ptr
        self.ctx.call("neo_audit_traj_batch_dev", map.scene_id, p(slots), B, M, D, p(x), p(head), p(tail), float(hz),
                      _lib.ptr(_audit_weights(weights)), p(audit), p(count), p(flags))

    def geo_init(self, map, start, target, scene_ids=None, max_expansions=0, path_cap=0):
        """the reference's `geo` warm start (geo_planner.py:19-35) for B requests on 2-D maps: AstarPlanner.plan from
        start (B, 2) to target (B, 2), prune_path_nodes, then int_wpts = pruned[1:3].T and ts = init_T * [1.5, 1, 1.5]
        (neo_geo_search_batch; every value equal to the reference's).  scene_ids as in `optimize`.  max_expansions > 0
        caps each search (CAPPED flag; such a result is not the reference's).  Returns a dict: int_wpts (B, 2, 2) and
        ts (B, 3) ready for `plan`, key_pts (B, 4, 2), path_len, path_cost, expansions, flags (NEO_GEO_FLAG_*), the
        masks no_path / capped, and paths (B, path_cap, 2) when path_cap > 0"""
        c = self.ctx
        start = _lib.as_f64(start).reshape(-1, 2); target = _lib.as_f64(target).reshape(-1, 2)
        B = start.shape[0]
        if target.shape[0] != B:
            raise ValueError("BatchPlanner.geo_init: start and target need the same number of requests")
        key_pts = np.zeros((B, 4, 2)); cost = np.zeros(B)
        plen = np.zeros(B, np.int32); nexp = np.zeros(B, np.int32); flags = np.zeros(B, np.int32)
        paths = np.zeros((B, path_cap, 2)) if path_cap > 0 else None
        c.call("neo_geo_search_batch", map.scene_id, _lib.ptr(_scene_ids(scene_ids)), B, _lib.ptr(start), _lib.ptr(target),
               int(max_expansions), int(path_cap), *_ptrs(key_pts, paths, plen, cost, nexp, flags))
        out = dict(int_wpts=key_pts[:, 1:3, :].transpose(0, 2, 1).copy(), ts=np.tile(self._start_ts(2), (B, 1)),
                   key_pts=key_pts, path_len=plen,
                   path_cost=cost, expansions=nexp, flags=flags, no_path=(flags & _lib.NEO_GEO_FLAG_NO_PATH) != 0,
                   capped=(flags & _lib.NEO_GEO_FLAG_CAPPED) != 0)
        if paths is not None:
            out["paths"] = paths
        return out

    def geo_init_dev(self, map, start, target, key_pts, path_len, path_cost, expansions, flags, slots=None,
                     max_expansions=0, paths=None):
        """`geo_init`'s search on device tensors, asynchronous on the context's stream: start / target (B, 2) float64,
        results into key_pts (B, 4, 2), path_cost (B,) float64, path_len, expansions, flags (B,) int32 and, when given,
        paths (B, path_cap, 2) float64.  `slots`: optional int32 device tensor of map-table slots, as in optimize_dev"""
        c = self.ctx
        p = _lib.dev_ptr
        B = start.shape[0]
        cap = 0 if paths is None else paths.shape[1]
        c.call("neo_geo_search_batch_dev", map.scene_id, p(slots), B, p(start), p(target), int(max_expansions), cap,
               p(key_pts), p(paths), p(path_len), p(path_cost), p(expansions), p(flags))

    def geo_prune(self, map, paths, path_len=None, scene_ids=None):
        """GeoPlanner.prune_path_nodes (geo_planner.py:61-101) of B given paths: paths (B, L, 2) (the first path_len[b]
        nodes of row b; all L without path_len) -> key_pts (B, 4, 2)"""
        c = self.ctx
        paths = _lib.as_f64(paths)
        B, L = paths.shape[0], paths.shape[1]
        plen = np.full(B, L, np.int32) if path_len is None else np.ascontiguousarray(path_len, dtype=np.int32)
        key_pts = np.zeros((B, 4, 2))
        c.call("neo_geo_prune_batch", map.scene_id, _lib.ptr(_scene_ids(scene_ids)), B, _lib.ptr(paths), _lib.ptr(plen), L,
               _lib.ptr(key_pts))
        return key_pts

    def geo_plan(self, map, head, tail, scene_ids=None, max_expansions=0, **kw):
        """`geo_init` from head[:, 0] to tail[:, 0], then `plan(int_wpts=..., ts=...)`: the reference's geo_traj_plan
        (geo_planner.py:19-35) for a batch of 2-D requests head / tail (B, 2, 2).  Retries re-seed from straight lines,
        as the reference's warm_start_plan does after a geo start.  `plan`'s dict plus the search's results under
        "geo" """
        head, tail = _f64(head, tail)
        g = self.geo_init(map, head[:, 0, :2], tail[:, 0, :2], scene_ids=scene_ids, max_expansions=max_expansions)
        out = self.plan(map, head, tail, int_wpts=g["int_wpts"], ts=g["ts"], scene_ids=scene_ids, **kw)
        out["geo"] = g
        return out

    def optimize_budgeted_dev(self, map, x0, x, head, tail, costs, costs_last, nit, nfev, status, state, eval_budget,
                              max_launches=4096):
        """optimize_dev with an evaluation budget per launch (neo_optimize_batch_budget_dev): the first launch gives every
        trajectory `eval_budget` evaluations, then the trajectories still running (status NEO_TRAJ_SUSPENDED) are
        re-launched COMPACTED -- one workgroup per straggler -- until none is left.  Finished results are valid as soon as
        their launch has ended; the finals are bit for bit those of `optimize_dev`.  torch CUDA tensors; `state` a uint8
        tensor of B * neo_optimize_state_bytes(M, D) bytes.  Returns the launch sizes."""
        import torch
        self._sync()
        c = self.ctx
        B, M, D, _ = _shape(x, head)
        pp = _lib.dev_ptr
        sizes = []
        subset, resume = None, 0
        for _ in range(max_launches):
            c.call("neo_optimize_batch_budget_dev", map.scene_id, B, M, D,
                   *_dev_ptrs(x0, x, head, tail, costs, costs_last, nit, nfev, status, state), int(eval_budget), pp(subset),
                   0 if subset is None else int(subset.numel()), resume)
            sizes.append(_lib.launch_count(subset, B))
            c.synchronize()
            # (the statuses decide the next launch: this is the host round trip a budget costs)
            subset = torch.nonzero(status == _lib.NEO_TRAJ_SUSPENDED).flatten().to(torch.int32)
            resume = 1
            if subset.numel() == 0:
                return sizes
        raise RuntimeError(f"{int(subset.numel())} trajectories still suspended after {max_launches} launches")

    def optimize_budgeted(self, map, x0, head, tail, eval_budget):
        """host-array form of optimize_budgeted_dev: the dict of `optimize` plus `launch_sizes`"""
        import torch
        c = self.ctx
        dev = torch.device("cuda", c.device)
        x0, head, tail = _f64(x0, head, tail)
        B, M, D, _ = _shape(x0, head)
        d_x0, d_h, d_t = _upload(dev, x0, head, tail)
        d_x = torch.empty_like(d_x0)
        res = _dev_results(B, dev)
        state = torch.empty(B * int(c.lib.neo_optimize_state_bytes(M, D)), dtype=torch.uint8, device=dev)
        _torch_done(dev)
        sizes = self.optimize_budgeted_dev(map, d_x0, d_x, d_h, d_t, *res, state, eval_budget)
        return dict(_result_dict(d_x.cpu().numpy(), [r.cpu().numpy() for r in res], self.cfg.weights), launch_sizes=sizes)

    def optimize_progressive(self, map, x0, head, tail, shares=(0.8,)):
        """`optimize` as a generator that hands results over as they finish (round 6, neo_optimize_progress_counter): ONE plain
        launch; the host polls the launch's counter of finished trajectories through a side stream and, each time it passes
        the next share of the batch, copies status first and then the results -- what status marks finished is final.
        Yields (indices, dict) -- indices int64 of the trajectories first seen finished, dict with their x, costs, costs_last,
        nit, nfev, status, collision, final_cost -- once per share and once more for the rest when the launch has ended.
        Every trajectory is yielded exactly once, with the bits `optimize` returns for it."""
        import torch
        c = self.ctx
        self._sync()
        dev = torch.device("cuda", c.device)
        x0, head, tail = _f64(x0, head, tail)
        B = x0.shape[0]
        d_x0, d_h, d_t = _upload(dev, x0, head, tail)
        bufs = dict(zip(RESULTS, _dev_results(B, dev)), x=torch.empty_like(d_x0))
        bufs["status"].fill_(-1)        # (no trajectory has finished)
        host = {k: torch.empty(tuple(v.shape), dtype=v.dtype).pin_memory() for k, v in bufs.items()}
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        h_cnt = torch.zeros(1, dtype=torch.int32).pin_memory()
        side = torch.cuda.Stream(device=dev)
        _torch_done(dev)
        seen = np.zeros(B, dtype=bool)

        def snapshot():
            with torch.cuda.stream(side):
                for k in ["status"] + [k_ for k_ in bufs if k_ != "status"]:     # status FIRST (include/neo_planner.h)
                    host[k].copy_(bufs[k], non_blocking=True)
                    side.synchronize()
            st = host["status"].numpy()
            new = np.flatnonzero((st != -1) & ~seen)
            seen[new] = True
            return new, _result_dict(host["x"].numpy()[new], [host[k].numpy()[new] for k in RESULTS], self.cfg.weights)

        try:
            self.optimize_dev(map, bufs["x"], d_h, d_t, *(bufs[k] for k in RESULTS), x0=d_x0, progress=counter)
            for share in sorted(float(s_) for s_ in shares):
                need = min(B, int(np.ceil(share * B)))
                while True:
                    with torch.cuda.stream(side):
                        h_cnt.copy_(counter, non_blocking=True)
                        side.synchronize()
                    if int(h_cnt[0]) >= need:
                        break
                new, res = snapshot()
                if new.size:
                    yield new, res
            c.synchronize()
            new, res = snapshot()
            if new.size:
                yield new, res
        finally:
            c.synchronize()
            c.call("neo_optimize_progress_counter", None)

    def init_guess(self, head, tail, count, rng=None, noise=0.0):
        """generate_init_variables (:82-101) for a batch: `count` waypoints on the straight line from start to target,
        durations init_T with the first and last piece 1.5 times as long; noise > 0 adds the N(0, noise) jitter of the
        reference's re-seeded attempts (:94; a numpy Generator here, the reference draws from the global RNG)"""
        head = np.asarray(head, dtype=np.float64); tail = np.asarray(tail, dtype=np.float64)
        start, target = head[:, 0], tail[:, 0]
        f = (np.arange(1, count + 1) / (count + 1))[None, None, :]
        wp = start[:, :, None] + (target - start)[:, :, None] * f                     # (B, D, count)
        if noise > 0.0:
            wp = wp + (rng if rng is not None else np.random.default_rng()).normal(0.0, noise, wp.shape)
        return wp, np.tile(self._start_ts(count), (head.shape[0], 1))

    @staticmethod
    def retry_noise(seed, stream_ids, attempt, D, count):
        """the N(0, 0.5) waypoint jitter (:94) of `plan`'s re-seeded attempt `attempt` for the requests with the streams
        `stream_ids`: request i draws (D, count) values from its OWN stream SeedSequence(seed, i, attempt)"""
        return np.stack([np.random.default_rng([int(seed), int(i), int(attempt)]).normal(0.0, 0.5, (D, count))
                         for i in stream_ids])

    @staticmethod
    def retry_noise_counter(seed, stream_ids, attempt, D, count):
        """`retry_noise` from the counter-based streams (counter_rng.py, the model of csrc/neo_counter_rng.hpp): request i's
        (D, count) block is 0.5 * the unit normals (seed, i, attempt, value d * count + k) -- a pure function of those, so
        neo_plan_jitter_dev draws the same bits on the device.  seed in 0 .. 2^64 - 1, ids in 0 .. 2^31 - 1."""
        return counter_rng.retry_noise(seed, stream_ids, attempt, D, count)

    def plan(self, map, head, tail, int_wpts=None, ts=None, waypoints=None, max_attempts=5, rng=None, scene_ids=None,
             seed=None, return_launch_sizes=False, stream_ids=None, jitter="numpy", max_waypoints=63):
        """warm_start_plan (:186-203) for a batch: every request gets up to `max_attempts` plan_once runs.  An attempt that
        ends the way the reference raises on -- OverflowError statuses or `collision cost too large` (:235-237) -- is
        re-seeded like the reference's retries (straight line + N(0, 0.5), :94, :201) and optimised again; only the
        failed requests are launched again (compacted re-launches).  The jitter of request i at attempt a comes from its
        OWN stream, SeedSequence(seed, i, a): a retry does not depend on which other requests of the batch failed, as the
        reference's warm_start_plan of one request does not depend on other requests (`seed`: an int; None draws one from
        `rng` or from the OS).  `stream_ids` (B,): the i of each request's streams in place of its position in the batch
        (None: the position) -- a caller that plans a changing subset of longer-lived requests (FleetReplanLoop: missions)
        passes their ids, so that a request's retries do not depend on who else is in the batch.  jitter="counter" draws
        the retries from `retry_noise_counter` instead (still on the host here: the oracle of plan_dev(jitter="counter"));
        a seed outside 0 .. 2^64 - 1 or an id outside 0 .. 2^31 - 1 then raises ValueError.  Returns the optimiser's
        dict plus `attempts` (B,), `nit_total` (B,: L-BFGS iterations over all attempts that ran to an answer, what the
        reference's planner.iter_num accumulates) and `solved` (B,): a request with solved False is one the reference
        answers with Exception("No solution for the given target").
        waypoints="adaptive": every request its own number of waypoints (`adaptive_counts`, at most `max_waypoints`), see
        `_plan_adaptive` for the ragged dict that comes back."""
        if isinstance(waypoints, str):
            return self._plan_adaptive(map, head, tail, int_wpts, ts, waypoints, max_attempts, rng, scene_ids, seed,
                                       return_launch_sizes, stream_ids, jitter, max_waypoints)
        if (int_wpts is None) != (ts is None):
            raise ValueError("BatchPlanner.plan: give both int_wpts and ts, or neither")
        counter = counter_rng.check_jitter(jitter, "BatchPlanner.plan")
        head, tail = _f64(head, tail)
        B, D = head.shape[0], head.shape[2]
        if counter:         # (before any device use)
            if seed is not None:
                seed = counter_rng.check_seed(seed, "BatchPlanner.plan")
            if stream_ids is not None:
                counter_rng.check_ids(stream_ids, "BatchPlanner.plan")
        draw = self.retry_noise_counter if counter else self.retry_noise
        if int_wpts is None:
            int_wpts, ts = self.init_guess(head, tail, waypoints if waypoints is not None else int(self.cfg.init_wpts_num))
        count = np.asarray(int_wpts).shape[2]
        out = self.optimize(map, self.pack_x(int_wpts, ts), head, tail, scene_ids=scene_ids)
        if np.any(out["status"] == _lib.NEO_TRAJ_BAD_SCENE):
            # not a planning failure: the request named a map-table slot that does not exist -- retrying cannot help
            raise _lib.NeoError("BatchPlanner.plan: requests %s name a scene without a map (NEO_TRAJ_BAD_SCENE)"
                                % np.flatnonzero(out["status"] == _lib.NEO_TRAJ_BAD_SCENE)[:8].tolist())
        out["attempts"] = np.ones(B, dtype=np.int32)
        stream_ids = _stream_ids(stream_ids, B, "BatchPlanner.plan")
        # (an attempt that overflowed raises before the reference counts it: expert_planner.py:226-232)
        counted = lambda r: np.where(r["status"] >= _lib.NEO_TRAJ_NUMERIC_RANGE, 0, r["nit"]).astype(np.int64)
        out["nit_total"] = counted(out)
        failed = lambda r: ((r["status"] > _lib.NEO_TRAJ_MAXITER) & (r["status"] != _lib.NEO_TRAJ_BAD_SCENE)) | r["collision"]
        todo = np.flatnonzero(failed(out))
        if seed is None:
            seed = _draw_seed(rng)
        launches = [B]
        for attempt in range(1, max_attempts):
            if todo.size == 0:
                break
            noise = draw(seed, stream_ids[todo], attempt, D, count)
            wp_n, ts_n = self.init_guess(head[todo], tail[todo], count)
            r = self.optimize(map, self.pack_x(wp_n + noise, ts_n), head[todo], tail[todo],
                              scene_ids=None if scene_ids is None else np.asarray(scene_ids)[todo])
            launches.append(int(todo.size))
            for k in ("x", "costs", "costs_last", "nit", "nfev", "status", "collision", "final_cost"):
                out[k][todo] = r[k]
            out["attempts"][todo] += 1
            out["nit_total"][todo] += counted(r)
            todo = todo[failed(r)]
        out["solved"] = ~failed(out)
        if return_launch_sizes:
            out["launch_sizes"] = launches
        return out

    # ------------------------------------------------------------ adaptive waypoint counts (:86-88) for a batch
    def _adaptive_args(self, max_waypoints, who):
        """init_seg_len as a float, after the checks of `adaptive_counts` (before any device use)"""
        if int(max_waypoints) != max_waypoints or not 1 <= max_waypoints <= _lib.NEO_MAX_PIECES - 1:
            raise ValueError("%s: max_waypoints must be in 1 .. %d" % (who, _lib.NEO_MAX_PIECES - 1))
        seg = float(self.cfg.init_seg_len)
        if not (math.isfinite(seg) and seg > 0.0):
            raise ValueError("%s: init_seg_len must be finite and > 0" % who)
        return seg

    def adaptive_counts(self, head, tail, max_waypoints=63):
        """the reference's adaptive waypoint count (generate_init_variables, :86-88) for B requests: one waypoint per
        init_seg_len metres of straight-line distance, max(ceil(L / init_seg_len - 1), 1).  head / tail (B, >= 1, D), D =
        2 or 3.  Every operation is rounded on its own, in this order -- the definition adaptive_count_kernel restates:
        d_k = tail[0][k] - head[0][k]; s = d_0 * d_0 + d_1 * d_1 (+ d_2 * d_2) from left to right; L = sqrt(s);
        c = ceil(L / init_seg_len - 1.0); count = max(c, 1).  A non-finite L gives 1 (the optimiser reports such a request
        as it does today); a count above `max_waypoints` becomes max_waypoints with `clamped` set.
        Returns (counts int32 (B,), clamped bool (B,))."""
        seg = self._adaptive_args(max_waypoints, "BatchPlanner.adaptive_counts")
        head = np.asarray(head, dtype=np.float64); tail = np.asarray(tail, dtype=np.float64)
        if head.ndim != 3 or head.shape[2] not in (2, 3) or tail.shape[0] != head.shape[0] or tail.shape[2] != head.shape[2]:
            raise ValueError("BatchPlanner.adaptive_counts: head and tail (B, 3, D), D = 2 or 3")
        with np.errstate(all="ignore"):
            d = tail[:, 0] - head[:, 0]
            s = d[:, 0] * d[:, 0]
            for k in range(1, d.shape[1]):
                s = s + d[:, k] * d[:, k]
            L = np.sqrt(s)
            c = np.ceil(L / seg - 1.0)
        finite = np.isfinite(L)
        clamped = finite & (c > max_waypoints)
        counts = np.where(finite, np.minimum(np.maximum(c, 1.0), float(max_waypoints)), 1.0)
        return counts.astype(np.int32), clamped

    @staticmethod
    def adaptive_groups(result, rows=None):
        """the ragged result of plan / plan_dev(waypoints="adaptive") group by group, for eval_traj, audit and every
        other consumer of one M: yields (count, indices (k,), x_dense (k, n)) by ascending count, indices ascending, n =
        D * count + count + 1 the group's own row length (D from the row length of `x` and the buffers' max_waypoints).
        `result`: the dict of either form (NumPy arrays or torch tensors).  `rows`: the request indices to look at
        (None: all) -- after a plan_dev over a subset, the subset."""
        host = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
        counts, x = host(result["counts"]), host(result["x"])
        W = int(result["max_waypoints"])
        D = (x.shape[1] - 1) // W - 1
        if D * W + W + 1 != x.shape[1]:
            raise ValueError("BatchPlanner.adaptive_groups: x is not (B, D * max_waypoints + max_waypoints + 1)")
        rows = np.arange(counts.shape[0]) if rows is None else np.sort(np.asarray(rows).reshape(-1))
        for c in np.unique(counts[rows]):
            if not 1 <= c <= W:
                raise ValueError("BatchPlanner.adaptive_groups: a count outside 1 .. max_waypoints (rows= names the planned requests)")
            idx = rows[counts[rows] == c]
            yield int(c), idx, np.ascontiguousarray(x[idx, :D * int(c) + int(c) + 1])

    def _plan_adaptive(self, map, head, tail, int_wpts, ts, waypoints, max_attempts, rng, scene_ids, seed,
                       return_launch_sizes, stream_ids, jitter, max_waypoints):
        """plan(waypoints="adaptive"), the host form and plan_dev's oracle: `adaptive_counts`, a stable grouping by
        count, `plan` per group with the group's count -- a request's streams are its own, so its retries are those of the
        request planned alone -- and the groups' results in one RAGGED dict: x (B, n_max), n_max = D * max_waypoints +
        max_waypoints + 1, request b's row its n_b = D * count_b + count_b + 1 values [q row-major ; tau], then NaN; the
        other arrays of `plan` by request; counts, clamped (`adaptive_counts`) and max_waypoints; launch_sizes
        (requests launched per attempt over all groups) and group_launch_sizes {count: sizes per attempt}."""
        if waypoints != "adaptive":
            raise ValueError("BatchPlanner.plan: waypoints is a number, None or 'adaptive'")
        if int_wpts is not None or ts is not None:
            raise ValueError("BatchPlanner.plan: int_wpts / ts fix their own shape: not with waypoints='adaptive'")
        self._adaptive_args(max_waypoints, "BatchPlanner.plan")
        counter = counter_rng.check_jitter(jitter, "BatchPlanner.plan")
        head, tail = _f64(head, tail)
        B, D = head.shape[0], head.shape[2]
        W = int(max_waypoints)
        counts, clamped = self.adaptive_counts(head, tail, W)
        if counter and seed is not None:
            seed = counter_rng.check_seed(seed, "BatchPlanner.plan")
        if seed is None:        # (one seed for every group)
            seed = _draw_seed(rng)
        stream_ids = _stream_ids(stream_ids, B, "BatchPlanner.plan")
        order = np.argsort(counts, kind="stable")
        out = dict(x=np.full((B, D * W + W + 1), np.nan), counts=counts, clamped=clamped, max_waypoints=W)
        launches, by_group = [], {}
        for c in np.unique(counts):
            g = order[counts[order] == c]
            r = self.plan(map, head[g], tail[g], waypoints=int(c), max_attempts=max_attempts, seed=seed, jitter=jitter,
                          scene_ids=None if scene_ids is None else np.asarray(scene_ids)[g], stream_ids=stream_ids[g],
                          return_launch_sizes=True)
            sizes = by_group[int(c)] = r.pop("launch_sizes")
            launches += [0] * (len(sizes) - len(launches))
            for a, k in enumerate(sizes):
                launches[a] += k
            xg = r.pop("x")
            out["x"][g, :xg.shape[1]] = xg
            for k, v in r.items():
                if k not in out:
                    out[k] = np.zeros((B,) + v.shape[1:], dtype=v.dtype)
                out[k][g] = v
        if return_launch_sizes:
            out.update(launch_sizes=launches, group_launch_sizes=by_group)
        return out

    # ------------------------------------------------------------ `plan` on resident arrays
    def _plan_frac_tau(self, count):
        """what neo_plan_guess takes from the host: init_guess's fractions f[k] = k / (count + 1) and the tau of its
        durations -- through pack_x's own expression (np.log: math.log may differ in the last bit)"""
        frac = np.arange(1, count + 1) / (count + 1)
        return frac, np.ascontiguousarray(self.pack_x(np.zeros((1, 1, count)), self._start_ts(count)[None])[0, count:])

    def warm_guess_dev(self, head, wpts_local, ts_carry, x0, subset=None):
        """the reference's `warmstart` planner on resident tensors (neo_fleet_warm_guess_dev, asynchronous on the
        context's stream): x0 (B, n) float64, plan_dev's first guess, from what the requests carry -- wpts_local
        (B, 2, M - 1), the last solved plan's waypoints relative to where that plan started, moved to head (B, 3, 2)'s
        position, and ts_carry (B, M), the durations held, through map_T2tau; a duration map_T2tau raises for gives a NaN
        tau, which plan_dev answers by re-seeding.  `subset`: an int32 tensor of request indices (None: all B).
        Returns x0."""
        self._sync()
        B, M = int(ts_carry.shape[0]), int(ts_carry.shape[1])
        if tuple(head.shape) != (B, 3, 2) or tuple(wpts_local.shape) != (B, 2, M - 1) or tuple(x0.shape) != (B, 3 * M - 2):
            raise ValueError("BatchPlanner.warm_guess_dev: head (B, 3, 2), wpts_local (B, 2, M - 1), ts_carry (B, M), x0 (B, 3 M - 2)")
        p = _lib.dev_ptr
        self.ctx.call("neo_fleet_warm_guess_dev", B, p(subset), _lib.launch_count(subset, B), M, p(head), p(wpts_local), p(ts_carry),
                      p(x0))
        return x0

    def warm_carry_dev(self, x, head, solved, status, attempts, wpts_local, ts_carry, subset=None):
        """what the requests keep of a plan call for the next warm start (neo_fleet_warm_carry_dev, asynchronous on the
        context's stream): x (B, n) and head (B, 3, 2) of the call, solved, status and attempts (B,) int32 as plan_dev
        leaves them, into wpts_local (B, 2, M - 1) and ts_carry (B, M).  A solved request keeps the plan's waypoints relative
        to head's position and its durations; an unsolved one keeps its waypoints, and the durations of the last attempt's
        answer or, where that attempt raised, its start durations (include/neo_planner.h)."""
        self._sync()
        B, M = int(ts_carry.shape[0]), int(ts_carry.shape[1])
        if tuple(head.shape) != (B, 3, 2) or tuple(wpts_local.shape) != (B, 2, M - 1) or tuple(x.shape) != (B, 3 * M - 2):
            raise ValueError("BatchPlanner.warm_carry_dev: x (B, 3 M - 2), head (B, 3, 2), wpts_local (B, 2, M - 1), ts_carry (B, M)")
        p = _lib.dev_ptr
        init_ts = self._batch_ts_tau(M - 1)[0]      # a re-seeded attempt's start durations
        self.ctx.call("neo_fleet_warm_carry_dev", B, p(subset), _lib.launch_count(subset, B), M, p(x), p(head), p(solved), p(status),
                      p(attempts), _lib.ptr(init_ts), p(wpts_local), p(ts_carry))

    def plan_buffers(self, B, device, D=2, waypoints=None, max_waypoints=63):
        """the resident arrays of `plan_dev` for up to B requests of dimension D with `waypoints` waypoints (None: the
        config's init_wpts_num): the packed work arrays of an attempt's launch, the two launch lists, and the
        request-indexed results (torch tensors, zeroed).  waypoints="adaptive": the same arrays sized for `max_waypoints`
        (x: rows of n_max), plus the request-indexed counts and clamped, the grouped list `group_order` and the group
        `table` the host reads (bucket_begin, the groups' failed counts, the bad-scene word, the total)"""
        import torch
        adaptive = isinstance(waypoints, str)
        if adaptive:
            if waypoints != "adaptive":
                raise ValueError("BatchPlanner.plan_buffers: waypoints is a number, None or 'adaptive'")
            self._adaptive_args(max_waypoints, "BatchPlanner.plan_buffers")
            waypoints = max_waypoints
        count = int(waypoints if waypoints is not None else self.cfg.init_wpts_num)
        R = max(B, 1)
        bufs, f, i = _work_buffers(device, dict(B=B, D=D, M=count + 1), R, B, D * count + count + 1, D)
        bufs.update(noise=f(R, D, count), todo=i(2, R), counts=i(2), attempts=i(B),
                    nit_total=torch.zeros(B, dtype=torch.int64, device=device), launch_sizes=[])
        if B > 1024:        # (launches this large are dispatched longest-expected first, as `optimize` does)
            nbytes = int(_lib.load().neo_effort_order_scratch_bytes(B))
            bufs.update(order=i(B), order_scratch=f(nbytes // 8 + 1))
        if adaptive:
            G = _lib.NEO_MAX_PIECES
            bufs.update(adaptive=True, max_waypoints=count, counts=i(B), clamped=i(B), group_order=i(R), table=i(2 * G + 3),
                        group_launch_sizes={}, host_waits={})
        return bufs

    @staticmethod
    def _plan_dev_streams(stream_ids, head, counter, seed):
        """plan_dev's stream ids and seed, checked before any device use: (the host array or None, the device tensor or
        None, the seed)"""
        import torch
        B = head.shape[0]
        ids_dev = None
        if counter and isinstance(stream_ids, torch.Tensor):
            if stream_ids.dtype != torch.int32 or stream_ids.device != head.device or stream_ids.numel() != B or \
                    not stream_ids.is_contiguous():
                raise ValueError("BatchPlanner.plan_dev: a device stream_ids is a contiguous int32 tensor, one id per request")
            ids_dev = stream_ids
        else:
            stream_ids = _stream_ids(stream_ids, B, "BatchPlanner.plan_dev")
        if counter:
            if seed is not None:
                seed = counter_rng.check_seed(seed, "BatchPlanner.plan_dev")
            if ids_dev is None:
                stream_ids = counter_rng.check_ids(stream_ids, "BatchPlanner.plan_dev").astype(np.int32)
        return stream_ids, ids_dev, seed

    def plan_dev(self, map, head, tail, bufs=None, x0=None, slots=None, subset=None, x=None, solved=None, max_attempts=5,
                 seed=None, rng=None, stream_ids=None, waypoints=None, _guessed=False, jitter="numpy", max_waypoints=63):
        """`plan` on RESIDENT torch tensors, every returned array bit for bit `plan`'s: head / tail (B, 3, D) float64 by
        request; `x0` (B, n) an optional first guess by request (plan's int_wpts / ts, packed: a warm start) -- without,
        attempt 0 starts from the straight line; `slots` (B,) int32 map-table slots by request or None; `subset` an
        int32 tensor of the request indices to plan (None: all B; each at most once).  Every attempt is neo_plan_guess_dev,
        neo_effort_order_dev for more than 1024 rows, neo_optimize_batch_from_dev over the packed rows and
        neo_plan_merge_dev; between two attempts the host reads two words and the list of the failed requests, draws
        `retry_noise` for those -- from the streams SeedSequence(seed, stream_ids[request], attempt), `stream_ids` a HOST
        array by request (None: the index) -- and uploads it.  seed / rng / max_attempts / waypoints as in `plan`.
        jitter="counter": plan(jitter="counter")'s arrays bit for bit, and the jitter never leaves the device --
        `stream_ids` is a host array (checked, uploaded once a call) or an int32 DEVICE tensor by request (not read by the
        host: ids in 0 .. 2^31 - 1 are the caller's word); between two attempts the host waits for the context's stream and
        reads the two count words only, then neo_plan_jitter_dev fills the packed noise over the failed list where it
        lies and the guess follows on the same stream: no list read-back, no host draw, no upload.
        Results by request in `bufs` (plan_buffers; made when None): x, costs, costs_last, nit, nfev, status (with the
        collision flag), attempts, nit_total (int64), solved (int32) and launch_sizes (a host list); `x` / `solved`: the
        caller's own resident arrays to write instead of the ones in bufs (FleetReplanLoop's).  Requests outside the
        subset keep what they had.  The chain has ended when the call returns (the context's stream is waited for).  A
        request that names a map-table slot without a map raises NeoError, as in `plan`.  Returns bufs.
        waypoints="adaptive": plan(waypoints="adaptive")'s ragged arrays bit for bit, every request with its own count of
        at most `max_waypoints` -- see `_plan_chain`."""
        if head.ndim != 3 or head.shape[1] != 3 or tuple(tail.shape) != tuple(head.shape):
            raise ValueError("BatchPlanner.plan_dev: head and tail (B, 3, D)")
        B, D = head.shape[0], head.shape[2]
        seg = None
        if isinstance(waypoints, str):
            if waypoints != "adaptive":
                raise ValueError("BatchPlanner.plan_dev: waypoints is a number, None or 'adaptive'")
            if x0 is not None:
                raise ValueError("BatchPlanner.plan_dev: a warm start x0 fixes its own shape: not with waypoints='adaptive'")
            seg = self._adaptive_args(max_waypoints, "BatchPlanner.plan_dev")
            count = int(max_waypoints)
        else:
            count = int(waypoints if waypoints is not None else self.cfg.init_wpts_num)
            if x0 is not None:
                B0, M0, _, n0 = _shape(x0, head)
                count = M0 - 1
                if B0 != B or count < 1 or D * count + count + 1 != n0 or (waypoints is not None and int(waypoints) != count):
                    raise ValueError("BatchPlanner.plan_dev: x0 (B, D * waypoints + waypoints + 1)")
        return self._plan_chain(map, head, tail, bufs, count, seg, x0, slots, subset, x, solved, max_attempts, seed, rng,
                                stream_ids, _guessed, jitter)

    def _plan_chain(self, map, head, tail, bufs, W, seg, x0, slots, subset, x, solved, max_attempts, seed, rng, stream_ids,
                    guessed, jitter):
        """the retry chain behind plan_dev, over GROUPS of requests with one waypoint count each.  `seg` None: the fixed
        form, ONE group -- the caller's subset (or all B) with W waypoints, packed from row 0.  Otherwise
        plan_dev(waypoints="adaptive"), `_plan_adaptive`'s arrays bit for bit: neo_adaptive_count_dev gives the launched
        requests their counts (at most W, segments of length `seg`), neo_adaptive_bucket_dev groups the launch list by
        count, and the host waits ONCE to read the group table.  The chain is attempt-major: in an attempt every group,
        longest first, gets its jitter (attempts after the first), its guess, its effort order above 1024 rows, its
        optimiser launch with M = count + 1 and its merge -- on rows of the packed arrays that start where the group's
        segment of the list starts, all on the context's stream, no wait in between.  The fixed form's merge
        (neo_plan_merge_dev) compacts its failed list itself; the groups' merges (neo_adaptive_merge_dev) are followed by
        ONE neo_adaptive_compact_dev that packs every group's failed requests to the front of its segment.  The host waits
        once per attempt and reads the failed counts and the bad-scene word: the two words of `counts`, or the table.
        jitter="counter": neo_plan_jitter_dev per group over its failed segment, no list is read; jitter="numpy": the
        failed lists are read and `retry_noise` drawn per group.
        Adaptive results in `bufs` (plan_buffers(..., waypoints="adaptive")): x (B, n_max) ragged with NaN behind a request's
        own values, counts, clamped (int32), the arrays of plan_dev, launch_sizes (requests per attempt over all groups),
        group_launch_sizes {count: sizes per attempt} and host_waits {"grouping": 1, "attempts": waits that followed an
        attempt}.  `x` / `solved` / `subset` as in plan_dev (`x`: rows of n_max)."""
        import torch
        adaptive = seg is not None
        B, D = head.shape[0], head.shape[2]
        n_max = D * W + W + 1
        if max_attempts < 1:
            raise ValueError("BatchPlanner.plan_dev: max_attempts must be >= 1")
        counter = counter_rng.check_jitter(jitter, "BatchPlanner.plan_dev")
        stream_ids, ids_dev, seed = self._plan_dev_streams(stream_ids, head, counter, seed)
        if bufs is not None and (bufs["B"] < B or bufs["D"] != D or bufs["M"] != W + 1 or (adaptive and not bufs.get("adaptive"))):
            raise ValueError("BatchPlanner.plan_dev: bufs were " +
                             ("not made for waypoints='adaptive' with this B, D and max_waypoints" if adaptive else
                              "made for another B, D or number of waypoints"))
        if adaptive and x is not None and (x.ndim != 2 or x.shape[1] != n_max):
            raise ValueError("BatchPlanner.plan_dev: x (B, D * max_waypoints + max_waypoints + 1) with waypoints='adaptive'")
        self._sync()
        c = self.ctx
        dev = head.device
        if bufs is None:
            bufs = self.plan_buffers(B, dev, D=D, waypoints="adaptive" if adaptive else W, max_waypoints=W)
            _torch_done(dev)
        d = bufs
        if seed is None:
            seed = _draw_seed(rng)
        p = _lib.dev_ptr
        # an array from row `first` on (no tensor is made for it)
        rows = lambda t, first: None if t is None else p(t, first * t.stride(0))
        if counter and ids_dev is None and max_attempts > 1:
            ids_dev = torch.from_numpy(stream_ids).to(dev)      # (a blocking copy: there before the context's stream starts)
        out_x, out_solved = (x if x is not None else d["x"]), (solved if solved is not None else d["solved"])
        # the groups: (count, first row, index of the group's word), `lens` the words' rows to launch, `lists` their requests;
        # `words`: what the host reads after an attempt's wait -- the groups' failed counts, then the bad-scene word
        lists, lens = subset, [_lib.launch_count(subset, B)]
        if adaptive:
            G = _lib.NEO_MAX_PIECES
            table = d["table"]      # bucket_begin [G + 1], the groups' failed counts [G], the bad-scene word, the total
            words = table[G + 1:2 * G + 2]
            if lens[0] == 0:       # (an empty list: nothing to count, nothing to wait for)
                d.update(launch_sizes=[], group_launch_sizes={}, host_waits=dict(grouping=0, attempts=0))
                return bufs
            c.call("neo_adaptive_count_dev", B, p(subset), lens[0], D, p(head), p(tail), seg, W, p(d["counts"]), p(d["clamped"]))
            c.call("neo_adaptive_bucket_dev", B, p(subset), lens[0], p(d["counts"]), p(d["group_order"]), p(table),
                   p(table[2 * G + 2:]))
            c.synchronize()
            begin = table[:G + 1].tolist()
            seg_begin = np.asarray(begin[:G], dtype=np.int32)
            segs = [(g, begin[g], g) for g in range(G - 1, 0, -1)]      # the longest M first
            lists, lens = d["group_order"], np.diff(begin).tolist()
        else:
            words = d["counts"]
            segs = [(W, 0, 0)]
            if subset is not None and lens[0] == 0:
                lists = d["todo"][1]    # (an empty tensor may own no memory, and a NULL list would mean all B requests)
        counts_at, bad_at = p(words), p(words[-1:])
        launches, by_group, waits, frac_tau = [], {}, 0, {}
        bad_scene = 0
        c.call("neo_optimize_progress_counter", None)
        try:
            for attempt in range(max_attempts):
                if attempt > 0:
                    c.synchronize()
                    waits += 1
                    *lens, bad_scene = words.tolist()
                    lists = d["todo"][(attempt - 1) % 2]
                # (the fixed form launches its first list even when it is empty: the merge zeroes the two words)
                groups = [(g, o, lens[k]) for g, o, k in segs if lens[k] > 0 or not (adaptive or attempt)]
                if bad_scene or not groups:
                    if not adaptive:
                        c.synchronize()     # (the fixed form ends with a wait of its own)
                    break
                if attempt > 0 and not counter:
                    for g, o, P in groups:
                        ids = lists[o:o + P].cpu().numpy()
                        noise = self.retry_noise(seed, stream_ids[ids], attempt, D, g)
                        d["noise"].view(-1)[o * D * W:o * D * W + P * D * g].copy_(torch.from_numpy(noise.reshape(-1)))
                    _torch_done(dev)
                pending = d["todo"][attempt % 2]
                for k, (g, o, P) in enumerate(groups):
                    M = g + 1
                    sub = rows(lists, o)
                    x_k, head_k, tail_k, noise_k, *res_k = (rows(d[k], o) for k in ("x_k", "head_k", "tail_k", "noise") + RESULTS_K)
                    slots_k = rows(d["slots_k"], o) if slots is not None else None
                    if g not in frac_tau:
                        frac_tau[g] = self._plan_frac_tau(g)
                    frac, tau = frac_tau[g]
                    if attempt > 0 and counter:
                        c.call("neo_plan_jitter_dev", B, sub, P, M, D, seed, attempt, p(ids_dev), noise_k)
                    if not (attempt == 0 and guessed):
                        c.call("neo_plan_guess_dev", B, sub, P, M, D, p(head), p(tail), p(slots), p(x0) if attempt == 0 else None,
                               noise_k if attempt > 0 else None, _lib.ptr(frac), _lib.ptr(tau), x_k, head_k, tail_k, slots_k)
                    if P > 0:
                        if P > 1024:
                            order = rows(d["order"], o)
                            c.call("neo_effort_order_dev", P, M, D, x_k, head_k, tail_k, p(d["order_scratch"]), order)
                            c.call("neo_optimize_dispatch_order", order, P)
                        else:
                            c.call("neo_optimize_dispatch_order", None, 0)
                        c.call("neo_optimize_batch_from_dev", map.scene_id, slots_k, P, M, D, x_k, x_k, head_k, tail_k, *res_k)
                    merged = (x_k, *res_k, p(out_x), *(p(d[k]) for k in RESULTS), p(d["attempts"]), p(d["nit_total"]), p(out_solved),
                              rows(pending, o))
                    if adaptive:
                        c.call("neo_adaptive_merge_dev", B, sub, P, M, D, n_max, int(attempt == 0), int(attempt == 0 and k == 0),
                               *merged, bad_at)
                    else:
                        c.call("neo_plan_merge_dev", B, sub, P, M, D, int(attempt == 0), *merged, counts_at, bad_at)
                    by_group.setdefault(g, []).append(P)
                if adaptive:
                    c.call("neo_adaptive_compact_dev", _lib.ptr(seg_begin), _lib.ptr(np.asarray(lens, dtype=np.int32)),
                           p(pending), counts_at)
                launches.append(sum(P for _, _, P in groups))
            else:
                c.synchronize()     # (every attempt has run: the last one's wait)
                waits += 1
                bad_scene = int(words[-1].item())
        finally:
            c.call("neo_optimize_dispatch_order", None, 0)     # (the order is in bufs: no launch after this reads it)
        if bad_scene:
            raise _lib.NeoError("BatchPlanner.plan_dev: a request names a scene without a map (NEO_TRAJ_BAD_SCENE)")
        d["launch_sizes"] = launches
        if adaptive:
            d.update(group_launch_sizes=by_group, host_waits=dict(grouping=1, attempts=waits))
        return bufs

    # ------------------------------------------------------------ the reference's `batch` mode (:103-168) for B requests
    def _batch_offsets(self, K, lateral_offsets):
        """the signed lateral offsets of K candidates: the reference's 0, +0.6, -0.6, +0.6, ... (0.6 * lateral_dir[(k - 1) % 2],
        :131-137 -- the distance does not grow) unless `lateral_offsets` (K values) is given"""
        if lateral_offsets is not None:
            off = _lib.as_f64(lateral_offsets).reshape(-1)
            if K is not None and off.shape[0] != int(K):
                raise ValueError("BatchPlanner.batch_plan: lateral_offsets needs one offset per candidate")
        else:
            K = 3 if K is None else int(K)         # the reference's batch_num
            off = np.array([0.0 if k == 0 else (0.6 if k % 2 else -0.6) for k in range(max(K, 0))])
        if not 1 <= off.shape[0] <= _lib.NEO_BATCH_MAX_CANDIDATES:
            raise ValueError("BatchPlanner.batch_plan: K must be in 1 .. %d" % _lib.NEO_BATCH_MAX_CANDIDATES)
        return off

    def _batch_ts_tau(self, count):
        """the shared durations init_T * [1.5, 1, ..., 1, 1.5] and their tau, element by element through math.log as
        MinJerkPlanner.map_T2tau computes it (:468-475)"""
        ts = self._start_ts(count)
        tau = np.array([-math.log((self.cfg.T_max - self.cfg.T_min) / (t - self.cfg.T_min) - 1) for t in ts])
        return ts, tau

    def batch_init_guess(self, head, tail, K=None, lateral_offsets=None):
        """batch_generate_init_variables (:103-140) for B 2-D requests, in NumPy: int_wpts (B, K, D, count) -- candidate k
        is the straight line shifted by lateral_offsets[k] along lateral_dir[0] -- and the shared ts (M,).  Request by
        request the values are MinJerkPlanner.batch_generate_init_variables', bit for bit (what neo_batch_candidates
        computes on the device).  start == target: candidate 0 finite, the shifted ones NaN, as in the reference."""
        head, tail = _f64(head, tail)
        B, D = head.shape[0], head.shape[2]
        if D != 2:
            raise ValueError("BatchPlanner.batch_init_guess: the reference's lateral candidates are 2-D (D = 2)")
        off = self._batch_offsets(K, lateral_offsets)
        count = int(self.cfg.init_wpts_num)
        out = np.zeros((B, off.shape[0], D, count))
        with np.errstate(invalid="ignore", divide="ignore"):
            for b in range(B):
                start, target = head[b, 0], tail[b, 0]
                forward = (target - start) / np.linalg.norm(target - start)
                side = np.array([forward[1], -forward[0]])           # lateral_dir[0]; lateral_dir[1] is its exact negative
                stride = (target - start) / (count + 1)
                c0 = np.linspace(start + stride, target, count, endpoint=False)
                for k, o in enumerate(off):
                    out[b, k] = (c0 + o * side if o != 0.0 else c0).T
        return out, self._batch_ts_tau(count)[0]

    def batch_buffers(self, B, K, device):
        """the resident arrays of `batch_plan_dev` for up to B requests of K candidates: the packed work arrays of the
        B * K optimiser runs and the request-indexed results (torch tensors, zeroed)"""
        count = int(self.cfg.init_wpts_num)
        bufs, f, i = _work_buffers(device, dict(B=B, K=K), B * K, B, 2 * count + count + 1, 2)
        bufs.update(chosen=i(B), candidate_cost=f(B, K), nit_total=i(B), opt_runs=i(B), fallback=i(max(B, 1)), n_fallback=i(1))
        return bufs

    def batch_plan_dev(self, map, head, tail, bufs=None, K=None, lateral_offsets=None, slots=None, subset=None, x=None,
                       solved=None):
        """the main path of `batch_plan` on RESIDENT torch tensors, asynchronous on the context's stream (as optimize_dev is
        to optimize): head / tail (B, 3, 2) float64 by request; `slots` (B,) int32 map-table slots by request or None;
        `subset` an int32 tensor of the request indices to plan (None: all B).  Three launches -- neo_batch_candidates_dev,
        neo_optimize_batch_from_dev over the P * K packed rows, neo_batch_select_dev -- and nothing passes through the
        host.  Results by request in `bufs` (batch_buffers; made when None): chosen, candidate_cost, solved, x, costs,
        costs_last, nit, nfev, status (with the collision flag), nit_total, opt_runs; `x` / `solved`: the caller's own
        resident arrays to write instead of the ones in bufs (FleetReplanLoop's).  The requests without a feasible candidate
        -- chosen -1, x untouched -- are listed in bufs["fallback"][:bufs["n_fallback"]]: `batch_fallback` fetches the list;
        they are the caller's to retry (`batch_plan` does).  Returns bufs."""
        self._sync()
        c = self.ctx
        B, D = head.shape[0], head.shape[2]
        if D != 2:
            raise ValueError("BatchPlanner.batch_plan_dev: the reference's lateral candidates are 2-D (D = 2)")
        off = self._batch_offsets(K, lateral_offsets)
        K = off.shape[0]
        if bufs is None:
            bufs = self.batch_buffers(B, K, head.device)
        if bufs["B"] < B or bufs["K"] != K:
            raise ValueError("BatchPlanner.batch_plan_dev: bufs were made for another B or K")
        count = int(self.cfg.init_wpts_num)
        M = count + 1
        _, tau = self._batch_ts_tau(count)
        P = _lib.launch_count(subset, B)
        p = _lib.dev_ptr
        d = bufs
        x_k, head_k, tail_k, *res_k = (p(d[k]) for k in ("x_k", "head_k", "tail_k") + RESULTS_K)
        slots_k = p(d["slots_k"]) if slots is not None else None
        c.call("neo_batch_candidates_dev", B, p(subset), P, M, D, K, p(head), p(tail), p(slots), _lib.ptr(tau), _lib.ptr(off),
               x_k, head_k, tail_k, slots_k)
        if P > 0:
            c.call("neo_optimize_dispatch_order_host", None, 0)
            c.call("neo_optimize_progress_counter", None)
            c.call("neo_optimize_batch_from_dev", map.scene_id, slots_k, P * K, M, D, x_k, x_k, head_k, tail_k, *res_k)
        w = _lib.as_f64(self.cfg.weights).reshape(4)
        c.call("neo_batch_select_dev", B, p(subset), P, M, D, K, x_k, *res_k, _lib.ptr(w), p(d["chosen"]), p(d["candidate_cost"]),
               p(solved if solved is not None else d["solved"]), p(x if x is not None else d["x"]), *(p(d[k]) for k in RESULTS),
               p(d["nit_total"]), p(d["opt_runs"]), p(d["fallback"]), p(d["n_fallback"]))
        return bufs

    def batch_fallback(self, bufs):
        """waits for the context's stream, then copies the number of fallback requests (4 bytes) and the list itself"""
        self.ctx.synchronize()
        nf = int(bufs["n_fallback"].item())
        return bufs["fallback"][:nf].cpu().numpy().astype(np.int64) if nf else np.zeros(0, np.int64)

    def batch_plan(self, map, head, tail, K=None, lateral_offsets=None, scene_ids=None, seed=None, stream_ids=None,
                   max_attempts=5):
        """MinJerkPlanner.batch_plan (:142-168) for B 2-D requests head / tail (B, 3, 2): K laterally shifted initial
        guesses a request (`batch_init_guess`), ONE optimiser launch of B * K trajectories, and the cheapest feasible
        candidate of each request kept -- candidates, launch and choice on the device (`batch_plan_dev`).  Only the
        requests WITHOUT a feasible candidate come back to the host: they take `plan(int_wpts=candidate 0, ts=...)`, the
        reference's warm_start_plan(cands[0], ts) (:166-168), with plan's per-request random streams (`seed`,
        `stream_ids`, `max_attempts` as there).  scene_ids as in `optimize`.  Returns the optimiser's dict for the kept
        trajectory (x, costs, costs_last, nit, nfev, status, collision) plus chosen (B,: the candidate kept, -1: the
        result comes from the fallback), candidate_cost (B, K: +inf for a candidate that is not feasible), final_cost
        (B,: the reference's (costs_last * weights).sum(), :233-234, summed by NumPy on the host -- `optimize`'s
        final_cost is taken from `costs`, the costs at x, instead), nit_total and attempts (B,: what the reference adds
        to iter_num and opt_running_times over the candidates, an overflowed run not counted, plus the fallback's
        nit_total and attempts) and solved (B,).  A scene without a map among the requests raises NeoError, as in `plan`."""
        import torch
        head, tail = _f64(head, tail)
        if head.ndim != 3 or head.shape[2] != 2 or head.shape != tail.shape:
            raise ValueError("BatchPlanner.batch_plan: head and tail (B, 3, 2): the reference's lateral candidates are 2-D")
        B = head.shape[0]
        off = self._batch_offsets(K, lateral_offsets)
        K = off.shape[0]
        stream_ids = _stream_ids(stream_ids, B, "BatchPlanner.batch_plan")
        sid = None if scene_ids is None else _scene_ids(scene_ids).reshape(-1)
        if sid is not None and sid.shape[0] != B:
            raise ValueError("BatchPlanner.batch_plan: scene_ids needs one id per request")
        count = int(self.cfg.init_wpts_num)
        n = 2 * count + count + 1
        w = np.asarray(self.cfg.weights, dtype=np.float64)
        if B == 0:
            return dict(_result_dict(np.zeros((0, n)), _host_results(0)), chosen=np.zeros(0, np.int32),
                        candidate_cost=np.zeros((0, K)), final_cost=np.zeros(0), nit_total=np.zeros(0, np.int64),
                        attempts=np.zeros(0, np.int32), solved=np.zeros(0, bool))
        c = self.ctx
        dev = torch.device("cuda", c.device)
        slots = None
        if sid is not None:
            slot_of = {int(s): int(c.lib.neo_scene_slot(c.h, int(s))) for s in np.unique(sid)}
            if min(slot_of.values()) < 0:
                raise _lib.NeoError("BatchPlanner.batch_plan: requests name a scene without a map")
            slots, = _upload(dev, np.array([slot_of[int(s)] for s in sid], dtype=np.int32))
        d_head, d_tail = _upload(dev, head, tail)
        bufs = self.batch_buffers(B, K, dev)
        _torch_done(dev)
        self.batch_plan_dev(map, d_head, d_tail, bufs, lateral_offsets=off, slots=slots)
        fb = self.batch_fallback(bufs)
        h = {k: bufs[k].cpu().numpy() for k in ("x", *RESULTS, "chosen", "candidate_cost", "solved", "nit_total", "opt_runs")}
        out = _result_dict(h["x"], [h[k] for k in RESULTS])      # (without weights: final_cost is this method's own, below)
        out.update(chosen=h["chosen"], candidate_cost=h["candidate_cost"], nit_total=h["nit_total"].astype(np.int64),
                   attempts=h["opt_runs"].copy(), solved=h["solved"] != 0)
        if fb.size:
            cand0 = self.batch_init_guess(head[fb], tail[fb], K=1)[0][:, 0]
            ts = np.tile(self._batch_ts_tau(count)[0], (fb.size, 1))
            r = self.plan(map, head[fb], tail[fb], int_wpts=cand0, ts=ts, max_attempts=max_attempts, seed=seed,
                          stream_ids=stream_ids[fb], scene_ids=None if sid is None else sid[fb])
            for k in ("x", "costs", "costs_last", "nit", "nfev", "status", "collision", "solved"):
                out[k][fb] = r[k]
            out["attempts"][fb] += r["attempts"]
            out["nit_total"][fb] += r["nit_total"]
        out["final_cost"] = (out["costs_last"] * w).sum(axis=1)      # costs_LAST, the reference's (:233-234); optimize: costs
        return out

    def expected_effort_order(self, head, tail, ts):
        """permutation that starts the runs expected to be long first.  Proxy: time slack of the initial
        guess, sum(ts) * v_max / distance -- a guess that is far too slow needs many iterations to shed
        duration (measured on the cfg2 batch: rank correlation 0.5 with the evaluation count).  A non-finite key (NaN or
        infinite start, goal or duration) is 0, as on the device (neo_effort_order_dev): such runs start last, in index order."""
        head = np.asarray(head); tail = np.asarray(tail); ts = np.asarray(ts)
        with np.errstate(invalid="ignore"):
            dist = np.linalg.norm(tail[:, 0] - head[:, 0], axis=1)
            slack = ts.sum(axis=1) * self.cfg.v_max / np.maximum(dist, 1e-9)
        slack[~np.isfinite(slack)] = 0.0
        return np.argsort(-slack, kind="stable").astype(np.int32)

    def expected_effort_order_dev(self, x0, head, tail):
        """the same order computed on the device from RESIDENT torch tensors x0 (B, n), head / tail (B, 3, D) -- a keys kernel
        and a radix sort on the context's stream (neo_effort_order_dev); returns (order int32 [B], keys float64 [B]) device tensors"""
        import torch
        self._sync()
        c = self.ctx
        B, M, D, _ = _shape(x0, head)
        scratch = torch.empty(int(c.lib.neo_effort_order_scratch_bytes(B)) // 8 + 1, dtype=torch.float64, device=x0.device)   # (keys first)
        order = torch.empty(B, dtype=torch.int32, device=x0.device)
        pp = _lib.dev_ptr
        c.call("neo_effort_order_dev", B, M, D, pp(x0), pp(head), pp(tail), pp(scratch), pp(order))
        return order, scratch[:B]

    @staticmethod
    def spatial_order(head, tail, xcds=8, cell=1.0, key=None, chunk=None):
        """XCD-aware spatial dispatch order for the ESDF-lookup kernel (neo_sampled_terms_dispatch_order): requests are keyed by
        a coarse Morton code of where they fly -- the midpoint of start and goal in cells of `cell` metres -- sorted, and
        the sorted list is dealt so that workgroups i, i + 8, i + 16, ... (one XCD: the hardware dispatches workgroups
        round-robin over the 8 XCDs, each with its own 4 MB L2) hold contiguous runs of it.  Requests whose
        corridors overlap then share an L2 and run at about the same time.  `chunk`: length of the runs dealt to the XCDs
        in turn (None: min(512, B / xcds); runs shorter than B / xcds make every XCD sweep the whole scene, which evens out
        their loads).  Results are in the caller's order and bit-identical whatever the order."""
        head = np.asarray(head); tail = np.asarray(tail)
        B = head.shape[0]
        if key is None:
            mid = 0.5 * (head[:, 0] + tail[:, 0])
            q = np.floor((mid - mid.min(axis=0)) / cell).astype(np.int64)
            bits = max(1, int(np.ceil(np.log2(max(int(q.max()) + 1, 2)))))
            key = np.zeros(B, dtype=np.int64)
            D = q.shape[1]
            for b in range(bits):
                for d in range(D):
                    key |= ((q[:, d] >> b) & 1) << (D * b + d)
        srt = np.argsort(key, kind="stable")
        if xcds <= 1:
            return srt.astype(np.int32)
        # default: runs of at most 512 requests -- what an XCD holds at four wavefronts per SIMD -- dealt to the XCDs in turn
        # (measured on the MI355X, cfg2, 163 840 requests in one launch: one run of B / 8 per XCD 0.385 of the roofline
        # figure, runs of 64 ... 512 0.401 ... 0.406, sorted without the deal 0.398; a 4096 launch has 512 per XCD either way)
        chunk = int(chunk) if chunk else min(512, -(-B // xcds))
        # run c of the sorted list goes to XCD c mod xcds; queue the runs per XCD, then workgroup i takes the next request
        # of XCD i mod xcds (XCDs that run out early are served from the others' leftovers: still a permutation)
        queues = [[] for _ in range(xcds)]
        for c, lo in enumerate(range(0, B, chunk)):
            queues[c % xcds].append(srt[lo:lo + chunk])
        queues = [np.concatenate(q_) if q_ else np.zeros(0, dtype=srt.dtype) for q_ in queues]
        out = np.full(B, -1, dtype=np.int64)
        left = []
        for k in range(xcds):
            slots = np.arange(k, B, xcds)
            m = min(len(slots), len(queues[k]))
            out[slots[:m]] = queues[k][:m]
            left.append(queues[k][m:])
        rest = np.concatenate(left)
        out[out < 0] = rest
        return out.astype(np.int32)

    def optimize_dev(self, map, x, head, tail, costs, costs_last, nit, nfev, status, slots=None, x0=None, progress=None):
        """torch CUDA tensors (float64 / int32), asynchronous on the context's stream.
        `slots`: optional int32 device tensor of map-table slots (Context.lib.neo_scene_slot).
        `x0`: optional start points (only read; results go to x) -- None: x is optimised in place.
        `progress`: optional int32 device tensor (one element, zeroed by the caller) that counts the trajectories as they
        finish (neo_optimize_progress_counter): poll it through a copy on another stream to use the finished results while
        the launch's long runs are still going"""
        B, M, D, _ = _shape(x, head)
        c = self.ctx
        p = _lib.dev_ptr
        c.call("neo_optimize_progress_counter", p(progress))
        c.call("neo_optimize_batch_from_dev", map.scene_id, p(slots), B, M, D, p(x0 if x0 is not None else x), p(x), p(head),
               p(tail), *_dev_ptrs(costs, costs_last, nit, nfev, status))
