"""
GeoPlanner: drop-in stand-in for the reference's traj_planner/geo_planner.py:GeoPlanner (selected_planner:=geo): an A*
path on the 2-D map (traj_planner/astar_planner.py), pruned to four key nodes, whose two inner nodes warm-start the
optimiser.  The search and the pruning run on the GPU (neo_geo_search_batch / neo_geo_prune_batch); every path, cost
and key node equals the reference's.
"""
import types

import numpy as np

from .planner import BatchPlanner, MinJerkPlanner, _map_scene


class _Astar:
    """astar_planner.py:AstarPlanner's interface: plan(map, start, target) -> the path as a list of [x, y]"""

    def __init__(self, owner):
        self._owner = owner
        self.target_cost = 0.0      # target_node.cost of the last plan
        self.flags = 0

    def plan(self, map, start_pos, target_pos, path_cap=1024):
        bp, m = self._owner._batch(map)
        while True:
            g = bp.geo_init(m, np.asarray(start_pos, dtype=np.float64)[None, :2],
                            np.asarray(target_pos, dtype=np.float64)[None, :2], path_cap=path_cap)
            n = int(g["path_len"][0])
            if n <= path_cap:
                break
            path_cap = n
        self.target_cost = float(g["path_cost"][0])
        self.flags = int(g["flags"][0])
        return [[float(p[0]), float(p[1])] for p in g["paths"][0, :n]]


class GeoPlanner(MinJerkPlanner):
    """geo_planner.py:GeoPlanner on the GPU"""

    def __init__(self, config=None, ctx=None, sample_dtype="f64", stale_T=True):
        super().__init__(config, ctx=ctx, sample_dtype=sample_dtype, stale_T=stale_T)
        self.astar_planner = _Astar(self)
        self.int_wpts_num = 2
        self._bp = None

    def _batch(self, map):
        """the BatchPlanner of this context and the device scene of `map` (foreign maps are snapshotted)"""
        if self._bp is None:
            self._bp = BatchPlanner(ctx=self.ctx)
        return self._bp, types.SimpleNamespace(scene_id=_map_scene(self.ctx, map, self._cache))

    def geo_traj_plan(self, map, plan_init_state, target_state):
        """geo_planner.py:19-35: A* from the start to the target, prune, warm_start_plan from the two inner key nodes"""
        bp, m = self._batch(map)
        g = bp.geo_init(m, np.asarray(plan_init_state.global_pos, dtype=np.float64)[None, :2],
                        np.asarray(target_state[0], dtype=np.float64)[None, :2])
        self.geo_result = {k: v[0] for k, v in g.items()}
        int_wpts = g["key_pts"][0, 1:3].T.copy()
        ts = self.init_T * np.ones((self.int_wpts_num + 1,))
        ts[0] *= 1.5
        ts[-1] *= 1.5
        drone_state_2d = np.array([plan_init_state.global_pos[:2], plan_init_state.global_vel[:2]])
        self.warm_start_plan(map, drone_state_2d, target_state, int_wpts, ts)

    def prune_path_nodes(self, map, path):
        """geo_planner.py:61-101: the four key nodes of `path` (a list of [x, y]) as a list"""
        bp, m = self._batch(map)
        kp = bp.geo_prune(m, np.asarray(path, dtype=np.float64).reshape(1, -1, 2))
        return [[float(p[0]), float(p[1])] for p in kp[0]]


__all__ = ["GeoPlanner"]
