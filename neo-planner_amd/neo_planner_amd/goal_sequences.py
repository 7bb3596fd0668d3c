"""
Goal sequences: missions that fly goal after goal (ros_node/manager_node.py:153-193 -- the manager sends the next goal as
soon as one is reached or given up, from its `predefined_goal` list or, in the `random` mission mode, from
set_random_goal: x flaps between two values, y is random).  Each goal is a leg of the mission's campaign.

This is the NumPy model of the goal part of csrc/neo_legs.hpp: the same operations in the same order, every one rounded on
its own, so `GoalSequences.goal` and neo_fleet_leg_goal / neo_fleet_leg_open_dev agree bit for bit.

  table   goals (NG, 2) and seq_begin (B + 1,), laid out as GoalRoutes lays out its vertices: mission b's goals are
          goals[seq_begin[b]:seq_begin[b + 1]], 1 to 64 of them
  flap    `legs` goals a mission: goal k = (x_pair[k & 1], y_scale * (u - y_shift)), u the 52-bit uniform of
          counter_rng.py from domain 3 with the counter (mission id, k, 0, 3 << 24), value 0.  The reference draws from
          NumPy's unseeded global stream; a counter stream makes a campaign reproducible, and a mission's goals the same
          alone and in any fleet.
"""
import ctypes

import numpy as np

from . import _lib, counter_rng

LEGS_MAX = _lib.NEO_FLEET_LEGS_MAX
DOMAIN_LEGS = 3


def flap_uniforms(seed, mission_ids, k):
    """(len(mission_ids),): the uniform leg k's y is made of"""
    return counter_rng.stream_uniforms(seed, mission_ids, k, 0, DOMAIN_LEGS, 1)[:, 0]


class GoalSequences:
    """B missions' goal lists.  `from_lists` makes a table, `flap` the reference's random campaign.  `goal(b, k)` is goal k
    of mission b (None where it has none), `count` (B,) the goals a mission has, `take(idx)` the lists of the missions
    `idx`, in that order, as a GoalSequences of their own (a mission flown alone keeps its id: FleetReplanLoop's
    mission_ids say which), `first()` every mission's goal 0."""

    def __init__(self, goals, seq_begin):
        g = _lib.as_f64(goals)
        if g.ndim != 2 or g.shape[1] != 2:
            raise ValueError("GoalSequences: goals must be (NG, 2)")
        sb = np.asarray(seq_begin)
        if sb.ndim != 1 or sb.shape[0] < 1 or not np.issubdtype(sb.dtype, np.integer):
            raise ValueError("GoalSequences: seq_begin must be (B + 1,) integers")
        sb = sb.astype(np.int64)
        if sb[0] != 0 or np.any(np.diff(sb) < 0) or sb[-1] != g.shape[0]:
            raise ValueError("GoalSequences: seq_begin must ascend from 0 to the number of goals")
        n = np.diff(sb)
        if np.any(n < 1):
            raise ValueError("GoalSequences: a mission needs at least 1 goal")
        if np.any(n > LEGS_MAX):
            raise ValueError("GoalSequences: a mission has at most %d goals" % LEGS_MAX)
        if not np.all(np.isfinite(g)):
            raise ValueError("GoalSequences: goals must be finite")
        self.kind = _lib.NEO_LEGS_TABLE
        self.goals, self.seq_begin = g, sb.astype(np.int32)
        self.B = sb.shape[0] - 1
        self.count = n.astype(np.int32)
        self.legs, self.seed, self.mission_ids = 0, 0, None
        self.x_pair, self.y_scale, self.y_shift = (0.0, 0.0), 0.0, 0.0

    @classmethod
    def from_lists(cls, lists):
        """lists: one (K_b, 2) list of goals per mission"""
        lists = [_lib.as_f64(g).reshape(-1, 2) for g in lists]
        begin = np.concatenate([[0], np.cumsum([len(g) for g in lists])]).astype(np.int32)
        return cls(np.concatenate(lists) if lists else np.zeros((0, 2)), begin)

    @classmethod
    def flap(cls, B, legs, seed, x_pair=(-1.0, 26.0), y_scale=4.0, y_shift=0.6, mission_ids=None):
        """the reference's set_random_goal for B missions and `legs` goals each; mission_ids (B,): the ids of the counter
        streams (None: 0 .. B - 1), in 0 .. 2^31 - 1; seed in 0 .. 2^64 - 1"""
        who = "GoalSequences.flap"
        self = cls.__new__(cls)
        B, legs = int(B), int(legs)
        if B < 0:
            raise ValueError(who + ": B must be >= 0")
        if not 1 <= legs <= LEGS_MAX:
            raise ValueError(who + ": legs must be in 1 .. %d" % LEGS_MAX)
        x = _lib.as_f64(x_pair).reshape(-1)
        if x.shape[0] != 2 or not (np.all(np.isfinite(x)) and np.isfinite(y_scale) and np.isfinite(y_shift)):
            raise ValueError(who + ": x_pair must be two finite numbers, y_scale and y_shift finite")
        ids = np.arange(B) if mission_ids is None else np.asarray(mission_ids).reshape(-1)
        if ids.shape[0] != B:
            raise ValueError(who + ": one mission id per mission")
        self.kind = _lib.NEO_LEGS_FLAP
        self.seed = counter_rng.check_seed(seed, who)
        self.mission_ids = counter_rng.check_ids(ids, who).astype(np.int32)
        self.B, self.legs = B, legs
        self.count = np.full(B, legs, np.int32)
        self.x_pair, self.y_scale, self.y_shift = (float(x[0]), float(x[1])), float(y_scale), float(y_shift)
        self.goals, self.seq_begin = np.zeros((0, 2)), np.zeros(B + 1, np.int32)
        return self

    def goals_of(self, b):
        """the (K, 2) goals of mission b"""
        if self.kind == _lib.NEO_LEGS_TABLE:
            return self.goals[self.seq_begin[b]:self.seq_begin[b + 1]]
        return np.stack([self.goal(b, k) for k in range(self.legs)])

    def goal(self, b, k):
        """goal k of mission b as (2,), or None where the mission has no goal k"""
        b, k = int(b), int(k)
        if not (0 <= b < self.B and 0 <= k < self.count[b]):
            return None
        if self.kind == _lib.NEO_LEGS_TABLE:
            return self.goals[self.seq_begin[b] + k].copy()
        u = flap_uniforms(self.seed, self.mission_ids[b:b + 1], k)[0]
        return np.array([self.x_pair[k & 1], np.float64(self.y_scale) * (u - np.float64(self.y_shift))])

    def leg_goals(self, k):
        """(B, 2): every mission's goal k, NaN where it has none"""
        out = np.full((self.B, 2), np.nan)
        have = np.flatnonzero(self.count > k) if k >= 0 else np.zeros(0, np.int64)
        if self.kind == _lib.NEO_LEGS_TABLE:
            out[have] = self.goals[self.seq_begin[have] + k]
        elif have.size:
            u = flap_uniforms(self.seed, self.mission_ids[have], k)
            out[have, 0] = self.x_pair[k & 1]
            out[have, 1] = np.float64(self.y_scale) * (u - np.float64(self.y_shift))
        return out

    def first(self):
        return self.leg_goals(0)

    def take(self, idx):
        idx = np.asarray(idx).reshape(-1)
        if self.kind == _lib.NEO_LEGS_TABLE:
            return GoalSequences.from_lists([self.goals_of(int(b)) for b in idx])
        return GoalSequences.flap(idx.shape[0], self.legs, self.seed, self.x_pair, self.y_scale, self.y_shift,
                                  mission_ids=self.mission_ids[idx])

    def struct(self, ptr_of, goals=None, seq_begin=None, mission_ids=None):
        """the neo_leg_sequences of these lists; goals / seq_begin / mission_ids: the arrays (host or device) whose addresses `ptr_of` gives -- None: this object's host arrays"""
        s = _lib.NeoLegSequences()
        s.kind, s.legs, s.n_goals, s.seed = int(self.kind), int(self.legs), int(self.goals.shape[0]), int(self.seed)
        s.x_pair[0], s.x_pair[1], s.y_scale, s.y_shift = self.x_pair[0], self.x_pair[1], self.y_scale, self.y_shift
        table = self.kind == _lib.NEO_LEGS_TABLE
        as_int = lambda p: None if p is None else ctypes.cast(p, ctypes.c_void_p).value
        s.goals = as_int(ptr_of(self.goals if goals is None else goals)) if table else None
        s.seq_begin = as_int(ptr_of(self.seq_begin if seq_begin is None else seq_begin)) if table else None
        s.mission_ids = None if table else as_int(ptr_of(self.mission_ids if mission_ids is None else mission_ids))
        return s
