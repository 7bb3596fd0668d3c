"""
The fleet's flight model: a drone that tracks its commands with lag and gusts, in place of PX4 / Gazebo.

The reference has no drone model (PX4 SITL does the flying there), so this file IS the definition; csrc/neo_flight.hpp
does the same operations in the same order, every one rounded on its own, and agrees with it bit for bit
(fleet_fly_kernel and fleet_fly_error_kernel on the device, tests/host_harness/flight_host.cpp on the host).  fp64
throughout, only + - * / and sqrt; every derived constant (h, alpha, rho, scale) is computed once, here, and handed
over, so both sides hold the same doubles.

A mission's state is drone[8]: position p, velocity v, lagged thrust acceleration a and gust acceleration g, 2-D each.
One sub-step is one command period h = 1 / cmd_hz.  Sub-step t is the absolute row index -- row t is the command at
t / cmd_hz: it takes the drone from time (t - 1) / cmd_hz to t / cmd_hz and leaves flown row t.  It works against the
command the drone holds during that period, r = cmd[min(t - 1, cmd_len - 1)] = (p_d, v_d, a_d), sampled with the state at
the period's start (the command of row t itself is h * v_d ahead of a drone that follows exactly: against it no flight
could have zero error):

  1  u = a_d + kp * (p_d - p) + kv * (v_d - v)          products rounded, the sums left to right
  2  n = sqrt(ux * ux + uy * uy);  n > a_max:  u *= (a_max / n), and the mission's saturation count goes up by one
  3  a += alpha * (u - a)                                alpha = h / (tau + h)
  4  t % gust_every == 0 and scale != 0:  g = rho * g + scale * z
       z = values 0 and 1 of counter_rng's stream (seed, mission id, t / gust_every, 0, domain 4)
       rho = exp(-gust_every * h / gust_tau), scale = gust_sigma * sqrt(1 - rho * rho);  with gust_sigma == 0 the scale is
       0, nothing is drawn and g stays what it is
  5  v += h * (a + g - drag * v),  then  p += h * v
  6  flown row t = (p, v, a + g - drag * v), of the new state, in the command rows' 48-byte layout

A drone that starts on row 0 of commands built by p += h * v with constant v and no acceleration follows them exactly
(drag = 0, no gusts).  The draw index is the absolute row, so a flight does not depend on how ticks cut it, and a mission
flies the same alone and in any fleet.

  FlightModel        the parameters and their refusals; derived(cmd_hz) the constants both sides compute with
  substep            one sub-step of one mission
  fly_launch         fleet_fly_kernel's launch on host arrays (the model of the kernel, in place)
  Flight / fly       one mission flown along a growing command array (replan.ReplanLoop, TrackerLoop)
  fly_error          fleet_fly_error_kernel's record: save_tracking_err (ros_node/traj_planner_node.py:310-331) per mission
"""
import collections
import math

import numpy as np

from . import _lib, counter_rng

DOMAIN_GUST = 4          # counter_rng's domains 1 - 3 are the retry noise, the target jitter and the flap goals
FLY_FIELDS = _lib.FLY_FIELDS
_F = np.float64

Derived = collections.namedtuple("Derived", "h kp kv a_max alpha drag rho scale gust_every seed")


class FlightModel:
    """kp, kv: the position and velocity gains of the tracking law; tau: the thrust lag in seconds (0: none); a_max: the
    largest commanded acceleration; drag: linear drag, 1 / s; gust_sigma: the stationary standard deviation of the gust
    acceleration per axis (0: no gusts, nothing drawn); gust_tau: its correlation time in seconds; gust_every: sub-steps
    between two draws (None: max(1, round(cmd_hz / 10))); seed: the key of the gust streams (counter_rng.check_seed)."""

    def __init__(self, kp=8.0, kv=5.0, tau=0.08, a_max=6.0, drag=0.1, gust_sigma=0.0, gust_tau=1.0, gust_every=None, seed=0):
        who = "FlightModel"
        vals = dict(kp=kp, kv=kv, tau=tau, a_max=a_max, drag=drag, gust_sigma=gust_sigma, gust_tau=gust_tau)
        for name, v in vals.items():
            if not np.isfinite(float(v)):
                raise ValueError("%s: %s must be finite" % (who, name))
            vals[name] = float(v)
        for name in ("kp", "kv", "drag", "gust_sigma", "tau"):
            if vals[name] < 0.0:
                raise ValueError("%s: %s must be >= 0" % (who, name))
        for name in ("a_max", "gust_tau"):
            if not vals[name] > 0.0:
                raise ValueError("%s: %s must be > 0" % (who, name))
        if gust_every is not None:
            if not np.isfinite(float(gust_every)) or int(gust_every) != gust_every or int(gust_every) < 1 or int(gust_every) >= 2 ** 31:
                raise ValueError("%s: gust_every must be an integer >= 1" % who)
            gust_every = int(gust_every)
        self.__dict__.update(vals)
        self.gust_every = gust_every
        self.seed = counter_rng.check_seed(seed, who)

    def derived(self, cmd_hz):
        """the constants of a flight at cmd_hz commands a second: what the kernels, the header and this model compute with"""
        hz = float(cmd_hz)
        if not (np.isfinite(hz) and hz > 0.0):
            raise ValueError("FlightModel: cmd_hz must be finite and > 0")
        h = 1.0 / hz
        every = self.gust_every if self.gust_every is not None else max(1, int(round(hz / 10.0)))
        rho = math.exp(-(every * h) / self.gust_tau)
        scale = self.gust_sigma * math.sqrt(1.0 - rho * rho)
        return Derived(h, self.kp, self.kv, self.a_max, h / (self.tau + h), self.drag, rho, scale, every, self.seed)


def gust_draws(seed, mission_id, draws):
    """(len(draws), 2): values 0 and 1 of the streams (seed, mission_id, a, 0, domain 4), a over `draws` --
    counter_rng.stream_normals(seed, [mission_id], a, 0, 4, 2) for every a, in one call of the block function"""
    a = np.asarray(draws, dtype=np.uint64).reshape(-1)
    counter = np.empty((a.shape[0], 4), dtype=np.uint64)
    counter[:, 0] = int(mission_id)
    counter[:, 1] = a
    counter[:, 2] = 0
    counter[:, 3] = DOMAIN_GUST << 24
    seed = int(seed)
    w = counter_rng.philox4x32_10(counter, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64))
    if a.shape[0] == 0:
        return np.zeros((0, 2))
    return counter_rng.probit(np.stack([counter_rng.uniform(w[:, 0], w[:, 1]), counter_rng.uniform(w[:, 2], w[:, 3])], axis=1))


def out_row(d, s):
    """the flown row of the state s: (p, v, a + g - drag * v)"""
    return np.array([s[0], s[1], s[2], s[3], (s[4] + s[6]) - d.drag * s[2], (s[5] + s[7]) - d.drag * s[3]])


def substep(d, mission_id, t, row, s, z=None):
    """sub-step t of one mission against the command row `row` (6 doubles); s (8 float64) is updated in place.  Returns
    (the flown row, 1 if the command saturated else 0).  z: the draw of this sub-step, where the caller has it already."""
    px, py, vx, vy, ax, ay, gx, gy = (_F(x) for x in s)
    pdx, pdy, vdx, vdy, adx, ady = (_F(x) for x in row)
    kp, kv, h = _F(d.kp), _F(d.kv), _F(d.h)
    ux = (adx + kp * (pdx - px)) + kv * (vdx - vx)
    uy = (ady + kp * (pdy - py)) + kv * (vdy - vy)
    n = np.sqrt(ux * ux + uy * uy)
    sat = 0
    if n > d.a_max:
        f = _F(d.a_max) / n
        ux, uy = ux * f, uy * f
        sat = 1
    al = _F(d.alpha)
    ax, ay = ax + al * (ux - ax), ay + al * (uy - ay)
    if d.scale != 0.0 and t % d.gust_every == 0:
        if z is None:
            z = gust_draws(d.seed, mission_id, [t // d.gust_every])[0]
        rho, sc = _F(d.rho), _F(d.scale)
        gx, gy = rho * gx + sc * _F(z[0]), rho * gy + sc * _F(z[1])
    dr = _F(d.drag)
    vx, vy = vx + h * ((ax + gx) - dr * vx), vy + h * ((ay + gy) - dr * vy)
    px, py = px + h * vx, py + h * vy
    s[:] = (px, py, vx, vy, ax, ay, gx, gy)
    return out_row(d, s), sat


def _fly_rows(d, mission_id, rows, t0, t1, hold, s, flown):
    """sub-steps t0 .. t1 of one mission: against rows[t - 1] (rows[hold] past it), flown rows into flown[t]; returns
    the saturation count"""
    if t1 < t0:
        return 0
    draws = {}
    if d.scale != 0.0:
        ks = [t // d.gust_every for t in range(t0, t1 + 1) if t % d.gust_every == 0]
        draws = dict(zip(ks, gust_draws(d.seed, mission_id, ks)))
    sat = 0
    for t in range(t0, t1 + 1):
        out, k = substep(d, mission_id, t, rows[min(t - 1, hold)], s, draws.get(t // d.gust_every))
        flown[t] = out
        sat += k
    return sat


def fly_launch(d, cmd, cmd_len, cmd_index, future_index, step, ahead, first, settle, reach, goal, drone, flown, flown_len,
               saturated, flags, cur_pos, head, mission_ids=None, subset=None):
    """fleet_fly_kernel's launch on host arrays, in place: cmd (B, cap, 6) read, flown (B, cap_f, 6) with cap_f >= cap
    written below row cap only, everything else (B, ...).  subset: the missions launched (None: all; an index outside
    0 .. B - 1 is skipped)."""
    B, cap = cmd.shape[0], cmd.shape[1]
    cmd, flown = cmd.reshape(B, cap, 6), flown.reshape(B, flown.shape[1], 6)
    with np.errstate(all="ignore"):
        for b in (range(B) if subset is None else subset):
            b = int(b)
            if b < 0 or b >= B:
                continue
            ln = min(int(cmd_len[b]), cap)
            if ln < 1:
                continue
            last = ln - 1
            mid = b if mission_ids is None else int(mission_ids[b])
            s = drone[b]
            idx0 = max(int(cmd_index[b]), 0)
            idx = last if idx0 > last - step else idx0 + step
            fut = last if idx > last - ahead else idx + ahead
            if (first or flown_len[b] < 1) and idx0 < cap:
                flown[b, idx0] = out_row(d, s)
            saturated[b] += _fly_rows(d, mid, cmd[b], idx0 + 1, idx, last, s, flown[b])
            n = idx + 1
            if settle > 0 and idx == last:
                for k in range(settle):
                    dx, dy = s[0] - goal[b, 0], s[1] - goal[b, 1]
                    if np.sqrt(dx * dx + dy * dy) < reach:
                        break
                    if n >= cap:
                        flags[b] |= _lib.NEO_FLEET_FLAG_CMD_FULL
                        break
                    saturated[b] += _fly_rows(d, mid, cmd[b], n, n, last, s, flown[b])
                    n += 1
            cmd_index[b], future_index[b], flown_len[b] = idx, fut, n
            cur_pos[b] = s[:2]
            head[b].reshape(6)[:4] = cmd[b, fut, :4]
            head[b].reshape(6)[4:] = 0.0


class Flight:
    """one mission flown along a command array that grows and is re-spliced ahead of the drone (replan.ReplanLoop):
    `advance(commands, upto)` flies the sub-steps behind the last one up to row `upto`; rows (n, 6) are the flown rows."""

    def __init__(self, model, cmd_hz, start_pos, start_vel=(0.0, 0.0), mission_id=0):
        self.d = model.derived(cmd_hz)
        self.mission_id = int(mission_id)
        self.s = np.zeros(8)
        self.s[:2], self.s[2:4] = np.asarray(start_pos, float)[:2], np.asarray(start_vel, float)[:2]
        self.flown = {0: out_row(self.d, self.s)}
        self.saturated_rows = []

    @property
    def n(self):
        return len(self.flown)

    @property
    def pos(self):
        return self.s[:2].copy()

    def advance(self, commands, upto, hold=None):
        """fly rows n .. upto against commands (n_cmd, 3, 2) (rows past `hold`, default the array's last, hold that row)"""
        rows = np.asarray(commands, dtype=np.float64).reshape(-1, 6)
        hold = rows.shape[0] - 1 if hold is None else hold
        with np.errstate(all="ignore"):
            for t in range(self.n, upto + 1):
                _, k = substep(self.d, self.mission_id, t, rows[min(t - 1, hold)], self.s)
                self.flown[t] = out_row(self.d, self.s)
                if k:
                    self.saturated_rows.append(t)

    def settle(self, commands, goal, settle, reach):
        """hold the array's last command for at most `settle` more sub-steps, up to the first with the drone within `reach`"""
        rows = np.asarray(commands, dtype=np.float64).reshape(-1, 6)
        goal = np.asarray(goal, dtype=np.float64)
        for _ in range(int(settle)):
            dx, dy = self.s[0] - goal[0], self.s[1] - goal[1]
            if np.sqrt(dx * dx + dy * dy) < reach:
                break
            self.advance(rows, self.n)

    def rows(self):
        return np.stack([self.flown[t] for t in range(self.n)]).reshape(-1, 3, 2)

    def result(self, commands, stride=1):
        """the fly_* keys of a loop's result"""
        rows, cmds = self.rows(), np.asarray(commands, dtype=np.float64).reshape(-1, 3, 2)
        rec, count, flag = fly_error(rows, cmds, stride)
        out = {"fly_" + k: rec[i] for i, k in enumerate(FLY_FIELDS)}
        out.update(fly_count=count, fly_flags=flag, fly_saturated=len(self.saturated_rows), fly_saturated_rows=list(self.saturated_rows),
                   flown=rows)
        return out


def fly(model, cmd_hz, commands, start_pos, start_vel=(0.0, 0.0), mission_id=0, settle=0, reach=0.0, goal=None):
    """the whole array flown from the start state: row 0 is the start state, rows 1 .. n_cmd - 1 the sub-steps, then the
    settle rows.  Returns the Flight."""
    f = Flight(model, cmd_hz, start_pos, start_vel, mission_id)
    n = np.asarray(commands).reshape(-1, 6).shape[0]
    f.advance(commands, n - 1)
    if settle > 0 and n >= 1:
        f.settle(commands, goal, settle, reach)
    return f


def fly_error(flown, commands, stride):
    """one mission's tracking-error record, save_tracking_err's table reduced: flown (n, 3, 2) the flown rows, commands
    (n_cmd, 3, 2); sample j is row j * stride < n against command row min(j * stride, n_cmd - 1).  Returns (record
    (len(FLY_FIELDS),), count, flags): pos_err_rms = sqrt(sum(e * e) / count) with e = sqrt(dx * dx + dy * dy),
    pos_err_max and the row it is at (the first wins ties), the same two for the velocity without the row, and
    pos_err_final, e at row n - 1 whatever the stride.  No sample or no command: a NaN record, count 0, flags 0; a sampled
    row that is not finite: a NaN record, count 0, NEO_AUDIT_FLAG_NONFINITE."""
    fl = np.asarray(flown, dtype=np.float64).reshape(-1, 6)
    cm = np.asarray(commands, dtype=np.float64).reshape(-1, 6)
    nan = np.full(len(FLY_FIELDS), np.nan)
    n = fl.shape[0]
    if n < 1 or cm.shape[0] < 1:
        return nan, 0, 0
    at = np.arange(0, n, stride)
    with np.errstate(all="ignore"):
        a, c = fl[at], cm[np.minimum(at, cm.shape[0] - 1)]
        if not (np.all(np.isfinite(a[:, :4])) and np.all(np.isfinite(c[:, :4]))):      # (the accelerations are not compared)
            return nan, 0, _lib.NEO_AUDIT_FLAG_NONFINITE
        dx, dy, du, dv = a[:, 0] - c[:, 0], a[:, 1] - c[:, 1], a[:, 2] - c[:, 2], a[:, 3] - c[:, 3]
        p2, v2 = dx * dx + dy * dy, du * du + dv * dv
        pe, ve = np.sqrt(p2), np.sqrt(v2)
        lf, lc = fl[n - 1], cm[min(n - 1, cm.shape[0] - 1)]
        ex, ey = lf[0] - lc[0], lf[1] - lc[1]
        cnt = at.shape[0]
        rec = np.array([np.sqrt(np.sum(p2) / cnt), pe.max(), float(at[int(np.argmax(pe))]), np.sqrt(np.sum(v2) / cnt), ve.max(),
                        np.sqrt(ex * ex + ey * ey)])
    if not np.all(np.isfinite(rec)):
        return nan, 0, _lib.NEO_AUDIT_FLAG_NONFINITE
    return rec, cnt, 0
