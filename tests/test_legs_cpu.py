"""Fleet campaigns, the parts that need no GPU: the goal model of csrc/neo_legs.hpp compiled by the host compiler
(tests/host_harness/legs_host.cpp) against its NumPy model goal_sequences.GoalSequences bit for bit, the flap's uniform
against counter_rng's streams, take, header and exports, and every refusal of GoalSequences and of FleetReplanLoop's
campaign arguments."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO

import neo_planner_amd as npa
from neo_planner_amd import _lib, build, counter_rng
from neo_planner_amd.goal_routes import GoalRoutes
from neo_planner_amd.goal_sequences import GoalSequences, flap_uniforms

INC = os.path.join(REPO, "neo-planner_amd", "csrc")
SRC = os.path.join(REPO, "tests", "host_harness", "legs_host.cpp")
IDS = np.array([0, 1, 2 ** 31 - 1])
SEEDS = (7, 2 ** 32 + 12345)      # the second uses the key's high word
LEGS = range(6)


def _hex(a):
    return " ".join("0x%016x" % w for w in np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64))


def _table():
    rng = np.random.default_rng(77)
    return GoalSequences.from_lists([rng.uniform(-5.0, 30.0, (k, 2)) for k in (1, 6, 3, 64, 2)])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("legs") / "legs_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-I", INC, SRC, "-o", out])
    return out


def _ask(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[-1] == "" and len(out) == len(lines) + 1
    return out[:-1]


def _want(g):
    return "0" if g is None else "1 " + _hex(g).replace("0x", "")


# ------------------------------------------------------------------ header against model
def test_table_goals_equal_the_header_bit_for_bit(exe):
    seq = _table()
    lines = ["S %d %d %s %s" % (seq.B, len(seq.goals), " ".join(str(int(v)) for v in seq.seq_begin), _hex(seq.goals))]
    want = [" ".join(str(int(c)) for c in seq.count)]
    for b in range(seq.B):
        for k in list(LEGS) + [63, 64]:
            lines.append("G %d %d" % (b, k))
            want.append(_want(seq.goal(b, k)))
    got = _ask(exe, lines)
    assert got == want, [(l, g, w) for l, g, w in zip(lines, got, want) if g != w][:5]
    assert sum(w == "0" for w in want) >= 10 and sum(w != "0" for w in want) >= 15      # goals there and goals not there
    assert np.array_equal(seq.leg_goals(2), np.stack([seq.goal(b, 2) if seq.count[b] > 2 else [np.nan] * 2 for b in range(seq.B)]),
                          equal_nan=True)


@pytest.mark.parametrize("seed", SEEDS)
def test_flap_goals_equal_the_header_bit_for_bit(exe, seed):
    for kw in (dict(), dict(x_pair=(2.0, 26.0), y_scale=3.3, y_shift=0.45)):
        seq = GoalSequences.flap(len(IDS), 6, seed, mission_ids=IDS, **kw)
        lines = ["F 6 %d %s %s %s %s" % (seed, _hex(seq.x_pair[0]), _hex(seq.x_pair[1]), _hex(seq.y_scale), _hex(seq.y_shift)),
                 "I %d %s" % (len(IDS), " ".join(str(int(i)) for i in IDS))]
        want = ["ok", "ok"]
        for b in range(len(IDS)):
            for k in list(LEGS) + [6]:
                lines.append("G %d %d" % (b, k))
                want.append(_want(seq.goal(b, k)))
                lines.append("U %d %d" % (IDS[b], k))
                want.append(_hex(flap_uniforms(seed, IDS[b:b + 1], k)).replace("0x", ""))
        got = _ask(exe, lines)
        assert got == want, [(l, g, w) for l, g, w in zip(lines, got, want) if g != w][:5]
        assert want.count("0") == len(IDS)      # leg 6 of 6
        for k in LEGS:      # the model says what the issue says
            g = seq.leg_goals(k)
            assert np.all(g[:, 0] == seq.x_pair[k & 1])
            u = counter_rng.stream_uniforms(seed, IDS, k, 0, 3, 1)[:, 0]
            assert np.array_equal(g[:, 1], seq.y_scale * (u - seq.y_shift)) and np.all((u > 0.0) & (u < 1.0))
            assert np.array_equal(flap_uniforms(seed, IDS, k), u)
            assert np.array_equal(g, np.stack([seq.goal(b, k) for b in range(seq.B)]))


def test_flap_defaults_are_the_reference_set_random_goal():
    seq = GoalSequences.flap(4, 3, 5)
    assert seq.x_pair == (-1.0, 26.0) and seq.y_scale == 4.0 and seq.y_shift == 0.6 and np.array_equal(seq.mission_ids, np.arange(4))
    g = np.stack([seq.goals_of(b) for b in range(4)])
    assert np.array_equal(g[:, :, 0], np.tile([-1.0, 26.0, -1.0], (4, 1)))
    assert np.all((g[:, :, 1] > 4.0 * (0.0 - 0.6)) & (g[:, :, 1] < 4.0 * (1.0 - 0.6))) and len(np.unique(g[:, :, 1])) == 12
    assert np.array_equal(seq.count, [3] * 4) and seq.B == 4 and seq.goal(0, 3) is None and seq.goal(4, 0) is None
    # another seed, other goals; the same seed, the same goals
    assert not np.array_equal(GoalSequences.flap(4, 3, 6).leg_goals(1), seq.leg_goals(1))
    assert np.array_equal(GoalSequences.flap(4, 3, 5).leg_goals(1), seq.leg_goals(1))


def test_take():
    seq = _table()
    sub = seq.take([3, 0, 3])
    assert sub.B == 3 and np.array_equal(sub.count, [64, 1, 64]) and np.array_equal(sub.seq_begin, [0, 64, 65, 129])
    for j, b in enumerate([3, 0, 3]):
        assert np.array_equal(sub.goals_of(j), seq.goals_of(b))
    assert np.array_equal(sub.first(), seq.first()[[3, 0, 3]])
    flap = GoalSequences.flap(5, 4, 99, mission_ids=[10, 11, 12, 2 ** 31 - 1, 14])
    one = flap.take([3, 1])
    assert one.B == 2 and np.array_equal(one.mission_ids, [2 ** 31 - 1, 11]) and one.legs == 4 and one.seed == 99
    for k in range(4):      # a mission's goals do not depend on the fleet it is listed in
        assert np.array_equal(one.leg_goals(k), flap.leg_goals(k)[[3, 1]])


# ------------------------------------------------------------------ header and exports
NEW = {"neo_fleet_leg_close_dev": 14, "neo_fleet_leg_open_dev": 24, "neo_fleet_leg_goal": 8}


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(REPO, "include", "neo_planner.h")).read()
    build.build()
    lib = _lib.load()
    for name, nargs in NEW.items():
        m = re.search(r"^int %s\(neo_ctx \*ctx,([^)]*)\)\s*;" % name, header, re.M)
        assert m, name
        assert len(m.group(1).split(",")) + 1 == nargs, name
        assert name in _lib.EXPORTS
        assert len(getattr(lib, name).argtypes) == nargs, name
    for gone in ("neo_fleet_leg_close", "neo_fleet_leg_open", "neo_fleet_leg_goal_dev"):      # resident arrays only; the goal call is the host's
        assert not re.search(r"\b%s\s*\(" % gone, header)
    assert re.search(r"#define\s+NEO_ABI_VERSION\s+1\b", header)
    assert re.search(r"^#define NEO_FLEET_LEGS_MAX 64\b", header, re.M) and _lib.NEO_FLEET_LEGS_MAX == 64
    assert re.search(r"^#define NEO_LEG_FIELDS %d\b" % len(_lib.LEG_FIELDS), header, re.M) and _lib.NEO_LEG_FIELDS == 21
    for name in ("LANDED", "ABANDONED", "TIMEOUT", "STUCK", "OPEN"):
        assert re.search(r"^#define NEO_LEG_%s %d\b" % (name, getattr(_lib, "NEO_LEG_" + name)), header, re.M), name
    for name in ("TABLE", "FLAP"):
        assert re.search(r"^#define NEO_LEGS_%s %d\b" % (name, getattr(_lib, "NEO_LEGS_" + name)), header, re.M), name
    at = {name: k for k, name in enumerate(_lib.LEG_FIELDS)}
    for name in ("goal_x", "goal_y", "start_x", "start_y", "outcome", "n_flown", "final_dist", "flags", "count", "audit_flags", "success"):
        assert re.search(r"^\s*NEO_LEG_%s = %d\b" % (name.upper(), at[name]), header, re.M), name
    assert re.search(r"^\s*NEO_LEG_AUDIT = %d\b" % at[_lib.AUDIT_FIELDS[0]], header, re.M)
    assert _lib.LEG_FIELDS[at["path_length"]:at["success"]] == _lib.AUDIT_FIELDS
    # the struct the binding hands over is the header's, field for field
    body = re.search(r"typedef struct neo_leg_sequences \{(.*?)\} neo_leg_sequences;", header, re.S).group(1)
    names = re.findall(r"(\w+)(?:\[\d+\])?\s*[;,]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f[0] for f in _lib.NeoLegSequences._fields_]
    assert npa.GoalSequences is GoalSequences and "GoalSequences" in npa.__all__


# ------------------------------------------------------------------ argument errors
def test_goal_sequences_argument_errors():
    g = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [2.0, 2.0]])
    ok = GoalSequences(g, [0, 1, 4])
    assert ok.B == 2 and np.array_equal(ok.count, [1, 3]) and ok.kind == _lib.NEO_LEGS_TABLE
    bad_g = g.copy()
    bad_g[2, 1] = np.inf
    for args in ((bad_g, [0, 1, 4]),                          # not finite
                 (g, [0, 0, 4]),                              # a mission without a goal
                 (g, [1, 4]),                                 # not from 0
                 (g, [0, 3, 2, 4]),                           # not ascending
                 (g, [0, 2]),                                 # not all the goals
                 (g, [0.0, 4.0]),                             # not integers
                 (g.reshape(-1), [0, 4]),                     # not (NG, 2)
                 (np.zeros((65, 2)), [0, 65])):               # more than 64 goals
        with pytest.raises(ValueError):
            GoalSequences(*args)
    GoalSequences(np.zeros((64, 2)), [0, 64])
    with pytest.raises(ValueError):
        GoalSequences.from_lists([[[1.0, 2.0]], []])
    for kw in (dict(legs=0), dict(legs=65), dict(B=-1), dict(seed=-1), dict(seed=2 ** 64), dict(mission_ids=[0, 1]),
               dict(mission_ids=[0, 1, 2 ** 31]), dict(mission_ids=[0, -1, 2]), dict(mission_ids=[0.0, 1.0, 2.0]),
               dict(x_pair=(1.0, np.nan)), dict(x_pair=(1.0, 2.0, 3.0)), dict(y_scale=np.inf), dict(y_shift=np.nan)):
        args = dict(B=3, legs=2, seed=1)
        args.update(kw)
        with pytest.raises(ValueError):
            GoalSequences.flap(**args)
    assert GoalSequences.flap(3, 64, 2 ** 64 - 1, mission_ids=[0, 1, 2 ** 31 - 1]).B == 3


def test_fleet_loop_campaign_argument_errors_without_a_device():
    class Cfg:
        v_max, init_wpts_num = 1.0, 2

    class FakePlanner:
        cfg = Cfg()
    seq = GoalSequences.from_lists([[[5.0, 0.0], [9.0, 1.0]], [[4.0, 2.0]], [[3.0, 3.0], [2.0, 2.0], [1.0, 1.0]]])
    sig = inspect.signature(npa.FleetReplanLoop.__init__).parameters
    assert sig["goal_sequences"].default is None and sig["leg_timeout"].default is None and sig["max_legs"].default is None
    loop = npa.FleetReplanLoop(FakePlanner(), None, None, goal_sequences=seq)
    assert loop.B == 3 and np.array_equal(loop.goals, seq.first()) and loop.max_legs == 3 and loop.leg_timeout is None
    assert loop.sequences is seq and loop._dev is None
    loop = npa.FleetReplanLoop(FakePlanner(), None, np.zeros((3, 2)), goal_sequences=seq, max_legs=2, leg_timeout=45, mode="batch",
                               jitter="counter", resident=True)
    assert loop.max_legs == 2 and loop.leg_timeout == 45.0 and np.array_equal(loop.goals, seq.first())
    routes = GoalRoutes.from_lists([[[0.0, 0.0], [1.0, 1.0]]] * 3, [1.0] * 3)
    for kw in (dict(goal_sequences=seq, goal_routes=routes),            # a route never lands
               dict(goal_sequences=seq, mode="warmstart"),              # which plan is a leg's first is not kept per mission
               dict(goal_sequences=seq, mode="geo"),
               dict(goal_sequences=[[[1.0, 2.0]]] * 3),                 # not a GoalSequences
               dict(goal_sequences=seq, leg_timeout=0.0),
               dict(goal_sequences=seq, leg_timeout=-1.0),
               dict(goal_sequences=seq, leg_timeout=float("nan")),
               dict(goal_sequences=seq, leg_timeout=float("inf")),
               dict(goal_sequences=seq, max_legs=0),
               dict(goal_sequences=seq, max_legs=65),
               dict(goal_sequences=seq, max_legs=1.5),
               dict(goal_sequences=seq, mission_ids=[0, 1]),
               dict(leg_timeout=3.0),                                   # campaign arguments without a campaign
               dict(max_legs=2)):
        with pytest.raises(ValueError):
            npa.FleetReplanLoop(FakePlanner(), None, None if "goal_sequences" in kw else np.zeros((3, 2)), **kw)
    with pytest.raises(ValueError):
        npa.FleetReplanLoop(FakePlanner(), None, np.zeros((2, 2)), goal_sequences=seq)
    # a flap's streams are keyed by the loop's mission ids
    flap = GoalSequences.flap(3, 2, 1, mission_ids=[4, 5, 6])
    assert npa.FleetReplanLoop(FakePlanner(), None, None, goal_sequences=flap, mission_ids=[4, 5, 6]).max_legs == 2
    with pytest.raises(ValueError, match="mission ids"):
        npa.FleetReplanLoop(FakePlanner(), None, None, goal_sequences=flap)
    # and nothing moved for a loop without one
    plain = npa.FleetReplanLoop(FakePlanner(), None, np.zeros((3, 2)))
    assert plain.sequences is None and plain.max_legs is None and plain.leg_timeout is None
