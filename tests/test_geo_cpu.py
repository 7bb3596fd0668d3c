"""The CPU restatement of the geo warm start (tests/geo_oracle_np.py) against the reference's own results
(tests/golden/g7_geo_*.npz, tools/gen_golden_geo.py): equal, not close.  No GPU."""
import glob
import math
import os

import numpy as np
import pytest
from scipy import ndimage

import geo_oracle_np as geo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENES = ("scene0", "scene1", "scene2", "res025", "pocket")


def fixture(name):
    return np.load(os.path.join(GOLDEN, f"g7_geo_{name}.npz"))


def oracle_map(d):
    """esdf.py:occupancy_map_cb on the stored occupancy"""
    occ = (np.asarray(d["occ"]) == 100).astype(np.int64)
    esdf = ndimage.distance_transform_edt(1 - occ) * float(d["res"])
    return geo.Map(esdf, float(d["res"]), d["origin"])


def test_fixtures_exist():
    assert len(glob.glob(os.path.join(GOLDEN, "g7_geo_*.npz"))) == 6


@pytest.mark.parametrize("name", SCENES)
def test_restatement_equals_reference(name):
    d = fixture(name)
    m = oracle_map(d)
    g = geo.Grid(m)
    for i in range(len(d["start"])):
        path, cost, _, flags = geo.astar(g, d["start"][i], d["target"][i])
        n = int(d["path_len"][i])
        assert len(path) == n, (name, i)
        assert np.array_equal(np.array(path), d["paths"][i, :n]), (name, i)
        assert cost == d["path_cost"][i], (name, i)
        pruned, _ = geo.prune(m, path)
        assert np.array_equal(np.array(pruned), d["pruned"][i]), (name, i)


def test_fixtures_cover_the_cases():
    """no path (blocked target and the sealed pocket), start == target, a start in collision, every prune branch"""
    flags, branches, lengths = [], set(), []
    for name in SCENES:
        d = fixture(name)
        m = oracle_map(d)
        g = geo.Grid(m)
        for i in range(len(d["start"])):
            path, _, nexp, f = geo.astar(g, d["start"][i], d["target"][i])
            flags.append(f)
            lengths.append(len(path))
            branches.add(min(geo.prune(m, path)[1], 5))
            sx, sy = g.index(*d["start"][i])
            if 0 <= sx < g.We and 0 <= sy < g.He and g.blocked[sy, sx] and len(path) > 1:
                branches.add("start_blocked")
        if name == "pocket":
            assert nexp > 0 and f == 0
    assert geo.NO_PATH in flags and 1 in lengths
    assert {1, 2, 3, 4, 5, "start_blocked"} <= branches, branches
    # the sealed pocket: a free target, searched exhaustively
    d = fixture("pocket")
    g = geo.Grid(oracle_map(d))
    _, _, nexp, f = geo.astar(g, d["start"][0], d["target"][0])
    tx, ty = g.index(*d["target"][0])
    assert f == geo.NO_PATH and not g.blocked[ty, tx] and nexp > 1000


def test_hypot_is_the_correctly_rounded_sqrt():
    """math.hypot of two integers equals sqrt(i*i + j*j) over the index range the tests use (the kernel's formula)"""
    i = np.arange(0, 1200)
    for a in range(0, 1200):
        ref = np.array([math.hypot(a, b) for b in range(0, 1200)])
        assert np.array_equal(ref, np.sqrt((a * a + i * i).astype(np.float64))), a


def _free_map():
    return geo.Map(np.full((100, 100), 5.0), 0.1, (0.0, 0.0))


def test_prune_branches_on_constructed_paths():
    m = _free_map()
    line = [[0.5 + 0.1 * k, 0.5] for k in range(31)]
    # one node: four copies of it
    assert geo.prune(m, line[:1]) == ([line[0]] * 4, 1)
    # a straight feasible path: two key indices, np.linspace(0, 30, 4).astype(int) = 0, 10, 20, 30
    assert geo.prune(m, line) == ([line[0], line[10], line[20], line[30]], 2)
    # a wall across the middle: keys at the corners
    esdf = np.full((100, 100), 5.0)
    esdf[0:60, 40] = 0.0
    mw = geo.Map(esdf, 0.1, (0.0, 0.0))
    up = [[0.5 + 0.1 * k, 0.5] for k in range(30)]            # to (3.4, 0.5)
    climb = [[3.4, 0.6 + 0.1 * k] for k in range(60)]         # to (3.4, 6.5)
    over = [[3.5 + 0.1 * k, 6.5] for k in range(20)]          # to (5.4, 6.5)
    path = up + climb + over
    pruned, nkeys = geo.prune(mw, path)
    assert nkeys >= 3 and pruned[0] == path[0] and pruned[-1] == path[-1]
