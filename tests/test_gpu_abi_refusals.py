"""Refusals of the C ABI's list-launch entry points, call by call against a recording.

Every function of include/neo_planner.h whose parameters contain `int B, const int32_t *subset, int n_subset` -- the
`_dev` and the host forms -- is called four times:

  a  B = -1
  b  B = 0
  c  B = 1, a real one-element subset, n_subset = 2
  d  B = 1, the same subset, n_subset = 0

with every other pointer NULL, the scalars at their smallest valid values and, where one is taken, the scene id of an
uploaded 4 x 4 2-D map.  tests/golden/abi_refusals.json holds the (return code, neo_last_error text) of each call as the
library gave them BEFORE the entry points were rewritten on the shared skeletons of csrc/neo_abi_util.hpp (recorded with
NEO_PLANNER_LIB pointing at that build: `python tests/test_gpu_abi_refusals.py --record [path]`); the text counts only
where the code is not 0.

No call reaches a launch or a copy: (a) and (c) fall to list_check; in (b) and (d) the launch list is empty and a
pointer the entry needs is NULL, so its null check -- or a range check before it -- refuses.  Read for every listed
entry before recording: each checks its required pointers before it takes the lock, the entries that clear a counter
on an empty list (neo_batch_select*, neo_plan_merge*, neo_adaptive_merge_dev, neo_adaptive_bucket*) among them, so
case (d) is left out for none."""
import json
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(REPO, "tests", "golden", "abi_refusals.json")

# the scalars by parameter name: the smallest value the entry accepts (a new name must be added here on purpose)
INTS = {"M": 3, "D": 2, "K": 1, "cap": 1, "step": 1, "stride": 1, "tick": 0, "target": 0, "attempt": 0, "round": 0,
        "seed": 0, "ahead": 0, "first": 0, "reset": 0, "clear_bad": 0, "n_vertices": 0, "width": 1, "height": 1,
        "capacity": 1, "max_waypoints": 1, "grid_w": 1, "grid_h": 1, "hit": 0, "miss": 0, "lo": 0, "hi": 0,
        "feature_rows": 1, "n_weights": 20817, "x_stride": 7}          # x_stride >= n = D (M - 1) + M
CASES = ("a", "b", "c", "d")


def list_entry_points():
    header = open(os.path.join(REPO, "include", "neo_planner.h")).read()
    out = {}
    for m in re.finditer(r"\bint\s+(neo_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", header):
        params = " ".join(m.group(2).split())
        if "int B, const int32_t *subset, int n_subset" in params:
            out[m.group(1)] = [p.strip() for p in params.split(",")]
    assert out, "no list-launch entry points found in the header"
    return out


def arguments(name, params, case, ctx, scene_id, subset_dev, subset_host):
    subset = None if case in "ab" else (subset_dev if name.endswith("_dev") else subset_host)
    special = {"ctx": ctx.h, "scene_id": scene_id, "B": {"a": -1, "b": 0}.get(case, 1), "subset": subset,
               "n_subset": {"c": 2}.get(case, 0)}
    args = []
    for p in params:
        pname = p.split()[-1].lstrip("*")
        if pname in special:
            args.append(special[pname])
        elif "*" in p:
            args.append(None)
        elif p.startswith("double"):
            args.append(1.0)
        else:
            args.append(INTS[pname])
    return args


def run_calls():
    import torch
    from neo_planner_amd import _lib
    ctx = _lib.Context(0)
    try:
        field = np.ones((4, 4))
        zero = np.zeros((4, 4))
        scene_id = ctx.new_scene_id()
        ctx.check(ctx.lib.neo_esdf_upload_2d(ctx.h, scene_id, _lib.ptr(field), _lib.ptr(zero), _lib.ptr(zero), 4, 4, 1.0,
                                             0.0, 0.0))
        subset_t = torch.zeros(1, dtype=torch.int32, device="cuda")
        subset_np = np.zeros(1, np.int32)
        got = {}
        for name, params in list_entry_points().items():
            for case in CASES:
                args = arguments(name, params, case, ctx, scene_id, _lib.dev_ptr(subset_t), _lib.ptr(subset_np))
                rc = getattr(ctx.lib, name)(*args)
                got[f"{name}/{case}"] = [int(rc), ctx.lib.neo_last_error(ctx.h).decode() if rc else ""]
        ctx.synchronize()
        return got
    finally:
        ctx.close()


def test_refusals_match_the_recording():
    want = json.load(open(FIXTURE))
    assert sorted(want) == sorted(f"{n}/{c}" for n in list_entry_points() for c in CASES)
    got = run_calls()
    for key in sorted(want):
        assert got[key] == want[key], key
    # cases a and c are list_check's; nothing here is allowed to pass as a launch
    for key, (rc, msg) in want.items():
        if key[-1] in "ac":
            assert rc == 1 and (": B must be " in msg or msg.endswith(": bad subset size")), key


if __name__ == "__main__":
    for p in (REPO, os.path.join(REPO, "neo-planner_amd")):
        sys.path.insert(0, p)
    assert sys.argv[1:2] == ["--record"], "usage: test_gpu_abi_refusals.py --record [path]"
    path = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    got = run_calls()
    with open(path, "w") as f:      # one call a line
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(got[k])}" for k in sorted(got)) + "\n}\n")
    print("recorded", path)
