"""The planners' host layer, the parts that need no GPU, against what tools/gen_golden_planner.py recorded before the
layer was folded (tests/golden/planner_calls.json): the public signatures, the first error of every refused argument set
(tests/planner_cases.py: none may get as far as the device), and the structure the fold left behind -- one call layer, one
definition per idiom."""
import inspect
import json
import os
import re

import pytest

from conftest import GOLDEN
from helpers import _code_lines

import planner_cases as pc
from neo_planner_amd import _lib, depth, esdf, initializer, onboard, planner, record, sharding

RECORDED = json.load(open(os.path.join(GOLDEN, "planner_calls.json")))
# entry points that return a value, not a status, and the one drop whose status is deliberately not looked at
DIRECT = ("neo_scene_slot", "neo_optimize_state_bytes", "neo_effort_order_scratch_bytes", "neo_esdf_drop")


def test_the_public_signatures_are_the_recorded_ones():
    got = pc.signatures()
    assert set(got) == set(RECORDED["signatures"])
    for name, sig in RECORDED["signatures"].items():
        assert got[name] == sig, name
    # where importers find the classes
    import neo_planner_amd as npa
    assert npa.BatchPlanner is planner.BatchPlanner and npa.MinJerkPlanner is planner.MinJerkPlanner


def test_the_fixture_holds_every_refusal():
    assert set(RECORDED["refusals"]) == set(pc.REFUSALS)
    assert all(v.startswith(("ValueError: BatchPlanner.", "ValueError: ")) for v in RECORDED["refusals"].values())


@pytest.mark.parametrize("name", pc.REFUSALS)
def test_an_argument_set_is_refused_as_recorded(name):
    """type and full message of the first error, raised before any device use (the planner's context is a plain object)"""
    assert pc.refusal(name) == RECORDED["refusals"][name]


def test_context_call_looks_lib_up_when_called():
    """Context.call(name, *args) is check(lib.name(h, *args)), with `lib` read at call time: the recording proxy of the
    golden tests works by replacing ctx.lib"""
    class Lib:
        def __init__(self, rc):
            self.rc, self.seen = rc, []

        def neo_thing(self, h, *args):
            self.seen.append((h, args))
            return self.rc

        def neo_last_error(self, h):
            return b"what went wrong"

    c = _lib.Context.__new__(_lib.Context)
    c.h, c.lib = "handle", Lib(0)
    assert c.call("neo_thing", 1, None, "x") is None and c.lib.seen == [("handle", (1, None, "x"))]
    c.lib = other = Lib(3)
    with pytest.raises(_lib.NeoError, match="error 3: what went wrong"):
        c.call("neo_thing", 2)
    assert other.seen == [("handle", (2,))]
    c.h = None      # (nothing for __del__ to destroy)


def _code(module):
    return re.sub(r'""".*?"""', "", inspect.getsource(module), flags=re.S)


def test_the_host_layer_keeps_its_structure():
    """every status-returning entry point goes through Context.call -- in planner.py and its six siblings no `lib.neo_`
    outside the four direct calls --, BatchPlanner's part of the file derives a batch's shape, decodes a batch status and
    words the stream_ids refusal once each, and planner.py stays below what it had before the fold"""
    for module in (planner, esdf, onboard, initializer, depth, record, sharding):
        assert not re.search(r"\blib\.neo_(?!(?:%s)\b)" % "|".join(n[4:] for n in DIRECT), _code(module)), module.__name__
    source = inspect.getsource(planner)
    # BatchPlanner's part: the file without MinJerkPlanner, whose bodies keep the reference's shape
    batch = _code(planner).replace(re.sub(r'""".*?"""', "", inspect.getsource(planner.MinJerkPlanner), flags=re.S), "")
    assert "class BatchPlanner" in batch and "class MinJerkPlanner" not in batch
    for text in ("(n + D) // (D + 1)", "& 0xff", "stream_ids needs one id per request", "integers(0, 2 ** 62)",
                 "torch.cuda.synchronize", "np.ascontiguousarray(scene_ids, dtype=np.int32)"):
        assert batch.count(text) == 1, text
    assert batch.count("*= 1.5") == 2        # the first and the last start duration, in one function
    assert _code_lines(source) < 1148        # what planner.py had before
