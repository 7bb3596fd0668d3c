"""The walk of the all-fp32 optimiser's two-loop recursion over a memory of exactly COL pairs (csrc/neo_lbfgs_dir.hpp
hist_walk_full: the control flow DevBackend::direction_full of csrc/neo_kernels.hpp runs on the device for COL = m = 10, with
the arithmetic behind a visitor), compiled for the host with a visitor that prints its events
(tests/host_harness/hist_schedule_host.cpp).  For every COL in 1 .. 10 and head in 0 .. 9 (col = 0 is the steepest-descent
direction: no walk; on the device every col below m runs the plain loops themselves):

  * the steps are those of the two plain loops of DevBackend::direction, in their order: (loop, slot of pair A, slot of
    pair B), with the scaling by 1 / theta between the loops; the slots a step is given are those of the pairs it names;
  * every pair is read exactly once, from its slot, and what a step takes from registers is a pair that was read: before
    the step IN FRONT of the one that first uses it computes (one step ahead), the first step's pairs before anything;
  * no read follows the scaling: loop 2 works on what loop 1 left in the registers."""
import os
import subprocess

import pytest

from conftest import REPO

SRC = os.path.join(REPO, "tests", "host_harness", "hist_schedule_host.cpp")
INC = os.path.join(REPO, "neo-planner_amd", "csrc")
M = 10


def plain_loops(col, head, m):
    """(loop, A, B) of every step of DevBackend::direction as it is written: B = -1 in the single-pair tail steps"""
    slot_of = lambda k: head + k if head + k < m else head + k - m
    out = []
    k = col - 1
    while k >= 1:
        out.append((1, slot_of(k), slot_of(k - 1)))
        k -= 2
    if k == 0:
        out.append((1, slot_of(0), -1))
    k = 0
    while k + 1 < col:
        out.append((2, slot_of(k), slot_of(k + 1)))
        k += 2
    if k < col:
        out.append((2, slot_of(k), -1))
    return out


@pytest.fixture(scope="module")
def walks(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hist") / "hist_schedule_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I", INC, SRC, "-o", exe])
    table, cur = {}, None
    for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines():
        w = line.split()
        if w[0] == "walk":
            cur = table.setdefault((int(w[1]), int(w[2])), [])
        else:
            cur.append((w[0],) + tuple(int(x) for x in w[1:]))
    return table


def steps_of(events):
    """the arithmetic of a walk: (event index, loop, pairs (KA, KB), slots (A, B)) per step; KB = B = -1 in a single-pair step"""
    out = []
    for i, e in enumerate(events):
        if e[0] in ("pair1", "pair2"):
            out.append((i, int(e[0][-1]), (e[1], e[2]), (e[3], e[4])))
        elif e[0] in ("single1", "single2"):
            out.append((i, int(e[0][-1]), (e[1], -1), (e[2], -1)))
    return out


def test_every_col_and_head_is_walked(walks):
    assert sorted(walks) == [(col, head) for col in range(1, M + 1) for head in range(M)]


def test_the_steps_are_the_two_plain_loops(walks):
    for (col, head), events in walks.items():
        steps = steps_of(events)
        assert [(loop, A, B) for _, loop, _, (A, B) in steps] == plain_loops(col, head, M), (col, head)
        for _, _, pairs, slots in steps:                     # the slot handed to a step is the slot of the pair it names
            for k, slot in zip(pairs, slots):
                assert (k, slot) == (-1, -1) or slot == (head + k) % M, (col, head, pairs, slots)
        # q is scaled once, after the last step of loop 1 and before the first of loop 2
        seam = [i for i, e in enumerate(events) if e[0] == "seam"]
        assert len(seam) == 1
        assert all((i < seam[0]) == (loop == 1) for i, loop, _, _ in steps), (col, head)


def test_every_pair_is_read_once_and_one_step_ahead_of_its_first_use(walks):
    for (col, head), events in walks.items():
        reads = {}
        for i, e in enumerate(events):
            if e[0] == "read":
                k, slot = e[1:]
                assert k not in reads and 0 <= k < col and slot == (head + k) % M, (col, head, e)
                reads[k] = i
        assert sorted(reads) == list(range(col)), (col, head)          # every stored pair, and nothing else
        steps = steps_of(events)
        first_use = {}
        for n, (i, _, pairs, _) in enumerate(steps):
            for k in pairs:
                if k >= 0:
                    first_use.setdefault(k, n)
        for k, n in first_use.items():
            # read before the step in front of its first user computes; the first step's pairs before any step
            assert reads[k] < steps[max(n - 1, 0)][0], (col, head, k, n)
            # ... and not earlier than one step ahead: after the step two in front
            assert n < 2 or reads[k] > steps[n - 2][0], (col, head, k, n)
        seam = next(i for i, e in enumerate(events) if e[0] == "seam")
        assert max(reads.values()) < seam, (col, head)                  # loop 2 reads nothing
