"""Where the optimiser kernels keep their L-BFGS pairs in LDS (csrc/neo_lbfgs_dir.hpp hist_index, hist_record,
hist_index_rows: the one place DevBackend and GroupBackend take their positions from), and the launcher's condition for the
kernel that reads behind them (csrc/neo_launch_opt.hpp opt_lds_plan, opt_plan_fixed).

  * fp32 pairs: element e of the pair in `slot` is the record (s_e, y_e) at hist[(slot * n + e) * 2 + {0, 1}]; over
    (slot, e, which) the index is a bijection onto the 2 m n elements of the region, for m = 10 and every n in 1 .. 128
    (tests/host_harness/hist_layout_host.cpp, compiled with g++).  fp64 pairs keep the rows [2][m][n]: a bijection as well.
  * Under the fixed plan the written-out recursion reads a whole pair from one per-lane address without a condition: lane
    l of FLAT slot k reads record k * 64 + l of the pair whether or not the pair has one, so the reads of the last pair end
    (64 NS - n) records behind the region.  For every (D, M) a member with a fixed plan can be launched with, without and
    with the velocity stash: either the launcher does not call the launch fixed, or those reads end inside the launch's
    dynamic LDS (tests/host_harness/opt_plan_host.cpp: host code of a HIP header, compiled with hipcc for the host alone).
    The bytes are worked out here, from n alone, and not taken from the program."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO

HARNESS = os.path.join(REPO, "tests", "host_harness")
INC = os.path.join(REPO, "neo-planner_amd", "csrc")
M_PAIRS, N_MAX, WAVE = 10, 128, 64


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hist_layout") / "hist_layout_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I", INC,
                           os.path.join(HARNESS, "hist_layout_host.cpp"), "-o", exe])
    table, cur = {}, None
    for line in subprocess.run([exe, str(M_PAIRS), str(N_MAX)], capture_output=True, text=True, check=True).stdout.splitlines():
        w = line.split()
        if w[0] == "n":
            cur = table.setdefault(int(w[1]), [])
        else:
            cur.append(tuple(int(x) for x in w))
    return table


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("opt_plan") / "opt_plan_host")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-Wno-unused-value", "-I", INC,
                           "-I", os.path.join(REPO, "include"), os.path.join(HARNESS, "opt_plan_host.cpp"), "-o", exe])
    keys = ("D", "M", "NS", "stash", "stage", "pcr_off", "dyn", "over_read_elems", "fixed")
    return [dict(zip(keys, (int(x) for x in line.split())))
            for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()]


def test_the_index_is_a_bijection_onto_the_region(layout):
    assert sorted(layout) == list(range(1, N_MAX + 1))
    for n, rows in layout.items():
        assert [(slot, e) for slot, e, *_ in rows] == [(slot, e) for slot in range(M_PAIRS) for e in range(n)]
        seen = [i for _, _, i_s, i_y, *_ in rows for i in (i_s, i_y)]
        assert sorted(seen) == list(range(2 * M_PAIRS * n)), n


def test_the_rows_of_the_fp64_pairs_are_a_bijection_too(layout):
    for n, rows in layout.items():
        seen = [i for *_, r_s, r_y in rows for i in (r_s, r_y)]
        assert sorted(seen) == list(range(2 * M_PAIRS * n)), n
        for slot, e, _, _, _, r_s, r_y in rows:
            assert (r_s, r_y) == (slot * n + e, (M_PAIRS + slot) * n + e), (n, slot, e)


def test_s_and_y_of_an_element_are_one_record_and_a_pair_is_contiguous(layout):
    for n, rows in layout.items():
        for slot, e, i_s, i_y, rec, *_ in rows:
            assert (i_s, i_y) == (2 * rec, 2 * rec + 1) == ((slot * n + e) * 2, (slot * n + e) * 2 + 1), (n, slot, e)
        # the records of a pair in element order, pair after pair: FLAT slot k of a lane lies 64 records behind its slot 0
        assert [rec for _, _, _, _, rec, *_ in rows] == list(range(M_PAIRS * n)), n


def test_every_fixed_launch_keeps_the_reads_behind_the_pairs_inside_its_lds(plans):
    seen = set()
    for p in plans:
        D, M, NS = p["D"], p["M"], p["NS"]
        n = D * (M - 1) + M
        assert NS == -(-n // WAVE) and NS in (1, 2) and D * M <= WAVE, p
        seen.add((D, M))
        pairs_end = p["stage"] * 8 + 2 * M_PAIRS * n * 4                  # fp32 pairs behind `stage` doubles of staging
        over = (WAVE * NS - n) * 2 * 4                                    # the last pair read from lane records 0 .. 64 NS - 1
        assert p["over_read_elems"] * 4 == over, p
        assert not p["fixed"] or pairs_end + over <= p["dyn"], p
        if p["fixed"]:
            assert p["pcr_off"] * 8 >= pairs_end, p                       # what lies behind the pairs is the multipliers
    assert seen == {(D, M) for D in (2, 3) for M in range(1, WAVE // D + 1) if D * (M - 1) + M <= 2 * WAVE}


def test_the_shapes_the_gpu_tests_rely_on(plans):
    at = {(p["D"], p["M"], p["stash"] != 0): p for p in plans}
    # M = 2 with one FLAT slot: 472 bytes behind the pairs against 48 of multipliers -- the dynamic kernel; M = 3 likewise
    for M, over in ((2, 472), (3, 440)):
        assert at[3, M, True]["over_read_elems"] * 4 == over and not at[3, M, True]["fixed"] and not at[3, M, False]["fixed"]
    # the shapes of the fixed-plan tests stay fixed; cfg2's launch keeps its dynamic LDS
    for M in (12, 16, 17, 19, 21):
        assert at[3, M, True]["fixed"], M
    assert at[3, 21, True]["dyn"] == 12032 and at[3, 21, True]["over_read_elems"] * 4 == 376
