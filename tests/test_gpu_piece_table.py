"""The piece table (csrc/neo_pieces.hpp) behind neo_eval_traj_batch, neo_audit_traj_batch and neo_fleet_splice_dev at the
shapes where its scatter of x from global memory into LDS can go wrong: where a 64-element FLAT slot ends.  At every
shape the three consumers are laid beside each other (the audit against the rows, the splice against the rows bit for
bit) and the rows beside the NumPy oracle; one request of every batch has a tau beyond exp's range, where each consumer
refuses in its own way."""
import ctypes

import numpy as np
import pytest

import neo_planner_amd as npa
from neo_planner_amd import _lib, synth
from test_gpu_audit import _check_self_consistent, _eval_rows

pytestmark = pytest.mark.gpu

B, HZ = 8, 10.0
BAD = 5  # the request whose solve fails
# (D, M): n = D (M - 1) + M around the slot ends 64, 128 and 192, the smallest problems and the largest
SHAPES_2D = [1, 2, 22, 23, 43, 44, 64]      # n = 1, 4, 64 (first slot exactly full), 67, 127, 130, 190
SHAPES_3D = [17, 33, 49, 64]                # n = 65, 129, 193 (first element of the fourth slot), 253
SHAPES = [(2, M) for M in SHAPES_2D] + [(3, M) for M in SHAPES_3D]

# Largest relative row error against OraclePlanner.get_full_state_cmd, max |row - oracle| / max |oracle| per order
# (position, velocity, acceleration) over the batch and the largest of the three, MEASURED with the library of the commit
# before the piece table on exactly these inputs (the kernels' outputs have the same bits since).  The oracle solves the
# dense 6M x 6M system with LAPACK, the kernel the block-tridiagonal one; the acceleration rows carry most of it at every
# M.  The test asserts four times the measured value, the margin the suite's other oracle bars leave for another
# summation order in NumPy.
MEASURED = {
    (2, 1): 1.186e-14, (2, 2): 9.028e-15, (2, 22): 1.057e-14, (2, 23): 1.365e-14, (2, 43): 8.900e-15, (2, 44): 1.196e-14,
    (2, 64): 1.195e-14,
    (3, 17): 1.232e-14, (3, 33): 1.614e-14, (3, 49): 1.037e-14, (3, 64): 9.969e-15,
}


_CTX = []


def context():
    """a context of this module's own: its maps add no slot to the default context's map tables, which other modules'
    tests count on"""
    if not _CTX:
        _CTX.append(_lib.Context())
    return _CTX[0]


def requests(D, M):
    """B requests drawn like synth.replan_requests, durations inside [T_min, T_max] = [0.5, 5] and all different; row BAD
    has one tau with -tau > 709.79"""
    kw = synth.VOLUME if D == 3 else {}
    head, tail, wp, ts = synth.replan_requests(3, B, M - 1, D=D, init_T=0.8, **kw)
    ts = ts * np.random.default_rng(100 * D + M).uniform(0.8, 1.25, ts.shape)
    bp = npa.BatchPlanner(ctx=context())
    x = bp.pack_x(wp, ts)
    x[BAD, D * (M - 1) + M // 2] = -720.0
    return bp, x, head, tail


_CASES = {}


def case(D, M):
    """the inputs of a shape and neo_eval_traj_batch's rows and counts for them: computed once, read by every test"""
    if (D, M) not in _CASES:
        bp, x, head, tail = requests(D, M)
        with np.errstate(over="ignore"):  # (unpack_x of the row whose exp(-tau) overflows)
            rows, cnt = _eval_rows(bp, x, head, tail, HZ)
        rows.setflags(write=False)
        cnt.setflags(write=False)
        _CASES[(D, M)] = (bp, x, head, tail, rows, cnt)
    return _CASES[(D, M)]


def oracle_error(D, M):
    """(largest relative row error, per-order errors) of a shape's rows against the oracle"""
    from oracle import minco_np as onp
    bp, x, head, tail, rows, cnt = case(D, M)
    with np.errstate(over="ignore"):
        wp, ts = bp.unpack_x(x, M, D)
    diff, scale = np.zeros(3), np.zeros(3)
    for b in range(B):
        if b == BAD:
            continue
        pl = onp.OraclePlanner(onp.PlannerParams())
        pl.read_planning_conditions(None, head[b], tail[b], wp[b], ts[b])
        st = pl.get_full_state_cmd(HZ)
        frac = ts[b].sum() * HZ
        if abs(frac - round(frac)) > 1e-9:  # (np.arange's length is not a matter of the last bit of the duration)
            assert len(st) == cnt[b], (b, len(st), cnt[b])
        k = min(len(st), cnt[b])
        for o in range(3):
            diff[o] = max(diff[o], np.abs(rows[b, :k, o] - st[:k, o]).max())
            scale[o] = max(scale[o], np.abs(st[:k, o]).max())
    rel = diff / scale
    return rel.max(), rel


@pytest.fixture(scope="module")
def map2d():
    m = npa.ESDF(ctx=context())
    m.occupancy_map_cb(synth.OccupancyGridMsg(synth.occupancy_2d(1)))
    return m


@pytest.fixture(scope="module")
def map3d():
    return npa.ESDF3D(synth.esdf_3d(2, n=120, res=0.25), 0.25, synth.DOMAIN_ORIGIN, store="f32", layout="linear",
                      ctx=context())


@pytest.mark.parametrize("D,M", SHAPES)
def test_rows_counts_and_audit_are_consistent(D, M, map2d, map3d):
    bp, x, head, tail, rows, cnt = case(D, M)
    assert cnt[BAD] == -1 and np.all(np.delete(cnt, BAD) > 0)       # the rows' refusal: count -1
    with np.errstate(over="ignore"):
        out = _check_self_consistent(bp, map2d if D == 2 else map3d, x, head, tail, HZ)
    # the audit's refusal: a NaN record, no samples, NONFINITE
    assert out["count"][BAD] == 0 and out["flags"][BAD] == _lib.NEO_AUDIT_FLAG_NONFINITE
    assert all(np.isnan(out[f][BAD]) for f in ("path_length", "min_clearance", "max_speed", "duration"))
    assert not np.isnan(np.delete(out["weighted"], BAD)).any()


@pytest.mark.parametrize("M", SHAPES_2D)
def test_splice_writes_the_rows_bit_for_bit(M):
    """as test_gpu_fleet.py::test_splice_writes_eval_traj_rows_at_the_look_ahead_index does at M = 3"""
    import torch
    dev = torch.device("cuda", 0)
    bp, x, head, tail, rows, cnt = case(2, M)
    ctx = bp.ctx
    cap, sentinel, guard = int(cnt.max()) + 7, 777.0, 1024
    fut = (np.arange(B) % 5).astype(np.int32)
    old = np.random.default_rng(M).normal(0, 1, (B, cap, 3, 2))
    buf = torch.full((B * cap * 6 + guard,), sentinel, dtype=torch.float64, device=dev)
    buf[:B * cap * 6] = torch.from_numpy(old).to(dev).reshape(-1)
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (x, head, tail)]
    d_len = torch.full((B,), 3, dtype=torch.int32, device=dev)
    d_idx = torch.full((B,), 2, dtype=torch.int32, device=dev)
    d_fut = torch.from_numpy(fut).to(dev)
    d_flags = torch.zeros(B, dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    torch.cuda.synchronize(dev)
    ctx.check(ctx.lib.neo_fleet_splice_dev(ctx.h, B, None, 0, M, p(d[0]), p(d[1]), p(d[2]), None, HZ, 0, p(buf), cap, p(d_len),
                                           p(d_idx), p(d_fut), p(d_flags)))
    ctx.synchronize()
    out = buf.cpu().numpy()
    assert np.all(out[B * cap * 6:] == sentinel), "written past the buffer"
    new = out[:B * cap * 6].reshape(B, cap, 3, 2)
    flags, new_len = d_flags.cpu().numpy(), d_len.cpu().numpy()
    for b in range(B):
        if b == BAD:    # the splice's refusal: the array and its length stay, SPLICE_FAILED
            assert np.array_equal(new[b], old[b]) and new_len[b] == 3 and flags[b] == _lib.NEO_FLEET_FLAG_SPLICE_FAILED
            continue
        at = int(fut[b])
        k = min(int(cnt[b]), cap - at)
        assert np.array_equal(new[b, :at], old[b, :at])
        assert np.array_equal(new[b, at:at + k], rows[b, :k])     # neo_eval_traj_batch's rows, bit for bit
        assert np.array_equal(new[b, at + k:], old[b, at + k:])
        assert new_len[b] == at + k
        assert flags[b] == (_lib.NEO_FLEET_FLAG_CMD_FULL if at + cnt[b] > cap else 0)
    assert np.array_equal(d_idx.cpu().numpy(), np.full(B, 2)) and np.array_equal(d_fut.cpu().numpy(), fut)


@pytest.mark.parametrize("D,M", SHAPES)
def test_rows_against_the_oracle(D, M):
    err, per_order = oracle_error(D, M)
    print(f"D = {D} M = {M}: relative row error {err:.3e} (pos / vel / acc {per_order}), measured {MEASURED[(D, M)]:.3e}")
    assert err <= 4.0 * MEASURED[(D, M)], (D, M, err, MEASURED[(D, M)])
