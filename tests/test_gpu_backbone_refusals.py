"""neo_backbone_features_dev's argument errors: every refusal include/neo_planner.h lists returns NEO_ERR_INVALID with a
neo_last_error text before anything is launched, and n = 0 is a no-op.  The same for its measuring forms,
neo_backbone_launch_times and neo_backbone_activation_dev (launch, act_out, act_floats)."""
import ctypes

import numpy as np
import pytest

from neo_planner_amd import _lib

pytestmark = pytest.mark.gpu

NEO_ERR_INVALID = 1
N, H, W = 2, 9, 13


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def test_refusals_and_the_empty_call():
    import torch
    dev = torch.device("cuda", 0)
    c = _lib.default_context()
    L = c.lib
    need = int(L.neo_backbone_workspace_bytes(N, H, W))
    blob = torch.zeros(_lib.NEO_BACKBONE_FLOATS, dtype=torch.float32, device=dev)
    img = torch.zeros((N, H, W), dtype=torch.uint8, device=dev)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    out = torch.full((N, 24), -7.25, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    good = dict(weights=_p(blob), n_weights=blob.numel(), images=_p(img), n=N, H=H, W=W, workspace=_p(ws), workspace_bytes=need,
                out=_p(out))

    def call(**change):
        a = dict(good, **change)
        return L.neo_backbone_features_dev(c.h, a["weights"], a["n_weights"], a["images"], a["n"], a["H"], a["W"], a["workspace"],
                                           a["workspace_bytes"], a["out"])

    bad = [dict(weights=None), dict(images=None), dict(workspace=None), dict(out=None), dict(n=-1), dict(H=0), dict(W=0),
           dict(H=-3), dict(n_weights=blob.numel() - 1), dict(n_weights=blob.numel() + 1), dict(n_weights=0),
           dict(workspace_bytes=need - 1), dict(workspace_bytes=0)]
    for change in bad:
        assert call(**change) == NEO_ERR_INVALID, change
        assert b"backbone" in L.neo_last_error(c.h), change
    assert L.neo_backbone_features_dev(None, *[good[k] for k in ("weights", "n_weights", "images", "n", "H", "W", "workspace",
                                                                 "workspace_bytes", "out")]) == NEO_ERR_INVALID
    assert call(n=0) == _lib.NEO_OK and call(n=0, workspace_bytes=0) == _lib.NEO_OK
    c.synchronize()
    assert (out.cpu().numpy() == np.float32(-7.25)).all()          # nothing was launched by any of them
    assert call() == _lib.NEO_OK
    c.synchronize()
    got = out.cpu().numpy()
    assert np.isfinite(got).all() and (got == 0.0).all()            # a zero blob: zero features
    # the measuring form: the same checks, the same features, and a time for each of the 21 launches
    ms = (ctypes.c_float * _lib.NEO_BACKBONE_LAUNCHES)()
    a = good
    args = (a["weights"], a["n_weights"], a["images"], a["n"], a["H"], a["W"], a["workspace"], a["workspace_bytes"], a["out"])
    assert L.neo_backbone_launch_times(c.h, *args, None) == NEO_ERR_INVALID
    assert L.neo_backbone_launch_times(c.h, *args[:1], 5, *args[2:], ms) == NEO_ERR_INVALID
    assert L.neo_backbone_launch_times(c.h, *args, ms) == _lib.NEO_OK
    assert all(0.0 < t < 1e3 for t in ms) and (out.cpu().numpy() == 0.0).all()
    # one launch's output: the same checks (act_out in feature_out's place), and its own three arguments
    h, w, ch = (ctypes.c_int() for _ in range(3))
    launch = 7
    assert L.neo_backbone_activation_shape(launch, H, W, ctypes.byref(h), ctypes.byref(w), ctypes.byref(ch)) == _lib.NEO_OK
    floats = N * h.value * w.value * ch.value
    act = torch.full((floats,), -7.25, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    good_act = dict(good, launch=launch, out=_p(act), act_floats=floats)

    def call_act(**change):
        a = dict(good_act, **change)
        return L.neo_backbone_activation_dev(c.h, a["weights"], a["n_weights"], a["images"], a["n"], a["H"], a["W"], a["workspace"],
                                             a["workspace_bytes"], a["launch"], a["out"], a["act_floats"])

    for change in bad + [dict(launch=-1), dict(launch=_lib.NEO_BACKBONE_LAUNCHES), dict(act_floats=floats - 1),
                         dict(act_floats=floats + 1), dict(act_floats=0), dict(launch=20), dict(launch=0), dict(n=0)]:
        assert call_act(**change) == NEO_ERR_INVALID, change       # (launches 20 and 0 and n = 0: other sizes than `floats`)
        assert b"backbone" in L.neo_last_error(c.h), change
    assert L.neo_backbone_activation_dev(None, *args[:8], launch, _p(act), floats) == NEO_ERR_INVALID
    assert call_act(n=0, act_floats=0) == _lib.NEO_OK
    c.synchronize()
    assert (act.cpu().numpy() == np.float32(-7.25)).all()          # nothing was launched or copied by any of them
    assert call_act() == _lib.NEO_OK
    c.synchronize()
    assert (act.cpu().numpy() == 0.0).all() and (out.cpu().numpy() == 0.0).all()
