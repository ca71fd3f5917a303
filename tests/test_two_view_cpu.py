"""CPU-only checks of the batched two-view bundle adjustment's entry point (include/fgo.h fgo_two_view_ba_batch): the symbols
are exported, the defaults are the reference's (gtsam/gtsam_graph.cpp:513, 537, 539, 574), every bad argument is refused
before any HIP call, and a valid call FAILS LOUDLY without a GPU (no CPU fallback), as fgo_preint_batch does."""
import ctypes as C

import numpy as np

import graph_slam_amd as G

CALIB = np.array([250.5773, 250.5773, 0, 90, 70, -0.8466, 0.5370, 0, 0])


def _call(mp, n=None, xyz=True, uvi=True, uvj=True, calib=True, pose_j=True, res=True, params=None, bps=None):
    mp = np.asarray(mp, np.int64)
    n = len(mp) - 1 if n is None else n
    m = max(int(np.abs(mp).max()), 1)
    a = np.zeros((m, 3)); a[:, 2] = 1.5
    b = np.full((m, 2), 80.0); c = np.full((m, 2), 80.0)
    out = np.zeros((max(n, 1), 7)); r = (G.TwoViewResult * max(n, 1))()
    return G.lib.fgo_two_view_ba_batch(0, n, G._i64p(mp), G._dp(a) if xyz else None, G._dp(b) if uvi else None, G._dp(c) if uvj else None,
                                       None, G._dp(CALIB) if calib else None, None if bps is None else G._dp(np.asarray(bps, np.float64)),
                                       None if params is None else C.byref(params), G._dp(out) if pose_j else None, None, None, None,
                                       r if res else None)


def test_symbols_and_defaults():
    assert hasattr(G.lib, "fgo_two_view_ba_batch") and hasattr(G.lib, "fgo_two_view_params_default")
    p = G.TwoViewParams()
    G.lib.fgo_two_view_params_default(C.byref(p))
    assert (p.pose_prior_sigma, p.point_sigma, p.pixel_sigma, p.max_iters, p.min_matches) == (1e-7, 0.014, 1.0, 100, 5)
    G.lib.fgo_two_view_params_default(None)                      # tolerated
    assert C.sizeof(G.TwoViewResult) == 40 and C.sizeof(G.TwoViewParams) == 32
    assert G.two_view_params(min_matches=3).min_matches == 3


def test_bad_arguments_are_refused_without_a_device():
    assert _call([0, 6], n=-1) == -1
    assert _call([-1, 6]) == -1                                  # negative offset
    assert _call([0, 8, 6]) == -1                                # decreasing
    assert _call([0, 6], xyz=False) == -1
    assert _call([0, 6], uvi=False) == -1
    assert _call([0, 6], uvj=False) == -1
    assert _call([0, 6], calib=False) == -1
    assert _call([0, 6], pose_j=False) == -1
    assert _call([0, 6], res=False) == -1
    assert G.lib.fgo_two_view_ba_batch(0, 1, None, None, None, None, None, G._dp(CALIB), None, None, G._dp(np.zeros(7)), None, None, None,
                                       (G.TwoViewResult * 1)()) == -1
    big = np.array([0, (2 ** 31 - 1) // 3 + 1], np.int64)          # more matches in one pair than the kernel's int indices reach
    one = np.zeros(8)
    assert G.lib.fgo_two_view_ba_batch(0, 1, G._i64p(big), G._dp(one), G._dp(one), G._dp(one), None, G._dp(CALIB), None, None, G._dp(one), None,
                                       None, None, (G.TwoViewResult * 1)()) == -1
    for field in ("pose_prior_sigma", "point_sigma", "pixel_sigma"):
        for bad in (0.0, -1.0, float("nan")):
            assert _call([0, 6], params=G.two_view_params(**{field: bad})) == -1, (field, bad)
    assert _call([0, 6], params=G.two_view_params(min_matches=2)) == -1
    assert _call([0, 6], bps=[0, 0, 0, 0, 0, 0, 0]) == -1        # zero quaternion, as fgo_set_calib_ds2 refuses it


def test_empty_batch_is_ok_and_a_valid_call_needs_a_device():
    assert _call([0], n=0) == 0
    if G.lib.fgo_device_count() <= 0:
        assert _call([0, 6]) == -2
        assert _call([0, 6], params=G.two_view_params(min_matches=3, max_iters=0)) == -2
        try:
            G.two_view_ba_batch([0, 6], np.zeros((6, 3)), np.zeros((6, 2)), np.zeros((6, 2)), CALIB)
        except G.FgoError as e:
            assert "-2" in str(e)
        else:
            raise AssertionError("two_view_ba_batch returned without a device")


def test_python_wrapper_checks_shapes_before_the_call():
    import pytest
    ok = ([0, 6], np.zeros((6, 3)), np.zeros((6, 2)), np.zeros((6, 2)))
    with pytest.raises(G.FgoError, match="body_P_sensor"):
        G.two_view_ba_batch(*ok, CALIB, body_P_sensor=np.zeros(6))
    with pytest.raises(G.FgoError, match="calib9"):
        G.two_view_ba_batch(*ok, CALIB[:8])
    with pytest.raises(G.FgoError, match="pose_j0"):
        G.two_view_ba_batch(*ok, CALIB, pose_j0=np.zeros((2, 7)))
    with pytest.raises(G.FgoError, match="fewer"):
        G.two_view_ba_batch([0, 7], *ok[1:], CALIB)
