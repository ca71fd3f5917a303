"""CPU-only checks of the VRO RANSAC entry point (include/fgo.h fgo_vro_ransac_batch): the symbols are exported, the defaults are
the declared ones, the structs have the declared layout, every bad argument is refused before any HIP call, and a valid call FAILS
LOUDLY without a GPU (no CPU fallback), as fgo_two_view_ba_batch does."""
import ctypes as C

import numpy as np
import pytest

import graph_slam_amd as G

INT_MAX = 2 ** 31 - 1


def _call(n=1, ptr=None, params=None, drop=(), info=True, cov=True, inl=True, hyp=False):
    """one pair of 10 matches unless told otherwise; `drop` names required pointers passed as NULL"""
    mp = np.asarray([0, 10] if ptr is None else ptr, np.int64)
    m = 16
    xi = np.random.default_rng(0).uniform(1, 2, (m, 3)); xj = xi.copy()
    k = G.vro_params().hypotheses if params is None else max(params.hypotheses, 1)
    pose = np.zeros((max(n, 1), 7)); nf = np.zeros((max(n, 1), 21)); cv = np.zeros((max(n, 1), 36)); mask = np.zeros(m, np.uint8)
    hc = np.zeros((max(n, 1), min(k, 1 << 20)), np.int32)
    res = (G.VroResult * max(n, 1))()
    arg = lambda name, v: None if name in drop else v
    return G.lib.fgo_vro_ransac_batch(
        0, n, arg("ptr", G._i64p(mp)), arg("xi", G._dp(xi)), arg("xj", G._dp(xj)), None if params is None else C.byref(params),
        arg("pose", G._dp(pose)), G._dp(nf) if info else None, G._dp(cv) if cov else None,
        mask.ctypes.data_as(C.POINTER(C.c_ubyte)) if inl else None, hc.ctypes.data_as(C.POINTER(C.c_int32)) if hyp else None,
        arg("res", res))


def test_symbols_defaults_and_struct_layout():
    for s in ("fgo_vro_ransac_batch", "fgo_vro_params_default"):
        assert hasattr(G.lib, s), s
    for s in ("vro_ransac_batch", "vro_params", "VroParams", "VroResult", "FGO_VRO_OK", "FGO_VRO_TOO_FEW", "FGO_VRO_NUM"):
        assert hasattr(G, s), s
    assert (G.FGO_VRO_OK, G.FGO_VRO_TOO_FEW, G.FGO_VRO_NUM) == (0, 1, 2)
    p = G.VroParams()
    G.lib.fgo_vro_params_default(C.byref(p))
    assert (p.hypotheses, p.seed, p.max_dist, p.min_side, p.rigid_tol, p.refine_rounds, p.min_inliers) == (5000, 0, 0.03, 0.05, 0.03, 3, 8)
    assert (p.fx, p.fy, p.sigma_px, list(p.sigma_z)) == (250.5773, 250.5773, 1.0, [0.014, 0.0, 0.0])
    G.lib.fgo_vro_params_default(None)                           # tolerated
    # C layout: int, (pad), uint64, 3 doubles, 2 ints, 3 doubles, double[3]
    assert C.sizeof(G.VroParams) == 96 and C.sizeof(G.VroResult) == 32
    V = G.VroParams
    assert (V.hypotheses.offset, V.seed.offset, V.max_dist.offset, V.refine_rounds.offset, V.min_inliers.offset, V.fx.offset,
            V.sigma_z.offset) == (0, 8, 16, 40, 44, 48, 72)
    R = G.VroResult
    assert (R.status.offset, R.n_inliers.offset, R.best_hypothesis.offset, R.best_count.offset, R.n_valid.offset, R.rounds.offset,
            R.rmse.offset) == (0, 4, 8, 12, 16, 20, 24)
    q = G.vro_params(hypotheses=7, sigma_z=(0.01, 0.002, 0.0), seed=2 ** 63 + 5)
    assert (q.hypotheses, list(q.sigma_z), q.seed, q.max_dist) == (7, [0.01, 0.002, 0.0], 2 ** 63 + 5, 0.03)
    with pytest.raises(TypeError):
        G.vro_params(no_such_field=1)


def test_bad_arguments_are_refused_without_a_device():
    E = -1
    assert _call(n=-1) == E
    for name in ("ptr", "xi", "xj", "pose", "res"):               # a NULL required pointer
        assert _call(drop=(name,)) == E, name
    assert _call(ptr=[-1, 5]) == E                                # negative
    assert _call(n=2, ptr=[0, 8, 4]) == E                         # decreasing
    assert _call(ptr=[0, INT_MAX // 3 + 1]) == E                  # too many matches in one pair
    nan = float("nan")
    bad = dict(hypotheses=(0, -5, (1 << 20) + 1), max_dist=(0.0, -1.0, nan), min_side=(0.0, -0.1, nan), fx=(0.0, -250.0, nan),
               fy=(0.0, -250.0, nan), sigma_px=(0.0, -1.0, nan), rigid_tol=(-1e-9, nan), refine_rounds=(-1, 11), min_inliers=(2, 0, -1),
               sigma_z=((0.0, 0.0, 0.0), (-0.014, 0.0, 0.0), (0.014, -1e-3, 0.0), (0.014, 0.0, -1e-6), (nan, 0.0, 0.0)))
    for field, values in bad.items():
        for v in values:
            assert _call(params=G.vro_params(**{field: v})) == E, (field, v)
    # the bad arguments are refused for an empty batch as well; the optional outputs may all be NULL
    assert _call(n=0, params=G.vro_params(hypotheses=0)) == E


def test_empty_batch_is_ok_and_a_valid_call_needs_a_device():
    assert _call(n=0) == 0
    assert _call(n=0, drop=("ptr", "xi", "xj", "pose", "res"), info=False, cov=False, inl=False) == 0
    if G.lib.fgo_device_count() <= 0:
        assert _call() == -2
        assert _call(info=False, cov=False, inl=False) == -2
        assert _call(n=2, ptr=[0, 0, 16], hyp=True, params=G.vro_params(hypotheses=1, refine_rounds=0, rigid_tol=0.0, min_inliers=3,
                                                                        sigma_z=(0.0, 0.0, 1e-3))) == -2
        assert _call(ptr=[0, INT_MAX // 3]) == -2                 # the bound itself is accepted (the arrays are not read before the device check)
        with pytest.raises(G.FgoError, match="-2"):
            G.vro_ransac_batch([0, 10], np.ones((10, 3)), np.ones((10, 3)))


def test_python_wrapper_checks_shapes_before_the_call():
    with pytest.raises(G.FgoError, match="holds? fewer|fewer"):
        G.vro_ransac_batch([0, 10], np.ones((9, 3)), np.ones((10, 3)))
    with pytest.raises(G.FgoError, match="n_pairs \\+ 1"):
        G.vro_ransac_batch([], np.ones((1, 3)), np.ones((1, 3)))
