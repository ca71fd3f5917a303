"""CPU-only checks of the plane extraction entry point (include/fgo.h fgo_plane_extract_batch): the symbols are exported, the
defaults are the declared ones, the structs have the declared layout, every bad argument is refused before any HIP call, and a valid
call FAILS LOUDLY without a GPU (no CPU fallback), as fgo_vro_ransac_batch does."""
import ctypes as C

import numpy as np
import pytest

import graph_slam_amd as G


def _call(n=1, w=16, h=12, params=None, drop=(), ut6=True, planes=True, labels=True, hyp=False):
    """one frame of 16 x 12 unless told otherwise; `drop` names required pointers passed as NULL"""
    m = max(n, 1)
    depth = np.full((m, 12, 16), 2000, np.uint16)
    mp = G.FGO_PX_MAX_PLANES
    k = G.plane_extract_params().hypotheses if params is None else min(max(params.hypotheses, 1), 1 << 16)
    abcd = np.zeros((m, mp, 4)); c16 = np.zeros((m, mp, 16)); u6 = np.zeros((m, mp, 6)); lab = np.zeros((m, 12, 16), np.int8)
    hc = np.zeros((m, mp, k), np.int32)
    res = (G.PlaneExtractResult * m)(); pl = (G.PlaneExtractPlane * (m * mp))()
    arg = lambda name, v: None if name in drop else v
    return G.lib.fgo_plane_extract_batch(
        0, n, w, h, arg("depth", depth.ctypes.data_as(C.POINTER(C.c_uint16))), None if params is None else C.byref(params), arg("res", res),
        arg("abcd", G._dp(abcd)), arg("cov16", G._dp(c16)), G._dp(u6) if ut6 else None, pl if planes else None,
        lab.ctypes.data_as(C.POINTER(C.c_int8)) if labels else None, hc.ctypes.data_as(C.POINTER(C.c_int32)) if hyp else None)


def test_symbols_defaults_and_struct_layout():
    for s in ("fgo_plane_extract_batch", "fgo_plane_extract_params_default", "fgo_debug_plane_extract_kernel_ms"):
        assert hasattr(G.lib, s), s
    for s in ("plane_extract_batch", "plane_extract_params", "PlaneExtractParams", "PlaneExtractResult", "PlaneExtractPlane", "FGO_PX_OK",
              "FGO_PX_NUM", "FGO_PX_MAX_PLANES"):
        assert hasattr(G, s), s
    assert (G.FGO_PX_OK, G.FGO_PX_NUM, G.FGO_PX_MAX_PLANES) == (0, 2, 8)
    p = G.PlaneExtractParams()
    G.lib.fgo_plane_extract_params_default(C.byref(p))
    assert (p.fx, p.fy, p.cx, p.cy, p.z_scale, p.z_min, p.z_max) == (250.5773, 250.5773, 90.0, 70.0, 0.001, 0.1, 5.0)
    assert (p.hypotheses, p.seed, p.max_dist, p.min_area, p.min_pixels, p.max_planes, p.refine_rounds) == (512, 0, 0.05, 1e-3, 1500, 4, 3)
    assert (p.sigma_px, list(p.sigma_z)) == (1.0, [0.014, 0.0, 0.0])
    G.lib.fgo_plane_extract_params_default(None)                  # tolerated
    # C layout: 7 doubles, int, (pad), uint64, 2 doubles, 3 ints, (pad), double, double[3]
    assert C.sizeof(G.PlaneExtractParams) == 136 and C.sizeof(G.PlaneExtractResult) == 16 and C.sizeof(G.PlaneExtractPlane) == 56
    V = G.PlaneExtractParams
    assert (V.fx.offset, V.z_scale.offset, V.hypotheses.offset, V.seed.offset, V.max_dist.offset, V.min_pixels.offset, V.max_planes.offset,
            V.refine_rounds.offset, V.sigma_px.offset, V.sigma_z.offset) == (0, 32, 56, 64, 72, 88, 92, 96, 104, 112)
    R = G.PlaneExtractPlane
    assert (R.n_pixels.offset, R.best_hypothesis.offset, R.best_count.offset, R.n_valid_hyp.offset, R.fits.offset, R.rmse.offset,
            R.centroid.offset) == (0, 4, 8, 12, 16, 24, 32)
    q = G.plane_extract_params(hypotheses=7, sigma_z=(0.01, 0.002, 0.0), seed=2 ** 63 + 5, cx=24.0)
    assert (q.hypotheses, list(q.sigma_z), q.seed, q.cx, q.max_dist) == (7, [0.01, 0.002, 0.0], 2 ** 63 + 5, 24.0, 0.05)
    with pytest.raises(TypeError):
        G.plane_extract_params(no_such_field=1)
    assert G.lib.fgo_debug_plane_extract_kernel_ms() >= 0.0


def test_bad_arguments_are_refused_without_a_device():
    E = -1
    assert _call(n=-1) == E
    for name in ("depth", "res", "abcd", "cov16"):                # a NULL required pointer
        assert _call(drop=(name,)) == E, name
    for w, h in ((0, 12), (16, 0), (-1, 12), (16, -3), (4097, 4096), (1 << 24, 2)):      # a side < 1, more than 2^24 pixels
        assert _call(w=w, h=h) == E, (w, h)
    nan = float("nan")
    bad = dict(fx=(0.0, -250.0, nan), fy=(0.0, -250.0, nan), z_scale=(0.0, -0.001, nan), max_dist=(0.0, -1.0, nan), min_area=(0.0, -1e-3, nan),
               sigma_px=(0.0, -1.0, nan), z_min=(5.0, 6.0, nan), z_max=(0.1, 0.0, nan), hypotheses=(0, -5, 65537), max_planes=(0, -1, 9),
               refine_rounds=(-1, 11), min_pixels=(2, 0, -1),
               sigma_z=((0.0, 0.0, 0.0), (-0.014, 0.0, 0.0), (0.014, -1e-3, 0.0), (0.014, 0.0, -1e-6), (nan, 0.0, 0.0)))
    for field, values in bad.items():
        for v in values:
            assert _call(params=G.plane_extract_params(**{field: v})) == E, (field, v)
    # the bad arguments are refused for an empty batch as well
    assert _call(n=0, params=G.plane_extract_params(hypotheses=0)) == E
    assert _call(n=0, w=0) == E


def test_empty_batch_is_ok_and_a_valid_call_needs_a_device():
    assert _call(n=0) == 0
    assert _call(n=0, drop=("depth", "res", "abcd", "cov16"), ut6=False, planes=False, labels=False) == 0
    if G.lib.fgo_device_count() <= 0:
        assert _call() == -2
        assert _call(ut6=False, planes=False, labels=False) == -2
        assert _call(n=2, w=12, h=16, hyp=True, params=G.plane_extract_params(hypotheses=1, refine_rounds=0, max_planes=8, min_pixels=3,
                                                                             sigma_z=(0.0, 0.0, 1e-3))) == -2
        assert _call(params=G.plane_extract_params(hypotheses=65536, max_planes=1, refine_rounds=10)) == -2      # the bounds themselves
        with pytest.raises(G.FgoError, match="-2"):
            G.plane_extract_batch(np.full((2, 12, 16), 2000, np.uint16))


def test_python_wrapper_shapes_dtypes_and_packed_ptr():
    with pytest.raises(G.FgoError, match="n x H x W"):
        G.plane_extract_batch(np.zeros(5, np.uint16))
    o = G.plane_extract_batch(np.zeros((0, 12, 16), np.uint16), params=G.plane_extract_params(max_planes=3, hypotheses=10), want_labels=True,
                              want_hyp_counts=True)
    shapes = dict(status=(0,), n_planes=(0,), n_valid_pixels=(0,), rounds_run=(0,), abcd_all=(0, 3, 4), cov16_all=(0, 3, 4, 4),
                  cov_ut6_all=(0, 3, 6), n_pixels=(0, 3), best_hypothesis=(0, 3), best_count=(0, 3), n_valid_hyp=(0, 3), fits=(0, 3),
                  rmse=(0, 3), centroid=(0, 3, 3), ptr=(1,), abcd=(0, 4), cov16=(0, 16), cov_ut6=(0, 6), labels=(0, 12, 16), hyp_counts=(0, 3, 10))
    assert {k: v.shape for k, v in o.items()} == shapes
    assert o["ptr"].dtype == np.int64 and o["ptr"][0] == 0 and o["labels"].dtype == np.int8 and o["hyp_counts"].dtype == np.int32
    assert o["status"].dtype == np.int32 and o["abcd"].dtype == np.float64 and o["cov16"].dtype == np.float64
    bare = G.plane_extract_batch(np.zeros((0, 12, 16), np.uint16))
    assert "labels" not in bare and "hyp_counts" not in bare and bare["abcd_all"].shape == (0, 4, 4)
