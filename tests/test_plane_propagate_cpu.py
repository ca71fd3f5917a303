"""CPU-only checks of the plane propagation entry point (include/fgo.h fgo_plane_propagate_batch): the symbols are exported, the
defaults are the declared ones, the structs have the declared layout, every bad argument is refused before any HIP call, an empty
batch is fine, and a valid call FAILS LOUDLY without a GPU (no CPU fallback), as fgo_plane_extract_batch does."""
import ctypes as C

import numpy as np
import pytest

import graph_slam_amd as G

E, OK, ENODEV = -1, 0, -2
MP = 8


def _call(n_pairs=1, n_frames=2, w=16, h=12, params=None, drop=(), optional=True, use="cov", npl=(1, 0), fi=(0,), fj=(1,), quat=(0, 0, 0, 1.0),
          normal=(0, 0, -1.0)):
    """one pair over two frames of 16 x 12 unless told otherwise; `drop` names required pointers passed as NULL"""
    nf, n = max(n_frames, 1), max(n_pairs, 1)
    depth = np.full((nf, 12, 16), 2000, np.uint16); inten = np.full((nf, 12, 16), 100, np.uint8); lab = np.zeros((nf, 12, 16), np.int8)
    npl_ = np.zeros(nf, np.int32); npl_[:len(npl)] = npl[:nf]
    abcd = np.zeros((nf, MP, 4)); abcd[:, :, :3] = normal; abcd[:, :, 3] = 2.0
    c16 = np.tile((1e-6 * np.eye(4)).reshape(16), (nf, MP, 1))
    fi_ = np.zeros(n, np.int64); fi_[:len(fi)] = fi[:n]
    fj_ = np.zeros(n, np.int64); fj_[:len(fj)] = fj[:n]
    pose = np.tile(np.array([0, 0, 0] + list(quat), np.float64), (n, 1))
    info = np.tile(G.np.eye(6)[np.triu_indices(6)] * 1e6, (n, 1)); cov = np.tile(1e-6 * np.eye(6).reshape(36), (n, 1))
    res = (G.PlanePropagateResult * n)(); pl = (G.PlanePropagatePlane * (n * MP))(); pd = (G.PlanePropagatePred * (n * MP))()
    ao = np.zeros((n, MP, 4)); co = np.zeros((n, MP, 16)); uo = np.zeros((n, MP, 6)); lo = np.zeros((n, 12, 16), np.int8)
    arg = lambda name, v: None if name in drop else v
    return G.lib.fgo_plane_propagate_batch(
        0, n_frames, w, h, arg("depth", depth.ctypes.data_as(C.POINTER(C.c_uint16))), arg("intensity", inten.ctypes.data_as(C.POINTER(C.c_uint8))),
        arg("label", lab.ctypes.data_as(C.POINTER(C.c_int8))), arg("n_planes", npl_.ctypes.data_as(C.POINTER(C.c_int32))),
        arg("abcd", G._dp(abcd)), arg("cov16", G._dp(c16)), n_pairs, arg("frame_i", G._i64p(fi_)), arg("frame_j", G._i64p(fj_)),
        arg("pose", G._dp(pose)), G._dp(info) if use in ("info", "both") else None, G._dp(cov) if use in ("cov", "both") else None,
        None if params is None else C.byref(params), arg("res", res), arg("abcd_out", G._dp(ao)), arg("cov16_out", G._dp(co)),
        G._dp(uo) if optional else None, pl if optional else None, pd if optional else None,
        lo.ctypes.data_as(C.POINTER(C.c_int8)) if optional else None)


def test_symbols_defaults_and_struct_layout():
    for s in ("fgo_plane_propagate_batch", "fgo_plane_propagate_params_default", "fgo_debug_plane_propagate_kernel_ms"):
        assert hasattr(G.lib, s), s
    for s in ("plane_propagate_batch", "plane_propagate_params", "plane_node_batch", "PlanePropagateParams", "PlanePropagateResult",
              "PlanePropagatePlane", "PlanePropagatePred", "FGO_PP_OK", "FGO_PP_NUM"):
        assert hasattr(G, s), s
    assert (G.FGO_PP_OK, G.FGO_PP_NUM) == (0, 2)
    p = G.PlanePropagateParams()
    G.lib.fgo_plane_propagate_params_default(C.byref(p))
    x = G.PlaneExtractParams()
    G.lib.fgo_plane_extract_params_default(C.byref(x))
    for f in ("fx", "fy", "cx", "cy", "z_scale", "z_min", "z_max", "sigma_px"):               # the camera and the depth range of the extraction
        assert getattr(p, f) == getattr(x, f), f
    assert list(p.sigma_z) == list(x.sigma_z) == [0.014, 0.0, 0.0]
    assert (p.fx, p.cx, p.cy, p.z_min, p.z_max) == (250.5773, 90.0, 70.0, 0.1, 5.0)
    assert (p.d_floor, p.intensity_tol, p.keep_ratio, p.rest_ratio) == (0.014, 5, 0.7, 0.5)
    G.lib.fgo_plane_propagate_params_default(None)                # tolerated
    # C layout: 12 doubles, int, (pad), 2 doubles;  4 ints;  4 ints, 4 doubles;  5 doubles, 4 ints
    assert C.sizeof(G.PlanePropagateParams) == 120 and C.sizeof(G.PlanePropagateResult) == 16
    assert C.sizeof(G.PlanePropagatePlane) == 48 and C.sizeof(G.PlanePropagatePred) == 56
    V = G.PlanePropagateParams
    assert (V.fx.offset, V.z_scale.offset, V.sigma_px.offset, V.sigma_z.offset, V.d_floor.offset, V.intensity_tol.offset, V.keep_ratio.offset,
            V.rest_ratio.offset) == (0, 32, 56, 64, 88, 96, 104, 112)
    R = G.PlanePropagatePlane
    assert (R.n_pixels.offset, R.n_seed.offset, R.source.offset, R.rmse.offset, R.centroid.offset) == (0, 4, 8, 16, 24)
    Q = G.PlanePropagatePred
    assert (Q.abcd.offset, Q.sdj.offset, Q.n_prev.offset, Q.n_seed.offset, Q.kept.offset) == (0, 32, 40, 44, 48)
    q = G.plane_propagate_params(intensity_tol=7, sigma_z=(0.01, 0.002, 0.0), keep_ratio=0.5, cx=24.0)
    assert (q.intensity_tol, list(q.sigma_z), q.keep_ratio, q.cx, q.d_floor) == (7, [0.01, 0.002, 0.0], 0.5, 24.0, 0.014)
    with pytest.raises(TypeError):
        G.plane_propagate_params(no_such_field=1)
    assert G.lib.fgo_debug_plane_propagate_kernel_ms() >= 0.0


def test_bad_arguments_are_refused_without_a_device():
    assert _call(n_pairs=-1) == E and _call(n_frames=-1) == E
    for name in ("depth", "intensity", "label", "n_planes", "abcd", "cov16", "frame_i", "frame_j", "pose", "res", "abcd_out", "cov16_out"):
        assert _call(drop=(name,)) == E, name                     # a NULL required pointer
    assert _call(use="both") == E and _call(use="neither") == E   # both or neither of info_ut21 / cov36
    for w, h in ((0, 12), (16, 0), (-1, 12), (16, -3), (4097, 4096), (1 << 24, 2)):
        assert _call(w=w, h=h) == E, (w, h)
    for fi, fj in (((2,), (1,)), ((-1,), (1,)), ((0,), (2,)), ((0,), (-1,))):              # a frame index out of range
        assert _call(fi=fi, fj=fj) == E, (fi, fj)
    assert _call(n_frames=0) == E                                 # no frame to index
    for npl in ((-1, 0), (9, 0), (0, 9), (0, -2)):                # n_planes outside [0, FGO_PX_MAX_PLANES], of any frame
        assert _call(npl=npl) == E, npl
    assert _call(quat=(0, 0, 0, 0)) == E and _call(quat=(float("nan"), 0, 0, 1)) == E      # a zero quaternion
    assert _call(normal=(0, 0, 0)) == E and _call(normal=(0, 0, 0), npl=(0, 1)) == E        # a zero normal among the first n_planes
    nan = float("nan")
    bad = dict(fx=(0.0, -250.0, nan), fy=(0.0, -250.0, nan), z_scale=(0.0, -0.001, nan), sigma_px=(0.0, -1.0, nan), z_min=(5.0, 6.0, nan),
               z_max=(0.1, 0.0, nan), cx=(nan, float("inf")), cy=(nan,),
               sigma_z=((0.0, 0.0, 0.0), (-0.014, 0.0, 0.0), (0.014, -1e-3, 0.0), (0.014, 0.0, -1e-6), (nan, 0.0, 0.0)),
               d_floor=(-0.014, nan, float("inf")), intensity_tol=(-1, -100), keep_ratio=(-0.1, 1.1, nan), rest_ratio=(-0.1, 1.1, nan))
    for field, values in bad.items():
        for v in values:
            assert _call(params=G.plane_propagate_params(**{field: v})) == E, (field, v)
    # the bad arguments are refused for an empty batch as well
    assert _call(n_pairs=0, params=G.plane_propagate_params(intensity_tol=-1)) == E
    assert _call(n_pairs=0, w=0) == E


def test_empty_batch_is_ok_and_a_valid_call_needs_a_device():
    assert _call(n_pairs=0) == OK
    assert _call(n_pairs=0, n_frames=0, optional=False, use="neither",
                 drop=("depth", "intensity", "label", "n_planes", "abcd", "cov16", "frame_i", "frame_j", "pose", "res", "abcd_out", "cov16_out")) == OK
    if G.lib.fgo_device_count() <= 0:
        assert _call() == ENODEV
        assert _call(use="info", optional=False) == ENODEV
        assert _call(normal=(0, 0, 0), npl=(0, 0)) == ENODEV      # a zero normal past n_planes is not read
        assert _call(params=G.plane_propagate_params(d_floor=0.0, intensity_tol=0, keep_ratio=0.0, rest_ratio=1.0)) == ENODEV   # the bounds themselves
        assert _call(n_pairs=2, fi=(0, 1), fj=(1, 1), npl=(8, 8)) == ENODEV
        with pytest.raises(G.FgoError, match="-2"):
            G.plane_propagate_batch(np.full((2, 12, 16), 2000, np.uint16), np.zeros((2, 12, 16), np.uint8), np.zeros((2, 12, 16), np.int8), [1, 0],
                                    np.tile([0, 0, -1.0, 2.0], (2, 1, 1)), np.tile(1e-6 * np.eye(4), (2, 1, 1, 1)), [0], [1], [[0, 0, 0, 0, 0, 0, 1.0]],
                                    cov=1e-6 * np.eye(6)[None])


def test_python_wrapper_shapes_and_refusals():
    z = np.zeros((2, 12, 16), np.uint16)
    args = (z, z.astype(np.uint8), z.astype(np.int8), [0, 0], np.zeros((2, 0, 4)), np.zeros((2, 0, 16)), [], [], np.zeros((0, 7)))
    with pytest.raises(G.FgoError, match="exactly one"):
        G.plane_propagate_batch(*args)
    with pytest.raises(G.FgoError, match="n x H x W"):
        G.plane_propagate_batch(z[0], *args[1:], cov=np.zeros((0, 36)))
    o = G.plane_propagate_batch(*args, cov=np.zeros((0, 6, 6)))
    shapes = dict(status=(0,), n_planes=(0,), num_added=(0,), search_rest=(0,), abcd_all=(0, 8, 4), cov16_all=(0, 8, 4, 4), cov_ut6_all=(0, 8, 6),
                  n_pixels=(0, 8), n_seed=(0, 8), source=(0, 8), rmse=(0, 8), centroid=(0, 8, 3), pred_abcd=(0, 8, 4), sdj=(0, 8), n_prev=(0, 8),
                  pred_n_seed=(0, 8), kept=(0, 8), ptr=(1,), abcd=(0, 4), cov16=(0, 16), cov_ut6=(0, 6), labels=(0, 12, 16))
    assert {k: v.shape for k, v in o.items()} == shapes
    assert o["labels"].dtype == np.int8 and o["ptr"].dtype == np.int64 and o["status"].dtype == np.int32
    bare = G.plane_propagate_batch(*args, info=np.zeros((0, 21)), want_labels=False, want_pred=False, want_planes=False, want_ut6=False)
    assert set(bare) == {"status", "n_planes", "num_added", "search_rest", "abcd_all", "cov16_all", "ptr", "abcd", "cov16"}
    node = G.plane_node_batch(*args, cov=np.zeros((0, 6, 6)))
    assert node["extracted"] is None and node["n_new"].shape == (0,)
