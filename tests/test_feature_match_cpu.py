"""CPU-only checks of the descriptor-matching entry point (include/fgo.h fgo_match_features_batch): the symbols are exported, the
defaults are the declared ones, the structs have the declared layout, every bad argument is refused before any HIP call, and a valid
call FAILS LOUDLY without a GPU (no CPU fallback), as fgo_vro_ransac_batch does."""
import ctypes as C

import numpy as np
import pytest

import graph_slam_amd as G

INT32_MAX = 2 ** 31 - 1


def _call(n=1, nf=2, ptr=None, fi=(0,), fj=(1,), pose=None, guided=None, params=None, drop=(), optional=True, dist=False):
    """two frames of 8 features and one pair unless told otherwise; `drop` names required pointers passed as NULL"""
    fp = np.asarray([0, 8, 16] if ptr is None else ptr, np.int64)
    F = 16
    rng = np.random.default_rng(0)
    desc = rng.integers(0, 256, (F, 128)).astype(np.uint8)
    xyz = rng.uniform(1, 2, (F, 3)); uv = rng.uniform(0, 100, (F, 2))
    a = np.asarray(fi, np.int64); b = np.asarray(fj, np.int64)
    Q = 64
    res = (G.MatchResult * max(n, 1))()
    qp = np.zeros(max(n, 0) + 1, np.int64); mp = np.zeros(max(n, 0) + 1, np.int64)
    i32 = lambda: np.zeros(Q, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    ii, ij = np.zeros(Q, np.int64), np.zeros(Q, np.int64)
    o3 = [np.zeros((Q, 3)) for _ in range(2)]; o2 = [np.zeros((Q, 2)) for _ in range(2)]
    why = np.zeros(Q, np.uint8); dd = np.zeros(Q * Q, np.int32)
    u8 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint8))
    arg = lambda name, v: None if name in drop else v
    opt = lambda v: v if optional else None
    ps = None if pose is None else np.ascontiguousarray(pose, np.float64)
    gd = None if guided is None else np.ascontiguousarray(guided, np.uint8)
    return G.lib.fgo_match_features_batch(
        0, nf, arg("ptr", G._i64p(fp)), arg("desc", u8(desc)), arg("xyz", G._dp(xyz)), arg("uv", G._dp(uv)), n, arg("fi", G._i64p(a)),
        arg("fj", G._i64p(b)), None if ps is None else G._dp(ps), None if gd is None else u8(gd), None if params is None else C.byref(params),
        arg("res", res), opt(G._i64p(qp)), opt(i32()), opt(i32()), opt(i32()), opt(u8(why)), arg("mptr", G._i64p(mp)), arg("ii", G._i64p(ii)),
        arg("ij", G._i64p(ij)), opt(G._dp(o3[0])), opt(G._dp(o3[1])), opt(G._dp(o2[0])), opt(G._dp(o2[1])),
        dd.ctypes.data_as(C.POINTER(C.c_int32)) if dist else None)


def test_symbols_defaults_and_struct_layout():
    for s in ("fgo_match_features_batch", "fgo_match_params_default", "fgo_debug_match_kernel_ms"):
        assert hasattr(G.lib, s), s
    for s in ("match_features_batch", "match_params", "vro_adjust_batch", "MatchParams", "MatchResult", "FGO_FM_OK", "FGO_FM_TOO_FEW"):
        assert hasattr(G, s), s
    assert (G.FGO_FM_OK, G.FGO_FM_TOO_FEW, G.FGO_FM_DIM, G.FGO_FM_MAX_FEATURES) == (0, 1, 128, 4096)
    p = G.MatchParams()
    G.lib.fgo_match_params_default(C.byref(p))
    assert (p.ratio, p.ratio_test, p.cross_check, p.max_desc_dist2, p.min_matches) == (0.5, 1, 1, INT32_MAX, 12)
    assert (p.radius_px, p.max_dist_3d, p.fx, p.fy, p.cx, p.cy) == (10.0, 0.0, 250.5773, 250.5773, 90.0, 70.0)
    G.lib.fgo_match_params_default(None)                         # tolerated
    # C layout: double, 4 ints, 6 doubles
    assert C.sizeof(G.MatchParams) == 72 and C.sizeof(G.MatchResult) == 24
    M = G.MatchParams
    assert (M.ratio.offset, M.ratio_test.offset, M.cross_check.offset, M.max_desc_dist2.offset, M.min_matches.offset, M.radius_px.offset,
            M.max_dist_3d.offset, M.fx.offset, M.cy.offset) == (0, 8, 12, 16, 20, 24, 32, 40, 64)
    R = G.MatchResult
    assert (R.status.offset, R.n_query.offset, R.n_train.offset, R.n_matches.offset, R.n_ratio.offset, R.n_cross.offset) == (0, 4, 8, 12, 16, 20)
    q = G.match_params(ratio=0.8, cross_check=0)
    assert (q.ratio, q.cross_check, q.ratio_test, q.min_matches) == (0.8, 0, 1, 12)
    with pytest.raises(TypeError):
        G.match_params(no_such_field=1)
    assert G.lib.fgo_debug_match_kernel_ms() >= 0.0


def test_bad_arguments_are_refused_without_a_device():
    E = -1
    assert _call(n=-1) == E and _call(nf=-1) == E
    for name in ("ptr", "desc", "xyz", "uv", "fi", "fj", "res", "mptr", "ii", "ij"):       # a NULL required pointer
        assert _call(drop=(name,)) == E, name
    assert _call(ptr=[-1, 8, 16]) == E                            # negative
    assert _call(ptr=[0, 9, 8]) == E                              # decreasing
    assert _call(ptr=[0, 4097, 4100]) == E                        # more than FGO_FM_MAX_FEATURES in a frame
    assert _call(fi=(2,)) == E and _call(fj=(-1,)) == E and _call(nf=1, ptr=[0, 8]) == E    # a frame index out of range
    ident = [0, 0, 0, 0, 0, 0, 1.0]
    zero, nanq = [0, 0, 0, 0, 0, 0, 0.0], [0, 0, 0, float("nan"), 0, 0, 1.0]
    assert _call(pose=zero) == E and _call(pose=nanq) == E and _call(pose=zero, guided=[1]) == E
    assert _call(n=2, fi=(0, 1), fj=(1, 0), pose=[ident, zero], guided=[1, 1]) == E
    nan = float("nan")
    bad = dict(ratio=(0.0, -0.5, 1.0000001, nan), radius_px=(0.0, -1.0, nan), fx=(0.0, -250.0, nan), fy=(0.0, -250.0, nan),
               max_dist_3d=(-1e-9, nan), max_desc_dist2=(-1,), min_matches=(-1,))
    for field, values in bad.items():
        for v in values:
            assert _call(params=G.match_params(**{field: v})) == E, (field, v)
    assert _call(n=0, params=G.match_params(ratio=0.0)) == E      # refused for an empty batch as well


def test_empty_batch_is_ok_and_a_valid_call_needs_a_device():
    assert _call(n=0) == 0
    assert _call(n=0, drop=("ptr", "desc", "xyz", "uv", "fi", "fj", "res", "mptr", "ii", "ij"), optional=False) == 0
    if G.lib.fgo_device_count() <= 0:
        ident = [0, 0, 0, 0, 0, 0, 1.0]
        assert _call() == -2
        assert _call(optional=False) == -2 and _call(dist=True) == -2
        assert _call(pose=ident) == -2 and _call(pose=[0, 0, 0, 0, 0, 0, 0.0], guided=[0]) == -2    # an unguided pair's pose is not read
        assert _call(ptr=[0, 0, 4096], params=G.match_params(ratio=1.0, min_matches=0, max_desc_dist2=0)) == -2   # the bounds themselves
        with pytest.raises(G.FgoError, match="-2"):
            G.match_features_batch([0, 4, 8], np.zeros((8, 128), np.uint8), np.ones((8, 3)), np.ones((8, 2)), [0], [1])
        with pytest.raises(G.FgoError, match="-2"):
            G.vro_adjust_batch([0, 4, 8], np.zeros((8, 128), np.uint8), np.ones((8, 3)), np.ones((8, 2)), [0], [1], [[0, 0, 0, 0, 0, 0, 1.0]])


def test_python_wrapper_checks_shapes_before_the_call():
    d, x, u = np.zeros((8, 128), np.uint8), np.ones((8, 3)), np.ones((8, 2))
    with pytest.raises(G.FgoError, match="fewer"):
        G.match_features_batch([0, 4, 9], d, x, u, [0], [1])
    with pytest.raises(G.FgoError, match="n_frames \\+ 1"):
        G.match_features_batch([], d, x, u, [0], [1])
    with pytest.raises(G.FgoError, match="one entry per pair"):
        G.match_features_batch([0, 4, 8], d, x, u, [0, 1], [1])
    with pytest.raises(G.FgoError, match="one entry per pair"):
        G.match_features_batch([0, 4, 8], d, x, u, [0], [1], pose_ij=np.zeros((2, 7)))
    with pytest.raises(G.FgoError, match="-1"):                  # a bad index is the library's to refuse
        G.match_features_batch([0, 4, 8], d, x, u, [0], [2])
