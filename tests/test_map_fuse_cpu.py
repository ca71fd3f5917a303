"""CPU-only checks of the map fusion entry point (include/fgo.h fgo_map_fuse_batch): the symbols are exported, the defaults are the
declared ones, the structs have the declared layout, every bad argument is refused before any HIP call, an empty batch is FGO_OK with
a zero result, and a valid call FAILS LOUDLY without a GPU (no CPU fallback), as fgo_plane_extract_batch does."""
import ctypes as C

import numpy as np
import pytest

import graph_slam_amd as G

E = -1


def _call(n=1, w=16, h=12, ch=0, params=None, drop=(), max_voxels=None, pose=None, ext=None, color="auto", outs=True):
    """one frame of 16 x 12 unless told otherwise; `drop` names required pointers passed as NULL.  Returns (rc, result)."""
    m = min(max(n, 1), 2)                                         # a refused call touches no array
    depth = np.full((m, 12, 16), 2000, np.uint16)
    ps = np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0]), (m, 1)) if pose is None else np.ascontiguousarray(pose, np.float64)
    col = np.zeros((m, 12, 16, max(ch, 1)), np.uint8)
    cap = 16 * 12 * m if max_voxels is None else max_voxels
    k = max(cap, 1)
    xyz = np.zeros((k, 3)); cout = np.zeros((k, 3), np.uint8); cnt = np.zeros(k, np.int32); key = np.zeros(k, np.int64)
    fp = np.zeros(m, np.int64); rt = np.zeros((m, 12))
    res = G.MapResult(7, 7, 7, 7, 7, 7, 7)
    u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    arg = lambda name, v: None if name in drop else v
    cptr = (u8(col) if ch else None) if color == "auto" else (u8(col) if color else None)
    e = None if ext is None else G._dp(np.ascontiguousarray(ext, np.float64))
    rc = G.lib.fgo_map_fuse_batch(0, n, w, h, arg("depth", depth.ctypes.data_as(C.POINTER(C.c_uint16))), cptr, ch, arg("pose", G._dp(ps)), e,
                                  None if params is None else C.byref(params), cap, arg("res", C.byref(res)), arg("xyz", G._dp(xyz)),
                                  u8(cout) if outs else None, cnt.ctypes.data_as(C.POINTER(C.c_int32)) if outs else None,
                                  G._i64p(key) if outs else None, G._i64p(fp) if outs else None, G._dp(rt) if outs else None)
    return rc, res


def test_symbols_defaults_and_struct_layout():
    for s in ("fgo_map_fuse_batch", "fgo_map_params_default", "fgo_debug_map_fuse_kernel_ms"):
        assert hasattr(G.lib, s), s
    for s in ("map_fuse_batch", "map_params", "write_ply", "MapParams", "MapResult", "FGO_MAP_OK", "FGO_MAP_TRUNCATED", "FGO_MAP_FULL"):
        assert hasattr(G, s), s
    assert (G.FGO_MAP_OK, G.FGO_MAP_TRUNCATED, G.FGO_MAP_FULL) == (0, 1, 2)
    p = G.MapParams()
    G.lib.fgo_map_params_default(C.byref(p))
    assert (p.fx, p.fy, p.cx, p.cy, p.z_scale, p.z_min, p.z_max) == (250.5773, 250.5773, 90.0, 70.0, 0.001, 0.1, 5.0)
    assert (p.skip, list(p.rect), p.leaf, p.min_points, p.table_log2) == (2, [0, 0, 0, 0], 0.02, 1, 0)
    G.lib.fgo_map_params_default(None)                            # tolerated
    # C layout: 7 doubles, 5 ints, (pad), double, 2 ints; int, int, 5 int64
    assert C.sizeof(G.MapParams) == 96 and C.sizeof(G.MapResult) == 48
    V = G.MapParams
    assert (V.fx.offset, V.z_scale.offset, V.z_max.offset, V.skip.offset, V.rect.offset, V.leaf.offset, V.min_points.offset,
            V.table_log2.offset) == (0, 32, 48, 56, 60, 80, 88, 92)
    R = G.MapResult
    assert (R.status.offset, R.table_log2.offset, R.n_sampled.offset, R.n_valid.offset, R.n_out_of_range.offset, R.n_voxels.offset,
            R.n_dropped.offset) == (0, 4, 8, 16, 24, 32, 40)
    q = G.map_params(skip=3, rect=(1, 2, 10, 11), leaf=0.05, cx=8.0)
    assert (q.skip, list(q.rect), q.leaf, q.cx, q.min_points) == (3, [1, 2, 10, 11], 0.05, 8.0, 1)
    with pytest.raises(TypeError):
        G.map_params(no_such_field=1)
    assert G.lib.fgo_debug_map_fuse_kernel_ms() >= 0.0


def test_bad_arguments_are_refused_without_a_device():
    assert _call(n=-1)[0] == E
    for name in ("depth", "pose", "res", "xyz"):                  # a NULL required pointer
        assert _call(drop=(name,))[0] == E, name
    assert _call(max_voxels=-1)[0] == E
    for w, h in ((0, 12), (16, 0), (-1, 12), (16, -3), (4097, 4096), (1 << 24, 2)):      # a side < 1, more than 2^24 pixels
        assert _call(w=w, h=h)[0] == E, (w, h)
    # n_frames x sampled pixels >= 2^31: 2^17 frames of 128 x 128 at skip 1 (the arrays are not touched: refused before)
    assert _call(n=1 << 17, w=128, h=128, params=G.map_params(skip=1))[0] == E
    assert _call(n=1 << 40, w=1, h=1, params=G.map_params(skip=1))[0] == E
    for ch in (-1, 2, 4):
        assert _call(ch=ch)[0] == E, ch
    assert _call(ch=3, color=False)[0] == E and _call(ch=1, color=False)[0] == E          # channels without colour
    assert _call(ch=0, color=True)[0] == E                                               # colour without channels
    zero_q = np.array([[1.0, 2, 3, 0, 0, 0, 0]])
    assert _call(pose=zero_q)[0] == E and _call(ext=zero_q[0])[0] == E
    assert _call(pose=np.array([[0, 0, 0, np.nan, 0, 0, 1.0]]))[0] == E
    two = np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0]), (2, 1)); two[1, 3:] = 0
    assert _call(n=2, pose=two)[0] == E                           # the second frame's
    nan = float("nan")
    bad = dict(fx=(0.0, -250.0, nan), fy=(0.0, -250.0, nan), z_scale=(0.0, -0.001, nan), z_min=(5.0, 6.0, nan), z_max=(0.1, 0.0, nan),
               skip=(0, -2), leaf=(0.0, -0.02, 2.0 ** -21, 1024.5, nan), min_points=(0, -1), table_log2=(1, 3, 33, -4),
               rect=((0, 0, 17, 12), (0, 0, 16, 13), (-1, 0, 16, 12), (0, -1, 16, 12), (5, 0, 5, 12), (0, 7, 16, 7), (9, 0, 4, 12),
                     (0, 0, 16, 0), (0, 0, 0, 12), (16, 12, 16, 12)))
    for field, values in bad.items():
        for v in values:
            assert _call(params=G.map_params(**{field: v}))[0] == E, (field, v)
    # the bad arguments are refused for an empty batch as well
    assert _call(n=0, params=G.map_params(skip=0))[0] == E
    assert _call(n=0, w=0)[0] == E and _call(n=0, ch=2)[0] == E and _call(n=0, drop=("res",))[0] == E


def test_empty_batch_is_ok_with_a_zero_result_and_a_valid_call_needs_a_device():
    for rc, res in (_call(n=0), _call(n=0, drop=("depth", "pose", "xyz"), outs=False), _call(n=0, ch=3, color=False)):
        assert rc == 0
        assert [getattr(res, f) for f, _ in G.MapResult._fields_] == [0] * 7
    o = G.map_fuse_batch(np.zeros((0, 12, 16), np.uint16), np.zeros((0, 7)), want_keys=True, want_rt=True)
    assert {k: (v.shape if hasattr(v, "shape") else v) for k, v in o.items()} == dict(
        status=0, table_log2=0, n_sampled=0, n_valid=0, n_out_of_range=0, n_voxels=0, n_dropped=0, xyz=(0, 3), color=None, count=(0,),
        frame_points=(0,), key=(0,), rt=(0, 12))
    assert o["count"].dtype == np.int32 and o["key"].dtype == np.int64 and o["frame_points"].dtype == np.int64
    if G.lib.fgo_device_count() <= 0:
        assert _call()[0] == -2
        assert _call(outs=False, max_voxels=0, drop=("xyz",))[0] == -2
        assert _call(ch=3, ext=[0.1, 0, 0, 0, 0, 1, 1], params=G.map_params(skip=1, rect=(3, 2, 16, 12), leaf=2.0 ** -20, table_log2=4,
                                                                            min_points=9))[0] == -2
        assert _call(n=2, w=12, h=16, ch=1, params=G.map_params(leaf=1024.0, table_log2=32, skip=40))[0] == -2       # the bounds themselves
        with pytest.raises(G.FgoError, match="-2"):
            G.map_fuse_batch(np.full((2, 12, 16), 2000, np.uint16), np.tile([0, 0, 0, 0, 0, 0, 1.0], (2, 1)))


def test_python_wrapper_refuses_misshapen_arrays():
    with pytest.raises(G.FgoError, match="n x H x W"):
        G.map_fuse_batch(np.zeros(5, np.uint16), np.zeros((1, 7)))
    with pytest.raises(G.FgoError, match="one row of 7"):
        G.map_fuse_batch(np.zeros((2, 12, 16), np.uint16), np.zeros((3, 7)))
    with pytest.raises(G.FgoError, match="color"):
        G.map_fuse_batch(np.zeros((2, 12, 16), np.uint16), np.zeros((2, 7)), color=np.zeros((2, 12, 16, 2), np.uint8))
