"""CPU-only checks of the map rendering entry point (include/fgo.h fgo_map_render_batch): the symbols are exported, the defaults are
the declared ones, the structs have the declared layout, every bad argument is refused before any HIP call, a call without views is
FGO_OK with a zero result, a valid call FAILS LOUDLY without a GPU (no CPU fallback), as fgo_map_fuse_batch does, and the Python
wrappers (map_render_batch, map_render_params, look_at, write_ppm) are there and refuse misshapen arrays."""
import ctypes as C

import numpy as np
import pytest

import graph_slam_amd as G

E = -1
IDENT = [0, 0, 0, 0, 0, 0, 1.0]


def _call(n=3, ch=0, nv=1, w=16, h=12, params=None, drop=(), pose=None, ext=None, off=None, color="auto", depth=False, outs=True, color_out="auto"):
    """three points seen from one view of 16 x 12 unless told otherwise; `drop` names required pointers passed as NULL.  Returns
    (rc, result).  A refused call touches no array, so the arrays stay small whatever n and nv say."""
    m, k = min(max(n, 1), 4), min(max(nv, 1), 2)
    xyz = np.tile([0.0, 0.0, 2.0], (m, 1))
    col = np.zeros((m, max(ch, 1)), np.uint8)
    ps = np.tile(np.array(IDENT), (k, 1)) if pose is None else np.ascontiguousarray(pose, np.float64)
    dm = np.full((k, 12, 16), 2000, np.uint16)
    zq = np.zeros((k, 12, 16), np.int32); idx = np.zeros((k, 12, 16), np.int32); cout = np.zeros((k, 12, 16, 3), np.uint8)
    rt = np.zeros((k, 12)); views = (G.MapRenderView * k)()
    res = G.MapRenderResult(7, 7, 7, 7)
    u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    arg = lambda name, v: None if name in drop else v
    opt = lambda a: None if a is None else G._dp(np.ascontiguousarray(a, np.float64))
    cptr = (u8(col) if ch else None) if color == "auto" else (u8(col) if color else None)
    coptr = (u8(cout) if ch > 0 and outs else None) if color_out == "auto" else (u8(cout) if color_out else None)
    rc = G.lib.fgo_map_render_batch(0, n, arg("xyz", G._dp(xyz)), cptr, ch, nv, arg("pose", G._dp(ps)), opt(ext), opt(off), w, h,
                                    None if params is None else C.byref(params), dm.ctypes.data_as(C.POINTER(C.c_uint16)) if depth else None,
                                    arg("res", C.byref(res)), views if outs else None, i32(zq) if outs else None, i32(idx) if outs else None,
                                    coptr, G._dp(rt) if outs else None)
    return rc, res


def test_symbols_defaults_and_struct_layout():
    for s in ("fgo_map_render_batch", "fgo_map_render_params_default", "fgo_debug_map_render_kernel_ms"):
        assert hasattr(G.lib, s), s
    for s in ("map_render_batch", "map_render_params", "look_at", "write_ppm", "MapRenderParams", "MapRenderView", "MapRenderResult",
              "FGO_MAP_RENDER_TILES", "FGO_MAP_RENDER_GLOBAL"):
        assert hasattr(G, s), s
    assert (G.FGO_MAP_RENDER_TILES, G.FGO_MAP_RENDER_GLOBAL) == (0, 1)
    p = G.MapRenderParams()
    G.lib.fgo_map_render_params_default(C.byref(p))
    m = G.MapParams()
    G.lib.fgo_map_params_default(C.byref(m))
    assert (p.fx, p.fy, p.cx, p.cy) == (m.fx, m.fy, m.cx, m.cy) == (250.5773, 250.5773, 90.0, 70.0)       # the SR4000 pinhole of fgo_map_params
    assert (p.z_scale, p.z_min, p.z_max, p.splat, p.radius, p.max_half, p.agree_tol, list(p.background)) == (0.001, 0.1, 50.0, 0, 0.0, 8, 0.05,
                                                                                                              [0, 0, 26])
    G.lib.fgo_map_render_params_default(None)                     # tolerated
    # C layout: 7 doubles, int, (pad), double, int, (pad), double, 3 bytes, (pad); 8 int64; 2 int64, 2 ints
    assert C.sizeof(G.MapRenderParams) == 96 and C.sizeof(G.MapRenderView) == 64 and C.sizeof(G.MapRenderResult) == 24
    V = G.MapRenderParams
    assert (V.fx.offset, V.z_scale.offset, V.z_max.offset, V.splat.offset, V.radius.offset, V.max_half.offset, V.agree_tol.offset,
            V.background.offset) == (0, 32, 48, 56, 64, 72, 80, 88)
    R = G.MapRenderResult
    assert (R.n_points.offset, R.n_nonfinite.offset, R.form.offset, R.tile_rows.offset) == (0, 8, 16, 20)
    assert [f for f, _ in G.MapRenderView._fields_] == ["n_valid", "n_drawn", "n_pixels", "n_meas", "n_both", "n_agree", "n_closer", "n_through"]
    q = G.map_render_params(splat=2, radius=0.02, background=(1, 2, 3), cx=8.0)
    assert (q.splat, q.radius, list(q.background), q.cx, q.max_half) == (2, 0.02, [1, 2, 3], 8.0, 8)
    with pytest.raises(TypeError):
        G.map_render_params(no_such_field=1)
    assert G.lib.fgo_debug_map_render_kernel_ms() >= 0.0


def test_bad_arguments_are_refused_without_a_device():
    assert _call(drop=("res",))[0] == E                           # result NULL
    assert _call(n=-1)[0] == E and _call(nv=-1)[0] == E           # a negative count
    assert _call(n=1 << 31)[0] == E and _call(n=1 << 40)[0] == E
    for w, h in ((0, 12), (16, 0), (-1, 12), (16, -3), (4097, 4096), (1 << 24, 2)):      # a side < 1, more than 2^24 pixels
        assert _call(w=w, h=h)[0] == E, (w, h)
    assert _call(nv=1 << 17, w=128, h=128)[0] == E                # n_views x width x height = 2^31
    assert _call(nv=1 << 62, w=1, h=1)[0] == E and _call(nv=1 << 40, w=4096, h=4096)[0] == E
    for ch in (-1, 2, 4):
        assert _call(ch=ch)[0] == E, ch
    nan, inf = float("nan"), float("inf")
    bad = dict(fx=(0.0, -250.0, nan, inf), fy=(0.0, -250.0, nan, inf), z_scale=(0.0, -0.001, nan, inf), cx=(nan, inf, -inf), cy=(nan, inf, -inf),
               z_min=(-0.1, 50.0, 60.0, nan), z_max=(2047.5, 0.1, 0.0, nan, inf), splat=(-1, 33), max_half=(-1, 33),
               radius=(-0.01, nan, inf, 2047.5), agree_tol=(-0.01, nan, inf, 2047.5))
    for field, values in bad.items():
        for v in values:
            assert _call(params=G.map_render_params(**{field: v}))[0] == E, (field, v)
    assert _call(params=G.map_render_params(splat=9))[0] == E     # max_half (8) below splat
    assert _call(params=G.map_render_params(splat=5, max_half=4))[0] == E
    for name in ("xyz", "pose"):                                  # a NULL required pointer
        assert _call(drop=(name,))[0] == E, name
    assert _call(ch=3, color=False)[0] == E and _call(ch=1, color=False)[0] == E          # channels without colour
    assert _call(ch=0, color=True)[0] == E                                               # colour without channels
    assert _call(ch=0, color_out=True)[0] == E                                           # a colour image without channels
    zero_q = np.array([[1.0, 2, 3, 0, 0, 0, 0]])
    assert _call(pose=zero_q)[0] == E and _call(ext=zero_q[0])[0] == E and _call(off=zero_q[0])[0] == E
    assert _call(pose=np.array([[0, 0, 0, np.nan, 0, 0, 1.0]]))[0] == E and _call(off=[0, 0, 0, np.inf, 0, 0, 1.0])[0] == E
    two = np.tile(np.array(IDENT), (2, 1)); two[1, 3:] = 0
    assert _call(nv=2, pose=two)[0] == E                          # the second view's
    # the bad arguments are refused for a call without views or points as well
    assert _call(nv=0, params=G.map_render_params(splat=-1))[0] == E and _call(n=0, params=G.map_render_params(z_max=4000.0))[0] == E
    assert _call(nv=0, w=0)[0] == E and _call(nv=0, ch=2)[0] == E and _call(nv=0, drop=("res",))[0] == E
    assert _call(nv=0, ch=0, color_out=True)[0] == E and _call(nv=0, ext=zero_q[0])[0] == E


def test_no_views_is_ok_with_a_zero_result_and_a_valid_call_needs_a_device():
    for rc, res in (_call(nv=0), _call(nv=0, drop=("pose",), outs=False), _call(nv=0, n=0, ch=3, color=False, drop=("xyz", "pose")), _call(nv=0, depth=True)):
        assert rc == 0
        assert [getattr(res, f) for f, _ in G.MapRenderResult._fields_] == [0] * 4
    o = G.map_render_batch(np.zeros((5, 3)), np.zeros((0, 7)), color=np.zeros((5, 3), np.uint8), width=16, height=12, want_index=True, want_rt=True)
    assert {k: (v.shape if hasattr(v, "shape") else v) for k, v in o.items()} == dict(
        n_points=0, n_nonfinite=0, form=0, tile_rows=0, n_valid=(0,), n_drawn=(0,), n_pixels=(0,), n_meas=(0,), n_both=(0,), n_agree=(0,),
        n_closer=(0,), n_through=(0,), zq=(0, 12, 16), index=(0, 12, 16), color=(0, 12, 16, 3), rt=(0, 12))
    assert o["zq"].dtype == np.int32 and o["index"].dtype == np.int32 and o["color"].dtype == np.uint8 and o["n_valid"].dtype == np.int64
    if G.lib.fgo_device_count() <= 0:
        assert _call()[0] == -2
        assert _call(outs=False)[0] == -2                         # counts only
        assert _call(n=0, drop=("xyz",))[0] == -2                 # no points: every view is background
        assert _call(ch=3, nv=2, ext=[0.1, 0, 0, 0, 0, 1, 1], off=[0, -2, -5, 0.1, 0, 0, 1], depth=True)[0] == -2
        assert _call(ch=1, params=G.map_render_params(z_min=0.0, z_max=2047.0, splat=32, max_half=32, radius=2047.0, agree_tol=2047.0))[0] == -2
        assert _call(w=4096, h=4096, outs=False)[0] == -2 and _call(n=(1 << 31) - 1, nv=0)[0] == 0                 # the bounds themselves
        with pytest.raises(G.FgoError, match="-2"):
            G.map_render_batch(np.zeros((2, 3)), [IDENT], width=16, height=12)


def test_python_wrappers_refuse_misshapen_arrays_and_write_ppm_writes_both_kinds(tmp_path):
    with pytest.raises(G.FgoError, match="n x 3"):
        G.map_render_batch(np.zeros(6), [IDENT])
    with pytest.raises(G.FgoError, match="V x 7"):
        G.map_render_batch(np.zeros((2, 3)), np.zeros((3, 6)))
    with pytest.raises(G.FgoError, match="color"):
        G.map_render_batch(np.zeros((2, 3)), [IDENT], color=np.zeros((2, 2), np.uint8))
    with pytest.raises(G.FgoError, match="want_color"):
        G.map_render_batch(np.zeros((2, 3)), [IDENT], want_color=True)
    with pytest.raises(G.FgoError, match="depth"):
        G.map_render_batch(np.zeros((2, 3)), [IDENT], width=16, height=12, depth=np.zeros((2, 12, 16), np.uint16))
    with pytest.raises(G.FgoError, match="look_at"):
        G.look_at((0, 0, 0), (0, 0, 0), (0, -1, 0))
    with pytest.raises(G.FgoError, match="look_at"):
        G.look_at((0, 0, 0), (0, 0, 1), (0, 0, -2))
    rgb = (np.arange(4 * 5 * 3) * 3 % 256).astype(np.uint8).reshape(4, 5, 3)
    G.write_ppm(tmp_path / "a.ppm", rgb)
    G.write_ppm(tmp_path / "a.pgm", rgb[..., 1])
    assert (tmp_path / "a.ppm").read_bytes() == b"P6\n5 4\n255\n" + rgb.tobytes()
    assert (tmp_path / "a.pgm").read_bytes() == b"P5\n5 4\n255\n" + np.ascontiguousarray(rgb[..., 1]).tobytes()
    with pytest.raises(G.FgoError, match="write_ppm"):
        G.write_ppm(tmp_path / "b.ppm", np.zeros((4, 5, 2), np.uint8))
    with pytest.raises(G.FgoError, match="write_ppm"):
        G.write_ppm(tmp_path / "b.ppm", np.zeros((4, 5)))
