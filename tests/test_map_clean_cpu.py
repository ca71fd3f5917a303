"""CPU-only checks of the map cleaning entry point (include/fgo.h fgo_map_clean): the symbols are exported, the defaults are the
declared ones, the structs have the declared layout, every bad argument is refused before any HIP call and every bound itself is
accepted, an empty cloud is FGO_OK with a zero result and floor_bin = -1, and a valid call FAILS LOUDLY without a GPU (no CPU
fallback), as fgo_map_fuse_batch does."""
import ctypes as C

import numpy as np
import pytest

import graph_slam_amd as G

E, NODEV = -1, -2
NO_GPU = G.lib.fgo_device_count() <= 0


def _call(n=4, params=None, drop=(), outs=True):
    """a cloud of 4 points unless told otherwise; `drop` names required pointers passed as NULL.  Returns (rc, result)."""
    m = min(max(n, 1), 4)                                         # a refused call touches no array
    xyz = np.arange(3.0 * m).reshape(m, 3)
    label = np.zeros(m, np.int32); reason = np.zeros(m, np.uint8); csize = np.zeros(m, np.int32)
    index = np.zeros(m, np.int64); out = np.zeros((m, 3))
    res = G.MapCleanResult(*([7] * 10 + [7.0]))
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if outs else None
    rc = G.lib.fgo_map_clean(0, n, None if "xyz" in drop else G._dp(xyz), None if params is None else C.byref(params),
                             None if "res" in drop else C.byref(res), i32(label), reason.ctypes.data_as(C.POINTER(C.c_uint8)) if outs else None,
                             i32(csize), G._i64p(index) if outs else None, G._dp(out) if outs else None)
    return rc, res


def _accepted(rc):
    """not refused: without a device the call gets as far as looking for one"""
    return rc == NODEV if NO_GPU else rc == 0


def test_symbols_defaults_and_struct_layout():
    for s in ("fgo_map_clean", "fgo_map_clean_params_default", "fgo_debug_map_clean_kernel_ms"):
        assert hasattr(G.lib, s), s
    for s in ("map_clean", "map_clean_params", "MapCleanParams", "MapCleanResult"):
        assert hasattr(G, s), s
    p = G.MapCleanParams()
    G.lib.fgo_map_clean_params_default(C.byref(p))
    assert (p.tolerance, p.min_cluster_size, p.max_cluster_size, p.remove_floor, p.up_axis, p.up_sign) == (0.03, 200, 0, 1, 2, 1)
    assert (p.floor_res, p.floor_span, p.floor_clearance) == (0.1, 2.0, 0.1)
    G.lib.fgo_map_clean_params_default(None)                      # tolerated
    # C layout: double, 5 ints, (pad), 3 doubles; 10 int64, double
    assert C.sizeof(G.MapCleanParams) == 56 and C.sizeof(G.MapCleanResult) == 88
    V = G.MapCleanParams
    assert (V.tolerance.offset, V.min_cluster_size.offset, V.max_cluster_size.offset, V.remove_floor.offset, V.up_axis.offset,
            V.up_sign.offset, V.floor_res.offset, V.floor_span.offset, V.floor_clearance.offset) == (0, 8, 12, 16, 20, 24, 32, 40, 48)
    R = G.MapCleanResult
    assert [getattr(R, f).offset for f, _ in R._fields_] == [8 * k for k in range(11)]
    assert [f for f, _ in R._fields_] == ["n_points", "n_out_of_range", "n_cells", "n_clusters", "n_clusters_kept", "n_after_clusters",
                                          "n_floor_removed", "n_kept", "floor_bin", "floor_bin_points", "floor_height"]
    q = G.map_clean_params(tolerance=0.05, min_cluster_size=20, up_axis=1, up_sign=-1)
    assert (q.tolerance, q.min_cluster_size, q.up_axis, q.up_sign, q.floor_res) == (0.05, 20, 1, -1, 0.1)
    with pytest.raises(TypeError):
        G.map_clean_params(no_such_field=1)
    assert G.lib.fgo_debug_map_clean_kernel_ms() >= 0.0


def test_bad_arguments_are_refused_without_a_device():
    assert _call(drop=("res",))[0] == E and _call(drop=("xyz",))[0] == E
    for n in (-1, 1 << 30, 1 << 40):
        assert _call(n=n)[0] == E, n
    nan, inf = float("nan"), float("inf")
    bad = dict(tolerance=(0.0, -0.03, 2.0 ** -21, 256.5, nan, inf), min_cluster_size=(0, -1), max_cluster_size=(-1, 1, 199),
               up_axis=(-1, 3), up_sign=(0, 2, -2), remove_floor=(-1, 2), floor_res=(0.0, -0.1, 2.0 ** -21, 1024.5, nan, inf),
               floor_span=(-1e-9, -2.0, nan, inf, 409.7), floor_clearance=(-1e-9, nan, inf))
    for field, values in bad.items():
        for v in values:
            assert _call(params=G.map_clean_params(**{field: v}))[0] == E, (field, v)
    assert _call(params=G.map_clean_params(min_cluster_size=5, max_cluster_size=4))[0] == E
    assert _call(params=G.map_clean_params(floor_res=2.0 ** -20, floor_span=4097 * 2.0 ** -20))[0] == E
    # the bad arguments are refused for an empty cloud as well
    assert _call(n=0, params=G.map_clean_params(tolerance=0.0))[0] == E and _call(n=0, drop=("res",))[0] == E
    assert _call(n=0, params=G.map_clean_params(up_sign=0))[0] == E


def test_the_bounds_themselves_and_unused_floor_fields_are_accepted():
    nan = float("nan")
    good = [dict(tolerance=2.0 ** -20), dict(tolerance=256.0), dict(min_cluster_size=1), dict(min_cluster_size=200, max_cluster_size=200),
            dict(max_cluster_size=0), dict(up_axis=0), dict(up_axis=2, up_sign=-1), dict(remove_floor=0),
            dict(floor_res=2.0 ** -20, floor_span=4096 * 2.0 ** -20), dict(floor_res=1024.0, floor_span=0.0), dict(floor_res=0.125, floor_span=512.0),
            dict(floor_clearance=0.0), dict(floor_clearance=1e300),
            dict(remove_floor=0, floor_res=nan, floor_span=-1.0, floor_clearance=nan)]     # not looked at without the floor stage
    for kw in good:
        assert _accepted(_call(params=G.map_clean_params(**kw))[0]), kw
    assert _accepted(_call(outs=False)[0]) and _accepted(_call(params=None)[0])


def test_empty_cloud_is_ok_with_a_zero_result_and_a_valid_call_needs_a_device():
    for rc, res in (_call(n=0), _call(n=0, drop=("xyz",), outs=False)):
        assert rc == 0
        assert [getattr(res, f) for f, _ in G.MapCleanResult._fields_] == [0] * 8 + [-1, 0, 0.0]
    o = G.map_clean(np.zeros((0, 3)), color=np.zeros((0, 3), np.uint8), count=np.zeros(0, np.int32))
    assert {k: (v.shape if hasattr(v, "shape") else v) for k, v in o.items()} == dict(
        n_points=0, n_out_of_range=0, n_cells=0, n_clusters=0, n_clusters_kept=0, n_after_clusters=0, n_floor_removed=0, n_kept=0,
        floor_bin=-1, floor_bin_points=0, floor_height=0.0, label=(0,), reason=(0,), cluster_size=(0,), index=(0,), xyz=(0, 3),
        color=(0, 3), count=(0,))
    assert o["label"].dtype == np.int32 and o["reason"].dtype == np.uint8 and o["cluster_size"].dtype == np.int32
    assert o["index"].dtype == np.int64 and o["xyz"].dtype == np.float64
    if NO_GPU:
        assert _call()[0] == NODEV and _call(outs=False)[0] == NODEV
        with pytest.raises(G.FgoError, match="-2"):
            G.map_clean(np.zeros((5, 3)))


def test_python_wrapper_refuses_misshapen_arrays():
    with pytest.raises(G.FgoError, match="n x 3"):
        G.map_clean(np.zeros(6))
    with pytest.raises(G.FgoError, match="n x 3"):
        G.map_clean(np.zeros((4, 2)))
    with pytest.raises(G.FgoError, match="color"):
        G.map_clean(np.zeros((4, 3)), color=np.zeros((3, 3), np.uint8))
    with pytest.raises(G.FgoError, match="color"):
        G.map_clean(np.zeros((4, 3)), color=np.zeros((4, 3, 1), np.uint8))
    with pytest.raises(G.FgoError, match="count"):
        G.map_clean(np.zeros((4, 3)), count=np.zeros(5, np.int32))
