"""CPU-only checks of the surface-normal entry point (include/fgo.h fgo_map_normals): the symbols are exported, the defaults are
the reference's (setKSearch(20)), the structs have the declared layout, every bad argument is refused before any HIP call and every
bound itself is accepted, an empty cloud is FGO_OK with a zero result, a valid call FAILS LOUDLY without a GPU (no CPU fallback),
the Python wrapper refuses misshapen arrays, and write_ply writes the normals when given and byte for byte what it always wrote
when not."""
import ctypes as C

import numpy as np
import pytest

import graph_slam_amd as G

E, NODEV = -1, -2
NO_GPU = G.lib.fgo_device_count() <= 0
REQUIRED = ("normal", "curvature", "nn", "status")


def _call(n=4, params=None, drop=(), optional=True):
    """a cloud of 4 points unless told otherwise; `drop` names pointers passed as NULL.  Returns (rc, result)."""
    m = min(max(n, 1), 4)                                         # a refused call touches no array
    k = 64
    xyz = np.arange(3.0 * m).reshape(m, 3)
    normal = np.zeros((m, 3)); curv = np.zeros(m); eig = np.zeros((m, 3)); nn = np.zeros(m, np.int32); status = np.zeros(m, np.uint8)
    nb = np.zeros((m, k), np.int32); d2 = np.zeros((m, k), np.int64); sc = np.zeros((m, 6), np.int64)
    res = G.MapNormalsResult(*([7] * 6))
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    rc = G.lib.fgo_map_normals(0, n, None if "xyz" in drop else G._dp(xyz), None if params is None else C.byref(params),
                               None if "res" in drop else C.byref(res), None if "normal" in drop else G._dp(normal),
                               None if "curvature" in drop else G._dp(curv), G._dp(eig) if optional else None,
                               None if "nn" in drop else i32(nn), None if "status" in drop else status.ctypes.data_as(C.POINTER(C.c_uint8)),
                               i32(nb) if optional else None, G._i64p(d2) if optional else None, G._i64p(sc) if optional else None)
    return rc, res


def _accepted(rc):
    """not refused: without a device the call gets as far as looking for one"""
    return rc == NODEV if NO_GPU else rc == 0


def test_symbols_defaults_and_struct_layout():
    for s in ("fgo_map_normals", "fgo_map_normals_params_default", "fgo_debug_map_normals_kernel_ms"):
        assert hasattr(G.lib, s), s
    for s in ("map_normals", "map_normals_params", "MapNormalsParams", "MapNormalsResult", "write_ply"):
        assert hasattr(G, s), s
    p = G.MapNormalsParams()
    G.lib.fgo_map_normals_params_default(C.byref(p))
    assert (p.k, p.max_radius, p.cell, tuple(p.viewpoint)) == (20, 0.16, 0.04, (0.0, 0.0, 0.0))      # setKSearch(20)
    G.lib.fgo_map_normals_params_default(None)                    # tolerated
    # C layout: int, (pad), double, double, double[3]; 6 int64
    assert C.sizeof(G.MapNormalsParams) == 48 and C.sizeof(G.MapNormalsResult) == 48
    V = G.MapNormalsParams
    assert (V.k.offset, V.max_radius.offset, V.cell.offset, V.viewpoint.offset) == (0, 8, 16, 24)
    R = G.MapNormalsResult
    assert [getattr(R, f).offset for f, _ in R._fields_] == [8 * j for j in range(6)]
    assert [f for f, _ in R._fields_] == ["n_points", "n_out_of_range", "n_cells", "n_valid", "n_few", "n_degenerate"]
    q = G.map_normals_params(k=8, viewpoint=(1.0, -2.0, 3.5))
    assert (q.k, q.max_radius, q.cell, tuple(q.viewpoint)) == (8, 0.16, 0.04, (1.0, -2.0, 3.5))
    with pytest.raises(TypeError):
        G.map_normals_params(no_such_field=1)
    assert G.lib.fgo_debug_map_normals_kernel_ms() >= 0.0


def test_bad_arguments_are_refused_without_a_device():
    assert _call(drop=("res",))[0] == E and _call(drop=("xyz",))[0] == E
    for name in REQUIRED:
        assert _call(drop=(name,))[0] == E, name
    for n in (-1, 1 << 30, 1 << 40):
        assert _call(n=n)[0] == E, n
    nan, inf = float("nan"), float("inf")
    bad = dict(k=(2, 0, -1, 65, 1 << 20), max_radius=(0.0, -0.16, 2.0 ** -21, 16.5, nan, inf),
               cell=(0.0, -0.04, 2.0 ** -7, 0.0156, 16.5, nan, inf))
    for field, values in bad.items():
        for v in values:
            assert _call(params=G.map_normals_params(**{field: v}))[0] == E, (field, v)
    for j in range(3):
        for v in (nan, inf, -inf):
            view = [0.0, 0.0, 0.0]
            view[j] = v
            assert _call(params=G.map_normals_params(viewpoint=view))[0] == E, (j, v)
    # more than 16 rings of cells
    assert _call(params=G.map_normals_params(max_radius=0.16, cell=2.0 ** -7 * 1.2))[0] == E
    assert _call(params=G.map_normals_params(max_radius=1.0, cell=0.0624))[0] == E
    assert _call(params=G.map_normals_params(max_radius=16.0, cell=0.99))[0] == E
    # the bad arguments are refused for an empty cloud as well
    assert _call(n=0, params=G.map_normals_params(k=2))[0] == E and _call(n=0, drop=("res",))[0] == E
    assert _call(n=0, params=G.map_normals_params(cell=1.0, max_radius=16.5))[0] == E


def test_the_bounds_themselves_are_accepted():
    good = [dict(k=3), dict(k=64), dict(max_radius=2.0 ** -20), dict(max_radius=16.0, cell=1.0), dict(max_radius=16.0, cell=16.0),
            dict(cell=2.0 ** -6), dict(max_radius=0.25, cell=2.0 ** -6), dict(max_radius=1.0, cell=0.0625),
            dict(viewpoint=(1e300, -1e300, 0.0))]
    for kw in good:
        assert _accepted(_call(params=G.map_normals_params(**kw))[0]), kw
    assert _accepted(_call(optional=False)[0]) and _accepted(_call(params=None)[0])


def test_empty_cloud_is_ok_with_a_zero_result_and_a_valid_call_needs_a_device():
    for rc, res in (_call(n=0), _call(n=0, drop=("xyz",) + REQUIRED, optional=False)):
        assert rc == 0
        assert [getattr(res, f) for f, _ in G.MapNormalsResult._fields_] == [0] * 6
    o = G.map_normals(np.zeros((0, 3)), want_neighbours=True, want_scatter=True)
    assert {k: (v.shape if hasattr(v, "shape") else v) for k, v in o.items()} == dict(
        n_points=0, n_out_of_range=0, n_cells=0, n_valid=0, n_few=0, n_degenerate=0, normal=(0, 3), curvature=(0,), eigenvalues=(0, 3),
        n_neighbours=(0,), status=(0,), neighbour=(0, 20), dist2=(0, 20), scatter=(0, 6))
    assert o["n_neighbours"].dtype == np.int32 and o["status"].dtype == np.uint8 and o["neighbour"].dtype == np.int32
    assert o["dist2"].dtype == np.int64 and o["scatter"].dtype == np.int64 and o["normal"].dtype == np.float64
    assert sorted(G.map_normals(np.zeros((0, 3)))) == sorted(["curvature", "eigenvalues", "n_cells", "n_degenerate", "n_few", "n_neighbours",
                                                              "n_out_of_range", "n_points", "n_valid", "normal", "status"])
    if NO_GPU:
        assert _call()[0] == NODEV and _call(optional=False)[0] == NODEV
        with pytest.raises(G.FgoError, match="-2"):
            G.map_normals(np.zeros((5, 3)))


def test_python_wrapper_refuses_misshapen_arrays():
    with pytest.raises(G.FgoError, match="n x 3"):
        G.map_normals(np.zeros(6))
    with pytest.raises(G.FgoError, match="n x 3"):
        G.map_normals(np.zeros((4, 2)))
    with pytest.raises(G.FgoError, match="n x 3"):
        G.map_normals(np.zeros((2, 4, 3)))
    with pytest.raises(G.FgoError, match="-1"):
        G.map_normals(np.zeros((4, 3)), params=G.map_normals_params(k=2))


def _present_writer(path, xyz, color=None):
    """the writer as it was before it learnt of normals, line for line"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    m = len(xyz)
    if color is None:
        rgb = np.full((m, 3), 255, np.uint8)
    else:
        rgb = np.asarray(color, np.uint8).reshape(m, -1)
        if rgb.shape[1] == 1:
            rgb = np.repeat(rgb, 3, 1)
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % m)
        for p, c in zip(xyz, rgb):
            f.write("%.9g %.9g %.9g %d %d %d\n" % (p[0], p[1], p[2], c[0], c[1], c[2]))


def test_write_ply_with_and_without_normals(tmp_path):
    rng = np.random.default_rng(31)
    xyz = rng.normal(0, 2, (17, 3)); rgb = rng.integers(0, 256, (17, 3)).astype(np.uint8); grey = rgb[:, 0]
    nrm = rng.normal(0, 1, (17, 3)); nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    for tag, color in (("none", None), ("rgb", rgb), ("grey", grey)):
        a, b = tmp_path / ("a_%s.ply" % tag), tmp_path / ("b_%s.ply" % tag)
        G.write_ply(str(a), xyz, color)
        _present_writer(str(b), xyz, color)
        assert a.read_bytes() == b.read_bytes(), tag
        G.write_ply(str(a), xyz, color, normals=None)
        assert a.read_bytes() == b.read_bytes(), tag
    p = tmp_path / "n.ply"
    G.write_ply(str(p), xyz, rgb, normals=nrm)
    lines = p.read_text().split("\n")
    head = lines[:lines.index("end_header") + 1]
    assert head == ["ply", "format ascii 1.0", "element vertex 17", "property float x", "property float y", "property float z",
                    "property float nx", "property float ny", "property float nz", "property uchar red", "property uchar green",
                    "property uchar blue", "end_header"]
    rows = np.array([[float(t) for t in ln.split()] for ln in lines[len(head):] if ln])
    assert rows.shape == (17, 9)
    assert np.allclose(rows[:, :3], xyz, rtol=1e-8, atol=0) and np.allclose(rows[:, 3:6], nrm, rtol=1e-8, atol=0)
    assert np.array_equal(rows[:, 6:], rgb)
    with pytest.raises(G.FgoError, match="normals"):
        G.write_ply(str(p), xyz, rgb, normals=nrm[:5])
