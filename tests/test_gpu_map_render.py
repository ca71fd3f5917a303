"""fgo_map_render_batch on the GPU against the numpy restatement (tests/map_render_reference.py): one call per case, rt first -- so
that a failure names the stage -- then zq, index, color, every per-view count and every result field compared for EQUALITY: the point
arithmetic is not contracted and a z-buffer is an integer minimum, so there is nothing to tolerate.  Then the points permuted, both
kernel forms (and the global form with its views in chunks), the calls without points, without views and without image outputs, the
same call twice, rt against the fusion's, and end to end: a wall fused from depth frames predicts those frames' depth."""
import os

import numpy as np
import pytest

import graph_slam_amd as G
from tests import map_fuse_reference as mf
from tests import map_render_reference as ref

pytestmark = pytest.mark.gpu

ARRAYS = ("zq", "index", "color")
PARAMS = tuple(ref.DEFAULTS)


def _run(c, **kw):
    P = {k: v for k, v in c.items() if k in PARAMS}
    a = dict(color=c.get("color"), extrinsic=c.get("extrinsic"), view_offset=c.get("view_offset"), width=c["width"], height=c["height"],
             depth=c.get("depth"), want_zq=True, want_index=True, want_rt=True)
    a.update(kw)
    return G.map_render_batch(c["xyz"], c["pose_w"], params=G.map_render_params(**P), **a)


def _equal(got, want, arrays=ARRAYS):
    assert np.array_equal(got["rt"], want["rt"]), "rt"
    for f in arrays:
        if want[f] is None:
            assert f not in got, f
            continue
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape and np.array_equal(got[f], want[f]), f
    for f in ref.VIEW_FIELDS:
        assert got[f].dtype == np.int64 and np.array_equal(got[f], want[f]), (f, got[f], want[f])
    for f in ref.RESULT_FIELDS:
        assert got[f] == want[f], (f, got[f], want[f])


class _env:
    """sets environment variables for a block and puts the old values back"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("name", list(ref.CASES))
def test_case_equals_the_restatement(name):
    c = ref.case(name)
    _equal(_run(c), c["want"])
    assert G.lib.fgo_debug_map_render_kernel_ms() > 0.0


@pytest.mark.parametrize("form", ["tiles", "global"])
def test_both_forms_give_the_same_outputs(form):
    """FGO_MAP_RENDER picks the kernel form of a call: a strip of a view per workgroup in an LDS z-buffer (tiles), or a device-wide
    z-buffer (global); only the two result fields that name the form differ.  one_column_more is too wide for a strip: global in
    both.  In the global form FGO_MAP_RENDER_ZWORDS makes the z-buffer small: 300 views of 44 x 36 then go in chunks of 6."""
    code = {"tiles": ref.TILES, "global": ref.GLOBAL}[form]
    with _env(FGO_MAP_RENDER=form):
        for name in ref.CASES:
            c = ref.case(name)
            _equal(_run(c), ref.with_form(c["want"], code, c["width"]))
    if form == "global":
        with _env(FGO_MAP_RENDER=form, FGO_MAP_RENDER_ZWORDS=str(6 * 44 * 36 + 100)):
            for name in ("many_views_rgb", "depth_check", "strips_176x144"):          # chunks of 6 views, of 1 view, and the floor of 1
                c = ref.case(name)
                _equal(_run(c), ref.with_form(c["want"], code, c["width"]))


def test_permuted_points_give_the_same_image():
    """zq and the counts do not depend on the order of the points; the index maps through the permutation wherever the pixel's
    minimum is unique -- everywhere but the two tied pixels of `ties`, where the smaller NEW index wins"""
    for name in ("ties", "strips_200x83", "footprints_radius"):
        c = ref.case(name)
        w = c["want"]
        perm = np.random.default_rng(12).permutation(len(c["xyz"]))
        pc = dict(c, xyz=c["xyz"][perm], color=None if c["color"] is None else c["color"][perm])
        got = _run(pc)
        _equal(got, ref.render(**{k: v for k, v in pc.items() if k != "want"}))
        assert np.array_equal(got["zq"], w["zq"]) and all(np.array_equal(got[f], w[f]) for f in ref.VIEW_FIELDS)
        # the pixels whose minimal zq is held by one point only
        P = dict(ref.DEFAULTS, **{k: v for k, v in c.items() if k in PARAMS})
        valid, drawn, zq, u0, v0, h = ref.project(c["xyz"], np.all(np.isfinite(c["xyz"]), 1), w["rt"][0], P, c["width"], c["height"])
        unique = np.zeros(w["zq"][0].shape, bool)
        for b in range(c["height"]):
            for a in range(c["width"]):
                if w["zq"][0, b, a] < 0:
                    continue
                hit = drawn & (np.abs(u0 - a) <= h) & (np.abs(v0 - b) <= h) & (zq == w["zq"][0, b, a])
                unique[b, a] = hit.sum() == 1
        assert unique.sum() >= (w["zq"][0] >= 0).sum() - 2 and unique.any()
        assert np.array_equal(perm[got["index"][0][unique]], w["index"][0][unique])


def test_rt_without_an_offset_equals_the_fusion_s():
    c = ref.case("many_views_plain")
    V = len(c["pose_w"])
    fused = G.map_fuse_batch(np.zeros((V, 4, 4), np.uint16), c["pose_w"], extrinsic=c["extrinsic"], want_rt=True)
    got = _run(c)
    assert np.array_equal(got["rt"], fused["rt"]) and got["rt"].tobytes() == fused["rt"].tobytes()
    off = _run(ref.case("many_views_grey"))
    assert not np.array_equal(off["rt"], fused["rt"])             # the chase camera moves every view


def test_no_points_no_views_and_counts_only():
    c = ref.case("depth_check")
    none = dict(c, xyz=np.zeros((0, 3)), color=np.zeros((0, 3), np.uint8))
    got = _run(none)
    _equal(got, ref.render(**{k: v for k, v in none.items() if k != "want"}))
    assert np.all(got["zq"] == -1) and np.all(got["index"] == -1) and np.all(got["color"] == np.array([0, 0, 26], np.uint8))
    assert got["n_pixels"].sum() == 0 and got["n_meas"].sum() > 0 and got["n_both"].sum() == 0
    empty = _run(dict(c, pose_w=np.zeros((0, 7)), depth=None))
    assert [empty[f] for f in ref.RESULT_FIELDS] == [0, 0, 0, 0] and empty["zq"].shape == (0, c["height"], c["width"])
    counts = _run(c, want_zq=False, want_index=False, want_rt=False)          # every image output NULL
    assert "zq" not in counts and "index" not in counts and "color" not in counts
    for f in ref.VIEW_FIELDS + ref.RESULT_FIELDS:
        assert np.array_equal(counts[f], c["want"][f]), f
    grey = ref.case("many_views_grey")
    only_color = _run(grey, want_zq=False, want_index=False)
    assert np.array_equal(only_color["color"], grey["want"]["color"]) and only_color["color"].shape == (300, 36, 44)


def test_same_call_twice_is_bit_identical():
    for name in ("strips_176x144", "many_views_rgb"):
        c = ref.case(name)
        a, b = _run(c), _run(c)
        for f in ARRAYS + ("rt",):
            assert a[f].tobytes() == b[f].tobytes(), f
        for f in ref.VIEW_FIELDS + ref.RESULT_FIELDS:
            assert np.array_equal(a[f], b[f]), f


def test_end_to_end_a_fused_wall_predicts_the_depth_of_its_frames():
    """A fronto-parallel wall at z = 2 m is seen by four cameras that differ by translations only, fused (leaf 0.02 m), and the map
    is rendered at the frames' own poses with the frames' intrinsics and radius = leaf.  The result equals the restatement, the
    depth check agrees on every pixel that is measured and covered, and with one camera moved 0.2 m forward the map stands in front
    of what that camera measured: every such pixel goes through.

    The bound on zq.  The depth words are 2^-10 m, the cameras' t_z are multiples of 2^-10 m and R is the identity, so a fused point
    has the world z-quantum Q_z = Z_w = 2 x 2^20 exactly.  The points of a voxel have their Q_z in [i L, (i + 1) L - 1] (L = the
    effective leaf in quanta), and so has their mean, the centroid: |centroid_z 2^20 - Q_z| <= L - 1 for each of its points, hence
    |centroid_z 2^20 - Z_w| <= L - 1.  The rendering subtracts t_z (an integer number of quanta) and rounds once, which moves the
    value by at most 1/2 + the rounding of one subtraction: |zq - (Z_w - t_z 2^20)| < L, an inequality between integers.  So every
    covered pixel's zq lies within one effective leaf of the wall's depth in that view."""
    W, H = 88, 72
    cam = dict(fx=150.0, fy=150.0, cx=43.5, cy=35.5, z_scale=2.0 ** -10, z_min=0.1, z_max=5.0)
    tz = np.array([0.0, 2.0 ** -6, 2.0 ** -5, -2.0 ** -6])
    poses = np.zeros((4, 7)); poses[:, 6] = 1.0
    poses[:, 0] = [0.0, 0.05, -0.04, 0.02]; poses[:, 1] = [0.0, 0.0, 0.03, -0.05]; poses[:, 2] = tz
    wall = 2.0
    words = ((wall - tz) * 1024.0).astype(np.uint16)
    assert np.array_equal(words.astype(np.float64) * 2.0 ** -10 + tz, np.full(4, wall))
    depth = np.broadcast_to(words[:, None, None], (4, H, W)).copy()
    leaf = 0.02
    fused = G.map_fuse_batch(depth, poses, params=G.map_params(skip=1, leaf=leaf, **cam))
    assert fused["status"] == G.FGO_MAP_OK and fused["n_voxels"] > 1000
    L = mf.leaf_quanta(leaf)
    c = dict(xyz=fused["xyz"], pose_w=poses, color=None, width=W, height=H, depth=depth, radius=leaf, agree_tol=0.05, **cam)
    got = _run(c)
    _equal(got, ref.render(**c))
    for v in range(4):
        covered = got["zq"][v] >= 0
        want_q = int((wall - tz[v]) * 2 ** 20)
        assert covered[10:-10, 10:-10].all()                       # radius = leaf closes the holes: no pixel of the middle is empty
        assert np.abs(got["zq"][v][covered].astype(np.int64) - want_q).max() <= L
        assert got["n_meas"][v] == W * H and got["n_both"][v] == got["n_pixels"][v] == got["n_agree"][v] > 0.9 * W * H
        assert got["n_closer"][v] == 0 and got["n_through"][v] == 0
    moved = poses.copy(); moved[2, 2] += 0.2                       # the camera believes it is 0.2 m nearer to the wall than it measured
    bad = _run(dict(c, pose_w=moved))
    assert bad["n_through"][2] == bad["n_both"][2] > 0 and bad["n_agree"][2] == 0
    assert all(bad["n_through"][v] == 0 and bad["n_agree"][v] == bad["n_both"][v] for v in (0, 1, 3))
