"""fgo_map_fuse_batch on the GPU against the numpy restatement (tests/map_fuse_reference.py): one call per configuration, rt first --
so that a failure names the stage -- then key, count, xyz, color, frame_points and every result field compared for EQUALITY: the
point arithmetic is not contracted, the sums are integers and the output is sorted, so there is nothing to tolerate.  Then the hash
table at a load above 0.9 with probes that wrap, a table that is too small, max_voxels below n_voxels, the same call twice and with
the frames reversed, both insert forms, and end to end: poses from an optimised context go in and the walls come out as planes."""
import os

import numpy as np
import pytest

import graph_slam_amd as G
from tests import map_fuse_reference as ref

pytestmark = pytest.mark.gpu

ARRAYS = ("key", "count", "xyz", "color", "frame_points")


def _run(c, **kw):
    P = dict(c["params"], **kw.pop("params", {}))
    return G.map_fuse_batch(c["depth"], c["pose_w"], c["color"], c["extrinsic"], params=G.map_params(**P), want_keys=True, want_rt=True, **kw)


def _equal(got, want, fields=ARRAYS + ref.RESULT_FIELDS, rows=None):
    assert np.array_equal(got["rt"], want["rt"]), "rt"
    for f in fields:
        w = want[f]
        if w is None:
            assert got[f] is None, f
            continue
        if rows is not None and f in ("key", "count", "xyz", "color"):
            w = w[:rows]
        assert np.shape(got[f]) == np.shape(w) and np.array_equal(got[f], w), f


@pytest.mark.parametrize("name", [c["name"] for c in ref.CONFIGS])
def test_configuration_equals_the_restatement(name):
    c = ref.case(name)
    got = _run(c)
    _equal(got, c["want"])
    assert got["count"].dtype == np.int32 and got["key"].dtype == np.int64 and got["xyz"].dtype == np.float64
    assert G.lib.fgo_debug_map_fuse_kernel_ms() > 0.0


def test_both_insert_forms_give_the_same_map():
    """FGO_MAP_INSERT picks the insert kernel of a call: the LDS pre-aggregation over a run of one frame's pixels (lds) or over a run
    of pixels of 128 consecutive frames (frames, the default), and the plain form"""
    old = os.environ.get("FGO_MAP_INSERT")
    try:
        for form in ("lds", "frames", "plain"):
            os.environ["FGO_MAP_INSERT"] = form
            for name in ("small_skip1", "one_pose_leaf8", "fine_leaf", "big_across_origin", "many_tiny", "empty_frame"):
                c = ref.case(name)
                _equal(_run(c), c["want"])
    finally:
        if old is None:
            os.environ.pop("FGO_MAP_INSERT", None)
        else:
            os.environ["FGO_MAP_INSERT"] = old


def test_a_nearly_full_table_whose_probes_wrap_gives_the_same_map():
    """fine_leaf has n_voxels distinct keys; with fewer rows of its frames the number of voxels is brought just under 2^T: the load is
    above 0.9, clusters of linear probing run past the last slot, and the output does not change"""
    c = ref.case("fine_leaf")
    T = 12
    w = ref.fuse(c["depth"], c["pose_w"], c["color"], c["extrinsic"], **dict(c["params"], rect=(0, 0, 44, 30), table_log2=T))
    occupied = w["n_voxels"] + w["n_dropped"]
    assert 0.9 * (1 << T) < occupied <= (1 << T), occupied
    got = _run(c, params=dict(rect=(0, 0, 44, 30), table_log2=T))
    _equal(got, w)
    assert got["status"] == G.FGO_MAP_OK and got["table_log2"] == T


def test_a_table_that_is_too_small_reports_full_and_writes_no_voxel():
    c = ref.case("fine_leaf")
    w = c["want"]
    assert w["n_voxels"] > 1 << 10
    got = _run(c, params=dict(table_log2=10))
    assert got["status"] == G.FGO_MAP_FULL and got["n_voxels"] == 0 and got["n_dropped"] == 0 and got["table_log2"] == 10
    assert got["xyz"].shape == (0, 3) and got["count"].shape == (0,) and got["key"].shape == (0,)
    assert got["n_sampled"] == w["n_sampled"] and got["n_valid"] == w["n_valid"] and np.array_equal(got["frame_points"], w["frame_points"])
    assert np.array_equal(got["rt"], w["rt"])


def test_max_voxels_below_n_voxels_truncates_in_key_order():
    c = ref.case("small_skip1")
    w = c["want"]
    for cap in (w["n_voxels"] - 1, 100, 1, 0):
        got = _run(c, max_voxels=cap)
        assert got["status"] == G.FGO_MAP_TRUNCATED and got["n_voxels"] == w["n_voxels"]
        _equal(got, w, fields=ARRAYS + tuple(f for f in ref.RESULT_FIELDS if f != "status"), rows=cap)
    assert _run(c, max_voxels=w["n_voxels"])["status"] == G.FGO_MAP_OK


def test_twice_and_reversed_are_bit_identical():
    c = ref.case("big_across_origin")
    a, b = _run(c), _run(c)
    rev = dict(c, depth=c["depth"][::-1].copy(), pose_w=c["pose_w"][::-1].copy(), color=c["color"][::-1].copy())
    r = _run(rev)
    for f in ("key", "count", "xyz", "color") + ref.RESULT_FIELDS:
        assert np.array_equal(a[f], b[f]) and np.array_equal(a[f], r[f]), f
    assert a["xyz"].tobytes() == b["xyz"].tobytes() == r["xyz"].tobytes()
    assert np.array_equal(a["frame_points"], b["frame_points"]) and np.array_equal(a["frame_points"], r["frame_points"][::-1])
    assert np.array_equal(a["rt"], r["rt"][::-1])


def test_out_of_range_points_and_a_single_frame_without_colour_outputs():
    """a pose far outside the grid and a non-finite one: their points are counted, the others stored; depth as H x W"""
    c = ref.case("empty_frame")
    pose = c["pose_w"].copy()
    pose[0, 0] = 1e9; pose[2, 1] = np.inf
    w = ref.fuse(c["depth"], pose, **c["params"])
    assert w["n_out_of_range"] > 0 and w["frame_points"][0] == 0 and w["frame_points"][2] == 0 and w["frame_points"][3] > 0
    got = G.map_fuse_batch(c["depth"], pose, params=G.map_params(**c["params"]), want_keys=True, want_rt=True)
    _equal(got, w, fields=ARRAYS + ref.RESULT_FIELDS)
    one = G.map_fuse_batch(c["depth"][3], c["pose_w"][3], params=G.map_params(**c["params"]))
    w1 = ref.fuse(c["depth"][3:4], c["pose_w"][3:4], **c["params"])
    assert "key" not in one and "rt" not in one and np.array_equal(one["xyz"], w1["xyz"]) and np.array_equal(one["count"], w1["count"])


def test_end_to_end_optimised_poses_give_walls_that_are_planes():
    """key-frame poses of the corner scene, chained by exact relative-pose edges, start off their places, are optimised
    (fgo_optimize) and read back (fgo_get_poses); the frames fused under them give the three walls: the centroids of each wall fit a
    plane with an rms below the sigma_z the scene was rendered with"""
    rng = np.random.default_rng(77)
    n, W, H = 8, 88, 72
    cam = ref.px.camera(W, H)
    truth = np.stack([ref.corner_pose(rng, ref.SHIFT) for _ in range(n)])
    depth = np.stack([ref.render_frame(truth[f], W, H, cam, ref.SIGMA_Z, rng, ref.SHIFT)[0] for f in range(n)])
    conj = lambda q: np.array([-q[0], -q[1], -q[2], q[3]])
    ei = np.concatenate([np.arange(n - 1), np.arange(n - 2)]); ej = np.concatenate([np.arange(1, n), np.arange(2, n)])
    meas = np.zeros((len(ei), 7))
    for k, (i, j) in enumerate(zip(ei, ej)):                       # z = x_i^-1 x_j
        Ri = ref.quat_matrix(truth[i, 3:])
        meas[k, :3] = Ri.T @ (truth[j, :3] - truth[i, :3])
        meas[k, 3:] = ref.quat_mul(conj(truth[i, 3:]), truth[j, 3:])
    info = np.tile(np.eye(6)[np.triu_indices(6)], (len(ei), 1))
    start = truth.copy()
    start[1:, :3] += 0.05 * rng.normal(size=(n - 1, 3))
    for f in range(1, n):
        start[f, 3:] = ref.quat_mul(start[f, 3:], ref.quat_axis(f % 3, 0.03 * rng.normal()))
    fixed = np.zeros(n, np.uint8); fixed[0] = 1
    gr = G.Graph(device=0)
    gr.add_poses(start, fixed)
    gr.add_edges(ei, ej, meas, info)
    assert gr.chi2() > 1e-3
    gr.optimize(20)
    assert gr.chi2() < 1e-10
    poses = gr.get_poses()
    gr.close()
    P = dict(cam, skip=1, leaf=0.11, min_points=4)                 # no wall within 2.8 sigma_z of a voxel face
    got = G.map_fuse_batch(depth, poses, params=G.map_params(**P))
    assert got["status"] == G.FGO_MAP_OK and got["n_voxels"] > 100
    # the walls of the world: x = 1.6, y = 1.1, z = 2.2, moved by -SHIFT
    walls = ref.ROOM_HI - ref.SHIFT
    dist = np.abs(got["xyz"] - walls)                              # m x 3: the distance of a centroid to each wall
    near = np.argmin(dist, 1)
    clear = np.sort(dist, 1)[:, 1] > 0.15                          # away from the edges where two walls meet
    for k in range(3):
        p = got["xyz"][(near == k) & clear]
        assert len(p) > 30, k
        q = p - p.mean(0)
        normal = np.linalg.svd(q, full_matrices=False)[2][2]
        rms = float(np.sqrt(np.mean((q @ normal) ** 2)))
        assert abs(normal[k]) > 0.999 and rms < ref.SIGMA_Z, (k, rms)
        assert abs(p.mean(0)[k] - walls[k]) < ref.SIGMA_Z
