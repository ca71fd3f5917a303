"""fgo_map_clean on the GPU against the numpy restatement (tests/map_clean_reference.py): label, reason, cluster_size, index, xyz and
every result field compared for EQUALITY -- everything that decides an outcome is integer arithmetic and the output is in input
order, so there is nothing to tolerate.  The clouds are built from quanta, so that a distance of exactly T is exactly T: the closed
radius, the 26 directions across a cell border on both sides of the origin, a chain of 20 000 points (the deepest union-find the
link kernel can be handed), 10 000 points in one cell (every lane hooks under the same root), a bridge, the size bounds, two fused
maps with many clusters, points out of range, the smallest clouds of the cell index, the floor stage at its ties and edges, the cell lookup at its edge, permutations of
the input, and end to end from depth frames."""
import numpy as np
import pytest

import graph_slam_amd as G
from tests import map_clean_reference as ref
from tests import map_fuse_reference as mf

pytestmark = pytest.mark.gpu


def _equal(got, want):
    for f in ref.RESULT_FIELDS:
        assert got[f] == want[f], (f, got[f], want[f])
    for f in ref.ARRAYS:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape and np.array_equal(got[f], want[f]), f
    assert got["xyz"].tobytes() == want["xyz"].tobytes()


def _check(x, P, **kw):
    """one call against the restatement; returns the restatement's outputs"""
    want = ref.clean(x, **P)
    _equal(G.map_clean(x, params=G.map_clean_params(**P), **kw), want)
    return want


def test_the_radius_is_closed():
    w = _check(*ref.closed_radius(0))
    assert w["n_clusters"] == 1 and list(w["label"]) == [0, 0]
    w = _check(*ref.closed_radius(1))
    assert w["n_clusters"] == 2 and list(w["label"]) == [0, 1]
    assert G.lib.fgo_debug_map_clean_kernel_ms() > 0.0


@pytest.mark.parametrize("far_at_origin", [False, True])
def test_all_26_directions_across_a_cell_border_on_both_sides_of_the_origin(far_at_origin):
    for o in ref.DIRECTIONS:
        w = _check(*ref.direction_pairs(o, far_at_origin))
        assert list(w["label"]) == [0, 0, 1, 2], o                       # the near pair is one cluster, the far pair two


def test_a_chain_of_20000_points_is_one_cluster_and_two_without_one_of_them():
    x, P = ref.chain()
    w = _check(x, P)
    assert w["n_clusters"] == 1 and w["cluster_size"][0] == 20000 and w["n_cells"] > 10000
    w = _check(*ref.chain(drop=7777))
    assert w["n_clusters"] == 2 and sorted(w["cluster_size"]) == [7777, 12222]


def test_contention_on_one_root():
    w = _check(*ref.one_cell())
    assert w["n_cells"] == 1 and w["n_clusters"] == 1
    w = _check(*ref.lattice())
    assert w["n_cells"] == 4800 and w["n_clusters"] == 1


def test_a_bridge_of_one_point_joins_two_blobs():
    w = _check(*ref.bridge(True))
    assert w["n_clusters"] == 1 and w["n_kept"] == 601
    w = _check(*ref.bridge(False))
    assert w["n_clusters"] == 2 and w["n_kept"] == 0 and list(w["cluster_size"]) == [300, 300] and np.all(w["reason"] == 2)


def test_cluster_size_bounds_are_inclusive():
    w = _check(*ref.sized_clusters((6, 7, 9, 10), min_cluster_size=7, max_cluster_size=9))
    assert sorted(w["cluster_size"]) == [6, 7, 9, 10] and w["n_clusters_kept"] == 2 and w["n_kept"] == 16
    w = _check(*ref.sized_clusters((6, 7, 9, 10), min_cluster_size=7))
    assert w["n_clusters_kept"] == 3 and w["n_kept"] == 26
    w = _check(*ref.sized_clusters((199, 200), min_cluster_size=200, max_cluster_size=200))
    assert w["n_clusters_kept"] == 1 and w["n_kept"] == 200


def test_fused_maps_with_many_clusters():
    x = ref.fused("fine_leaf")[0]
    P = dict(tolerance=0.03, min_cluster_size=20, remove_floor=0)
    w = ref.clean(x, **P)
    assert 1 < w["n_clusters"] < w["n_points"]
    assert (w["n_points"], w["n_clusters"], w["n_kept"]) == (4752, 1009, 2153)       # what scipy's connected components gave
    _check(x, P)
    w = _check(ref.fused("small_skip1")[0], dict(tolerance=0.05, min_cluster_size=1, remove_floor=0))
    assert w["n_clusters"] == 14


def test_points_out_of_range_take_no_part():
    x, P = ref.out_of_range()
    w = _check(x, P)
    assert w["n_out_of_range"] == 7 and np.all(w["label"][w["reason"] == 1] == -1) and w["n_clusters"] == 6
    w = _check(x[w["reason"] == 1], P)                                    # nothing but such points
    assert w["n_cells"] == 0 and w["n_clusters"] == 0 and w["n_kept"] == 0 and w["floor_bin"] == -1


def test_the_smallest_clouds_the_cell_index_can_go_wrong_on():
    P = dict(min_cluster_size=1)
    # nothing but the empty key for the sort, no run head for the gather
    w = _check(np.array([[np.nan, 0, 0], [1e30, 0, 0], [0, np.inf, 0], [0, 0, -1e30], [40000.0, 0, 0]]), P)
    assert w["n_cells"] == 0 and w["n_out_of_range"] == 5 and np.all(w["reason"] == 1)
    w = _check(np.array([[0.1, 0.2, 0.3]]), P)                              # the only run head is at s == 0
    assert w["n_cells"] == 1 and w["n_clusters"] == 1
    w = _check(np.full((257, 3), 0.5), P)                                   # one cell, one run, one point past a workgroup
    assert w["n_cells"] == 1 and w["n_clusters"] == 1 and w["cluster_size"][0] == 257


def test_floor_ties_go_to_the_lower_bin_and_the_clearance_is_strict():
    R, C = ref.quanta(0.1), ref.quanta(0.1)
    # bins 0 .. 5: 1, 4, 2, 4, 1, 3 points
    h = np.concatenate([[0], R + np.arange(4) * 7, 2 * R + np.arange(2), 3 * R - np.arange(4) * 5, [4 * R], 5 * R + np.arange(3)])
    w = _check(*ref.heights(h))
    assert (w["floor_bin"], w["floor_bin_points"]) == (1, 4)
    # the floor bin's five points at F, and points at F + C - 1, F + C (removed) and F + C + 1 (kept)
    h = np.concatenate([[0], np.full(5, R), [R + C - 1, R + C, R + C + 1, 9 * R]])
    x, P = ref.heights(h)
    w = _check(x, P)
    Q = np.rint(x[:, 2] * 2.0 ** 20).astype(np.int64)
    assert w["floor_bin"] == 1 and w["n_kept"] == 2 and sorted(Q[w["index"]]) == [R + C + 1, 9 * R]
    assert np.all(w["reason"][Q <= R + C] == 3)


@pytest.mark.parametrize("up_axis", [0, 1, 2])
@pytest.mark.parametrize("up_sign", [1, -1])
def test_floor_with_heights_straddling_zero_along_every_axis(up_axis, up_sign):
    R = ref.quanta(0.1)
    rng = np.random.default_rng(12)
    h = np.concatenate([-R - rng.integers(0, R // 4, 40), rng.integers(-R // 2, 12 * R, 100)])      # the floor below zero
    w = _check(*ref.heights(h, up_axis, up_sign))
    assert w["floor_bin"] == 0 and w["floor_height"] < 0 and 0 < w["n_kept"] < 140 and w["n_floor_removed"] >= 40


def test_floor_in_one_bin_above_the_span_and_with_nothing_left():
    R = ref.quanta(0.1)
    w = _check(*ref.heights(np.arange(50) * 3 + 17))                       # every point in bin 0: all of them are floor
    assert (w["floor_bin"], w["floor_bin_points"], w["n_kept"]) == (0, 50, 0)
    # 10 points at the bottom, 40 in a denser layer 3 m up: above floor_span = 2, so it is not the floor
    h = np.concatenate([np.arange(10) * 5, 30 * R + np.arange(40) * 5])
    w = _check(*ref.heights(h))
    assert (w["floor_bin"], w["floor_bin_points"], w["n_kept"]) == (0, 10, 40)
    w = _check(*ref.heights(h, floor_span=4.0))                            # inside the span it is
    assert (w["floor_bin"], w["floor_bin_points"], w["n_kept"]) == (30, 40, 0)
    w = _check(*ref.heights(h, min_cluster_size=2))                        # no cluster survives: no floor stage
    assert w["n_after_clusters"] == 0 and w["floor_bin"] == -1 and w["n_kept"] == 0 and np.all(w["reason"] == 2)
    w = _check(*ref.heights(h, floor_res=2.0 ** -20, floor_span=4096 * 2.0 ** -20, floor_clearance=0.0))      # the most bins there are
    assert w["floor_bin"] == 0 and w["floor_bin_points"] == 1 and w["n_kept"] == 49


def test_the_cell_lookup_at_its_edge():
    """the lookup is a binary search of the sorted cell keys: clouds whose queried neighbour cells fall before the first and after
    the last occupied cell, between occupied cells, and on the out-of-range mark that ends the sorted keys"""
    P = dict(tolerance=0.03, min_cluster_size=1, remove_floor=0)
    x = np.random.default_rng(3).uniform(-0.15, 0.15, (200, 3))
    w = _check(x, P)
    assert 1 < w["n_clusters"] < 200
    _check(x[:1], P)                                                       # one cell: every query misses, on either side
    _check(*ref.one_cell(3, 5))
    bad = np.array([[np.nan, 0.0, 0.0]])
    w = _check(np.concatenate([bad, x[:50], bad, x[50:], bad]), P)         # the searches end next to the marks
    assert w["n_out_of_range"] == 3
    T = ref.quanta(0.03)
    hi, lo = T * ref.IMAX - 1, -T * (ref.IMAX - 1)                        # in the cells 2^20 - 1 and -(2^20 - 1)
    corners = ref.from_quanta([[hi, hi, hi], [lo, lo, lo], [hi, lo, hi]])
    w = _check(np.concatenate([corners, x[:20]]), P)                       # the first and the last cell there is: no cell beyond
    assert w["n_out_of_range"] == 0


def test_twice_is_bit_identical_and_a_permutation_maps_through():
    x = ref.fused("fine_leaf")[0]
    P = dict(tolerance=0.03, min_cluster_size=20, up_axis=1, up_sign=-1)
    a, b = (G.map_clean(x, params=G.map_clean_params(**P)) for _ in range(2))
    _equal(a, b)
    _equal(a, ref.clean(x, **P))
    for perm in (np.arange(len(x))[::-1], np.random.default_rng(13).permutation(len(x))):
        r = G.map_clean(x[perm], params=G.map_clean_params(**P))
        for f in ref.RESULT_FIELDS:
            assert r[f] == a[f], f
        assert np.array_equal(np.sort(perm[r["index"]]), a["index"])                      # the kept set
        assert np.array_equal(r["reason"], a["reason"][perm])
        assert np.array_equal(np.sort(r["cluster_size"]), np.sort(a["cluster_size"]))
        # the partition: labels correspond one to one
        pairs = np.unique(np.stack([r["label"], a["label"][perm]], 1), axis=0)
        assert len(pairs) == len(np.unique(pairs[:, 0])) == len(np.unique(pairs[:, 1]))
        order = np.argsort(perm[r["index"]])
        assert r["xyz"][order].tobytes() == a["xyz"].tobytes()


def test_end_to_end_from_depth_frames_to_the_cleaned_map():
    c = mf.case("big_across_origin")
    m = G.map_fuse_batch(c["depth"], c["pose_w"], c["color"], c["extrinsic"], params=G.map_params(**c["params"]))
    assert m["n_voxels"] == 12994
    P = dict(up_axis=1, up_sign=-1)                                         # the floor of that scene is its y = 0.4 wall
    got = G.map_clean(m["xyz"], m["color"], m["count"], params=G.map_clean_params(**P))
    want = ref.clean(m["xyz"], **P)
    _equal(got, want)
    assert got["n_clusters"] == 37 and got["cluster_size"].max() == 12943 and got["n_clusters_kept"] == 1
    assert got["n_kept"] + got["n_floor_removed"] + (got["n_points"] - got["n_after_clusters"]) == got["n_points"]
    assert abs(got["floor_height"] + 0.4) < 0.05
    h = -np.rint(m["xyz"][got["index"], 1] * 2.0 ** 20).astype(np.int64)
    F, C = int(np.rint(got["floor_height"] * 2.0 ** 20)), ref.quanta(0.1)
    assert got["n_kept"] > 1000 and np.all(h > F + C)
    assert np.array_equal(got["color"], m["color"][got["index"]]) and np.array_equal(got["count"], m["count"][got["index"]])
    assert np.array_equal(got["xyz"][:, [0, 2]], m["xyz"][got["index"]][:, [0, 2]])
    assert np.array_equal(got["xyz"][:, 1], m["xyz"][got["index"], 1] + got["floor_height"])
