"""fgo_map_normals on the GPU against the numpy restatement (tests/map_normals_reference.py).

Integer outputs -- neighbour, dist2, n_neighbours, status, scatter and the result fields -- are compared for EQUALITY.  Floating
outputs are held to bounds in eps = 2^-52 with the constant K of the restatement (16 x its own error against 50 digits, measured in
tests/test_map_normals_reference_cpu.py, never fitted to the kernel): the eigenvalues within K eps l2; the normal's residual
|A n - l0 n| <= K eps l2 and | |n| - 1 | <= 4 eps always; its direction against the restatement sin(angle) <= K eps l2 / (l1 - l0),
the points with (l1 - l0) < 1e-6 l2 left out; its sign where |n.(v - p)| > 1e-9 |v - p| (against the restatement's normal where the direction is compared, and n.(v - p) >= 0 in the
stated arithmetic for every valid point); at most 5 % of a cloud's valid points may be
left out by either exclusion (the cases made to be degenerate are exempt).  The curvature is the stated quotient of the call's own
eigenvalues, bit for bit."""
import functools
import itertools

import numpy as np
import pytest

import graph_slam_amd as G
from tests import map_fuse_reference as mf
from tests import map_normals_reference as ref

pytestmark = pytest.mark.gpu

EPS, K = ref.EPS, ref.K


def _run(x, P):
    return G.map_normals(x, params=G.map_normals_params(**P), want_neighbours=True, want_scatter=True)


def _ints_equal(got, want, fields=ref.RESULT_FIELDS):
    for f in fields:
        assert got[f] == want[f], (f, got[f], want[f])
    for f in ref.INT_ARRAYS:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, f
        assert np.array_equal(got[f], want[f]), (f, np.nonzero(np.any(np.atleast_2d(got[f].T != want[f].T), 0))[0][:5])


def _floats_hold(got, want, P, exempt=False, only_residual=False):
    """the floating outputs of a call whose integer outputs equal the restatement's; returns the number of valid points"""
    v = want["status"] == 0
    for f in ref.FLOAT_ARRAYS:
        assert got[f].dtype == np.float64 and got[f].shape == want[f].shape, f
        assert np.all(np.isnan(got[f][~v])) and np.all(np.isfinite(got[f][v])), f
    if not v.any():
        return 0
    n, e, we, wn = got["normal"][v], got["eigenvalues"][v], want["eigenvalues"][v], want["normal"][v]
    l2 = we[:, 2]
    assert np.all(np.diff(e, axis=1) >= 0)
    assert np.all(np.abs(np.sqrt(np.sum(n * n, 1)) - 1.0) <= 4 * EPS)
    res = ref.residual(want["A"][v], n, e[:, 0], l2)
    print("residual %.2f" % res.max(), end=" ")
    assert np.all(res <= K), res.max()
    assert got["curvature"][v].tobytes() == (e[:, 0] / ((e[:, 0] + e[:, 1]) + e[:, 2])).tobytes()
    view = np.asarray(dict(ref.DEFAULTS, **P)["viewpoint"], np.float64)
    d = view[None, :] - want["Q"][v].astype(np.float64) * 2.0 ** -20
    assert np.all((n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2] >= 0)
    if only_residual:
        return int(v.sum())
    err = ref.eigenvalue_error(e, we, l2)
    print("eigenvalues %.2f" % err.max(), end=" ")
    assert np.all(err <= K), err.max()
    gap = (we[:, 1] - we[:, 0]) >= ref.GAP_MIN * l2
    if gap.any():
        dirn = ref.direction_error(n[gap], wn[gap], we[gap])
        print("direction %.2f" % dirn.max(), end=" ")
        assert np.all(dirn <= K), dirn.max()
    _, s, dist = ref.orient(wn, want["Q"][v], view)
    sure = s > ref.SIGN_MIN * dist
    # against the restatement's normal where the direction is comparable at all (in an eigenspace of l0 = l1 the two are different
    # vectors); the call's own n.(v - p) >= 0 was asserted above for EVERY valid point
    assert np.all(np.sum(n[sure & gap] * wn[sure & gap], 1) > 0)
    print("left out: gap %d sign %d of %d" % ((~gap).sum(), (~sure).sum(), v.sum()))
    if not exempt:
        assert (~gap).sum() <= ref.MAX_LEFT_OUT * v.sum() and (~sure).sum() <= ref.MAX_LEFT_OUT * v.sum()
    return int(v.sum())


def _check(x, P, **kw):
    """one call against the restatement; returns (the call's outputs, the restatement's)"""
    want = ref.normals(x, **P)
    got = _run(x, P)
    _ints_equal(got, want)
    _floats_hold(got, want, P, **kw)
    return got, want


@functools.lru_cache(maxsize=None)
def _corner_want(k):
    return ref.normals(ref.corner(), k=k)


def test_an_integer_lattice_where_every_shell_is_a_tie():
    x = ref.lattice()
    for P in (dict(k=20, max_radius=0.05), dict(k=7), dict(k=27, max_radius=0.02)):      # the last: the radius ends the lists
        assert ref.tie_at_the_end(x, **P).any() or P["k"] == 27
        got, want = _check(x, P, exempt=True)
        assert want["n_valid"] == len(x)
    assert want["n_neighbours"].max() == 7
    # the first 7 of an inner point: itself, then its six nearest in ascending INDEX
    Q = want["Q"]
    inner = int(np.nonzero(np.all(Q == 0, 1))[0][0])
    six = np.nonzero(np.sum(np.abs(Q), 1) == 20000)[0]
    assert list(_run(x, dict(k=7))["neighbour"][inner]) == [inner] + sorted(six)


def test_the_kth_neighbour_exactly_at_the_radius_is_taken_and_one_quantum_further_is_not():
    x, P = ref.closed_radius(0)
    got, _ = _check(x, P, exempt=True)
    assert list(got["neighbour"][0]) == [0, 1, 2, 3] and got["dist2"][0][3] == ref.R3 ** 2 and got["n_neighbours"][0] == 4
    x, P = ref.closed_radius(1)
    got, _ = _check(x, P, exempt=True)
    assert list(got["neighbour"][0]) == [0, 1, 2, -1] and got["n_neighbours"][0] == 3
    assert G.lib.fgo_debug_map_normals_kernel_ms() > 0.0


@pytest.mark.parametrize("at_origin", [True, False])
def test_neighbours_across_a_cell_border_in_all_26_directions(at_origin):
    for o in (o for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 0, 0)):
        x, P = ref.direction_cloud(o, at_origin)
        got, want = _check(x, P, exempt=True)
        assert np.all(got["n_neighbours"] == 5) and want["n_cells"] == 2, o


def test_reach_small_clouds_and_an_isolated_point_after_every_ring():
    c = ref.corner()
    got, _ = _check(c[:2], dict(k=20, max_radius=16.0, cell=1.0))
    assert list(got["status"]) == [2, 2] and got["n_few"] == 2 and list(got["n_neighbours"]) == [2, 2]
    got, _ = _check(c[:3], dict(k=20, max_radius=16.0, cell=1.0), exempt=True)
    assert list(got["n_neighbours"]) == [3, 3, 3] and list(got["status"]) == [0, 0, 0]
    got, _ = _check(c[:19], dict(k=20, max_radius=16.0, cell=1.0), exempt=True)
    assert np.all(got["n_neighbours"] == 19) and np.all(got["neighbour"][:, 19] == -1)
    x, P = ref.blob_and_loner()
    assert P["max_radius"] / P["cell"] == 16.0
    got, _ = _check(x, P)
    assert got["status"][-1] == 2 and got["n_neighbours"][-1] == 1 and list(got["neighbour"][-1][:2]) == [len(x) - 1, -1]
    assert got["n_few"] == 1 and got["n_valid"] == len(x) - 1


def test_coincident_points_are_degenerate_and_a_line_is_valid():
    x = np.zeros((30, 3)) + [0.1, -0.2, 0.3]
    got, _ = _check(x, dict(k=20))
    assert np.all(got["status"] == 3) and got["n_degenerate"] == 30 and got["n_cells"] == 1
    assert np.all(got["neighbour"] == np.arange(20)[None, :]) and np.all(got["dist2"] == 0) and np.all(got["scatter"] == 0)
    x = ref.line()
    want = ref.normals(x)
    got = _run(x, {})
    _ints_equal(got, want)
    assert _floats_hold(got, want, {}, only_residual=True) == len(x)


def test_the_worst_case_of_the_list_every_candidate_displaces_one():
    x, P = ref.one_cell_descending()
    got, want = _check(x, P)
    assert want["n_cells"] == 1 and list(got["neighbour"][0]) == [0] + list(range(5000, 4981, -1))


@pytest.mark.parametrize("k", [3, 20, 64])
def test_the_corner_cloud(k):
    want = _corner_want(k)
    got = _run(ref.corner(), dict(k=k))
    _ints_equal(got, want)
    assert _floats_hold(got, want, dict(k=k)) == 3000 and np.all(got["n_neighbours"] == k)


def test_points_out_of_range_take_no_part():
    x, n_bad = ref.out_of_range()
    got, want = _check(x, {})
    bad = got["status"] == 1
    assert got["n_out_of_range"] == n_bad == bad.sum() and np.all(got["n_neighbours"][bad] == 0)
    assert np.all(got["neighbour"][bad] == -1) and np.all(got["dist2"][bad] == -1) and np.all(got["scatter"][bad] == 0)
    assert not np.isin(np.nonzero(bad)[0], got["neighbour"]).any()                 # nobody's neighbour
    assert got["n_few"] == 3                                                        # the last quanta in range: on their own
    got, _ = _check(x[bad], {})                                                     # nothing but such points
    assert got["n_cells"] == 0 and got["n_out_of_range"] == n_bad and got["n_valid"] == 0


def test_the_smallest_clouds_the_cell_index_can_go_wrong_on():
    P = dict(k=3)
    # nothing but the empty key for the sort, no run head for the gather
    got, _ = _check(np.array([[np.nan, 0, 0], [1e30, 0, 0], [0, np.inf, 0], [0, 0, -1e30], [40000.0, 0, 0]]), P)
    assert np.all(got["status"] == 1) and got["n_out_of_range"] == 5 and got["n_cells"] == 0
    got, _ = _check(np.array([[0.1, 0.2, 0.3]]), P)                        # the only run head is at s == 0
    assert got["n_few"] == 1 and got["n_cells"] == 1
    got, _ = _check(np.full((257, 3), 0.5), P)                             # one cell, one run, one point past a workgroup
    assert got["n_degenerate"] == 257 and got["n_cells"] == 1


def test_every_output_is_bit_identical_for_every_cell():
    x = ref.corner()
    want = _corner_want(20)
    base = None
    for cell in (2.0 ** -6, 0.04, 0.16):
        got = _run(x, dict(cell=cell))
        _ints_equal(got, want, fields=[f for f in ref.RESULT_FIELDS if f != "n_cells"])
        assert got["n_cells"] == len(np.unique(want["Q"] // ref.quanta(cell), axis=0))
        if base is None:
            base = got
        for f in ref.INT_ARRAYS + ref.FLOAT_ARRAYS:
            assert got[f].tobytes() == base[f].tobytes(), (f, cell)
    x, P = ref.one_cell_descending(600)
    a, b = _run(x, dict(P, cell=2.0 ** -6, max_radius=0.25)), _run(x, dict(P, cell=16.0, max_radius=0.25))
    for f in ref.INT_ARRAYS + ref.FLOAT_ARRAYS:
        assert a[f].tobytes() == b[f].tobytes(), f


def test_twice_is_bit_identical_and_a_permutation_maps_through():
    x = ref.corner()
    assert not ref.tie_at_the_end(x).any()
    a, b = _run(x, {}), _run(x, {})
    _ints_equal(a, _corner_want(20))
    for f in ref.INT_ARRAYS + ref.FLOAT_ARRAYS:
        assert a[f].tobytes() == b[f].tobytes(), f
    for perm in (np.arange(len(x))[::-1], np.random.default_rng(27).permutation(len(x))):
        r = _run(x[perm], {})
        for f in ref.RESULT_FIELDS:
            assert r[f] == a[f], f
        for f in ("n_neighbours", "status", "dist2", "scatter", "normal", "curvature", "eigenvalues"):
            assert r[f].tobytes() == a[f][perm].tobytes(), f
        assert np.array_equal(perm[r["neighbour"]], a["neighbour"][perm])           # every list is full: no -1


def test_an_exact_plane_and_the_viewpoint_on_either_side_and_inside_it():
    x = ref.plane()
    for view, nz in (((0.0, 0.0, 3.0), 1.0), ((0.0, 0.0, 0.0), -1.0), ((0.05, -0.02, 1.0), 1.0)):
        P = dict(k=20, viewpoint=view)
        got, want = _check(x, P, exempt=view[2] == 1.0)                             # in the plane no sign can be compared
        assert want["n_valid"] == len(x)
        assert np.all(got["eigenvalues"][:, 0] == 0) and np.all(got["curvature"] == 0)
        assert np.all(np.abs(got["normal"] - [0.0, 0.0, nz]) <= K * EPS), view
    # the third viewpoint lies IN the plane: n.(v - p) is exactly 0 and the first non-zero component is made positive
    d = np.array([0.05, -0.02, 1.0])[None, :] - want["Q"].astype(np.float64) * 2.0 ** -20
    n = got["normal"]
    assert np.all((n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2] == 0) and np.all(n[:, 2] > 0)


def test_end_to_end_from_depth_frames_to_the_normals_of_the_cleaned_map():
    c = mf.case("big_across_origin")
    m = G.map_fuse_batch(c["depth"], c["pose_w"], c["color"], c["extrinsic"], params=G.map_params(**c["params"]))
    cl = G.map_clean(m["xyz"], m["color"], m["count"], params=G.map_clean_params(up_axis=1, up_sign=-1))
    assert cl["n_kept"] == 6280
    got, want = _check(cl["xyz"], {})
    assert got["n_valid"] == 6280 and np.all(got["n_neighbours"] == 20)
    assert G.lib.fgo_debug_map_normals_kernel_ms() > 0.0
    assert np.all(np.sum(got["normal"] * -cl["xyz"], 1) > -1e-6)                     # the viewpoint is the origin
    assert np.all(got["curvature"] >= -K * EPS) and np.all(got["curvature"] <= 1.0 / 3.0 + K * EPS)
