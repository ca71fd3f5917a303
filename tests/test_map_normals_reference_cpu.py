"""The numpy restatement of fgo_map_normals (tests/map_normals_reference.py) held to independent evaluations on the CPU: its
neighbour sets against scipy's cKDTree on tie-free clouds, its lists against a plain Python sort on an all-ties lattice, its
integer scatter against Python integers, and its eigen-decomposition (np.linalg.eigh) against mpmath at 50 digits.  The last one
MEASURES the constant K of the GPU test: K >= 16 x the largest error of eigh, in units of eps l2 (eigenvalues, residual) and
eps l2 / (l1 - l0) (direction), over a sample of every cloud the GPU test fits.

Measured over ALL points of these clouds (this file samples every `stride`-th to stay quick), worst cloud first:
    corner k = 3    eigenvalues 6.37  residual 2.05  direction 1.18        corner k = 64   6.31  2.45  1.82
    corner k = 20   5.25  2.00  1.60      lattice  2.75  1.72  0.81      plane  1.12  0  0      line  0.60  0.70  -
16 x 6.37 = 101.99 <= K = 102."""
import mpmath
import numpy as np
import pytest
from scipy.spatial import cKDTree

from tests import map_normals_reference as ref


def test_neighbour_sets_equal_scipys_kd_tree_on_tie_free_clouds():
    for x, P in ((ref.corner(), dict(k=20)), (ref.corner()[:700], dict(k=64, max_radius=0.2)), (ref.corner()[:500], dict(k=3, max_radius=0.01))):
        assert not ref.tie_at_the_end(x, **P).any()
        w = ref.normals(x, **P)
        k = P["k"]
        Q = w["Q"].astype(np.float64)                                  # integers below 2^53: the tree's distances are exact enough to rank
        d, i = cKDTree(Q).query(Q, k=k, distance_upper_bound=float(ref.quanta(P.get("max_radius", 0.16))) * (1 + 1e-12))
        i = np.where(np.isfinite(d), i, -1)
        assert np.array_equal(np.sort(i, 1), np.sort(w["neighbour"], 1))
        assert np.array_equal((i >= 0).sum(1), w["n_neighbours"])
        have = w["neighbour"] >= 0
        assert np.all(np.diff(np.where(have, w["dist2"], np.iinfo(np.int64).max), axis=1) >= 0)
        assert np.array_equal(w["dist2"][have], np.rint(np.sort(d, 1)[have] ** 2).astype(np.int64))
    assert (ref.normals(ref.corner()[:500], k=3, max_radius=0.01)["n_neighbours"] < 3).any()      # the radius did cut


def test_lists_on_a_lattice_equal_a_plain_sort_with_ties_by_index():
    x = ref.lattice()
    P = dict(k=20, max_radius=0.05)
    w = ref.normals(x, **P)
    Q = [tuple(int(v) for v in q) for q in w["Q"]]
    R2 = ref.quanta(0.05) ** 2
    assert ref.tie_at_the_end(x, **P).any()
    for p in range(0, len(Q), 7):
        pairs = sorted((sum((a - b) ** 2 for a, b in zip(Q[q], Q[p])), q) for q in range(len(Q)))
        pairs = [t for t in pairs if t[0] <= R2][:20]
        m = len(pairs)
        assert w["n_neighbours"][p] == m
        assert [int(v) for v in w["neighbour"][p][:m]] == [q for _, q in pairs] and np.all(w["neighbour"][p][m:] == -1)
        assert [int(v) for v in w["dist2"][p][:m]] == [d for d, _ in pairs] and np.all(w["dist2"][p][m:] == -1)
        # the scatter matrix in Python integers
        d = [[Q[q][c] - Q[p][c] for c in range(3)] for _, q in pairs]
        S1 = [sum(t[c] for t in d) for c in range(3)]
        M = [m * sum(t[a] * t[b] for t in d) - S1[a] * S1[b] for a, b in zip(*ref.TRI)]
        assert [int(v) for v in w["scatter"][p]] == M


def test_status_counts_and_the_orientation_rule():
    x, n_bad = ref.out_of_range()
    w = ref.normals(x)
    assert w["n_out_of_range"] == n_bad and np.all(w["n_neighbours"][w["status"] == 1] == 0)
    assert w["n_valid"] + w["n_few"] + w["n_degenerate"] + w["n_out_of_range"] == w["n_points"]
    assert np.all(np.isnan(w["normal"][w["status"] != 0])) and np.all(np.isfinite(w["normal"][w["status"] == 0]))
    w = ref.normals(np.zeros((30, 3)) + [0.1, 0.2, 0.3], k=20)
    assert np.all(w["status"] == 3) and w["n_degenerate"] == 30 and np.array_equal(w["neighbour"][29], np.arange(20))
    assert np.all(ref.normals(ref.corner()[:2])["status"] == 2)
    for v in ((0.0, 0.0, 0.0), (0.0, 0.0, 3.0)):
        w = ref.normals(ref.corner(), viewpoint=v)
        d = np.array(v) - w["Q"] * 2.0 ** -20
        assert np.all(np.sum(w["normal"] * d, 1) >= 0)
    n, _, _ = ref.orient(np.array([[0.0, 0.0, -1.0], [0.0, -1.0, 0.0], [0.0, 1.0, 0.0]]), np.zeros((3, 3), np.int64), (5.0, 0.0, 0.0))
    assert np.array_equal(n, [[0, 0, 1], [0, 1, 0], [0, 1, 0]])       # n.(v - p) == 0: the first non-zero component positive


def eigh_errors(x, P, stride):
    """the largest error of the restatement's eigh against mpmath at 50 digits over every stride-th valid point of the cloud, in the
    three units of the GPU test: (eigenvalues, residual, direction)"""
    w = ref.normals(x, **P)
    worst = [0.0, 0.0, 0.0]
    with mpmath.workdps(50):
        for p in np.nonzero(w["status"] == 0)[0][::stride]:
            m = int(w["n_neighbours"][p])
            s = [int(v) for v in w["scatter"][p]]
            # A as the call defines it: each entry converted to double once, then divided (the division is the double's)
            A = mpmath.matrix(3, 3)
            for (a, b), v in zip(zip(*ref.TRI), s):
                A[a, b] = A[b, a] = mpmath.mpf(float(np.float64(v) / np.float64(m * m * 2.0 ** 40)))
            E, V = mpmath.eigsy(A)
            order = sorted(range(3), key=lambda j: E[j])
            l = [E[j] for j in order]
            unit = mpmath.mpf(ref.EPS) * l[2]
            got = [mpmath.mpf(float(v)) for v in w["eigenvalues"][p]]
            worst[0] = max(worst[0], float(max(abs(g - t) for g, t in zip(got, l)) / unit))
            n = mpmath.matrix([mpmath.mpf(float(v)) for v in w["normal"][p]])
            r = A * n - got[0] * n
            worst[1] = max(worst[1], float(mpmath.norm(r) / unit))
            if l[1] - l[0] >= ref.GAP_MIN * l[2]:
                t = V[:, order[0]]
                c = [n[1] * t[2] - n[2] * t[1], n[2] * t[0] - n[0] * t[2], n[0] * t[1] - n[1] * t[0]]
                sin = mpmath.sqrt(sum(v * v for v in c)) / mpmath.norm(t)
                worst[2] = max(worst[2], float(sin * (l[1] - l[0]) / unit))
    return worst


CLOUDS = [("corner_k20", lambda: (ref.corner(), dict(k=20)), 5), ("corner_k3", lambda: (ref.corner(), dict(k=3)), 5),
          ("corner_k64", lambda: (ref.corner(), dict(k=64)), 5), ("lattice", lambda: (ref.lattice(), dict(k=20)), 5),
          ("plane", lambda: (ref.plane(), dict(k=20, viewpoint=(0.0, 0.0, 3.0))), 10), ("line", lambda: (ref.line(), dict(k=20)), 1)]


@pytest.mark.parametrize("name,make,stride", CLOUDS, ids=[c[0] for c in CLOUDS])
def test_eigh_against_50_digits_measures_k(name, make, stride):
    x, P = make()
    worst = eigh_errors(x, P, stride)
    print("%s: eigh against 50 digits, in eps units: eigenvalues %.2f residual %.2f direction %.2f" % ((name,) + tuple(worst)))
    assert ref.K >= 16.0 and 16.0 * max(worst) <= ref.K, worst
