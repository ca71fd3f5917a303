"""The numpy restatement of fgo_map_clean (tests/map_clean_reference.py) held to an INDEPENDENT brute force on the CPU: on clouds of
at most 400 points the dense matrix of integer squared distances, its transitive closure by repeated boolean squaring, the numbering
by smallest member and the floor stage in plain Python integers.  Partition, sizes, numbering, reasons and every floor output must be
EQUAL.  The clouds: the small cases of tests/test_gpu_map_clean.py, and 20 uniform clouds in boxes sized so that the number of
clusters lies strictly between 1 and n -- asserted per cloud, so that the test cannot pass on trivial partitions."""
import numpy as np
import pytest

from tests import map_clean_reference as ref


def brute(xyz, **params):
    P = dict(ref.DEFAULTS, **params)
    x = np.asarray(xyz, np.float64).reshape(-1, 3)
    n = len(x)
    assert n <= 400
    T = int(np.rint(P["tolerance"] * 2.0 ** 20))
    Q = [[0, 0, 0] for _ in range(n)]
    ok = np.zeros(n, bool)
    for p in range(n):                                             # Python integers: nothing can overflow
        if all(np.isfinite(v) and abs(v * 2.0 ** 20) < 2.0 ** 62 for v in x[p]):
            Q[p] = [int(np.rint(v * 2.0 ** 20)) for v in x[p]]
            ok[p] = all(abs(q // T) < (1 << 20) for q in Q[p])
    ids = [p for p in range(n) if ok[p]]
    A = np.zeros((n, n), bool)
    for a in ids:
        for b in ids:
            A[a, b] = sum((Q[a][k] - Q[b][k]) ** 2 for k in range(3)) <= T * T
    while True:                                                    # reachability in 1, 2, 4, ... steps
        B = (A.astype(np.float32) @ A.astype(np.float32)) > 0
        if np.array_equal(A, B):
            break
        A = B
    first = {p: int(np.argmax(A[p])) for p in ids}                 # the smallest member of p's component
    roots = sorted(set(first.values()))
    label = np.full(n, -1, np.int32)
    for p in ids:
        label[p] = roots.index(first[p])
    size = np.array([int(np.sum(label == c)) for c in range(len(roots))], np.int32)
    reason = np.where(ok, 0, 1).astype(np.uint8)
    for p in ids:
        s = size[label[p]]
        if s < P["min_cluster_size"] or (P["max_cluster_size"] and s > P["max_cluster_size"]):
            reason[p] = 2
    left = [p for p in ids if reason[p] == 0]
    out = dict(n_points=n, n_out_of_range=n - len(ids), n_cells=len({tuple(q // T for q in Q[p]) for p in ids}), n_clusters=len(roots),
               n_clusters_kept=len({label[p] for p in left}), n_after_clusters=len(left), n_floor_removed=0, floor_bin=-1,
               floor_bin_points=0, floor_height=0.0)
    lift = 0.0
    if P["remove_floor"] and left:
        R, S, C = (int(np.rint(P[f] * 2.0 ** 20)) for f in ("floor_res", "floor_span", "floor_clearance"))
        h = {p: P["up_sign"] * Q[p][P["up_axis"]] for p in left}
        h_min = min(h.values())
        count = {}
        for p in left:
            if h[p] - h_min <= S:
                b = (h[p] - h_min + R // 2) // R
                count[b] = count.get(b, 0) + 1
        fb = min(b for b in count if count[b] == max(count.values()))
        F = h_min + fb * R
        for p in left:
            if not h[p] > F + C:
                reason[p] = 3
        out.update(n_floor_removed=int(np.sum(reason == 3)), floor_bin=fb, floor_bin_points=count[fb], floor_height=float(F) * 2.0 ** -20)
        lift = P["up_sign"] * out["floor_height"]
    index = np.nonzero(ok & (reason == 0))[0].astype(np.int64)
    rows = x[index].copy()
    if out["floor_bin"] >= 0:
        rows[:, P["up_axis"]] = rows[:, P["up_axis"]] - lift
    out.update(n_kept=len(index), label=label, reason=reason, cluster_size=size, index=index, xyz=rows)
    return out


def _same(x, P):
    got, want = ref.clean(x, **P), brute(x, **P)
    for f in ref.RESULT_FIELDS:
        assert got[f] == want[f], (f, got[f], want[f])
    for f in ref.ARRAYS:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape and np.array_equal(got[f], want[f]), f
    assert got["xyz"].tobytes() == want["xyz"].tobytes()
    return got


def test_small_cases_equal_the_brute_force():
    for extra, k in ((0, 1), (1, 2)):
        assert _same(*ref.closed_radius(extra))["n_clusters"] == k
    for far in (False, True):
        for o in ref.DIRECTIONS:
            assert list(_same(*ref.direction_pairs(o, far))["label"]) == [0, 0, 1, 2], o
    assert _same(*ref.chain(300))["n_clusters"] == 1 and _same(*ref.chain(300, drop=100))["n_clusters"] == 2
    assert _same(*ref.one_cell(150, 150))["n_cells"] == 1
    assert _same(*ref.lattice(9, 8, 3))["n_clusters"] == 1
    assert _same(*ref.sized_clusters((6, 7, 9, 10), min_cluster_size=7, max_cluster_size=9))["n_kept"] == 16
    assert _same(*ref.sized_clusters((30, 29), min_cluster_size=30, max_cluster_size=30))["n_kept"] == 30
    assert _same(*ref.out_of_range())["n_out_of_range"] == 7
    x, P = ref.out_of_range()
    _same(x, dict(P, remove_floor=1, floor_clearance=1e300))


def test_floor_cases_equal_the_brute_force():
    R = ref.quanta(0.1)
    rng = np.random.default_rng(12)
    h = np.concatenate([[0], R + np.arange(4) * 7, 2 * R + np.arange(2), 3 * R - np.arange(4) * 5, [4 * R], 5 * R + np.arange(3)])
    assert _same(*ref.heights(h))["floor_bin"] == 1
    assert _same(*ref.heights(np.concatenate([[0], np.full(5, R), [2 * R - 1, 2 * R, 2 * R + 1, 9 * R]])))["n_kept"] == 2
    h = np.concatenate([-R - rng.integers(0, R // 4, 40), rng.integers(-R // 2, 12 * R, 100)])
    for up_axis in range(3):
        for up_sign in (1, -1):
            assert _same(*ref.heights(h, up_axis, up_sign))["floor_height"] < 0
    h = np.concatenate([np.arange(10) * 5, 30 * R + np.arange(40) * 5])
    assert _same(*ref.heights(h))["floor_bin"] == 0 and _same(*ref.heights(h, floor_span=4.0))["floor_bin"] == 30
    assert _same(*ref.heights(h, min_cluster_size=2))["floor_bin"] == -1
    assert _same(*ref.heights(h, floor_res=2.0 ** -20, floor_span=4096 * 2.0 ** -20, floor_clearance=0.0))["n_kept"] == 49
    assert _same(*ref.heights(np.arange(50) * 3 + 17))["n_kept"] == 0


@pytest.mark.parametrize("seed", range(20))
def test_random_clouds_equal_the_brute_force(seed):
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(150, 401))
    tol = 0.03 * (1 + seed % 3)
    # the box, side x side x 3 side, holds 0.7 to 2.2 neighbours per point within tol: below the percolation threshold of spheres
    # (about 2.7), so neither one cluster nor n of them
    side = tol * (n * (4.0 / 3.0) * np.pi / (3.0 * rng.uniform(0.7, 2.2))) ** (1.0 / 3.0)
    x = rng.uniform(-0.5 * side, 0.5 * side, (n, 3)) + rng.uniform(-1, 1, 3)
    x[:, 2] *= 3.0                                                 # a few bins of height
    P = dict(tolerance=tol, min_cluster_size=1 + seed % 4, max_cluster_size=(0, 40)[seed % 2], up_axis=seed % 3,
             up_sign=(1, -1)[seed % 2], floor_res=0.05, floor_clearance=0.02)
    got = _same(x, P)
    assert 1 < got["n_clusters"] < n, got["n_clusters"]
