"""Numpy restatement of fgo_map_clean (include/fgo.h), written from the stated semantics and not from the kernel: np.rint for the
quantum, int64 floor division for the cell, the cells around a point found by np.searchsorted in the sorted cell keys, the integer
distance test on every candidate pair, and the connected components by label propagation -- every point carries the smallest index
it has heard of, an edge hands the smaller label of its ends to the larger one's owner, labels jump to their label's label, until no
edge joins two labels.  PCL's EuclideanClusterExtraction is not in the reference tree, so this file IS the yardstick of
csrc/kernels_map_clean.hip; tests/test_map_clean_reference_cpu.py pins it to a dense brute force on the CPU.

clean() returns the outputs of the call.  The case makers build the clouds of tests/test_gpu_map_clean.py from QUANTA (integers,
exact as doubles), so that a distance of exactly T is exactly T."""
import functools
import itertools

import numpy as np

from tests import map_fuse_reference as mf

QBITS = 20
IMAX = 1 << 20
DEFAULTS = dict(tolerance=0.03, min_cluster_size=200, max_cluster_size=0, remove_floor=1, up_axis=2, up_sign=1, floor_res=0.1,
                floor_span=2.0, floor_clearance=0.1)
RESULT_FIELDS = ("n_points", "n_out_of_range", "n_cells", "n_clusters", "n_clusters_kept", "n_after_clusters", "n_floor_removed",
                 "n_kept", "floor_bin", "floor_bin_points", "floor_height")
ARRAYS = ("label", "reason", "cluster_size", "index", "xyz")
PAIR_BUDGET = 1 << 22                 # candidate pairs tested at a time


def quanta(v):
    """llrint(v 2^20) of a parameter"""
    return int(np.rint(float(v) * float(1 << QBITS)))


def quantise(xyz, T):
    """Q, the cell c of the points (n x 3) and the mask of those in range"""
    x = np.asarray(xyz, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        y = x * float(1 << QBITS)
        ok = np.all(np.isfinite(x), 1) & np.all(np.abs(y) < 2.0 ** 62, 1)
    Q = np.zeros(x.shape, np.int64)
    Q[ok] = np.rint(y[ok]).astype(np.int64)
    c = Q // T
    ok &= np.all(np.abs(c) < IMAX, 1)
    return Q, c, ok


def _expand(cnt):
    """for counts (k): the owner of every one of sum(cnt) entries and its rank among its owner's"""
    owner = np.repeat(np.arange(len(cnt)), cnt)
    rank = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return owner, rank


def linked_pairs(Q, T):
    """every pair of the DISTINCT points Q (m x 3, int64) with |Q_a - Q_b|^2 <= T^2, once, and the number of occupied cells: the
    candidates of a point are the later points of its own cell and the points of the 13 neighbour cells whose offset is the smaller
    of the two opposite ones -- every pair of adjacent cells is visited from one side"""
    m = len(Q)
    if m == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), 0
    c = Q // T
    key = mf.make_key(c[:, 0], c[:, 1], c[:, 2])
    order = np.argsort(key, kind="stable")
    skey, sc, sQ = key[order], c[order], Q[order]
    ukey, start, cnt = np.unique(skey, return_index=True, return_counts=True)
    ea, eb = [], []
    for off in (o for o in itertools.product((-1, 0, 1), repeat=3) if o <= (0, 0, 0)):
        nc = sc + np.array(off)
        valid = np.all(np.abs(nc) < IMAX, 1)
        nkey = mf.make_key(nc[:, 0], nc[:, 1], nc[:, 2])
        at = np.minimum(np.searchsorted(ukey, nkey), len(ukey) - 1)
        src = np.nonzero(valid & (ukey[at] == nkey))[0]
        s0, n0 = start[at[src]], cnt[at[src]]
        if off == (0, 0, 0):                                       # its own cell: the points behind it
            s0, n0 = src + 1, s0 + n0 - (src + 1)
        lo = 0
        while lo < len(src):                                       # slices of sources whose candidates fit the budget
            hi = lo + max(1, int(np.searchsorted(np.cumsum(n0[lo:]), PAIR_BUDGET, side="right")))
            owner, rank = _expand(n0[lo:hi])
            a, b = src[lo:hi][owner], s0[lo:hi][owner] + rank
            d = sQ[a] - sQ[b]
            hit = np.sum(d * d, 1) <= T * T
            ea.append(order[a[hit]]); eb.append(order[b[hit]])
            lo = hi
    return np.concatenate(ea), np.concatenate(eb), len(ukey)


def components(m, ea, eb):
    """the smallest member of every point's connected component, by label propagation"""
    lab = np.arange(m)
    while True:
        la, lb = lab[ea], lab[eb]
        diff = la != lb
        if not diff.any():
            return lab
        np.minimum.at(lab, np.maximum(la, lb)[diff], np.minimum(la, lb)[diff])
        while True:
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt


def clean(xyz, **params):
    P = dict(DEFAULTS, **params)
    x = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    n = len(x)
    T = quanta(P["tolerance"])
    Q, _, ok = quantise(x, T)
    ids = np.nonzero(ok)[0]
    # coincident points are linked and have the same links: the components are those of the distinct points
    uq, inv = np.unique(Q[ids], axis=0, return_inverse=True) if len(ids) else (np.zeros((0, 3), np.int64), np.zeros(0, np.int64))
    inv = inv.reshape(-1)
    ea, eb, n_cells = linked_pairs(uq, T)
    lab = components(len(uq), ea, eb)
    first = np.full(len(uq), n, np.int64)                          # the smallest INPUT index of a component
    np.minimum.at(first, lab[inv], ids)
    root = np.full(n, -1, np.int64)
    root[ids] = first[lab[inv]]
    roots, size = np.unique(root[ids], return_counts=True)         # ascending: the numbering
    label = np.full(n, -1, np.int32)
    label[ids] = np.searchsorted(roots, root[ids])
    big = (size >= P["min_cluster_size"]) & ((P["max_cluster_size"] == 0) | (size <= P["max_cluster_size"]))
    reason = np.where(ok, 0, 1).astype(np.uint8)
    stage = ok.copy()
    stage[ids] = big[label[ids]]
    reason[ok & ~stage] = 2
    out = dict(n_points=n, n_out_of_range=int(n - len(ids)), n_cells=n_cells, n_clusters=len(roots), n_clusters_kept=int(big.sum()),
               n_after_clusters=int(stage.sum()), n_floor_removed=0, floor_bin=-1, floor_bin_points=0, floor_height=0.0)
    keep = stage.copy()
    lift = None
    if P["remove_floor"] and stage.any():
        h = P["up_sign"] * Q[:, P["up_axis"]]
        R, S = quanta(P["floor_res"]), quanta(P["floor_span"])
        C = min(quanta(P["floor_clearance"]), 1 << 62)             # no height reaches 2^49
        h_min = int(h[stage].min())
        low = stage & (h - h_min <= S)
        bins = np.bincount((h[low] - h_min + R // 2) // R)
        fb = int(np.argmax(bins))                                  # the first of the largest
        F = h_min + fb * R
        keep = stage & (h > F + C)
        reason[stage & ~keep] = 3
        lift = float(P["up_sign"]) * (float(F) * 2.0 ** -QBITS)
        out.update(n_floor_removed=int((stage & ~keep).sum()), floor_bin=fb, floor_bin_points=int(bins[fb]), floor_height=float(F) * 2.0 ** -QBITS)
    index = np.nonzero(keep)[0].astype(np.int64)
    rows = x[index].copy()
    if lift is not None:
        rows[:, P["up_axis"]] = rows[:, P["up_axis"]] - lift
    out.update(n_kept=len(index), label=label, reason=reason, cluster_size=size.astype(np.int32), index=index, xyz=rows)
    return out


# ---- the case makers: clouds in quanta

def from_quanta(Q):
    """points whose quantisation is exactly Q (|Q| < 2^53)"""
    return np.asarray(Q, np.int64).astype(np.float64).reshape(-1, 3) * 2.0 ** -QBITS


T3 = 3 << 13                          # 24576 quanta: (1, 2, 2) x 8192 has length exactly T3
TOL3 = T3 * 2.0 ** -QBITS
STEP3 = np.array([8192, 16384, 16384], np.int64)
NO_FLOOR = dict(remove_floor=0)


def closed_radius(extra):
    """two points at distance exactly T3 (extra = 0), or one quantum further in z"""
    return from_quanta([[0, 0, 0], STEP3 + [0, 0, extra]]), dict(tolerance=TOL3, min_cluster_size=1, **NO_FLOOR)


DIRECTIONS = [o for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 0, 0)]


def direction_pairs(o, far_at_origin):
    """4 points: a pair that straddles the border of cell 0 towards o at a distance of at most sqrt(3) quanta, and a pair in the same two
    cells T3 + 1 apart along every axis of o; one pair at the origin, the other 1024 cells away"""
    o = np.array(o, np.int64)
    near_a = np.where(o > 0, T3 - 1, np.where(o < 0, 0, 5)); near_b = np.where(o > 0, T3, np.where(o < 0, -1, 5))
    far_a = np.full(3, T3 // 2, np.int64); far_b = far_a + o * (T3 + 1)
    away = np.full(3, 1024 * T3, np.int64)
    shift_near, shift_far = (away, 0) if far_at_origin else (0, away)
    return from_quanta([near_a + shift_near, near_b + shift_near, far_a + shift_far, far_b + shift_far]), dict(tolerance=TOL3, min_cluster_size=1, **NO_FLOOR)


def chain(n=20000, drop=None, seed=5):
    """n points T3 apart along (1, 2, 2), through the origin, in shuffled order; without point `drop` of the chain if given"""
    k = np.arange(n, dtype=np.int64) - n // 2
    if drop is not None:
        k = np.delete(k, drop)
    Q = k[:, None] * STEP3
    return from_quanta(Q[np.random.default_rng(seed).permutation(len(Q))]), dict(tolerance=TOL3, min_cluster_size=1, **NO_FLOOR)


def one_cell(n_same=5000, n_more=5000, seed=6):
    """n_same coincident points and n_more others inside the same cell of the default tolerance"""
    T = quanta(DEFAULTS["tolerance"])
    rng = np.random.default_rng(seed)
    Q = np.concatenate([np.tile([[T // 2, T // 3, T // 5]], (n_same, 1)), rng.integers(0, T, (n_more, 3))])
    return from_quanta(Q[rng.permutation(len(Q))]), dict(min_cluster_size=1, **NO_FLOOR)


def lattice(nx=40, ny=40, nz=3, seed=7):
    """a lattice at a spacing of exactly T"""
    T = quanta(DEFAULTS["tolerance"])
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3).astype(np.int64)
    Q = (g - [nx // 2, ny // 2, 1]) * T
    return from_quanta(Q[np.random.default_rng(seed).permutation(len(Q))]), dict(min_cluster_size=1, **NO_FLOOR)


def bridge(with_bridge, seed=8):
    """two blobs of 300 points, each inside half a cell (a clique), 1.5 T apart, and the one point between them that links both"""
    T = quanta(DEFAULTS["tolerance"])
    rng = np.random.default_rng(seed)
    a = rng.integers(0, T // 2, (300, 3)); b = rng.integers(0, T // 2, (300, 3)) + [2 * T, 0, 0]
    a[0] = [T // 2, T // 4, T // 4]; b[0] = [2 * T, T // 4, T // 4]
    Q = np.concatenate([a, b] + ([[[T + T // 4, T // 4, T // 4]]] if with_bridge else []))
    return from_quanta(Q[rng.permutation(len(Q))]), dict(min_cluster_size=400, **NO_FLOOR)


def sized_clusters(sizes, seed=9, **params):
    """clusters of the given sizes: the points of one within a few quanta, the clusters 10 T apart along x, in shuffled order"""
    T = quanta(DEFAULTS["tolerance"])
    rng = np.random.default_rng(seed)
    Q = np.concatenate([rng.integers(-3, 4, (s, 3)) + [10 * T * (k - len(sizes) // 2), 0, 0] for k, s in enumerate(sizes)])
    return from_quanta(Q[rng.permutation(len(Q))]), dict(NO_FLOOR, **params)


def out_of_range(seed=10):
    """a small cloud with NaN, inf, 1e30 and a coordinate beyond 2^20 cells mixed in"""
    x, P = sized_clusters((3, 1, 4, 2), seed, min_cluster_size=1)
    T = quanta(DEFAULTS["tolerance"])
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e30, 0, 0], [0, -1e300, 0], [0, 0, float(T * IMAX) * 2.0 ** -QBITS],
                    [float(-T * IMAX - 1) * 2.0 ** -QBITS, 0, 0]])
    edge = np.array([[float(T * IMAX - 1) * 2.0 ** -QBITS, 0, 0], [float(-T * IMAX + T) * 2.0 ** -QBITS, 0, 0]])       # the last cells in range
    x = np.concatenate([x, bad, edge])
    return x[np.random.default_rng(seed).permutation(len(x))], P


def heights(h, up_axis=2, up_sign=1, seed=11, **params):
    """one point per height h (quanta) along the up axis, the points 10 T apart along the next axis: with min_cluster_size = 1 every
    point is its own cluster and all of them reach the floor stage"""
    T = quanta(DEFAULTS["tolerance"])
    h = np.asarray(h, np.int64)
    Q = np.zeros((len(h), 3), np.int64)
    Q[:, up_axis] = up_sign * h
    Q[:, (up_axis + 1) % 3] = 10 * T * (np.arange(len(h)) - len(h) // 2)
    P = dict(min_cluster_size=1, remove_floor=1, up_axis=up_axis, up_sign=up_sign)
    return from_quanta(Q[np.random.default_rng(seed).permutation(len(Q))]), dict(P, **params)


@functools.lru_cache(maxsize=None)
def fused(name):
    """the fused map of a configuration of tests/map_fuse_reference.py: xyz, color, count"""
    w = mf.case(name)["want"]
    return w["xyz"], w["color"], w["count"]
