"""Numpy restatement of fgo_map_normals (include/fgo.h), written from the stated semantics and not from the kernel: np.rint for the
quantum, DENSE integer distances between all pairs in chunks of rows (no cells, no rings: `cell` is not looked at, except to count
the occupied cells), np.lexsort by (d2, input index) for the neighbours, the integer scatter matrix, np.linalg.eigh on A, and the
orientation rule.  PCL's NormalEstimation is not in the reference tree, so this file IS the yardstick of
csrc/kernels_map_normals.hip; tests/test_map_normals_reference_cpu.py pins its neighbour sets to scipy's cKDTree and its
eigen-decomposition to mpmath at 50 digits, and measures K.

normals() returns the outputs of the call.  The case makers build the clouds of tests/test_gpu_map_normals.py from QUANTA
(integers, exact as doubles), so that a distance of exactly Rq is exactly Rq."""
import functools

import numpy as np

QBITS = 20
QMAX = 1 << 34
EPS = 2.0 ** -52
DEFAULTS = dict(k=20, max_radius=0.16, cell=0.04, viewpoint=(0.0, 0.0, 0.0))
RESULT_FIELDS = ("n_points", "n_out_of_range", "n_cells", "n_valid", "n_few", "n_degenerate")
INT_ARRAYS = ("n_neighbours", "status", "neighbour", "dist2", "scatter")
FLOAT_ARRAYS = ("normal", "curvature", "eigenvalues")
ROW_BUDGET = 1 << 22                  # pairs of a chunk of rows
FAR = np.int64(1) << 62               # the d2 of a pair that does not count

# The bound of every floating comparison of the GPU test is K eps l2 (eigenvalues, residual) or K eps l2 / (l1 - l0) (direction).
# K = 16 x the largest error of THIS restatement (np.linalg.eigh) against the 50-digit evaluation over the test clouds, in the same
# three units, and not below 16: measured over ALL points of those clouds 6.37 (eigenvalues), 2.45 (residual), 1.82 (direction), the
# worst of them on the corner cloud at k = 3; 16 x 6.37 = 101.99.  tests/test_map_normals_reference_cpu.py measures a sample again
# and asserts 16 x what it measures <= K.  Both the kernel's Jacobi and LAPACK are
# backward stable to a small multiple of eps |A|; the factor 16 covers the other algorithm's constant.  Never fitted to the kernel.
K = 102.0
GAP_MIN = 1e-6                        # points with (l1 - l0) < GAP_MIN l2 are left out of the direction comparison
SIGN_MIN = 1e-9                       # the sign is compared where |n.(v - p)| > SIGN_MIN |v - p|
MAX_LEFT_OUT = 0.05                   # of a cloud's valid points, by either exclusion


def quanta(v):
    """llrint(v 2^20) of a parameter"""
    return int(np.rint(float(v) * float(1 << QBITS)))


def quantise(xyz):
    """Q of the points (n x 3) and the mask of those in range"""
    x = np.asarray(xyz, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        y = x * float(1 << QBITS)
        ok = np.all(np.isfinite(x), 1) & np.all(np.abs(y) < 2.0 ** 35, 1)
    Q = np.zeros(x.shape, np.int64)
    Q[ok] = np.rint(y[ok]).astype(np.int64)
    ok &= np.all(np.abs(Q) < QMAX, 1)
    return Q, ok


def neighbours(Q, ok, k, Rq, sel):
    """for the points sel: neighbour (len(sel) x k, -1 padded), dist2 alike and their number: the first k of the in-range points
    within Rq in ascending (d2, index), by dense distances to ALL points"""
    n = len(Q)
    nb = np.full((len(sel), k), -1, np.int32); d2o = np.full((len(sel), k), -1, np.int64); cnt = np.zeros(len(sel), np.int32)
    rows = np.nonzero(ok[sel])[0]                                      # places in sel
    step = max(1, ROW_BUDGET // max(n, 1))
    for lo in range(0, len(rows), step):
        at = rows[lo:lo + step]
        r = sel[at]
        d = Q[None, :, :] - Q[r, None, :]                              # |d| < 2^35
        near = np.all(np.abs(d) <= Rq, 2) & ok[None, :]                # only these are squared: |d| <= 2^24
        d = np.where(near[:, :, None], d, 0)
        d2 = np.where(near, np.sum(d * d, 2), FAR)
        d2[d2 > Rq * Rq] = FAR
        kth = min(k, n) - 1
        t = np.partition(d2, kth, axis=1)[:, kth]                      # the k-th smallest d2: the first k pairs are among d2 <= t
        a, b = np.nonzero((d2 <= t[:, None]) & (d2 < FAR))
        v = d2[a, b]
        o = np.lexsort((b, v, a))                                      # by row, then d2, then index
        a, b, v = a[o], b[o], v[o]
        rank = np.arange(len(a)) - np.searchsorted(a, a)               # the place of a pair in its row
        keep = rank < k
        nb[at[a[keep]], rank[keep]] = b[keep]
        d2o[at[a[keep]], rank[keep]] = v[keep]
        cnt[at] = np.bincount(a[keep], minlength=len(at))
    return nb, d2o, cnt


def scatter(Q, sel, nb, cnt):
    """M = m S2 - S1 S1^T (len(sel) x 3 x 3, int64) of the neighbour lists of the points sel"""
    have = nb >= 0
    d = np.where(have[:, :, None], Q[np.maximum(nb, 0)] - Q[sel][:, None, :], 0)
    S1 = d.sum(1)
    S2 = np.einsum("nki,nkj->nij", d, d)
    return cnt.astype(np.int64)[:, None, None] * S2 - S1[:, :, None] * S1[:, None, :]


TRI = ([0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2])


def matrix_a(M, m):
    """A = (double)M / (m^2 2^40), each entry converted once, then divided"""
    return M.astype(np.float64) / (np.asarray(m, np.float64) ** 2 * 2.0 ** 40)[..., None, None]


def orient(nrm, Q, viewpoint):
    """the sign rule: n.(v - p) >= 0, and at exactly 0 the first non-zero component positive"""
    d = np.asarray(viewpoint, np.float64)[None, :] - Q.astype(np.float64) * 2.0 ** -QBITS
    s = (nrm[:, 0] * d[:, 0] + nrm[:, 1] * d[:, 1]) + nrm[:, 2] * d[:, 2]
    first = np.take_along_axis(nrm, np.argmax(nrm != 0, 1)[:, None], 1)[:, 0]
    flip = (s < 0) | ((s == 0) & (first < 0))
    return np.where(flip[:, None], -nrm, nrm), np.abs(s), np.sqrt(np.sum(d * d, 1))


def normals(xyz, rows=None, **params):
    """the outputs of the call; with rows (indices) the per-point arrays hold those points only, in that order -- a cloud too large
    for all pairs is checked on a sample -- and the result fields still describe the whole cloud, n_valid, n_few and n_degenerate
    excepted, which count among rows"""
    P = dict(DEFAULTS, **params)
    x = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    k = int(P["k"])
    Q, ok_all = quantise(x)
    sel = np.arange(len(x)) if rows is None else np.asarray(rows, np.int64)
    nb, d2, cnt = neighbours(Q, ok_all, k, quanta(P["max_radius"]), sel)
    M = scatter(Q, sel, nb, cnt)
    n, ok = len(sel), ok_all[sel]
    status = np.where(ok, 0, 1).astype(np.uint8)
    status[ok & (cnt < 3)] = 2
    status[ok & (cnt >= 3) & ~np.any(M.reshape(n, 9) != 0, 1)] = 3
    nrm = np.full((n, 3), np.nan); curv = np.full(n, np.nan); eig = np.full((n, 3), np.nan)
    v = np.nonzero(status == 0)[0]
    A = np.zeros((n, 3, 3))
    if len(v):
        A[v] = matrix_a(M[v], cnt[v])
        w, vec = np.linalg.eigh(A[v])
        eig[v] = w
        nrm[v] = orient(vec[:, :, 0] / np.linalg.norm(vec[:, :, 0], axis=1)[:, None], Q[sel][v], P["viewpoint"])[0]
        curv[v] = w[:, 0] / ((w[:, 0] + w[:, 1]) + w[:, 2])
    c = Q[ok_all] // quanta(P["cell"])
    return dict(n_points=len(x), n_out_of_range=int((~ok_all).sum()), n_cells=len(np.unique(c, axis=0)) if len(c) else 0, n_valid=len(v),
                n_few=int((status == 2).sum()), n_degenerate=int((status == 3).sum()), n_neighbours=cnt, status=status, neighbour=nb,
                dist2=d2, scatter=M[:, TRI[0], TRI[1]], normal=nrm, curvature=curv, eigenvalues=eig, A=A, Q=Q[sel])


def tie_at_the_end(xyz, **params):
    """the points whose list ends on a tie in d2: the (k + 1)-th pair has the d2 of the k-th.  A permutation of a cloud without any
    maps every output through exactly."""
    P = dict(DEFAULTS, **params)
    w = normals(xyz, **dict(P, k=P["k"] + 1))
    full = w["n_neighbours"] == P["k"] + 1
    return full & (w["dist2"][:, -1] == w["dist2"][:, -2])


# ---- what the float comparisons measure, in units of eps: used on the kernel's outputs and on eigh's against 50 digits alike

def eigenvalue_error(eig, want, l2):
    return np.max(np.abs(eig - want), 1) / (EPS * l2)


def residual(A, nrm, l0, l2):
    """|A n - l0 n| / (eps l2)"""
    r = np.einsum("nij,nj->ni", A, nrm) - l0[:, None] * nrm
    return np.sqrt(np.sum(r * r, 1)) / (EPS * l2)


def direction_error(nrm, want, eig):
    """sin(angle) (l1 - l0) / (eps l2), the sign left aside"""
    s = np.linalg.norm(np.cross(nrm, want), axis=1)
    return s * (eig[:, 1] - eig[:, 0]) / (EPS * eig[:, 2])


# ---- the case makers: clouds in quanta

def from_quanta(Q):
    """points whose quantisation is exactly Q (|Q| < 2^53)"""
    return np.asarray(Q, np.int64).astype(np.float64).reshape(-1, 3) * 2.0 ** -QBITS


@functools.lru_cache(maxsize=None)
def corner(n=3000, seed=21):
    """three walls of 0.6 m that meet in a corner 1.5 m in front of the viewpoint, 2 mm of noise"""
    rng = np.random.default_rng(seed)
    m = n // 3
    u = rng.uniform(0, 0.6, (n, 2)); e = rng.normal(0, 0.002, n)
    x = np.zeros((n, 3))
    x[:m] = np.stack([u[:m, 0], u[:m, 1], e[:m]], 1)
    x[m:2 * m] = np.stack([u[m:2 * m, 0], e[m:2 * m], u[m:2 * m, 1]], 1)
    x[2 * m:] = np.stack([e[2 * m:], u[2 * m:, 0], u[2 * m:, 1]], 1)
    x = x + [-0.25, -0.35, 1.5]                                        # across the origin in x and y
    x = x[rng.permutation(n)]
    x.setflags(write=False)
    return x


def lattice(nx=12, ny=11, nz=5, step=20000, seed=22):
    """an integer lattice across the origin in shuffled order: every shell of neighbours is a tie"""
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3).astype(np.int64)
    Q = (g - [nx // 2, ny // 2, nz // 2]) * step
    return from_quanta(Q[np.random.default_rng(seed).permutation(len(Q))])


R3 = 3 << 15                          # 98304 quanta = 0.09375 m: (1, 2, 2) x 32768 has length exactly R3
RAD3 = R3 * 2.0 ** -QBITS
STEP3 = np.array([32768, 65536, 65536], np.int64)


def closed_radius(extra, k=4):
    """k - 1 points within a few quanta of the origin and one at exactly R3 (extra = 0) or one quantum further: the k-th neighbour
    of point 0"""
    near = [[0, 0, 0]] + [[3 * i + 1, 2 * i, -i] for i in range(1, k - 1)]
    return from_quanta(near + [list(STEP3 + [0, 0, extra])]), dict(k=k, max_radius=RAD3, cell=RAD3 / 2)


def direction_cloud(o, at_origin, cell=0.04):
    """5 points within a few quanta: three just inside the cell of the origin at its border towards o, two just across it; the
    whole 37 cells down every axis (negative cells only) unless at_origin.  With k = 5 every list crosses the border."""
    T = quanta(cell)
    o = np.array(o, np.int64)
    free = (o == 0).astype(np.int64)                                   # the axes along which the border is not crossed
    a = np.where(o > 0, T - 1, np.where(o < 0, 0, T // 2)); b = np.where(o > 0, T, np.where(o < 0, -1, T // 2))
    Q = np.array([a, a - 2 * o + free * [3, -3, 3], a - 4 * o + free * [-5, 5, 1], b, b + 3 * o + free * [2, 2, -2]], np.int64)
    if not at_origin:
        Q = Q - 37 * T
    return from_quanta(Q), dict(k=5, max_radius=2 * cell, cell=cell)


def blob_and_loner(n=400, seed=23):
    """a blob inside 0.02 m and one point 0.5 m away, max_radius / cell = 16: the loner's search runs every ring there is"""
    rng = np.random.default_rng(seed)
    Q = np.concatenate([rng.integers(-10000, 10000, (n, 3)), [[quanta(0.5), 77, -5]]])
    return from_quanta(Q), dict(k=20, max_radius=0.25, cell=2.0 ** -6)


def one_cell_descending(n=5000, seed=24):
    """a probe and n points in ONE cell, listed in descending distance from the probe: every candidate displaces one"""
    rng = np.random.default_rng(seed)
    T = quanta(0.04)
    Q = rng.integers(0, T, (n, 3))
    probe = np.array([T // 2, T // 2, T // 2])
    d2 = np.sum((Q - probe) ** 2, 1)
    return from_quanta(np.concatenate([[probe], Q[np.argsort(-d2, kind="stable")]])), dict(k=20)


def line(n=40, step=3000):
    """points on a straight line: l0 = l1 = 0, any normal across the line will do"""
    return from_quanta(np.arange(n, dtype=np.int64)[:, None] * np.array([[step, 2 * step, -step]]) + [5, -7, 1 << 20])


def out_of_range(seed=25):
    """the corner cloud's first 300 points with NaN, inf, |Q| = 2^34 and beyond mixed in; 2^34 - 1 is the last quantum in range"""
    e = float(QMAX) * 2.0 ** -QBITS
    bad = np.array([[np.nan, 0, 1], [0, np.inf, 1], [0, 0, -np.inf], [e, 0, 1], [0, -e, 1], [1e30, 0, 1], [0, 0, -1e300]])
    edge = from_quanta([[QMAX - 1, 0, 0], [0, -(QMAX - 1), 0], [QMAX - 1, QMAX - 1, -(QMAX - 1)]])
    x = np.concatenate([corner()[:300], bad, edge])
    return x[np.random.default_rng(seed).permutation(len(x))], len(bad)


def plane(n=500, z=1 << 20, seed=26):
    """an exact plane z = 1 m built from quanta"""
    rng = np.random.default_rng(seed)
    Q = np.concatenate([rng.integers(-200000, 200000, (n, 2)), np.full((n, 1), z)], 1)
    return from_quanta(np.unique(Q, axis=0))
