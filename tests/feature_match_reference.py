"""Numpy restatement of fgo_match_features_batch (include/fgo.h), written from the semantics stated there: the yardstick of
tests/test_gpu_feature_match.py, itself pinned by tests/test_feature_match_reference_cpu.py.  The VRO library's matching is not in
the reference tree; the definition is this project's.

Per pair: queries are the features of frame j (local index a), trains those of frame i (local index b).
  usable      three finite coordinates and z > 0
  distance    d(a, b) = sum_k (desc_a[k] - desc_b[k])^2, from the differences themselves, in integers
  candidates  usable (a, b); guided: also gate(a, b), with p = R^T (xyz_b - t): p.z > 0, the pixel distance of the projection of p
              from uv_a <= radius_px, and with max_dist_3d > 0 also |p - xyz_a| <= max_dist_3d
  verdict     best / second over the candidates (ties to the lowest b; a tied minimum gives d2 = d1), the ratio test
              (double) d1 < r2 * (double) d2 with r2 = ratio * ratio, the cap, the cross-check (ties to the lowest a)
The gate is floating point: `tables` returns the relative margin of every threshold test that decides a candidate, and the generated
cases keep every one of them above DECIDE, so that the rounding of the device (fused multiply-adds, the order of a sum) cannot
move a candidate in or out."""
import numpy as np

DIM = 128
MAX_FEATURES = 4096
INT32_MAX = 2 ** 31 - 1
DECIDE = 1e-6
DEFAULTS = dict(ratio=0.5, ratio_test=1, cross_check=1, max_desc_dist2=INT32_MAX, min_matches=12, radius_px=10.0, max_dist_3d=0.0,
                fx=250.5773, fy=250.5773, cx=90.0, cy=70.0)
FM_OK, FM_TOO_FEW = 0, 1


def usable(xyz):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return np.isfinite(xyz).all(1) & (xyz[:, 2] > 0)


def distances(desc_j, desc_i):
    """N_j x N_i int64: the squared differences summed, a block of rows at a time"""
    dj = np.asarray(desc_j, np.uint8).reshape(-1, DIM).astype(np.int32); di = np.asarray(desc_i, np.uint8).reshape(-1, DIM).astype(np.int32)
    out = np.zeros((len(dj), len(di)), np.int64)
    for a in range(0, len(dj), 32):
        e = dj[a:a + 32, None, :] - di[None, :, :]
        out[a:a + 32] = (e * e).sum(2)
    return out


def quat_matrix(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def gate(xyz_j, uv_j, xyz_i, pose7, P):
    """(in, undecided), both N_j x N_i, over ALL (a, b) (usability is applied by the caller): the gate of (a, b), and whether one
    of the threshold tests that decide it has a relative margin below DECIDE"""
    xj = np.asarray(xyz_j, np.float64).reshape(-1, 3); uj = np.asarray(uv_j, np.float64).reshape(-1, 2)
    xi = np.asarray(xyz_i, np.float64).reshape(-1, 3)
    R, t = quat_matrix(pose7[3:]), np.asarray(pose7[:3], np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        e = xi - t
        p = e @ R                                                # rows: R^T (xyz_b - t)
        scale = np.maximum(np.abs(e).sum(1), 1e-300)
        z_ok = p[:, 2] > 0
        m_z = np.abs(p[:, 2]) / scale
        pu = P["fx"] * p[:, 0] / p[:, 2] + P["cx"]; pv = P["fy"] * p[:, 1] / p[:, 2] + P["cy"]
        r2 = (pu[None, :] - uj[:, 0:1]) ** 2 + (pv[None, :] - uj[:, 1:2]) ** 2
        rad2 = P["radius_px"] ** 2
        px_ok = r2 <= rad2
        m_px = np.abs(r2 - rad2) / rad2
        inside = z_ok[None, :] & px_ok
        und = (m_z < DECIDE)[None, :] | (z_ok[None, :] & (m_px < DECIDE))
        if P["max_dist_3d"] > 0:
            s2 = ((p[None, :, :] - xj[:, None, :]) ** 2).sum(2)
            m2 = P["max_dist_3d"] ** 2
            und |= inside & (np.abs(s2 - m2) / m2 < DECIDE)
            inside = inside & (s2 <= m2)
    return inside, und


def tables(fj, fi, pose7=None, **params):
    """the tables of a pair that do not depend on the verdict's parameters: dist (N_j x N_i int64, -1 where (a, b) is no candidate),
    the usable masks, and the number of undecided gates among the usable (a, b)"""
    P = dict(DEFAULTS, **params)
    d = distances(fj["desc"], fi["desc"])
    uq, ut = usable(fj["xyz"]), usable(fi["xyz"])
    cand = uq[:, None] & ut[None, :]
    undecided = 0
    if pose7 is not None:
        inside, und = gate(fj["xyz"], fj["uv"], fi["xyz"], pose7, P)
        undecided = int((und & cand).sum())
        cand = cand & inside
    return dict(dist=np.where(cand, d, -1), uq=uq, ut=ut, undecided=undecided)


def verdict(T, **params):
    """best, d1, d2, reason per query; the matches (a, b) in ascending a; the counts and the status"""
    P = dict(DEFAULTS, **params)
    D = T["dist"]
    nj, ni = D.shape
    big = np.int64(1) << 40
    E = np.where(D >= 0, D, big)
    best = np.full(nj, -1, np.int64); d1 = np.full(nj, -1, np.int64); d2 = np.full(nj, -1, np.int64)
    reason = np.zeros(nj, np.uint8)
    r2 = P["ratio"] * P["ratio"]
    if ni and nj:
        col_best = np.where((D >= 0).any(0), E.argmin(0), -1)    # argmin: the first of a tie, the lowest a
    for a in range(nj):
        if not T["uq"][a]:
            reason[a] = 1
            continue
        n_cand = int((D[a] >= 0).sum()) if ni else 0
        if n_cand == 0:
            reason[a] = 2
            continue
        b = int(E[a].argmin())                                   # the lowest b of a tie
        best[a] = b; d1[a] = D[a, b]
        if n_cand > 1:
            rest = E[a].copy(); rest[b] = big
            d2[a] = rest.min()
        if P["ratio_test"] and d2[a] >= 0 and not (float(d1[a]) < r2 * float(d2[a])):
            reason[a] = 3
        elif d1[a] > P["max_desc_dist2"]:
            reason[a] = 4
        elif P["cross_check"] and col_best[b] != a:
            reason[a] = 5
    kept = np.nonzero((reason == 0) & (best >= 0) & T["uq"])[0]
    n = len(kept)
    return dict(best=best.astype(np.int32), d1=d1.astype(np.int32), d2=d2.astype(np.int32), reason=reason, a=kept, b=best[kept],
                n_query=int(T["uq"].sum()), n_train=int(T["ut"].sum()), n_matches=n, n_ratio=int((reason == 3).sum()),
                n_cross=int((reason == 5).sum()), status=FM_TOO_FEW if n < P["min_matches"] else FM_OK)


def match_pair(fj, fi, pose7=None, **params):
    T = tables(fj, fi, pose7, **params)
    return dict(verdict(T, **params), dist=T["dist"], undecided=T["undecided"])


# ---- generated cases ------------------------------------------------------------------------------------------------------------

def so3_exp(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def quat_xyzw(R):
    w = 0.5 * np.sqrt(max(1 + np.trace(R), 1e-300))              # the cases rotate by far less than pi
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def relative_pose(Ti, Tj):
    """pose_ij7 with p_i = R p_j + t, from the poses (R, t) of the two cameras in the world: p_w = R_f p_f + t_f"""
    R = Ti[0].T @ Tj[0]
    t = Ti[0].T @ (Tj[1] - Ti[1])
    return np.concatenate([t, quat_xyzw(R)])


def project(xyz, P=DEFAULTS):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.stack([P["fx"] * xyz[:, 0] / xyz[:, 2] + P["cx"], P["fy"] * xyz[:, 1] / xyz[:, 2] + P["cy"]], 1)


def make_world(rng, n_base, n_twins, twin_noise=10):
    """n_base points with random descriptors; the last n_twins points look like the first n_twins (repeated texture) elsewhere"""
    desc = rng.integers(0, 256, (n_base, DIM)).astype(np.int64)
    tw = np.clip(desc[:n_twins] + rng.integers(-twin_noise, twin_noise + 1, (n_twins, DIM)), 0, 255)
    pts = np.stack([rng.uniform(-1.5, 1.5, n_base + n_twins), rng.uniform(-1.0, 1.0, n_base + n_twins), rng.uniform(2.0, 5.0, n_base + n_twins)], 1)
    return np.concatenate([desc, tw]), pts


def make_frame(rng, world, T, ids, desc_noise=8, point_noise=0.002, no_depth=0.0):
    desc, pts = world
    ids = np.asarray(ids, np.int64)
    d = np.clip(desc[ids] + rng.integers(-desc_noise, desc_noise + 1, (len(ids), DIM)), 0, 255).astype(np.uint8)
    xyz = (pts[ids] - T[1]) @ T[0] + point_noise * rng.normal(size=(len(ids), 3))
    uv = project(xyz)
    lost = rng.uniform(size=len(ids)) < no_depth
    xyz[lost] = np.where(rng.uniform(size=(int(lost.sum()), 1)) < 0.5, 0.0, np.nan)
    return dict(desc=d, xyz=xyz, uv=uv, ids=ids, T=T)


SIZES = (0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 600)   # either side of a tile, a wave's strips (64), the
                                                                               # 128-train chunk and the 256-query block
CONFIGS = (dict(ratio_test=1, cross_check=1), dict(ratio_test=1, cross_check=0), dict(ratio_test=0, cross_check=1),
           dict(ratio_test=0, cross_check=0),
           dict(ratio=0.8, max_desc_dist2=9000, max_dist_3d=0.05, radius_px=15.0))
_cache = {}


def gpu_cases(seed=20262):
    """(frames, pairs): frames of every size in SIZES over one world of 600 points + 100 look-alikes, 10 % of the features of a
    frame without depth, and two frames of extremes; pairs (frame_j, frame_i, pose7 or None) -- see tests/test_gpu_feature_match.py"""
    if seed in _cache:
        return _cache[seed]
    rng = np.random.default_rng(seed)
    world = make_world(rng, 600, 100)
    frames = []
    for n in SIZES:
        T = (so3_exp(rng.uniform(-0.05, 0.05, 3)), rng.uniform(-0.1, 0.1, 3))
        f = make_frame(rng, world, T, rng.permutation(700)[:n], no_depth=0.1 if n >= 15 else 0.0)
        if n >= 63:                                              # a duplicated descriptor: a tie among the trains, a conflict among the queries
            f["desc"][9] = f["desc"][5]
            f["xyz"][[5, 9]] = (world[1][f["ids"][[5, 9]]] - T[1]) @ T[0]       # both keep their depth
        frames.append(f)
    # the global nearest neighbour outside the gate: three trains of frame 14 take the exact descriptor of a query of frame 15 whose
    # own point projects elsewhere
    f15, f14 = frames[15], frames[14]
    uq, ut = usable(f15["xyz"]), usable(f14["xyz"])
    planted = []
    for a in np.nonzero(uq & np.isin(f15["ids"], f14["ids"]))[0][20:23]:
        far = np.nonzero(ut & (np.abs(f14["uv"] - f15["uv"][a]).max(1) > 60) & (f14["ids"] != f15["ids"][a]))[0]
        b = int(far[len(planted)])
        f14["desc"][b] = f15["desc"][a]
        planted.append((int(a), b))
    # extremes: all 0 against all 255 gives the largest distance there is, 128 * 255^2
    I = (np.eye(3), np.zeros(3))
    fa = make_frame(rng, world, I, rng.permutation(600)[:20]); fb = make_frame(rng, world, I, rng.permutation(600)[:18])
    fa["desc"][0] = 0; fa["desc"][1] = 255; fb["desc"][0] = 255; fb["desc"][1] = 0; fb["desc"][2] = 0
    frames += [fa, fb]
    rel = lambda j, i: relative_pose(frames[i]["T"], frames[j]["T"])
    far_pose = lambda j, i: np.concatenate([rel(j, i)[:3] + [40.0, 0, 0], rel(j, i)[3:]])       # every projection leaves the gate
    behind = lambda j, i: np.array([0, 0, 0, 0, 1.0, 0, 0])                                     # half a turn about y: p.z < 0
    pairs = [(15, 14, None), (14, 15, None), (13, 12, None), (12, 13, None), (11, 10, None), (10, 11, None), (9, 8, None), (8, 9, None),
             (7, 15, None), (6, 5, None), (5, 6, None), (4, 3, None), (3, 4, None), (2, 15, None), (15, 2, None), (1, 2, None), (2, 1, None),
             (0, 5, None), (5, 0, None), (0, 0, None), (1, 1, None), (9, 9, None), (16, 17, None), (17, 16, None), (15, 11, None),
             (15, 14, rel(15, 14)), (14, 15, rel(14, 15)), (12, 13, rel(12, 13)), (10, 11, rel(10, 11) * [1, 1, 1, 3, 3, 3, 3]),
             (6, 5, rel(6, 5)), (2, 15, rel(2, 15)), (9, 9, np.array([0, 0, 0, 0, 0, 0, 1.0])), (3, 16, rel(3, 16)),
             (13, 12, far_pose(13, 12)), (11, 10, behind(11, 10)),
             (15, 14, None), (15, 14, rel(15, 14)), (9, 8, None)]                # the same pairs at other places of the batch
    _cache[seed] = (frames, pairs, planted)
    return _cache[seed]


def pack(frames):
    """feat_ptr, desc, xyz, uv of the call"""
    ptr = np.concatenate([[0], np.cumsum([len(f["desc"]) for f in frames])]).astype(np.int64)
    cat = lambda k, w, t: np.concatenate([np.asarray(f[k], t).reshape(-1, w) for f in frames])
    return ptr, cat("desc", DIM, np.uint8), cat("xyz", 3, np.float64), cat("uv", 2, np.float64)


def e2e_cases(seed=20263, n_pairs=4, n=300, share=0.3):
    """Frames under planted poses: frame 2 p + 1 sees the points of frame 2 p moved by a planted pose, 2 mm of noise on every point,
    descriptor noise +-8, half of the points with a look-alike elsewhere in the frame (repeated texture: the ratio test of the
    unguided match rejects them, the gate tells them apart), and `share` of the features of the second frame with their
    descriptors swapped among themselves: wrong matches for the registration to reject."""
    rng = np.random.default_rng(seed)
    frames, planted = [], []
    for _ in range(n_pairs):
        world = make_world(rng, n // 2 + n // 4, n // 4)
        ids = np.arange(n)
        Ti = (np.eye(3), np.zeros(3))
        axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
        Tj = (so3_exp(0.1 * axis), rng.uniform(-0.1, 0.1, 3))
        fi = make_frame(rng, world, Ti, ids); fj = make_frame(rng, world, Tj, rng.permutation(n))
        sw = rng.permutation(n)[:int(share * n)]
        fj["desc"][sw] = fj["desc"][np.roll(sw, 1)]
        frames += [fi, fj]
        planted.append(Tj)                                       # p_i = R_j p_j + t_j
    return frames, planted
