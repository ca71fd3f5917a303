"""Numpy restatement of fgo_plane_propagate_batch (include/fgo.h): part 1 of the reference's CGraphGT::predictPlaneNode with
computeSdj, inThisPlane, intensityTol and regionGrow (gtsam/gtsam_graph.cpp:725-1041), written from the stated semantics and not from
the kernel.  The refit is plane_extract_reference's fit and covariance (numpy.linalg.eigh, numpy.linalg.inv).

The growth has two forms.  growth="queue" is the literal queue of :779-859, pixel by pixel, with its `visited` image;
growth="closure" computes the fixed point the header defines: the pixels that conduct (claimed, or free and in the plane) are the
nodes of a graph whose edges join 4-neighbours within the intensity tolerance, and E is the union of the connected components
(scipy.sparse.csgraph) that hold a seed.  tests/test_plane_propagate_reference_cpu.py holds the two to each other.

Besides the outputs of the call, propagate_pair returns what the GPU test's tolerances and its well-posedness test need: `margin`,
the smallest distance of any decision from its threshold -- | |e| - sqrt(max(S_dj, d_floor^2)) | of every in-plane test made (seed
candidates, and every free pixel when a kept plane grows), |z - z_min| and |z - z_max| of every candidate, the z of a carried-over
point from 0, and of a projected coordinate the distance to the nearest half-integer: the three truncations (int)(u - 0.5), (int)(u),
(int)(u + 0.5) are taken as a SET, and u crossing an integer only moves a value between the du = 0 candidate and a neighbour, which
leaves the set as it is, while u +- 0.5 crossing an integer (0 included: the set {0} becomes {0, 1}) changes it -- `keep_margin`,
the smallest |n_seed - (int)(keep_ratio n_prev)| + (0 if kept else 1) in pixels (how many seeds from the other outcome),
`d_min` (the smallest |d| of a refit), and per output plane g, cond_A and p_max as plane_extract_reference defines them.

gpu_cases() builds the calls of tests/test_gpu_plane_propagate.py: rendered rooms (plane_extract_reference.room_planes / render) from
several camera poses and synthetic fronto-parallel scenes, each with an intensity image of one level per wall and a texture of at
most +-2.  The labels and planes of a previous frame are the render's wall index and plane_extract_reference's fit of those pixels:
they stand in for the extraction, which has its own tests."""
import collections

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

from tests import plane_check_reference as pcr
from tests import plane_extract_reference as ref

PP_OK, PP_NUM = 0, 2
MAX_PLANES = 8
DECIDE = 1e-9
FREE, REJECTED = 0, 255                                           # flag image: 1 + l = claimed by plane l

DEFAULTS = dict(fx=250.5773, fy=250.5773, cx=90.0, cy=70.0, z_scale=0.001, z_min=0.1, z_max=5.0, sigma_px=1.0, sigma_z=(0.014, 0.0, 0.0),
                d_floor=0.014, intensity_tol=5, keep_ratio=0.7, rest_ratio=0.5)


def points(depth, P):
    """every pixel back-projected, no depth-range test: a pixel without a return lies at the origin"""
    return ref.backproject(depth, P)[0]


def predict(abcd, cov16, pose, S_t):
    """computeSdj: (n_j, d_j) and S_dj"""
    p = pcr.normalize(abcd)
    return pcr.transform(p, pose), float(pcr.sdj(p, cov16, pose, S_t))


def half_margin(x):
    """distance of x to the nearest half-integer"""
    return np.abs(x - np.floor(x) - 0.5)


def grow_queue(flag, seeds, inten, eligible, tol, W, H):
    """regionGrow (:779-859): the pixels that join, in the order the queue meets them.  flag is not changed."""
    visited = np.zeros(W * H, np.uint8)
    joined_mark = np.zeros(W * H, bool)
    q = collections.deque(int(s) for s in seeds)
    fl = flag.tolist(); it = inten.astype(np.int64).tolist(); el = eligible.tolist()
    joined = []
    while q:
        c = q.popleft()
        if visited[c] == 2:
            continue
        visited[c] = 2
        if fl[c] == REJECTED:
            continue
        if fl[c] == FREE and not joined_mark[c]:
            if el[c]:
                joined_mark[c] = True; joined.append(c)
            else:
                continue
        v, u = divmod(c, W)
        for ok, nb in ((u >= 1, c - 1), (u + 1 < W, c + 1), (v >= 1, c - W), (v + 1 < H, c + W)):
            if ok and visited[nb] == 0 and abs(it[nb] - it[c]) <= tol:
                q.append(nb); visited[nb] = 1
    return np.array(sorted(joined), np.int64)


def grow_closure(flag, seeds, inten, eligible, tol, W, H):
    """the fixed point: the free eligible pixels of the connected components, over the conducting pixels, that hold a seed"""
    claimed = (flag != FREE) & (flag != REJECTED)
    node = claimed | ((flag == FREE) & eligible)
    idx = np.arange(W * H).reshape(H, W); nd = node.reshape(H, W); it = inten.reshape(H, W).astype(np.int64)
    rows, cols = [], []
    for a, b in ((np.s_[:, :-1], np.s_[:, 1:]), (np.s_[:-1, :], np.s_[1:, :])):
        e = nd[a] & nd[b] & (np.abs(it[a] - it[b]) <= tol)
        rows.append(idx[a][e]); cols.append(idx[b][e])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    g = sp.coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(W * H, W * H))
    _, comp = connected_components(g, directed=False)
    inE = np.isin(comp, np.unique(comp[seeds])) & node
    return np.nonzero(inE & (flag == FREE))[0]


def propagate_pair(depth_i, label_i, abcd_i, cov16_i, depth_j, inten_j, pose, S, growth="closure", **params):
    """one pair.  abcd_i (npl x 4), cov16_i (npl x 16); S = the 6x6 covariance of the pose in [omega; v], or None for a pair whose
    information is not positive definite."""
    P = dict(DEFAULTS, **params)
    H, W = depth_j.shape
    NP = W * H
    MP = MAX_PLANES
    abcd_i = np.asarray(abcd_i, np.float64).reshape(-1, 4); cov16_i = np.asarray(cov16_i, np.float64).reshape(-1, 16)
    npl = len(abcd_i)
    out = dict(status=PP_OK, n_planes=0, num_added=0, search_rest=2, abcd=np.zeros((MP, 4)), cov16=np.zeros((MP, 4, 4)), cov_ut6=np.zeros((MP, 6)),
               n_pixels=np.zeros(MP, int), n_seed=np.zeros(MP, int), source=np.zeros(MP, int), rmse=np.zeros(MP), centroid=np.zeros((MP, 3)),
               pred_abcd=np.zeros((MP, 4)), sdj=np.zeros(MP), n_prev=np.zeros(MP, int), pred_n_seed=np.zeros(MP, int), kept=np.zeros(MP, int),
               g=np.ones(MP), cond_A=np.ones(MP), p_max=0.0, margin=np.inf, keep_margin=np.inf, d_min=np.inf, joined=np.zeros(MP, int),
               n_by_sdj=0)
    zj = depth_j.reshape(-1).astype(np.float64) * P["z_scale"]
    in_range = (zj > P["z_min"]) & (zj < P["z_max"])
    plain = np.where(in_range, -1, -2).astype(np.int8).reshape(H, W)

    def failed():
        for k, v in out.items():
            if isinstance(v, np.ndarray):
                v[...] = 1 if k in ("g", "cond_A") else 0
        out.update(status=PP_NUM, n_planes=0, num_added=0, search_rest=2, labels=plain)
        return out

    if S is None:
        return failed()
    S_t = pcr.sym_upper(S)[3:, 3:]
    pred = [predict(abcd_i[l], cov16_i[l], pose, S_t) for l in range(npl)]
    if any(not (np.isfinite(s) and s >= 0) for _, s in pred):
        return failed()
    R, t = pcr.qmat(pose[3:]), np.asarray(pose[:3], np.float64)
    pts_i, pts_j = points(depth_i, P), points(depth_j, P)
    out["p_max"] = float(np.linalg.norm(pts_j[in_range], axis=1).max()) if in_range.any() else 0.0
    inten = inten_j.reshape(-1)
    flag = np.zeros(NP, np.uint8)
    lab_i = label_i.reshape(-1)
    dfl2 = P["d_floor"] * P["d_floor"]
    slot = {}
    kept = 0

    def note(m):
        if np.size(m):
            out["margin"] = min(out["margin"], float(np.min(m)))

    for l in range(npl):
        (pe, sdj) = pred[l]
        nj, dj = pe[:3], pe[3]
        out["pred_abcd"][l] = pe; out["sdj"][l] = sdj
        thr = np.sqrt(max(sdj, dfl2))
        e_all = np.abs(pts_j @ nj + dj)
        in_plane = (e_all * e_all <= sdj) | (e_all * e_all <= dfl2)
        # seeds
        src = np.nonzero(lab_i == l)[0]
        n_prev = len(src)
        q = (pts_i[src] - t) @ R                                  # R^T (p - t)
        note(np.abs(q[:, 2]))
        front = q[:, 2] > 0
        q = q[front]
        uf = P["fx"] * q[:, 0] / q[:, 2] + P["cx"]; vf = P["fy"] * q[:, 1] / q[:, 2] + P["cy"]
        ok = (np.abs(uf) < 2.0 ** 30) & (np.abs(vf) < 2.0 ** 30)
        uf, vf = uf[ok], vf[ok]
        # a coordinate far outside the image decides nothing by its fraction
        near_u = (uf > -2) & (uf < W + 1); near_v = (vf > -2) & (vf < H + 1)
        note(half_margin(uf[near_u & near_v])); note(half_margin(vf[near_u & near_v]))
        cand = []
        for du in (-0.5, 0.0, 0.5):
            uj = np.trunc(uf + du).astype(np.int64)
            for dv in (-0.5, 0.0, 0.5):
                vj = np.trunc(vf + dv).astype(np.int64)
                m = (uj >= 0) & (uj < W) & (vj >= 0) & (vj < H)
                cand.append(vj[m] * W + uj[m])
        cand = np.unique(np.concatenate(cand)) if cand else np.zeros(0, np.int64)
        cand = cand[flag[cand] == FREE]
        note(np.abs(zj[cand] - P["z_min"])); note(np.abs(zj[cand] - P["z_max"]))
        tested = cand[in_range[cand]]
        note(np.abs(e_all[tested] - thr))
        claim = tested[in_plane[tested]]
        out["n_by_sdj"] += int(np.sum(e_all[claim] ** 2 > dfl2))
        flag[cand] = REJECTED
        flag[claim] = 1 + l
        n_seed = len(claim)
        thresh = int(P["keep_ratio"] * float(n_prev))
        keep = n_seed > thresh
        out["keep_margin"] = min(out["keep_margin"], abs(n_seed - thresh) + (0 if keep else 1))
        out["n_prev"][l] = n_prev; out["pred_n_seed"][l] = n_seed; out["kept"][l] = int(keep)
        if not keep:
            slot[l] = -4
            out["num_added"] += n_seed
            continue
        free = np.nonzero(flag == FREE)[0]
        note(np.abs(e_all[free] - thr))
        grow = grow_queue if growth == "queue" else grow_closure
        joined = grow(flag, claim, inten, in_plane, P["intensity_tol"], W, H) if n_seed else np.zeros(0, np.int64)
        out["n_by_sdj"] += int(np.sum(e_all[joined] ** 2 > dfl2))
        flag[joined] = 1 + l
        members = np.nonzero(flag == 1 + l)[0]
        n_pixels = n_seed + len(joined)
        assert n_pixels == len(members)
        out["num_added"] += n_pixels
        p = pts_j[members]
        with np.errstate(all="ignore"):
            n, d, c, w = ref.fit(p)
            cov = ref.covariance(n, p, P)
        vals = np.concatenate([n, [d], c])
        if cov is None or not (np.all(np.isfinite(vals)) and np.all(np.isfinite(cov[0]))):
            return failed()
        k = kept
        out["abcd"][k] = np.append(n, d); out["cov_ut6"][k] = ref.ut6(cov[0]); out["cov16"][k] = cov[1]; out["cond_A"][k] = cov[2]
        out["g"][k] = ref.gap(w); out["d_min"] = min(out["d_min"], abs(d))
        out["n_pixels"][k] = n_pixels; out["n_seed"][k] = n_seed; out["source"][k] = l; out["joined"][k] = len(joined)
        out["rmse"][k] = float(np.sqrt(np.mean((p @ n + d) ** 2))); out["centroid"][k] = c
        slot[l] = k
        kept += 1
    out["n_planes"] = kept
    na = out["num_added"]
    out["search_rest"] = 0 if na > int(P["rest_ratio"] * float(NP)) else 2 if na == 0 else 1
    lab = np.where(flag == REJECTED, -3, plain.reshape(-1)).astype(np.int8)
    for l, k in slot.items():
        lab[flag == 1 + l] = k
    out["labels"] = lab.reshape(H, W)
    return out


# ---- scenes

LO, HI = np.array([-40.0, -40.0, -40.0]), np.array([1.6, 1.1, 2.2])


def intensity_of(wall, rng, texture=2):
    """one level per wall (40 apart), a texture of at most +-texture"""
    base = 60 + 40 * np.where(wall >= 0, wall, 0)
    return np.clip(base + rng.integers(-texture, texture + 1, wall.shape), 0, 255).astype(np.uint8)


def stand_in(depth, wall, P):
    """the labels and planes that stand in for the extraction: the wall index of every pixel with a depth in range, renumbered from 0 in
    order of appearance, and plane_extract_reference's fit and covariance of those pixels"""
    pts, valid = ref.backproject(depth, P)
    lab = np.full(depth.size, -1, np.int8); lab[~valid] = -2
    abcd, cov16 = [], []
    for w in np.unique(wall[wall >= 0]):
        m = (wall.reshape(-1) == w) & valid
        if m.sum() < 3:
            continue
        n, d, _, _ = ref.fit(pts[m])
        cov = ref.covariance(n, pts[m], P)
        if cov is None:
            continue
        lab[m] = len(abcd)
        abcd.append(np.append(n, d)); cov16.append(cov[1].reshape(16))
    return lab.reshape(depth.shape), np.array(abcd).reshape(-1, 4), np.array(cov16).reshape(-1, 16)


def rel_pose(Ri, ti, Rj, tj):
    """the pose of frame j in frame i: p_i = R p_j + t"""
    return np.concatenate([Ri.T @ (tj - ti), ref.vro_quat(Ri.T @ Rj)])


IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])
SMALL_COV = np.diag([1e-6] * 3 + [1e-6] * 3)


def fronto(W, H, z, rng, noise_words=1):
    """a scene of fronto-parallel patches: depth z metres, per column (W) or per pixel (H x W); +-noise_words of noise"""
    z = np.broadcast_to(np.asarray(z, np.float64), (H, W))
    return (np.rint(z / 0.001) + rng.integers(-noise_words, noise_words + 1, (H, W))).astype(np.uint16)


def make_call(W, H, seed):
    """the frames and pairs of one call of the GPU test at W x H: dict of cam, depth, intensity, labels, n_planes, abcd (n x 8 x 4), cov16
    (n x 8 x 16), and pairs: a list of dicts (name, i, j, pose, S (None = an information that is not positive definite))"""
    rng = np.random.default_rng(seed)
    cam = ref.camera(W, H)
    P = dict(DEFAULTS, **cam)
    frames, pairs = [], []

    def add(depth, inten, lab, abcd, cov16):
        frames.append(dict(depth=depth, inten=inten, lab=lab, abcd=abcd, cov16=cov16))
        return len(frames) - 1

    def room(R, t):
        depth, wall = ref.render(ref.room_planes(LO, HI, R, t), W, H, cam, 0.002, rng)
        return add(depth, intensity_of(wall, rng), *stand_in(depth, wall, P))

    # the three-wall corner from three poses
    Ra, ta = ref.rot_y(np.deg2rad(40.0)) @ ref.rot_x(np.deg2rad(-25.0)), np.zeros(3)
    Rb, tb = ref.rot_y(np.deg2rad(43.0)) @ ref.rot_x(np.deg2rad(-23.5)), np.array([0.04, -0.02, 0.06])
    Rc, tc = ref.rot_y(np.deg2rad(48.0)) @ ref.rot_x(np.deg2rad(-25.0)), np.array([0.05, 0.0, 0.05])
    fa, fb, fc = room(Ra, ta), room(Rb, tb), room(Rc, tc)
    pairs.append(dict(name="identity", i=fa, j=fa, pose=IDENT, S=SMALL_COV))
    pairs.append(dict(name="small-motion", i=fa, j=fb, pose=rel_pose(Ra, ta, Rb, tb), S=SMALL_COV))
    pairs.append(dict(name="wall-dropped", i=fa, j=fc, pose=rel_pose(Ra, ta, Rc, tc), S=SMALL_COV))
    # a pose off by 3 cm with a covariance that says so: the S_dj branch admits what d_floor does not
    off = rel_pose(Ra, ta, Rb, tb + Ra @ np.array([0.0, 0.0, 0.03]))
    pairs.append(dict(name="large-covariance", i=fa, j=fb, pose=off, S=np.diag([1e-6] * 3 + [0.05 ** 2] * 3)))
    pairs.append(dict(name="not-positive-definite", i=fa, j=fb, pose=rel_pose(Ra, ta, Rb, tb), S=None))
    # a previous frame without planes
    f0 = add(frames[fa]["depth"], frames[fa]["inten"], frames[fa]["lab"], np.zeros((0, 4)), np.zeros((0, 16)))
    pairs.append(dict(name="no-planes", i=f0, j=fb, pose=rel_pose(Ra, ta, Rb, tb), S=SMALL_COV))

    # one fronto-parallel wall at 2 m, the previous support in the top left corner only
    def wall_frame(inten):
        depth = fronto(W, H, np.full(W, 2.0), rng)
        wall = np.full((H, W), -1); wall[:1, :max(3, W // 4)] = 0                          # row 0 only: a seed is not asked for its intensity
        lab, abcd, cov16 = stand_in(depth, np.zeros((H, W), int), P)
        lab = np.where(wall == 0, 0, -1).astype(np.int8)
        return add(depth, inten, lab, abcd, cov16)

    # ... with a rectangle whose intensity jumps
    inten = intensity_of(np.zeros((H, W), int), rng)
    inten[H // 3:max(H // 3 + 1, 2 * H // 3), W // 3:2 * W // 3] += 60
    fr = wall_frame(inten)
    pairs.append(dict(name="rectangle", i=fr, j=fr, pose=IDENT, S=SMALL_COV))
    # ... with a serpentine: every odd row is a barrier, open at alternating ends
    inten = intensity_of(np.zeros((H, W), int), rng)
    for k, v in enumerate(range(1, H, 2)):
        inten[v, :] += 100
        gap = W - 1 if k % 2 == 0 else 0
        inten[v, gap] -= 100
    fs = wall_frame(inten)
    pairs.append(dict(name="serpentine", i=fs, j=fs, pose=IDENT, S=SMALL_COV))

    # two planes: A at 2.5 m fills the top left corner (plane 0), B at 2 m the rest (plane 1): B1 to the right of A, B2 below; a barrier
    # row of another intensity under B1 cuts the way round A's corner.  A seed claims or rejects the pixels to its LEFT and ABOVE
    # (the candidates of du, dv = -0.5), so A lies at the image border and is entered from the right and left at the bottom.  Plane 0's
    # previous support wrongly takes a few pixels of B2 under A: they become REJECTED and are lost to plane 1.  Plane 1's support lies
    # in B1 only: it reaches B2 through the pixels plane 0 claimed.
    r1, c1 = max(2, H // 3), W // 2                                # two rows at the least: A needs a fit
    band = max(1, c1 // 4)
    zmap = np.full((H, W), 2.0); zmap[:r1, :c1] = 2.5
    depth = fronto(W, H, zmap, rng)
    wall = np.ones((H, W), int); wall[:r1, :c1] = 0
    _, abcd, cov16 = stand_in(depth, wall, P)
    lab = np.full((H, W), -1, np.int8)
    lab[:r1, :c1] = 0; lab[r1, :band] = 0
    lab[:r1, c1:] = 1
    inten = intensity_of(np.zeros((H, W), int), rng)
    inten[r1, c1:] += 100
    ft = add(depth, inten, lab, abcd, cov16)
    pairs.append(dict(name="block-and-conduct", i=ft, j=ft, pose=IDENT, S=SMALL_COV))

    # eight planes: strips at eight depths, one intensity level each
    edges = np.linspace(0, W, 9).astype(int)
    strip = np.searchsorted(edges, np.arange(W), side="right") - 1
    depth = fronto(W, H, 1.5 + 0.3 * strip, rng)
    wall = np.tile(strip[None, :], (H, 1))
    inten = np.clip(20 + 25 * wall + rng.integers(-2, 3, (H, W)), 0, 255).astype(np.uint8)
    f8 = add(depth, inten, *stand_in(depth, wall, P))
    pairs.append(dict(name="eight-planes", i=f8, j=f8, pose=IDENT, S=SMALL_COV))

    n = len(frames)
    abcd = np.zeros((n, MAX_PLANES, 4)); cov16 = np.zeros((n, MAX_PLANES, 16))
    for f, fr_ in enumerate(frames):
        k = len(fr_["abcd"])
        abcd[f, :k] = fr_["abcd"]; cov16[f, :k] = fr_["cov16"]
    return dict(W=W, H=H, cam=cam, depth=np.stack([f["depth"] for f in frames]), intensity=np.stack([f["inten"] for f in frames]),
                labels=np.stack([f["lab"] for f in frames]), n_planes=np.array([len(f["abcd"]) for f in frames], np.int32), abcd=abcd,
                cov16=cov16, pairs=pairs)


SHAPES = ((16, 12), (67, 3), (48, 40), (176, 144), (256, 256), (257, 256))
SEEDS = {(16, 12): 1, (67, 3): 1, (48, 40): 1, (176, 144): 1, (256, 256): 1, (257, 256): 1}


def gpu_cases():
    return [make_call(W, H, SEEDS[(W, H)]) for W, H in SHAPES]


def reference_of(call, p, growth="closure", **params):
    """propagate_pair on pair p of a call"""
    pr = call["pairs"][p]
    i, j = pr["i"], pr["j"]
    k = int(call["n_planes"][i])
    return propagate_pair(call["depth"][i], call["labels"][i], call["abcd"][i, :k], call["cov16"][i, :k], call["depth"][j], call["intensity"][j],
                          pr["pose"], pr["S"], growth=growth, **dict(call["cam"], **params))


def info_of(call):
    """info_ut21 of every pair of a call: S^-1, and minus the identity where S is None"""
    return np.array([pcr.info_ut21(-np.eye(6) if p["S"] is None else np.linalg.inv(p["S"])) for p in call["pairs"]])
