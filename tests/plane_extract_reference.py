"""Numpy restatement of fgo_plane_extract_batch (include/fgo.h), written from the stated semantics and not from the kernel: Python
integers for the hash, numpy.linalg.eigh for the total-least-squares fit (the kernel uses cyclic Jacobi sweeps), numpy.linalg for
the sandwich covariance.  The plane package's own arithmetic is not in the reference tree, so this file IS the yardstick of
csrc/kernels_plane_extract.hip; tests/test_plane_extract_reference_cpu.py pins it on the CPU.

Besides the outputs of the call, extract_frame returns what the GPU test's tolerances and its well-posedness test need: per round a
`decided` mask over the hypotheses (no candidate's |n.p + d| within 1e-9 of max_dist, and |m| not within 1e-9 relative of
min_area), per plane the gap g = min(1, (l1 - l0) / l2) of the final fit's scatter matrix (the normal is determined to rounding / g)
and cond(A), the smallest g over every fit made (g_min), p_max (the largest |p| of a valid pixel), and `margin`: the smallest
distance of any decision after the scoring from its threshold (a refinement or final-pass | |n.p + d| - max_dist |, and the gap
between the nearest and the second nearest plane of a pixel in the final pass), and `d_min`: the smallest |d| of a winner or
of a fit (a plane through the camera has no orientation: the pixels of one image row lie on such a plane).

The scene generator renders a box room seen from a pose inside: each pixel's ray takes the nearest wall, Gaussian depth noise is
added and the result is rounded to depth words.  gpu_cases() lists the calls of tests/test_gpu_plane_extract.py."""
import numpy as np

from tests.vro_ransac_reference import GOLDEN, MASK64, mix, quat_xyzw as vro_quat, sample3 as vro_sample3  # noqa: F401  (the sampler is the VRO one)

PX_OK, PX_NUM = 0, 2
DECIDE = 1e-9
CHUNK = 2048                 # the kernel's staging chunk (PX_CHUNK)
PASS = 512                   # the kernel's hypotheses per pass (PX_PASS)

DEFAULTS = dict(fx=250.5773, fy=250.5773, cx=90.0, cy=70.0, z_scale=0.001, z_min=0.1, z_max=5.0, hypotheses=512, seed=0, max_dist=0.05,
                min_area=1e-3, min_pixels=1500, max_planes=4, refine_rounds=3, sigma_px=1.0, sigma_z=(0.014, 0.0, 0.0))


def sample3(seed, r, h, K, M):
    """the three distinct candidates of hypothesis h of round r among M >= 3: the VRO sampler at the counter r K + h, which draws
    u_k = mix(seed + ((r K + h) 3 + k + 1) GOLDEN)"""
    return vro_sample3(seed, r * K + h, M)


def backproject(depth, P):
    """points (H W x 3) in pixel order v W + u, and the valid mask"""
    H, W = depth.shape
    v, u = np.divmod(np.arange(H * W), W)
    z = depth.reshape(-1).astype(np.float64) * P["z_scale"]
    valid = (z > P["z_min"]) & (z < P["z_max"])
    return np.stack([(u - P["cx"]) * z / P["fx"], (v - P["cy"]) * z / P["fy"], z], 1), valid


def orient(n, d):
    """the camera on the positive side"""
    return (-n, -d) if d < 0 else (n, d)


def axis_of(n):
    """Unit3::basis(): the coordinate axis of the smallest |n_i| (ties: x, then y, then z)"""
    m = np.abs(n)
    if m[0] <= m[1] and m[0] <= m[2]:
        return np.array([1.0, 0, 0])
    if m[1] <= m[0] and m[1] <= m[2]:
        return np.array([0, 1.0, 0])
    return np.array([0, 0, 1.0])


def basis(n):
    c = np.cross(n, axis_of(n))
    b1 = c / np.sqrt(c @ c)
    return np.stack([b1, np.cross(n, b1)], 1)                   # 3x2


def score(pc, P, r):
    """the hypotheses of round r over the candidates pc (M x 3): count (-1 = invalid), decided, n (K x 3), d (K)"""
    K, M, md, ma = P["hypotheses"], len(pc), P["max_dist"], P["min_area"]
    idx = np.array([sample3(P["seed"], r, h, K, M) for h in range(K)])
    pa, pb, pk = pc[idx[:, 0]], pc[idx[:, 1]], pc[idx[:, 2]]
    m = np.cross(pb - pa, pk - pa)
    nm = np.linalg.norm(m, axis=1)
    invalid = nm < ma
    near = np.abs(nm - ma) <= DECIDE * ma
    n = m / np.where(nm > 0, nm, 1.0)[:, None]
    d = -np.sum(n * pa, 1)
    flip = d < 0
    n[flip] = -n[flip]; d[flip] = -d[flip]
    count = np.zeros(K, np.int64); close = np.zeros(K, bool)
    for k0 in range(0, K, 128):                                   # in slabs: M x K doubles at once is a lot at 176 x 144
        dist = np.abs(pc @ n[k0:k0 + 128].T + d[k0:k0 + 128])
        count[k0:k0 + 128] = np.sum(dist <= md, 0)
        close[k0:k0 + 128] = np.any(np.abs(dist - md) <= DECIDE, 0)
    count = np.where(invalid, -1, count)
    # an invalid hypothesis is decided by its area alone
    return count, ~near & (invalid | ~close), n, d


def fit(p):
    """total least squares: n, d, centroid, and the eigenvalues of the scatter of the centred points (ascending)"""
    c = p.mean(0)
    q = p - c
    w, V = np.linalg.eigh(q.T @ q)
    n, d = orient(V[:, 0], -(V[:, 0] @ c))
    return n, d, c, w


def gap(w):
    return float(min(1.0, (w[1] - w[0]) / w[2])) if w[2] > 0 else 0.0


def sigma2(n, p, P):
    """n^T Sigma(p) n of the pixel-plus-depth model"""
    z = p[:, 2]
    s = P["sigma_z"]
    sz = s[0] + s[1] * z + s[2] * z * z
    nr = (p @ n) / z
    return P["sigma_px"] ** 2 * ((n[0] * z / P["fx"]) ** 2 + (n[1] * z / P["fy"]) ** 2) + sz ** 2 * nr ** 2


def covariance(n, p, P):
    """the sandwich C = A^-1 M A^-1 in the tangent [dn(2); dd], cov16 = E C E^T, cond(A); None if A is not positive definite"""
    B = basis(n)
    J = np.hstack([p @ B, np.ones((len(p), 1))])
    A = J.T @ J
    Mm = (J * sigma2(n, p, P)[:, None]).T @ J
    try:
        if not (np.all(np.isfinite(A)) and np.all(np.isfinite(Mm))):
            raise np.linalg.LinAlgError
        np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None
    Ai = np.linalg.inv(A)
    C = Ai @ Mm @ Ai
    C = 0.5 * (C + C.T)
    E = np.zeros((4, 3)); E[:3, :2] = B; E[3, 2] = 1
    S = E @ C @ E.T
    return C, 0.5 * (S + S.T), float(np.linalg.cond(A))


def ut6(C):
    return np.asarray(C)[np.triu_indices(3)]


def extract_frame(depth, **params):
    P = dict(DEFAULTS, **params)
    depth = np.asarray(depth)
    H, W = depth.shape
    K, md, mp, minpx = P["hypotheses"], P["max_dist"], P["max_planes"], P["min_pixels"]
    pts, valid = backproject(depth, P)
    out = dict(status=PX_OK, n_planes=0, n_valid_pixels=int(valid.sum()), rounds_run=0, abcd=np.zeros((mp, 4)), cov16=np.zeros((mp, 4, 4)),
               cov_ut6=np.zeros((mp, 6)), n_pixels=np.zeros(mp, int), best_hypothesis=np.zeros(mp, int), best_count=np.zeros(mp, int),
               n_valid_hyp=np.zeros(mp, int), fits=np.zeros(mp, int), round=np.zeros(mp, int), rmse=np.zeros(mp), centroid=np.zeros((mp, 3)),
               hyp_counts=np.full((mp, K), -2), decided=np.ones((mp, K), bool), g=np.ones(mp), cond_A=np.ones(mp), g_min=1.0,
               margin=np.inf, d_min=np.inf, p_max=float(np.linalg.norm(pts[valid], axis=1).max()) if valid.any() else 0.0)
    label = np.where(valid, -1, -2).astype(np.int8)
    free = valid.copy()
    kept = []                                                     # (n, d, meta)

    def near(dist):
        if len(dist):
            out["margin"] = min(out["margin"], float(np.abs(dist - md).min()))

    for r in range(mp):
        ci = np.nonzero(free)[0]
        M = len(ci)
        if M < max(3, minpx):
            break
        out["rounds_run"] += 1
        pc = pts[ci]
        count, dec, nh, dh = score(pc, P, r)
        out["hyp_counts"][r] = count; out["decided"][r] = dec
        best = int(np.argmax(count))                              # the first of the largest: ties go to the lowest h
        if count[best] < 0 or count[best] < minpx:
            break
        n, d = nh[best], dh[best]
        out["d_min"] = min(out["d_min"], abs(d))
        s = np.abs(pc @ n + d) <= md
        fits, ok = 0, True
        for _ in range(P["refine_rounds"]):
            n, d, _, w = fit(pc[s])
            out["g_min"] = min(out["g_min"], gap(w)); out["d_min"] = min(out["d_min"], abs(d))
            fits += 1
            dist = np.abs(pc @ n + d)
            near(dist)
            new = dist <= md
            same = np.array_equal(new, s)
            s = new
            if s.sum() < minpx:
                ok = False
                break
            if same:
                break
        if not ok:
            break
        free[ci[s]] = False
        kept.append((n, d, dict(best_hypothesis=best, best_count=int(count[best]), n_valid_hyp=int(np.sum(count >= 0)), fits=fits,
                                 round=r)))

    # final pass: every valid pixel to the nearest kept plane
    vi = np.nonzero(valid)[0]
    if kept and len(vi):
        dist = np.stack([np.abs(pts[vi] @ n + d) for n, d, _ in kept], 1)
        best = np.argmin(dist, 1)                                 # the first of the smallest: ties go to the lower index
        bd = dist[np.arange(len(vi)), best]
        near(bd)
        if len(kept) > 1:
            two = np.sort(dist, 1)[:, :2]
            close = two[:, 0] <= md + DECIDE
            if close.any():
                out["margin"] = min(out["margin"], float((two[close, 1] - two[close, 0]).min()))
        label[vi] = np.where(bd <= md, best, -1)
    final = []
    for k, (n, d, meta) in enumerate(kept):
        if np.sum(label == k) >= minpx:
            final.append((k, meta))
    remap = np.full(len(kept) + 2, -1); remap[-2] = -2            # label -2 -> -2, -1 -> -1 (numpy's negative indices)
    for new, (k, _) in enumerate(final):
        remap[k] = new
    label = remap[label].astype(np.int8)
    for new, (k, meta) in enumerate(final):
        p = pts[label == new]
        n, d, c, w = fit(p)
        cov = covariance(n, p, P)
        vals = np.concatenate([n, [d], c])
        if cov is None or not (np.all(np.isfinite(vals)) and np.all(np.isfinite(cov[0]))):
            out["status"] = PX_NUM
            break
        out["abcd"][new] = np.append(n, d); out["cov_ut6"][new] = ut6(cov[0]); out["cov16"][new] = cov[1]; out["cond_A"][new] = cov[2]
        out["g"][new] = gap(w); out["g_min"] = min(out["g_min"], gap(w)); out["d_min"] = min(out["d_min"], abs(d))
        out["n_pixels"][new] = len(p); out["rmse"][new] = float(np.sqrt(np.mean((p @ n + d) ** 2))); out["centroid"][new] = c
        for f, v in meta.items():
            out[f][new] = v
    if out["status"] == PX_OK:
        out["n_planes"] = len(final)
    else:
        for f in ("abcd", "cov16", "cov_ut6", "n_pixels", "best_hypothesis", "best_count", "n_valid_hyp", "fits", "round", "rmse", "centroid"):
            out[f][...] = 0
        label[label >= 0] = -1
    out["labels"] = label.reshape(H, W)
    return out


# ---- the scene generator

def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def camera(W, H):
    """the SR4000's field of view (176 x 144 at 250.5773) at another resolution"""
    return dict(fx=250.5773 * W / 176.0, fy=250.5773 * H / 144.0, cx=0.5 * W, cy=0.5 * H)


def room_planes(lo, hi, R, t):
    """the six walls of the box [lo, hi] (world) in the frame of the camera with pose (R, t), t inside the box: (n, d) with the
    camera on the positive side.  World wall n_w.x + d_w = 0 becomes n = R^T n_w, d = n_w.t + d_w."""
    planes = []
    for ax in range(3):
        for bound, sign in ((lo[ax], 1.0), (hi[ax], -1.0)):
            nw = np.zeros(3); nw[ax] = sign
            planes.append((R.T @ nw, float(nw @ t - sign * bound)))
    return planes


def render(planes, W, H, cam, sigma=0.014, rng=None, z_scale=0.001):
    """depth words (H x W): each pixel's ray r = ((u - cx) / fx, (v - cy) / fy, 1) takes the nearest wall in front of it, z = the ray
    parameter; Gaussian noise of sigma on z; rounded to depth words (0 = no return; clipped to 16 bits).  Also the index of the wall."""
    v, u = np.divmod(np.arange(H * W), W)
    rays = np.stack([(u - cam["cx"]) / cam["fx"], (v - cam["cy"]) / cam["fy"], np.ones(H * W)], 1)
    z = np.full(H * W, np.inf); wall = np.full(H * W, -1)
    for k, (n, d) in enumerate(planes):
        den = rays @ n
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.where(den < 0, -d / den, np.inf)              # the camera is on the positive side: a ray that nears the wall
        hit = (s > 0) & (s < z)
        z[hit] = s[hit]; wall[hit] = k
    z = np.where(np.isfinite(z), z, 0.0)
    if rng is not None and sigma > 0:
        z = z + sigma * rng.normal(size=z.shape) * (z > 0)
    words = np.clip(np.rint(z / z_scale), 0, 65535).astype(np.uint16)
    return words.reshape(H, W), wall.reshape(H, W)


def wall_scene(yaw, dist=2.0):
    """one wall `dist` metres ahead, yawed: the other walls of the room are beyond z_max"""
    R = rot_y(yaw)
    return room_planes(np.array([-40.0, -40.0, -40.0]), np.array([40.0, 40.0, dist]), R, np.zeros(3))


def corner_scene():
    """a corner of the room: the front wall, the right wall and the floor are in view"""
    R = rot_y(np.deg2rad(40.0)) @ rot_x(np.deg2rad(-25.0))
    return room_planes(np.array([-40.0, -40.0, -40.0]), np.array([1.6, 1.1, 2.2]), R, np.zeros(3))


SCENES = ("zero", "few", "wall", "corner", "outliers", "corner_one_plane")


def make_frame(kind, W, H, rng, sigma=0.014):
    """one frame of the GPU test: depth words, the camera, and the true planes in view"""
    cam = camera(W, H)
    if kind == "zero":
        return np.zeros((H, W), np.uint16), cam, []
    planes = corner_scene() if kind.startswith("corner") else wall_scene(np.deg2rad(20.0))
    depth, wall = render(planes, W, H, cam, sigma, rng)
    if kind == "few":                                             # fewer valid pixels than min_pixels = W H / 8: one pixel in 32
        keep = np.zeros(W * H, bool); keep[::32] = True
        depth = np.where(keep.reshape(H, W), depth, 0).astype(np.uint16)
    if kind == "outliers":                                        # 30 % of the pixels at random depths
        out = rng.uniform(size=(H, W)) < 0.3
        depth = np.where(out, rng.integers(300, 4800, (H, W)), depth).astype(np.uint16)
    return depth, cam, [planes[k] for k in np.unique(wall[wall >= 0])]


SHAPES = ((16, 12), (48, 40), (23, 89), (64, 32), (683, 3))       # fewer pixels than lanes; small; the staging chunk - 1, the chunk, the chunk + 1
BIG = (176, 144)
HYPOTHESES = (1, 100, PASS, PASS + 8)                             # one hypothesis, a partial pass, exactly one pass, one pass and a bit


def gpu_cases(seed=20262):
    """the calls of the GPU test: dicts of W, H, hypotheses, max_planes, min_pixels, seed, cam, depth (n x H x W), kinds.  Every small shape
    with every number of hypotheses: one call of five frames (the scenes in order) at max_planes = 4 and one call of the corner at
    max_planes = 1 (more walls than it allows); 176 x 144: one call of three frames (wall, corner, outliers) per number of hypotheses."""
    rng = np.random.default_rng(seed)
    calls = []
    for W, H in SHAPES + (BIG,):
        kinds = SCENES[:5] if (W, H) != BIG else SCENES[2:5]
        frames = [make_frame(k, W, H, rng) for k in kinds]
        depth = np.stack([f[0] for f in frames])
        for K in HYPOTHESES:
            seed = 1 if K == 1 else 0                               # seed 0's only hypothesis is a plane through the camera at 683 x 3
            calls.append(dict(W=W, H=H, hypotheses=K, max_planes=4, min_pixels=max(3, W * H // 8), cam=frames[0][1], depth=depth, kinds=kinds,
                              seed=seed))
            if (W, H) != BIG:
                calls.append(dict(W=W, H=H, hypotheses=K, max_planes=1, min_pixels=max(3, W * H // 8), cam=frames[0][1],
                                  depth=depth[3:4], kinds=SCENES[5:6], seed=seed))
    return calls


def call_params(c):
    return dict(c["cam"], hypotheses=c["hypotheses"], max_planes=c["max_planes"], min_pixels=c["min_pixels"], seed=c["seed"])
