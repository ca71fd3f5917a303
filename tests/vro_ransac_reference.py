"""Numpy restatement of fgo_vro_ransac_batch (include/fgo.h), written from the stated semantics and not from the kernel: Python
integers for the hash, numpy.linalg.svd for the least-squares fit (the kernel uses Horn's quaternion form), numpy.linalg for the
information and its inverse.  The VRO library's own arithmetic is not in the reference tree, so this file IS the yardstick of
csrc/kernels_vro_ransac.hip; tests/test_vro_ransac_reference_cpu.py pins it on the CPU.

Besides the outputs of the call, ransac_pair returns what the GPU test's tolerances need: fit_gap (the relative gap
(s2 + d s3) / s1 of the singular values of the last fit's cross-covariance, d = the determinant sign: the rotation is
determined to rounding / fit_gap), cond_info, cond_S (the largest cond(S_k) over the final inliers), p_max (the largest |p_j|),
and per hypothesis a `decided` flag: no validity test within 1e-7 (relative) of its threshold and no match residual within 1e-7
(relative) of max_dist^2."""
import numpy as np

VRO_OK, VRO_TOO_FEW, VRO_NUM = 0, 1, 2
MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
DECIDE = 1e-7

DEFAULTS = dict(hypotheses=5000, seed=0, max_dist=0.03, min_side=0.05, rigid_tol=0.03, refine_rounds=3, min_inliers=8,
                fx=250.5773, fy=250.5773, sigma_px=1.0, sigma_z=(0.014, 0.0, 0.0))


def mix(z):
    """the splitmix64 finaliser on a Python integer"""
    z &= MASK64
    z ^= z >> 30; z = (z * 0xBF58476D1CE4E5B9) & MASK64
    z ^= z >> 27; z = (z * 0x94D049BB133111EB) & MASK64
    z ^= z >> 31
    return z


def sample3(seed, h, M):
    """the three distinct matches of hypothesis h among M >= 3"""
    u = [mix(seed + (3 * h + k + 1) * GOLDEN) for k in range(3)]
    a = u[0] % M
    b = u[1] % (M - 1); b += b >= a
    c = u[2] % (M - 2); c += c >= min(a, b); c += c >= max(a, b)
    return a, b, c


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def triad(pa, pb, pc):
    """F = [e1 e2 e3] (columns) of three points; leading axes are batched"""
    e1 = _unit(pb - pa)
    e3 = _unit(np.cross(e1, pc - pa))
    e2 = np.cross(e3, e1)
    return np.stack([e1, e2, e3], -1)


def triad_fit(pi3, pj3):
    """R, t of one sample: pi3 / pj3 are (..., 3 points, 3)"""
    Fi = triad(pi3[..., 0, :], pi3[..., 1, :], pi3[..., 2, :]); Fj = triad(pj3[..., 0, :], pj3[..., 1, :], pj3[..., 2, :])
    R = Fi @ np.swapaxes(Fj, -1, -2)
    t = pi3.mean(-2) - np.einsum("...ab,...b->...a", R, pj3.mean(-2))
    return R, t


def _sides(p3):
    ab = np.linalg.norm(p3[..., 1, :] - p3[..., 0, :], axis=-1); ac = np.linalg.norm(p3[..., 2, :] - p3[..., 0, :], axis=-1)
    bc = np.linalg.norm(p3[..., 2, :] - p3[..., 1, :], axis=-1)
    area = np.linalg.norm(np.cross(p3[..., 1, :] - p3[..., 0, :], p3[..., 2, :] - p3[..., 0, :]), axis=-1)
    return ab, ac, bc, area


def residual2(R, t, xi, xj):
    r = xi - (xj @ R.T + t)
    return np.sum(r * r, -1)


def score(xi, xj, P):
    """per hypothesis: count (-1 = invalid), decided, and the sample's R, t"""
    K, M = P["hypotheses"], len(xi)
    if M < 3:
        return np.full(K, -1), np.ones(K, bool), None, None
    idx = np.array([sample3(P["seed"], h, M) for h in range(K)])
    pi3, pj3 = xi[idx], xj[idx]
    si, sj = _sides(pi3), _sides(pj3)
    ms, ma, rt = P["min_side"], P["min_side"] ** 2, P["rigid_tol"]
    d2 = P["max_dist"] ** 2
    with np.errstate(all="ignore"):
        invalid = (si[0] < ms) | (sj[0] < ms) | (si[3] < ma) | (sj[3] < ma)
        near = (np.abs(si[0] - ms) <= DECIDE * ms) | (np.abs(sj[0] - ms) <= DECIDE * ms)
        near |= (np.abs(si[3] - ma) <= DECIDE * ma) | (np.abs(sj[3] - ma) <= DECIDE * ma)
        for k in range(3):
            diff = np.abs(si[k] - sj[k])
            invalid |= diff > rt
            near |= np.abs(diff - rt) <= DECIDE * max(rt, np.finfo(float).tiny)
        R, t = triad_fit(pi3, pj3)
        res = xi[None] - (np.einsum("kab,mb->kma", R, xj) + t[:, None])
        r2 = np.sum(res * res, -1)
    count = np.where(invalid, -1, np.sum(r2 <= d2, 1))
    # an invalid hypothesis is decided by its validity tests alone: its residuals decide nothing
    decided = ~near & (invalid | ~np.any(np.abs(r2 - d2) <= DECIDE * d2, 1))
    return count, decided, R, t


def fit(xi, xj):
    """least squares: R, t with xi ~ R xj + t, and the relative gap of the singular values"""
    ci, cj = xi.mean(0), xj.mean(0)
    C = (xi - ci).T @ (xj - cj)
    U, s, Vt = np.linalg.svd(C)
    d = 1.0 if np.linalg.det(U @ Vt) > 0 else -1.0
    R = U @ np.diag([1.0, 1.0, d]) @ Vt
    return R, ci - R @ cj, (s[1] + d * s[2]) / s[0]


def quat_xyzw(R):
    """unit quaternion x y z w of a rotation matrix, w >= 0 (the branch of the largest component)"""
    tr = np.trace(R)
    c = [1 + tr, 1 + 2 * R[0, 0] - tr, 1 + 2 * R[1, 1] - tr, 1 + 2 * R[2, 2] - tr]
    k = int(np.argmax(c))
    if k == 0:
        q = [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], c[0]]
    elif k == 1:
        q = [c[1], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0], R[2, 1] - R[1, 2]]
    elif k == 2:
        q = [R[0, 1] + R[1, 0], c[2], R[1, 2] + R[2, 1], R[0, 2] - R[2, 0]]
    else:
        q = [R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], c[3], R[1, 0] - R[0, 1]]
    q = np.array(q) / np.linalg.norm(q)
    return -q if q[3] < 0 else q


def quat_matrix(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def skew(p):
    return np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0.0]])


def point_cov(p, P):
    x, y, z = p
    s = P["sigma_z"]
    sz = s[0] + s[1] * z + s[2] * z * z
    G = np.array([[z / P["fx"], 0, x / z], [0, z / P["fy"], y / z], [0, 0, 1.0]])
    return G @ np.diag([P["sigma_px"] ** 2, P["sigma_px"] ** 2, sz ** 2]) @ G.T


def residual_cov(R, pi, pj, P):
    return point_cov(pi, P) + R @ point_cov(pj, P) @ R.T


def information(R, t, xi, xj, P):
    """sum J^T S^-1 J over the given matches, with the largest cond(S_k)"""
    info = np.zeros((6, 6)); cond = 1.0
    for pi, pj in zip(xi, xj):
        J = np.hstack([-R @ skew(pj), R])
        S = residual_cov(R, pi, pj, P)
        cond = max(cond, np.linalg.cond(S))
        info += J.T @ np.linalg.solve(S, J)
    return 0.5 * (info + info.T), cond


def void_record(M):
    return dict(pose=np.array([0, 0, 0, 0, 0, 0, 1.0]), info=10000.0 * np.eye(6), cov=np.zeros((6, 6)), mask=np.zeros(M, bool),
                n_inliers=0, rmse=0.0)


def ransac_pair(xi, xj, **params):
    P = dict(DEFAULTS, **params)
    xi = np.asarray(xi, float).reshape(-1, 3); xj = np.asarray(xj, float).reshape(-1, 3)
    M, d2 = len(xi), P["max_dist"] ** 2
    count, decided, Rh, th = score(xi, xj, P)
    out = dict(hyp_counts=count, decided=decided, n_valid=int(np.sum(count >= 0)), rounds=0, fit_gap=1.0, cond_info=1.0, cond_S=1.0,
               p_max=float(np.linalg.norm(xj, axis=1).max()) if M else 0.0)
    best = int(np.argmax(count))                                  # the first of the largest: ties go to the lowest h
    out["best_hypothesis"], out["best_count"] = (best, int(count[best])) if count[best] >= 0 else (-1, -1)
    status = VRO_OK if out["best_count"] >= P["min_inliers"] else VRO_TOO_FEW
    if status == VRO_OK:
        R, t = Rh[best], th[best]
        mask = residual2(R, t, xi, xj) <= d2
        for _ in range(P["refine_rounds"]):
            R, t, out["fit_gap"] = fit(xi[mask], xj[mask])
            out["rounds"] += 1
            if not (np.all(np.isfinite(R)) and np.all(np.isfinite(t))):
                status = VRO_NUM
                break
            new = residual2(R, t, xi, xj) <= d2
            same = np.array_equal(new, mask)
            mask = new
            if mask.sum() < P["min_inliers"]:
                status = VRO_TOO_FEW
                break
            if same:
                break
    if status == VRO_OK:
        if np.any(xi[mask, 2] <= 0) or np.any(xj[mask, 2] <= 0):
            status = VRO_NUM
        else:
            info, out["cond_S"] = information(R, t, xi[mask], xj[mask], P)
            if not np.all(np.isfinite(info)) or np.linalg.eigvalsh(info)[0] <= 0:
                status = VRO_NUM
            else:
                cov = np.linalg.inv(info)
                out.update(pose=np.concatenate([t, quat_xyzw(R)]), info=info, cov=0.5 * (cov + cov.T), mask=mask, n_inliers=int(mask.sum()),
                           rmse=float(np.sqrt(residual2(R, t, xi[mask], xj[mask]).mean())), cond_info=float(np.linalg.cond(info)))
    if status != VRO_OK:
        out.update(void_record(M))
    out["status"] = status
    return out


def ut21(A):
    return np.asarray(A)[np.triu_indices(6)]


# ---- generated cases: the inputs of the GPU test (tests/test_gpu_vro_ransac.py), checked for being well posed on the CPU

BOX_LO, BOX_HI = np.array([-1.5, -1.0, 0.8]), np.array([1.5, 1.0, 5.0])
NOISE = 0.002


def so3_exp(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    K = skew(w / th)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def make_pair(rng, M, outlier_share, angle):
    """M matches: points of camera i in the box, the planted transform a rotation by `angle` about an axis near the optical one (so
    every depth stays positive in both frames) and a small translation, 2 mm noise in either frame, round(share M) outliers displaced
    by 0.3 - 1 m in camera j"""
    axis = _unit(np.array([0.05, -0.03, 1.0]) + 0.02 * rng.normal(size=3))
    R = so3_exp(angle * axis); t = rng.uniform(-0.2, 0.2, 3)
    pi = rng.uniform(BOX_LO, BOX_HI, (M, 3))
    pj = (pi - t) @ R                                             # R^T (p_i - t)
    out = np.zeros(M, bool)
    out[rng.permutation(M)[:int(round(outlier_share * M))]] = True
    pj = pj + out[:, None] * (_unit(rng.normal(size=(M, 3))) * rng.uniform(0.3, 1.0, (M, 1)))
    return dict(xi=pi + NOISE * rng.normal(size=(M, 3)), xj=pj + NOISE * rng.normal(size=(M, 3)), R=R, t=t, planted=~out, kind="general")


SIZES = (0, 2, 3, 4, 7, 8, 63, 64, 65, 127, 128, 129, 130, 300)      # the issue's list + either side of the 128-match LDS chunk
SHARES = (0.0, 0.3, 0.6)
ANGLES = (0.0, 0.1, 1.0, np.pi - 1e-3)


def gpu_cases(seed=20261):
    """the batch of the GPU test: every size three times (the shares and the angles cycle against each other), and four status
    pairs in the middle of the batch"""
    rng = np.random.default_rng(seed)
    pairs = []
    for rep in range(3):
        for k, M in enumerate(SIZES):
            n = rep * len(SIZES) + k
            pairs.append(make_pair(rng, M, SHARES[(n + rep) % 3], ANGLES[n % 4]))
    few = make_pair(rng, 2, 0.0, 0.1); few["kind"] = "too_few"
    line = make_pair(rng, 20, 0.0, 0.1)                              # all points on one line, no noise: no valid hypothesis
    s = np.linspace(-1.0, 1.0, 20)[:, None]
    line["xi"] = np.array([0.1, 0.0, 2.5]) + s * _unit(np.array([1.0, 0.4, 0.3]))
    line["xj"] = (line["xi"] - line["t"]) @ line["R"]; line["kind"] = "collinear"
    low = make_pair(rng, 12, 0.5, 1.0); low["kind"] = "below_min"   # 6 inliers < min_inliers = 8
    neg = make_pair(rng, 40, 0.0, 0.1); neg["kind"] = "z_nonpositive"
    neg["xi"][5, 2] -= 3.0 + neg["xi"][5, 2]                         # an inlier at z_i = -3, consistent in both frames
    neg["xj"][5] = (neg["xi"][5] - neg["t"]) @ neg["R"]
    mid = len(pairs) // 2
    pairs[mid:mid] = [few, line, low, neg]
    return pairs


def pack(pairs):
    ptr = np.concatenate([[0], np.cumsum([len(p["xi"]) for p in pairs])]).astype(np.int64)
    xi = np.concatenate([p["xi"].reshape(-1, 3) for p in pairs]); xj = np.concatenate([p["xj"].reshape(-1, 3) for p in pairs])
    return ptr, np.ascontiguousarray(xi), np.ascontiguousarray(xj)
