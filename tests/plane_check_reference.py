"""numpy restatement of the plane check of visual-odometry records (include/fgo.h fgo_plane_check_vro_batch; the reference's
gtsam/test_plane_check_vo.cpp computePlaneNodeDis :328-379 and computePlaneDis :383-445, CGraphGT::computeSdj
gtsam/gtsam_graph.cpp:725-748), written for reading, not for speed, and the generator of consistent records the tests share.
tests/test_plane_check_reference_cpu.py holds this restatement to the golden errorVector regression, to central differences and
to the chi-square law; tests/test_gpu_plane_check.py then holds the kernel to it.

Conventions: a pose is t(3) q_xyzw(4), the pose of frame j in frame i; its tangent is [omega; v] (right perturbation, GTSAM);
a plane is (nx, ny, nz, d) with its tangent [dn(2); dd]; a plane's cov16 is CPlane::m_CP (4x4)."""
import numpy as np

COS_MIN = float(np.cos(np.deg2rad(10.0)))
D_MAX = 0.2
FAILED_INFO00 = 10000.0
PC_OK, PC_SKIPPED, PC_NUM = 0, 1, 2
_UT = np.triu_indices(6)


def info_full(ut21):
    A = np.zeros((6, 6)); A[_UT] = ut21
    return A + np.triu(A, 1).T


def info_ut21(A):
    return np.asarray(A, np.float64)[_UT].copy()


def sym_upper(A):
    """the symmetric matrix the entry point reads: the upper triangle, mirrored"""
    A = np.asarray(A, np.float64)
    return np.triu(A) + np.triu(A, 1).T


def normalize(abcd):
    p = np.array(abcd, np.float64)
    p[:3] /= np.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])
    return p


def axis_of(n):
    """Unit3::basis(): the coordinate axis of the smallest |n_i| (ties: x, then y, then z)"""
    m = np.abs(n)
    if m[0] <= m[1] and m[0] <= m[2]:
        return np.array([1.0, 0, 0])
    if m[1] <= m[0] and m[1] <= m[2]:
        return np.array([0, 1.0, 0])
    return np.array([0, 0, 1.0])


def axis_margin(n):
    """distance of the two smallest |n_i|: 0 on the basis rule's axis switch"""
    m = np.sort(np.abs(n))
    return m[1] - m[0]


def basis(n):
    c = np.cross(n, axis_of(n))
    b1 = c / np.sqrt(c @ c)
    return np.stack([b1, np.cross(n, b1)], 1)                   # 3x2


def qmat(q):
    x, y, z, w = np.asarray(q, np.float64) / np.sqrt(np.dot(q, q))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def transform(p, pose, jac=False):
    """OrientedPlane3::transform: n' = R^T n, d' = n.t + d, with D_pose (3x6) and D_plane (3x3) in the tangent of the result"""
    R, t, n = qmat(pose[3:]), np.asarray(pose[:3], np.float64), p[:3]
    out = np.append(R.T @ n, n @ t + p[3])
    if not jac:
        return out
    Bp, B = basis(out[:3]), basis(n)
    Dx = np.zeros((3, 6)); Dp = np.zeros((3, 3))
    Dx[:2, :3] = Bp.T @ skew(out[:3]); Dx[2, 3:] = out[:3]
    Dp[:2, :2] = Bp.T @ R.T @ B; Dp[2, :2] = t @ B; Dp[2, 2] = 1
    return out, Dx, Dp


def tangent_cov(p, cov16):
    """S_P = diag(B^T S_n B, S_d) (:395-406)"""
    C = sym_upper(np.asarray(cov16, np.float64).reshape(4, 4))
    B = basis(p[:3])
    S = np.zeros((3, 3)); S[:2, :2] = B.T @ C[:3, :3] @ B; S[2, 2] = C[3, 3]
    return S


def error_vector(pe, pj, jac=False):
    """OrientedPlane3::errorVector: e = [B(n')^T n_j; d' - d_j]; H1 = d e / d PE, H2 = d e / d Pj in their tangents.  Hp (the
    normal block of H1) goes through the basis rule with the axis held fixed (GTSAM 4.0's Unit3::errorVector)."""
    n, q = pe[:3], pj[:3]
    B = basis(n)
    e = np.append(B.T @ q, pe[3] - pj[3])
    if not jac:
        return e
    ax = axis_of(n)
    c = np.cross(n, ax); nc = np.sqrt(c @ c)
    b1 = B[:, 0]
    H1 = np.zeros((3, 3)); H2 = np.zeros((3, 3))
    for k in range(2):
        dn = B[:, k]
        db1 = (np.eye(3) - np.outer(b1, b1)) @ np.cross(dn, ax) / nc
        db2 = np.cross(dn, b1) + np.cross(n, db1)
        H1[0, k] = q @ db1; H1[1, k] = q @ db2
    H1[2, 2] = 1
    H2[:2, :2] = B.T @ basis(q); H2[2, 2] = -1
    return e, H1, H2


def pair_distance(pe, S_pe, pj, S_pj):
    """computePlaneDis :431-443: (d2, raw, positive definite?, cond(S_e))"""
    e, H1, H2 = error_vector(pe, pj, True)
    S_e = H1 @ S_pe @ H1.T + H2 @ S_pj @ H2.T
    try:
        np.linalg.cholesky(S_e)
    except np.linalg.LinAlgError:
        return np.inf, np.inf, False, np.inf
    return float(e @ np.linalg.solve(S_e, e)), float(e @ e), True, float(np.linalg.cond(S_e))


def sdj(p, cov16, pose, S_t):
    """CGraphGT::computeSdj with CP(3, 3) standing in for m_E_Sdi"""
    C = sym_upper(np.asarray(cov16, np.float64).reshape(4, 4))
    n, t = p[:3], np.asarray(pose[:3], np.float64)
    g = (np.eye(3) - np.outer(n, n)) @ t
    return C[3, 3] + n @ S_t @ n + g @ C[:3, :3] @ g


def check_record(pose, pi, ci, pj, cj, info=None, cov=None, cos_min=COS_MIN, d_max=D_MAX, failed_info00=FAILED_INFO00):
    """One record.  pi (ni x 4), ci (ni x 16), pj, cj likewise; exactly one of info (21) and cov (6x6).  Returns what the entry
    point returns for it, and cond_e (per plane i; 0 where unmatched) / cond_info for the tolerances."""
    pi = np.asarray(pi, np.float64).reshape(-1, 4); pj = np.asarray(pj, np.float64).reshape(-1, 4)
    ci = np.asarray(ci, np.float64).reshape(-1, 16); cj = np.asarray(cj, np.float64).reshape(-1, 16)
    ni, nj = len(pi), len(pj)
    out = dict(status=PC_OK, n_matched=0, n_bad=0, best_i=-1, best_j=-1, err=0.0, err_raw=0.0, cond_info=1.0,
               match=np.full(ni, -1, np.int64), d2=np.zeros(ni), raw=np.zeros(ni), pred_abcd=np.zeros((ni, 4)),
               pred_cov=np.zeros((ni, 3, 3)), sdj=np.zeros(ni), cond_e=np.zeros(ni))
    assert (info is None) != (cov is None)
    if cov is not None:
        Sij = sym_upper(np.asarray(cov, np.float64).reshape(6, 6))
    else:
        A = info_full(info)
        if failed_info00 > 0 and A[0, 0] == failed_info00:
            out["status"] = PC_SKIPPED
            return out
        try:
            if not np.all(np.isfinite(A)):
                raise np.linalg.LinAlgError
            np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            out["status"] = PC_NUM
            return out
        Sij = np.linalg.inv(A)
        out["cond_info"] = float(np.linalg.cond(A))
    Pj = [normalize(p) for p in pj]
    for i in range(ni):
        P = normalize(pi[i])
        pe, Dx, Dp = transform(P, pose, True)
        S_pe = Dx @ Sij @ Dx.T + Dp @ tangent_cov(P, ci[i]) @ Dp.T
        out["pred_abcd"][i] = pe; out["pred_cov"][i] = S_pe
        out["sdj"][i] = sdj(P, ci[i], pose, Sij[3:, 3:])
        for j in range(nj):
            if abs(pe[:3] @ Pj[j][:3]) >= cos_min and abs(pe[3] - Pj[j][3]) <= d_max:
                out["match"][i] = j
                break
        else:
            continue
        j = int(out["match"][i])
        d2, raw, pd, cond = pair_distance(pe, S_pe, Pj[j], tangent_cov(Pj[j], cj[j]))
        out["n_matched"] += 1
        out["d2"][i] = d2; out["raw"][i] = raw; out["cond_e"][i] = cond
        if not pd:
            out["n_bad"] += 1
        elif d2 > out["err"]:
            out["err"] = d2; out["err_raw"] = raw; out["best_i"] = i; out["best_j"] = j
    return out


# ---- the generator: consistent records, every quantity drawn from the covariance the check is told

def plane_retract(p, v):
    """OrientedPlane3::retract: the exponential map on the sphere, and d + v[2]"""
    xi = basis(p[:3]) @ np.asarray(v[:2], np.float64)
    th = np.sqrt(xi @ xi)
    n = np.cos(th) * p[:3] + (np.sin(th) / th if th > 1e-300 else 1.0) * xi
    return np.append(n / np.sqrt(n @ n), p[3] + v[2])


def pose_retract(pose, xi):
    """Pose3 retract: pose * Expmap([omega; v])"""
    w, v = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
    th = np.sqrt(w @ w)
    W = skew(w)
    if th < 1e-8:
        V = np.eye(3) + 0.5 * W; qd = np.append(0.5 * w, 1.0)
    else:
        V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * W + (th - np.sin(th)) / th ** 3 * W @ W
        qd = np.append(np.sin(0.5 * th) / th * w, np.cos(0.5 * th))
    x, y, z, s = pose[3:]
    a, b, c, d = qd
    q = np.array([s * a + d * x + (y * c - z * b), s * b + d * y + (z * a - x * c), s * c + d * z + (x * b - y * a),
                  s * d - (x * a + y * b + z * c)])
    return np.concatenate([np.asarray(pose[:3]) + qmat(pose[3:]) @ (V @ v), q / np.sqrt(q @ q)])


def _spd(rng, k):
    """a random symmetric positive definite k x k with eigenvalues in about [0.5, 2.5]"""
    A = rng.normal(size=(k, k))
    return A @ A.T / k + 0.5 * np.eye(k)


def random_plane_cov(rng, sigma_n=0.01, sigma_d=0.01):
    C = np.zeros((4, 4)); C[:3, :3] = sigma_n ** 2 * _spd(rng, 3); C[3, 3] = sigma_d ** 2 * rng.uniform(0.5, 2.0)
    return C.reshape(16)


def random_pose_cov(rng, sigma_r=0.005, sigma_t=0.01):
    D = np.diag([sigma_r] * 3 + [sigma_t] * 3)
    return D @ _spd(rng, 6) @ D


def random_unit(rng, margin=1e-2):
    """a unit vector whose two smallest |n_i| are at least `margin` apart (off the basis rule's axis switch)"""
    while True:
        v = rng.normal(size=3); v /= np.sqrt(v @ v)
        if axis_margin(v) >= margin:
            return v


def random_pose(rng, angle=0.3, step=0.3):
    w = random_unit(rng, 0) * rng.uniform(0, angle)
    return pose_retract(np.array([0, 0, 0, 0, 0, 0, 1.0]), np.concatenate([w, rng.uniform(-step, step, 3)]))


def _draw(rng, S):
    return np.linalg.cholesky(S) @ rng.normal(size=len(S))


def draw_planes(rng, pose_true, i_src, j_src):
    """True planes in frame i (as many as i_src / j_src name); plane i k is true plane i_src[k] plus noise from its S_P, plane j k
    is true plane j_src[k] carried through the true pose plus noise from its S_P.  Returns pi, ci, pj, cj."""
    true = [np.append(random_unit(rng), rng.uniform(0.5, 3.0)) for _ in range(1 + max(list(i_src) + list(j_src), default=-1))]
    ci = [random_plane_cov(rng) for _ in i_src]; cj = [random_plane_cov(rng) for _ in j_src]
    pi = [plane_retract(true[s], _draw(rng, tangent_cov(true[s], c))) for s, c in zip(i_src, ci)]
    tj = [transform(true[s], pose_true) for s in j_src]
    pj = [plane_retract(t, _draw(rng, tangent_cov(t, c))) for t, c in zip(tj, cj)]
    return np.array(pi).reshape(-1, 4), np.array(ci).reshape(-1, 16), np.array(pj).reshape(-1, 4), np.array(cj).reshape(-1, 16)


def well_separated(pose, pi, pj):
    """every candidate pair (i, j) under the pose the check is given lies within 5 deg and 0.1 m, or at least 20 deg or 0.4 m
    apart, so no match decision sits near a threshold; every normal keeps 1e-6 from the basis rule's axis switch"""
    pe = [transform(p, pose) for p in pi]
    ok = all(axis_margin(p[:3]) >= 1e-6 for p in list(pi) + list(pj) + pe)
    for a in pe:
        for b in pj:
            ang = np.degrees(np.arccos(min(1.0, abs(a[:3] @ b[:3])))); dd = abs(a[3] - b[3])
            ok = ok and ((ang <= 5 and dd <= 0.1) or ang >= 20 or dd >= 0.4)
    return ok


def draw_record(rng, i_src, j_src):
    """A consistent record: the true pose is the record's Tij retracted by noise from Sij, the planes are draw_planes' under the
    true pose; redrawn until well_separated under Tij."""
    while True:
        pose, Sij = random_pose(rng), random_pose_cov(rng)
        pi, ci, pj, cj = draw_planes(rng, pose_retract(pose, _draw(rng, Sij)), i_src, j_src)
        if well_separated(pose, pi, pj):
            return dict(pose=pose, cov=Sij, info=info_ut21(np.linalg.inv(Sij)), pi=pi, ci=ci, pj=pj, cj=cj)


def random_sources(rng, ni, nj):
    """plane lists of ni and nj planes that share a random number of true planes, the j-list in random order"""
    common = int(rng.integers(0, min(ni, nj) + 1))
    j_src = list(rng.permutation(ni)[:common]) + list(range(ni, ni + nj - common))
    return list(range(ni)), [int(s) for s in rng.permutation(j_src)] if nj else []


def pack(records):
    """the arrays of one batch: pose (n x 7), info (n x 21), cov (n x 6 x 6), pi_ptr, pi, ci, pj_ptr, pj, cj"""
    cat = lambda k, w: np.concatenate([r[k].reshape(-1, w) for r in records]) if records else np.zeros((0, w))
    ptr = lambda k: np.concatenate([[0], np.cumsum([len(r[k]) for r in records])]).astype(np.int64)
    return dict(pose=np.array([r["pose"] for r in records]).reshape(-1, 7), info=np.array([r["info"] for r in records]).reshape(-1, 21),
                cov=np.array([r["cov"] for r in records]).reshape(-1, 6, 6), pi_ptr=ptr("pi"), pi=cat("pi", 4), ci=cat("ci", 16),
                pj_ptr=ptr("pj"), pj=cat("pj", 4), cj=cat("cj", 16))
