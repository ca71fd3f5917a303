"""Numpy restatement of fgo_depth_align_batch (include/fgo_dense.h), written from the semantics stated there: the yardstick of
tests/test_gpu_depth_align.py, itself pinned to a per-pixel brute force by tests/test_depth_align_reference_cpu.py.  Every
per-sample quantity is formed with the header's own operations in the header's own order, element by element (numpy rounds every
operation on its own), so a sample's r, J and w carry the same bits as the kernel's; only the order of the sums over the samples
differs (a fixed binary tree here, lanes, butterfly and waves there).  `ft` is the float type the whole computation runs in:
np.float64, or np.longdouble for the measured yardstick of the GPU tolerances (the f64-against-longdouble difference of H, g, chi2
and the final pose).

Next to its numbers every evaluation reports `margins`: the smallest distance of any sample to any gate, in the unit the gate is
stated in.  Where they all exceed 1e-6 no rounding difference of the size that separates two f64 implementations (1e-12 and less)
can move a sample across a gate: the association sets of the kernel and of this file are then the same sets.
  z_range (m)       |z - z_min|, |z - z_max| over all pixels of both frames
  normal_jump (m)   ||dz| - normal_jump| over the neighbours of every target pixel whose five words are valid
  cross (m^2)       |a x b| over the target pixels that reach the normalisation
  flip (m)          |n . P| over the target normals
  qz (m)            |q_z| over the valid source samples
  rint (px)         |frac - 0.5| of both projected coordinates over the samples that land within a pixel of the image: the tie of
                    rint and, at -0.5 and W - 0.5, the image border
  max_dist (m)      ||e| - max_dist| over the samples that reach that gate
  min_cos (m)       ||n . q| - min_cos |q|| over the samples that reach that gate
and per solve, RELATIVE to the threshold (a step norm falls through 1e-6 by orders of magnitude, not by micrometres):
  eps_rel           | |delta_omega| / eps_rot - 1 |, | |delta_v| / eps_trans - 1 |
  pivot_rel         | min_pivot / params.min_pivot - 1 |"""
import math

import numpy as np

OK, TOO_FEW, DEGENERATE, NUM = 0, 1, 2, 3


def default_params(**kw):
    """fgo_depth_align_params_default as a dict, with the given fields replaced"""
    p = dict(fx=250.5773, fy=250.5773, cx=90.0, cy=70.0, z_scale=0.001, z_min=0.1, z_max=5.0, sigma_px=1.0, sigma_z=(0.014, 0.0, 0.0),
             n_levels=3, skip=(4, 2, 2), iters=(10, 10, 5), normal_step=2, normal_jump=0.05, max_dist=0.10,
             min_cos=0.17364817766693041, min_pairs=500, eps_rot=1e-6, eps_trans=1e-6, min_pivot=1e-6)
    for k in kw:
        if k not in p:
            raise TypeError("no parameter %r" % k)
    p.update(kw)
    return p


def ut6(r, c):
    return r * 6 - r * (r - 1) // 2 + c - r


# ---- frames ------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def frame(depth, P, ft=np.float64):
    """the points of a frame (3 x H x W), their validity, and as a target: the normals (3 x H x W), their validity, the margins"""
    d = np.asarray(depth)
    H, W = d.shape
    z = d.astype(ft) * ft(P["z_scale"])
    valid = (z > ft(P["z_min"])) & (z < ft(P["z_max"]))
    u = np.arange(W, dtype=ft)[None, :]; v = np.arange(H, dtype=ft)[:, None]
    x = ((u - ft(P["cx"])) * z) / ft(P["fx"]); y = ((v - ft(P["cy"])) * z) / ft(P["fy"])
    pts = np.stack([x, y, z])
    margins = {"z_range": float(min(np.abs(z - ft(P["z_min"])).min(), np.abs(z - ft(P["z_max"])).min()))}
    s = P["normal_step"]
    n = np.zeros((3, H, W), ft); nvalid = np.zeros((H, W), bool)
    if H > 2 * s and W > 2 * s:
        c = (slice(s, H - s), slice(s, W - s))
        le, ri = (slice(s, H - s), slice(0, W - 2 * s)), (slice(s, H - s), slice(2 * s, W))
        up, dn = (slice(0, H - 2 * s), slice(s, W - s)), (slice(2 * s, H), slice(s, W - s))
        ok = valid[c] & valid[le] & valid[ri] & valid[up] & valid[dn]
        dz = np.stack([np.abs(z[k] - z[c]) for k in (le, ri, up, dn)])
        if ok.any():
            margins["normal_jump"] = float(np.abs(dz - ft(P["normal_jump"]))[:, ok].min())
        ok &= (dz <= ft(P["normal_jump"])).all(axis=0)
        a = pts[(slice(None),) + ri] - pts[(slice(None),) + le]; b = pts[(slice(None),) + dn] - pts[(slice(None),) + up]
        cr = np.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
        l = np.sqrt(_dot(cr, cr))
        if ok.any():
            margins["cross"] = float(l[ok].min())
        ok &= l > 0
        with np.errstate(all="ignore"):
            nn = cr / l
        pc = pts[(slice(None),) + c]
        flip = _dot(nn, pc)
        if ok.any():
            margins["flip"] = float(np.abs(flip[ok]).min())
        nn = np.where(flip > 0, -nn, nn)
        n[(slice(None),) + c] = np.where(ok, nn, 0); nvalid[c] = ok
    return {"pts": pts, "valid": valid, "n": n, "nvalid": nvalid, "margins": margins, "W": W, "H": H}


# ---- pose arithmetic: graph_slam_amd/csrc/se3_device.hpp and pose3_device.hpp, operation for operation ----------------------------
def qmat(q):
    x, y, z, w = q
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]


def _qmul(a, b):
    return [a[3] * b[0] + b[3] * a[0] + (a[1] * b[2] - a[2] * b[1]), a[3] * b[1] + b[3] * a[1] + (a[2] * b[0] - a[0] * b[2]),
            a[3] * b[2] + b[3] * a[2] + (a[0] * b[1] - a[1] * b[0]), a[3] * b[3] - (a[0] * b[0] + a[1] * b[1] + a[2] * b[2])]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def se3_exp(xi, ft):
    w, v = list(xi[:3]), list(xi[3:])
    th2 = _dot3(w, w); th = np.sqrt(th2)
    s = ft(0.5) - th2 / ft(48.0) if th < 1e-10 else np.sin(ft(0.5) * th) / th
    q = [s * w[0], s * w[1], s * w[2], np.cos(ft(0.5) * th)]
    if th < 0.25:
        a = ft(0.5) - th2 * (ft(1.0) / ft(24.0) - th2 * (ft(1.0) / ft(720.0) - th2 * (ft(1.0) / ft(40320.0) - th2 / ft(3628800.0))))
        b = ft(1.0) / ft(6.0) - th2 * (ft(1.0) / ft(120.0) - th2 * (ft(1.0) / ft(5040.0) - th2 * (ft(1.0) / ft(362880.0) - th2 / ft(39916800.0))))
    else:
        a = (1 - np.cos(th)) / th2
        b = (th - np.sin(th)) / (th2 * th)
    c = _cross(w, v); cc = _cross(w, c)
    return [v[k] + a * c[k] + b * cc[k] for k in range(3)], q


def retract(t, q, xi, ft):
    """normalise(T Exp(xi))"""
    et, eq = se3_exp(xi, ft)
    R = qmat(q)
    t2 = [t[k] + (R[k][0] * et[0] + R[k][1] * et[1] + R[k][2] * et[2]) for k in range(3)]
    q2 = _qmul(q, eq)
    n = np.sqrt(q2[0] * q2[0] + q2[1] * q2[1] + q2[2] * q2[2] + q2[3] * q2[3])
    return t2, [c / n for c in q2]


def tree_sum(x, ft):
    """the sum of a vector by a fixed binary tree (zero-padded to a power of two, halves added element by element): the same
    additions on every machine, whatever numpy's own sums do with the vector units they find"""
    x = np.asarray(x, ft)
    if len(x) == 0:
        return ft(0)
    n = 1 << (len(x) - 1).bit_length()
    x = np.concatenate([x, np.zeros(n - len(x), ft)])
    while len(x) > 1:
        x = x[:len(x) // 2] + x[len(x) // 2:]
    return x[0]


# ---- one evaluation -----------------------------------------------------------------------------------------------------------
def _sigma2(n, p, P, ft):
    z = p[2]
    sz = ft(P["sigma_z"][0]) + z * (ft(P["sigma_z"][1]) + z * ft(P["sigma_z"][2]))
    gx = (n[0] * z) / ft(P["fx"]); gy = (n[1] * z) / ft(P["fy"])
    nr = (n[0] * (p[0] / z) + n[1] * (p[1] / z)) + n[2]
    spx = ft(P["sigma_px"])
    return (spx * spx) * (gx * gx + gy * gy) + (sz * sz) * (nr * nr)


def evaluate(src, tgt, t, q, k, P, ft=np.float64):
    """the sums of one evaluation at (t, q) on the level of stride k: a dict with H (21), g (6), chi2, ss, count, the margins and
    the source pixels (u, v) of the associations"""
    W, H = src["W"], src["H"]
    V, U = np.meshgrid(np.arange(0, H, k), np.arange(0, W, k), indexing="ij")
    u, v = U.ravel(), V.ravel()
    keep = src["valid"][v, u]
    u, v = u[keep], v[keep]
    pj = src["pts"][:, v, u]
    R = qmat([ft(c) for c in q]); t = [ft(c) for c in t]
    margins = {}

    def note(name, values):
        if len(values):
            margins[name] = min(margins.get(name, math.inf), float(np.min(values)))

    qv = np.stack([((R[c][0] * pj[0] + R[c][1] * pj[1]) + R[c][2] * pj[2]) + t[c] for c in range(3)])
    note("qz", np.abs(qv[2]))
    keep = qv[2] > 0
    u, v, pj, qv = u[keep], v[keep], pj[:, keep], qv[:, keep]
    xu = (ft(P["fx"]) * qv[0]) / qv[2] + ft(P["cx"]); xv = (ft(P["fy"]) * qv[1]) / qv[2] + ft(P["cy"])
    near = (xu >= -1) & (xu <= W) & (xv >= -1) & (xv <= H)
    for c in (xu[near], xv[near]):
        note("rint", np.abs((c - np.floor(c)) - ft(0.5)))
    ud, vd = np.rint(xu), np.rint(xv)
    keep = (ud >= 0) & (ud <= W - 1) & (vd >= 0) & (vd <= H - 1)
    u, v, pj, qv = u[keep], v[keep], pj[:, keep], qv[:, keep]
    ui, vi = ud[keep].astype(np.int64), vd[keep].astype(np.int64)
    keep = tgt["nvalid"][vi, ui]
    u, v, pj, qv, ui, vi = u[keep], v[keep], pj[:, keep], qv[:, keep], ui[keep], vi[keep]
    pi, n = tgt["pts"][:, vi, ui], tgt["n"][:, vi, ui]
    e = qv - pi
    dist = np.sqrt(_dot(e, e))
    note("max_dist", np.abs(dist - ft(P["max_dist"])))
    keep = ~(dist > ft(P["max_dist"]))
    u, v, pj, qv, pi, n, e = u[keep], v[keep], pj[:, keep], qv[:, keep], pi[:, keep], n[:, keep], e[:, keep]
    nq, lim = np.abs(_dot(n, qv)), ft(P["min_cos"]) * np.sqrt(_dot(qv, qv))
    note("min_cos", np.abs(nq - lim))
    keep = ~(nq < lim)
    u, v, pj, qv, pi, n, e = u[keep], v[keep], pj[:, keep], qv[:, keep], pi[:, keep], n[:, keep], e[:, keep]
    r = _dot(n, e)
    m = np.stack([(R[0][c] * n[0] + R[1][c] * n[1]) + R[2][c] * n[2] for c in range(3)])
    J = np.stack([pj[1] * m[2] - pj[2] * m[1], pj[2] * m[0] - pj[0] * m[2], pj[0] * m[1] - pj[1] * m[0], m[0], m[1], m[2]])
    with np.errstate(all="ignore"):
        w = ft(1.0) / (_sigma2(n, pi, P, ft) + _sigma2(m, pj, P, ft))
    Jw = w * J
    Hm = np.zeros(21, ft); g = np.zeros(6, ft)
    for a in range(6):
        for b in range(a, 6):
            Hm[ut6(a, b)] = tree_sum(Jw[a] * J[b], ft)
        g[a] = tree_sum(Jw[a] * r, ft)
    return {"H": Hm, "g": g, "chi2": tree_sum((w * r) * r, ft), "ss": tree_sum(r * r, ft), "count": len(r), "margins": margins,
            "u": u, "v": v, "r": r, "J": J, "w": w}


# ---- the solve: chol6_packed and tri6_inverse of small_dense_device.hpp, operation for operation ------------------------------
def factor(ev, P, ft=np.float64):
    """(status, min_pivot, s, M = L^-1 as a 6 x 6 lower triangle) of the normal equations of one evaluation"""
    Hm = ev["H"]
    if not (np.all(np.isfinite(Hm)) and np.all(np.isfinite(ev["g"])) and np.isfinite(ev["chi2"]) and np.isfinite(ev["ss"])):
        return NUM, 0.0, None, None
    if ev["count"] < P["min_pairs"]:
        return TOO_FEW, 0.0, None, None
    if not all(Hm[ut6(r, r)] > 0 for r in range(6)):
        return DEGENERATE, 0.0, None, None
    s = [ft(1.0) / np.sqrt(Hm[ut6(r, r)]) for r in range(6)]
    L = [[ft(0)] * 6 for _ in range(6)]
    for r in range(6):
        for c in range(r + 1):
            L[r][c] = (Hm[ut6(c, r)] * s[c]) * s[r]
    piv = []
    for j in range(6):
        d = L[j][j]
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        piv.append(d)
        okj = bool(d > 0 and np.isfinite(d))
        l = np.sqrt(d if okj else ft(1.0))
        L[j][j] = l
        for i in range(j + 1, 6):
            a = L[i][j]
            for k in range(j):
                a = a - L[i][k] * L[j][k]
            L[i][j] = a / l
    if any(d != d for d in piv):
        return DEGENERATE, 0.0, None, None
    mp = min(piv)
    if not mp >= P["min_pivot"]:
        return DEGENERATE, float(mp), None, None
    M = [[ft(0)] * 6 for _ in range(6)]
    for c in range(6):
        M[c][c] = ft(1.0) / L[c][c]
        for r in range(c + 1, 6):
            a = ft(0)
            for k in range(c, r):
                a = a + L[r][k] * M[k][c]
            M[r][c] = -a / L[r][r]
    return OK, mp, s, M


def step(ev, s, M, ft=np.float64):
    g = ev["g"]
    y = []
    for r in range(6):
        a = ft(0)
        for c in range(r + 1):
            a = a + M[r][c] * (s[c] * g[c])
        y.append(a)
    d = []
    for c in range(6):
        a = ft(0)
        for r in range(c, 6):
            a = a + M[r][c] * y[r]
        d.append(s[c] * a)
    return d


def covariance(s, M, ft=np.float64):
    cov = np.zeros((6, 6), ft)
    for r in range(6):
        for c in range(r, 6):
            a = ft(0)
            for k in range(c, 6):
                a = a + M[k][r] * M[k][c]
            cov[r, c] = cov[c, r] = (a * s[r]) * s[c]
    return cov


# ---- the whole call for one pair ------------------------------------------------------------------------------------------------
def _merge(into, m):
    for k, v in m.items():
        into[k] = min(into.get(k, math.inf), v)


def align(depth_i, depth_j, pose0=None, P=None, ft=np.float64):
    """fgo_depth_align_batch for one pair.  Returns a dict: pose_ij (7), info (21), cov (6 x 6), status, n_pairs_used, iterations,
    converged, rmse, chi2, min_pivot, normal_eq (28: the first evaluation), margins (the smallest of every kind over the frames,
    the evaluations and the solves) and evaluations (how many were made)."""
    P = P or default_params()
    src, tgt = frame(depth_j, P, ft), frame(depth_i, P, ft)
    margins = {}
    _merge(margins, {"z_range": min(src["margins"]["z_range"], tgt["margins"]["z_range"])})
    _merge(margins, {k: v for k, v in tgt["margins"].items() if k != "z_range"})
    if pose0 is None:
        t, q = [ft(0)] * 3, [ft(0), ft(0), ft(0), ft(1)]
    else:
        p = [ft(c) for c in pose0]
        n = np.sqrt(p[3] * p[3] + p[4] * p[4] + p[5] * p[5] + p[6] * p[6])
        t, q = p[:3], [c / n for c in p[3:]]
    status, steps, conv, neq, n_eval, mp, ev = OK, 0, 0, None, 0, 0.0, None

    def solve_here():
        nonlocal ev, neq, n_eval
        ev = evaluate(src, tgt, t, q, P["skip"][l], P, ft)
        n_eval += 1
        _merge(margins, ev["margins"])
        if neq is None:
            neq = np.concatenate([ev["H"], ev["g"], [ev["chi2"]]])
        st, piv, s, M = factor(ev, P, ft)
        if st in (OK, DEGENERATE) and P["min_pivot"] > 0 and ev["count"] >= P["min_pairs"] and np.isfinite(piv):
            _merge(margins, {"pivot_rel": abs(float(piv) / P["min_pivot"] - 1)})
        return st, piv, s, M

    for l in range(P["n_levels"]):
        conv = 0
        for _ in range(P["iters"][l]):
            status, mp, s, M = solve_here()
            if status != OK:
                break
            d = step(ev, s, M, ft)
            nw, nv = np.sqrt(_dot(d[:3], d[:3])), np.sqrt(_dot(d[3:], d[3:]))
            for nrm, eps in ((nw, P["eps_rot"]), (nv, P["eps_trans"])):
                if eps > 0:
                    _merge(margins, {"eps_rel": abs(float(nrm) / eps - 1)})
            conv = int(nw < P["eps_rot"] and nv < P["eps_trans"])
            t, q = retract(t, q, [-c for c in d], ft)
            if not np.all(np.isfinite(np.array(t + q, ft))):
                status = NUM
                break
            steps += 1
            if conv:
                break
        if status != OK:
            break
    if status == OK:
        l = P["n_levels"] - 1
        status, mp, s, M = solve_here()
    out = {"status": status, "n_pairs_used": ev["count"], "iterations": steps, "min_pivot": mp, "normal_eq": neq, "margins": margins,
           "evaluations": n_eval}
    if status == OK:
        sg = -1 if q[3] < 0 else 1
        out.update(pose_ij=np.array(t + [sg * c for c in q], ft), info=ev["H"].copy(), cov=covariance(s, M, ft), converged=conv,
                   rmse=np.sqrt(ev["ss"] / ft(ev["count"])), chi2=ev["chi2"])
    else:
        info = np.zeros(21, ft)
        for r in range(6):
            info[ut6(r, r)] = 10000.0
        out.update(pose_ij=np.array([0, 0, 0, 0, 0, 0, 1], ft), info=info, cov=np.zeros((6, 6), ft), converged=0, rmse=ft(0), chi2=ft(0))
    return out


# ---- scenes: a three-wall corner by analytic ray-plane intersection --------------------------------------------------------------
CORNER = ((np.array([1.0, 0.0, 0.0]), 1.5), (np.array([0.0, 1.0, 0.0]), 1.0), (np.array([0.0, 0.0, 1.0]), 3.0))   # n . X = h


def rot(axis, deg):
    a = np.asarray(axis, float); a = a / np.linalg.norm(a)
    th = math.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def camera(yaw=25.0, pitch=15.0, roll=0.0, pos=(0.0, 0.0, 0.0)):
    """(R, t) camera to world: x right, y down, z forward; yaw to the right, pitch downwards"""
    return rot((0, 1, 0), yaw) @ rot((1, 0, 0), -pitch) @ rot((0, 0, 1), roll), np.asarray(pos, float)


def render(cam, P, W, H, planes=CORNER):
    """the depth words of the planes seen from cam: the nearest intersection in front of the camera, z rounded to the word"""
    R, t = cam
    u, v = np.meshgrid(np.arange(W, dtype=float), np.arange(H, dtype=float))
    dc = np.stack([(u - P["cx"]) / P["fx"], (v - P["cy"]) / P["fy"], np.ones_like(u)])
    dw = np.tensordot(R, dc, 1)
    z = np.full((H, W), np.inf)
    for n, h in planes:
        with np.errstate(all="ignore"):
            lam = (h - n @ t) / np.tensordot(n, dw, 1)
        z = np.where((lam > 0) & (lam < z), lam, z)
    words = np.rint(z / P["z_scale"])
    return np.where(np.isfinite(words) & (words < 65535), words, 0).astype(np.uint16)


def relative_pose(cam_i, cam_j):
    """pose_ij (7): p_i = R p_j + t with the quaternion x y z w, w >= 0"""
    Ri, ti = cam_i; Rj, tj = cam_j
    R = Ri.T @ Rj; t = Ri.T @ (tj - ti)
    w = 0.5 * math.sqrt(max(1 + np.trace(R), 0))                       # small rotations only: w is far from 0
    q = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / (4 * w)
    return np.concatenate([t, q, [w]])


def pose_error(a, b):
    """(translation difference in m, rotation angle between the two in rad)"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    d = abs(float(a[3:] @ b[3:])) / (np.linalg.norm(a[3:]) * np.linalg.norm(b[3:]))
    cross = np.linalg.norm(a[6] * b[3:6] - b[6] * a[3:6] - np.cross(a[3:6], b[3:6])) / (np.linalg.norm(a[3:]) * np.linalg.norm(b[3:]))
    return float(np.linalg.norm(a[:3] - b[:3])), 2 * math.atan2(cross, d)


def small_params(**kw):
    """the parameters of the 40 x 30 scenes: the intrinsics scaled from 176 x 144, every pixel sampled on the finer levels; a
    pixel is 4.4 times as wide there, so the two gates in metres are opened to match"""
    base = dict(fx=57.0, fy=57.0, cx=20.0, cy=15.0, skip=(2, 1, 1), min_pairs=60, normal_jump=0.1505, max_dist=0.1503)
    base.update(kw)
    return default_params(**base)


# ---- the scenes of the tests ------------------------------------------------------------------------------------------------
# Chosen (by seed) so that every gate margin of this file exceeds 1e-6 at every evaluation of every pair below, in f64 and in
# longdouble: tests/test_depth_align_reference_cpu.py asserts it.  If a change to the semantics moves a sample onto a gate, another
# seed is chosen here; the tests stay as they are.
SCENE_SEEDS = {"big": (3, 4, 10, 12), "small": (1, 13, 8, 11)}
MARGIN, MARGIN_REL = 1e-6, 1e-3


def nearby_camera(seed):
    """a camera about 3 degrees (mostly roll; the yaw and pitch are offset by the translation, so that the scene moves by less
    than max_dist) and 2 to 5 cm from camera()"""
    r = np.random.default_rng(seed)
    yaw, pitch = r.uniform(-1.3, 1.3), r.uniform(-1.0, 1.0)
    roll = r.choice([-1, 1]) * r.uniform(2.3, 2.7)
    pos = (0.035 * yaw + r.uniform(-.01, .01), -0.03 * pitch + r.uniform(-.01, .01), r.uniform(-0.03, 0.03))
    return camera(yaw=25 + yaw, pitch=15 + pitch, roll=roll, pos=pos)


_SCENES = {}


def scene(kind):
    """{P, W, H, depth (5 frames), frame_i, frame_j (8 pairs: frame 0 against each other frame, both ways), truth (8 x 7)} of the
    176 x 144 ("big") or the 40 x 30 ("small") corner scene; built once"""
    if kind not in _SCENES:
        P, W, H = (default_params(normal_jump=0.0505), 176, 144) if kind == "big" else (small_params(), 40, 30)
        cams = [camera()] + [nearby_camera(s) for s in SCENE_SEEDS[kind]]
        fi = [0, 1, 0, 2, 0, 3, 0, 4]; fj = [1, 0, 2, 0, 3, 0, 4, 0]
        _SCENES[kind] = {"P": P, "W": W, "H": H, "depth": np.stack([render(c, P, W, H) for c in cams]), "frame_i": np.array(fi),
                         "frame_j": np.array(fj), "truth": np.stack([relative_pose(cams[a], cams[b]) for a, b in zip(fi, fj)])}
    return _SCENES[kind]


_RUNS = {}


def scene_run(kind, pair, ft=np.float64):
    """align() of one pair of a scene from the identity; computed once and shared"""
    key = (kind, pair, ft)
    if key not in _RUNS:
        S = scene(kind)
        _RUNS[key] = align(S["depth"][S["frame_i"][pair]], S["depth"][S["frame_j"][pair]], None, S["P"], ft)
    return _RUNS[key]


def rel_diff(a, b):
    """max |a - b| / max |b|, as a float: the norm-wise relative difference of two blocks"""
    a, b = np.asarray(a, np.longdouble), np.asarray(b, np.longdouble)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def params_struct(P):
    """the dict as the ctypes structure of graph_slam_amd.dense"""
    from graph_slam_amd import dense
    return dense.depth_align_params(**P)


# The f64-against-longdouble difference of this file over the 16 pairs above, norm-wise (rel_diff; the pose absolutely): the
# largest value met, rounded up in the second digit.  tests/test_depth_align_reference_cpu.py holds every pair inside it, and
# tests/test_gpu_depth_align.py allows the kernel YARDSTICK_FACTOR times as much against the f64 run.
YARDSTICK = {"H": 4.2e-16, "g": 5.5e-15, "chi2": 3.3e-15, "pose": 2.8e-16, "info": 2.4e-16}
YARDSTICK_FACTOR = 16


def truth_bound(kind):
    """(metres, radians): twice the largest error of this file's own result against the ground truth over the pairs of a scene --
    depth quantisation and nothing else"""
    errs = [pose_error(scene_run(kind, p)["pose_ij"], scene(kind)["truth"][p]) for p in range(8)]
    return 2 * max(e[0] for e in errs), 2 * max(e[1] for e in errs)
