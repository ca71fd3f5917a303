"""numpy restatement of the IMU check of visual-odometry records (include/fgo.h fgo_imu_check_vro_batch; the reference's
gtsam/test_vro_imu_graph.cpp:679-778), written for reading, not for speed, from the definitions: rotations are 3x3 matrices, every
inverse is numpy.linalg.inv, none of the kernel's factorisations or quaternion arithmetic is used.  It also holds the generator of
records the tests share.  tests/test_imu_check_reference_cpu.py holds this restatement to central differences, to a 40-digit matrix
logarithm and to the chi-square law; tests/test_gpu_imu_check.py then holds the kernel to it.

Conventions: a pose is t(3) q_xyzw(4) in the camera frame; a preintegration is the 287 doubles of fgo_preint (dt, dR 1..4,
dp 5..7, dv 8..10, J_R_bg 11..19, J_p_ba, J_p_bg, J_v_ba, J_v_bg, bhat 56..61, cov 62..286); a bias is acc(3), gyro(3); every
perturbation of a rotation is a right perturbation, R Exp(d)."""
import numpy as np

import graph_slam_amd as G

D2_GATE = 7.814727903251179           # the 95 % quantile of chi-square with 3 degrees of freedom
D2_REF_GATE = 40000.0
FAILED_INFO00 = 10000.0
IC_OK, IC_SKIPPED, IC_NUM = 0, 1, 2
DR, JRBG, BHAT, COV = slice(1, 5), slice(11, 20), slice(56, 62), slice(62, 287)
_UT = np.triu_indices(6)


def info_full(ut21):
    A = np.zeros((6, 6)); A[_UT] = ut21
    return A + np.triu(A, 1).T


def info_ut21(A):
    return np.asarray(A, np.float64)[_UT].copy()


def sentinel_info(ut21):
    """the information scaled so that entry (0, 0) is exactly the failed-VO sentinel; it stays positive definite"""
    A = info_full(ut21)
    A *= FAILED_INFO00 / A[0, 0]
    A[0, 0] = FAILED_INFO00
    return info_ut21(A)


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def qmat(q):
    x, y, z, w = np.asarray(q, np.float64) / np.sqrt(np.dot(q, q))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _sinc(x):
    return np.sinc(x / np.pi)                                   # sin(x) / x, 1 at 0


def rot_exp(w):
    """Rodrigues: I + (sin th / th) W + (1 - cos th) / th^2 W^2, the second coefficient as sinc^2(th / 2) / 2"""
    w = np.asarray(w, np.float64); th = np.sqrt(w @ w); W = skew(w)
    return np.eye(3) + _sinc(th) * W + 0.5 * _sinc(0.5 * th) ** 2 * W @ W


def rot_log(R):
    """the rotation vector of R (angle in [0, pi)): the axis from the antisymmetric part, the angle by atan2 of both parts"""
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])       # sin(th) axis
    s = np.sqrt(v @ v)
    return v * (np.arctan2(s, 0.5 * (np.trace(R) - 1.0)) / s) if s > 1e-300 else v


def right_jacobian(w):
    """Jr = I - a W + b W^2, a = (1 - cos th) / th^2, b = (th - sin th) / th^3:  Exp(w + d) = Exp(w) Exp(Jr d)"""
    w = np.asarray(w, np.float64); th = np.sqrt(w @ w); W = skew(w)
    b = (th - np.sin(th)) / th ** 3 if th > 1e-2 else 1.0 / 6.0 - th * th / 120.0 + th ** 4 / 5040.0
    return np.eye(3) - 0.5 * _sinc(0.5 * th) ** 2 * W + b * W @ W


def dlog(w):
    """the derivative of Log(R Exp(d)) by d at d = 0, w = Log(R): the inverse of the right Jacobian"""
    return np.linalg.inv(right_jacobian(w))


def _is_pd(A):
    if not np.all(np.isfinite(A)):
        return False
    try:
        np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return False
    return True


def rotations(pose, pre, bias_i=None, imu_q_cam=None):
    """dR_imu and dR_vro (:692-710)"""
    pre = np.asarray(pre, np.float64)
    dbg = np.zeros(3) if bias_i is None else np.asarray(bias_i, np.float64)[3:] - pre[BHAT][3:]
    R_imu = qmat(pre[DR]) @ rot_exp(pre[JRBG].reshape(3, 3) @ dbg)
    R_uc = np.eye(3) if imu_q_cam is None else qmat(imu_q_cam)
    return R_imu, R_uc @ qmat(np.asarray(pose, np.float64)[3:]) @ R_uc.T, R_uc


def residual(R_imu, R_vro, jac=False):
    """dw = Log(dR_imu^T dR_vro) with J_imu = d dw / d dR_imu and J_vro = d dw / d dR_vro (right perturbations)"""
    Rw = R_imu.T @ R_vro
    dw = rot_log(Rw)
    if not jac:
        return dw
    D = dlog(dw)
    return dw, -D @ Rw.T, D


def check_record(pose, pre, info=None, cov=None, bias_i=None, imu_q_cam=None, d2_gate=D2_GATE, d2_ref_gate=D2_REF_GATE,
                 failed_info00=FAILED_INFO00, conds=True):
    """One record: what the entry point returns for it, the pieces (J_imu, J_vro, Lth), and cond_S / cond_info / cond_cov15 for
    the tolerances (conds=False leaves the three at 1)."""
    out = dict(status=IC_OK, reject=0, d2=0.0, d2_ref=0.0, angle=0.0, dw=np.zeros(3), cov_dw=np.zeros((3, 3)), cond_S=1.0,
               cond_info=1.0, cond_cov15=1.0)
    assert (info is None) != (cov is None)
    pre = np.asarray(pre, np.float64)
    if cov is not None:
        C = np.asarray(cov, np.float64).reshape(6, 6)[:3, :3]
        Sww = np.triu(C) + np.triu(C, 1).T                      # the upper triangle is what is read
    else:
        A = info_full(info)
        if failed_info00 > 0 and A[0, 0] == failed_info00:
            out["status"] = IC_SKIPPED
            return out
        if not _is_pd(A):
            out["status"] = IC_NUM
            return out
        Sww = np.linalg.inv(A)[:3, :3]
        if conds:
            out["cond_info"] = float(np.linalg.cond(A))
    C15 = pre[COV].reshape(15, 15)
    C15 = 0.5 * (C15 + C15.T)
    if not _is_pd(C15):
        out["status"] = IC_NUM
        return out
    R_imu, R_vro, R_uc = rotations(pose, pre, bias_i, imu_q_cam)
    dw, J_imu, J_vro = residual(R_imu, R_vro, True)
    S = J_imu @ C15[:3, :3] @ J_imu.T + J_vro @ (R_uc @ Sww @ R_uc.T) @ J_vro.T
    S = 0.5 * (S + S.T)
    if not _is_pd(S):
        out["status"] = IC_NUM
        return out
    Lth = np.linalg.inv(C15)[:3, :3]
    d2 = float(dw @ np.linalg.inv(S) @ dw)
    d2_ref = float(dw @ (J_imu @ Lth @ J_imu.T) @ dw)
    out.update(d2=d2, d2_ref=d2_ref, angle=float(np.sqrt(dw @ dw)), dw=dw, cov_dw=S, J_imu=J_imu, J_vro=J_vro, Lth=Lth,
               reject=int(d2 > d2_gate) | (int(d2_ref > d2_ref_gate) << 1))
    if conds:
        out.update(cond_S=float(np.linalg.cond(S)), cond_cov15=float(np.linalg.cond(C15)))
    return out


# ---- the generator

def qmul(a, b):
    ax, ay, az, aw = a; bx, by, bz, bw = b
    return np.array([aw * bx + bw * ax + ay * bz - az * by, aw * by + bw * ay + az * bx - ax * bz,
                     aw * bz + bw * az + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def qconj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def qexp(w):
    w = np.asarray(w, np.float64); th = np.sqrt(w @ w)
    return np.append(0.5 * _sinc(0.5 * th) * w, np.cos(0.5 * th))


def random_unit(rng, k=3):
    v = rng.normal(size=k)
    return v / np.sqrt(v @ v)


def make_preint(rng, n_samples, bias_hat=None, dt=0.005):
    """a preintegration of n_samples IMU samples (fgo_imu_params_vn100; acc ~ N((0, 0, 9.7), 1), gyro ~ N(0, 0.3)), integrated on
    the host by fgo_preint_integrate"""
    p = G.Preintegrator(bias_hat=bias_hat)
    for _ in range(n_samples):
        p.integrate(np.array([0, 0, 9.7]) + rng.normal(size=3), 0.3 * rng.normal(size=3), dt)
    return p.buf.copy()


def random_rot_cov(rng, scale=1e-5):
    A = rng.normal(size=(3, 3))
    return scale * A @ A.T


def pose_cov(rng, Sww):
    """a 6x6 pose covariance (tangent [omega; v]) with the given rotation block and random, correlated other blocks"""
    A = rng.normal(size=(6, 6))
    M = A @ A.T / 6 + 0.5 * np.eye(6)
    L = np.linalg.cholesky(Sww)
    T = np.eye(6); T[:3, :3] = L @ np.linalg.inv(np.linalg.cholesky(M[:3, :3])); T[3:, 3:] *= 0.01
    S = T @ M @ T.T
    return 0.5 * (S + S.T)


def record_pose(pre, perturb, bias_i=None, imu_q_cam=None, t=(0.0, 0.0, 0.0)):
    """the camera-frame pose whose rotation, carried into the IMU frame, is dR_imu Exp(perturb): q_ij = q_uc^-1 q_imu q(perturb) q_uc"""
    pre = np.asarray(pre, np.float64)
    q = pre[DR] / np.sqrt(pre[DR] @ pre[DR])
    if bias_i is not None:
        q = qmul(q, qexp(pre[JRBG].reshape(3, 3) @ (np.asarray(bias_i, np.float64)[3:] - pre[BHAT][3:])))
    q = qmul(q, qexp(perturb))
    if imu_q_cam is not None:
        u = np.asarray(imu_q_cam, np.float64) / np.sqrt(np.dot(imu_q_cam, imu_q_cam))
        q = qmul(qmul(qconj(u), q), u)
    return np.concatenate([np.asarray(t, np.float64), q])


def draw_record(rng, pres, k, angle, with_bias, scale=1e-5, configs=((None, False),), gates=(D2_GATE, D2_REF_GATE)):
    """A record on preintegration k: the rotation it reports differs from the preintegrated one by `angle` about a random axis.
    The extrinsic belongs to a call and so does the presence of a bias array, hence a record keeps the perturbation and its pose
    is derived per configuration (q_uc, use_bias) by record_args.  Redrawn while, under any of `configs`, d2 or d2_ref lies
    within relative 1e-6 of its gate, so that no reject bit sits within rounding of a threshold."""
    while True:
        bias = None
        if with_bias:
            bias = pres[k][BHAT] + np.concatenate([1e-2 * rng.normal(size=3), 1e-3 * rng.normal(size=3)])
        S = pose_cov(rng, random_rot_cov(rng, scale))
        r = dict(k=k, perturb=angle * random_unit(rng), bias=bias, t=rng.uniform(-0.3, 0.3, 3), cov=S, info=info_ut21(np.linalg.inv(S)))
        ws = [check_record(cov=S, conds=False, **record_args(r, pres, *c)) for c in configs]
        if all(w["status"] != IC_OK or all(abs(w[f] - g) > 1e-6 * g for f, g in zip(("d2", "d2_ref"), gates)) for w in ws):
            return r


def record_args(r, pres, q_uc=None, use_bias=False):
    """pose, pre, bias_i, imu_q_cam of a record in a call with the extrinsic q_uc (or none) and with a bias array (or none): in a
    call with a bias array a record without a bias of its own passes the preintegration's bhat"""
    pre = pres[r["k"]]
    bias = (pre[BHAT].copy() if r["bias"] is None else r["bias"]) if use_bias else None
    pose = r["pose"] if "pose" in r else record_pose(pre, r["perturb"], bias, q_uc, r["t"])
    return dict(pose=pose, pre=pre, bias_i=bias, imu_q_cam=q_uc)


def pack(records, pres, q_uc=None, use_bias=False):
    """the arrays of one call: pose (n x 7), info (n x 21), cov (n x 6 x 6), index (n), bias (n x 6 or None)"""
    args = [record_args(r, pres, q_uc, use_bias) for r in records]
    return dict(pose=np.array([a["pose"] for a in args]).reshape(-1, 7), info=np.array([r["info"] for r in records]).reshape(-1, 21),
                cov=np.array([r["cov"] for r in records]).reshape(-1, 6, 6), index=np.array([r["k"] for r in records], np.int64),
                bias=np.array([a["bias_i"] for a in args]).reshape(-1, 6) if use_bias else None)
