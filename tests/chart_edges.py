"""Edge inputs for the manifold arithmetic and 40-digit references for them -- CHECKER SIDE ONLY.

The GTSAM-semantics code (csrc/pose3_device.hpp, imu_device.hpp, factors_device.hpp, preint_kernel.hip, imu_preint.cpp and its restatement in
oracle/orc_pose3.h, orc_imu.h, orc_plane.h) switches between a series and a closed form at small angles.  The oracle repeats those switches, so
parity with it cannot see an error in them.  This module holds

  * ONE deterministic generator of inputs at, around and far below every switch (ANGLES: exactly 0, 1e-12 ... 1 in half decades, 0.9 x and
    1.1 x each threshold, pi - {1e-1, 1e-2, 1e-3}; generic and coordinate axes; translation parts 0, 1e-3, 1, 5; plane normals on the axes,
    on ties of two and three components and a hair off them; depths on both sides of zero), shared by tests/test_chart_edges_cpu.py (oracle)
    and tests/test_gpu_chart_edges.py (device), and
  * references that share no formula with product or oracle, all in mpmath at 40 digits:
      - Pose3 between / prior: the residual is mpmath's MATRIX logarithm (tests/pose3_independent.py); the Jacobian comes from differentiating
        the MATRIX EXPONENTIAL: with r(d) = Log(M(d)), Exp(r(d)) = M(d), so (dExp/dr) J = dM/dd, where dExp/dr is a central difference of
        mpmath's expm (step 1e-12: truncation 1e-24) and dM/dd at d = 0 is M times the twist matrix of a unit vector (the first-order term of
        the exponential series).  One logarithm and twelve exponentials per factor instead of twenty-five logarithms; held to the
        all-differences route of tests/pose3_independent.py in tests/test_chart_edges_cpu.py.
      - SO(3) right Jacobian: R^T dR/dw by central differences of expm.
      - sphere chart of OrientedPlane3: local coordinates from the matrix logarithm of the rotation about n x y that takes n to y, retract
        from the matrix exponential; plane factor Jacobians by central differences of transform() in the chart at the prediction.
      - preintegration from its definition: R <- R Exp((w - bg) dt), p <- p + v dt + R (a - ba) dt^2 / 2, v <- v + R (a - ba) dt, bias
        Jacobians by central differences with respect to the bias.
"""
import functools

import mpmath as mp
import numpy as np

from tests import pose3_independent as p3
from tests.util import pose_mul, pose_inv

mp.mp.dps = 40

# ---------------------------------------------------------------------------------------------------------------- inputs
# 1e-10: so3_exp / so3_log;  1e-5: where so3_dlog / se3_dlog / so3_dexp switched before the series were extended;  0.25: where they switch now
THRESHOLDS = (1e-10, 1e-5, 0.25)
SWEEP = [10.0 ** (-12 + 0.5 * k) for k in range(25)]                       # 1e-12 ... 1
BRACKETS = [f * t for t in THRESHOLDS for f in (0.9, 1.1)]
NEAR_PI = [np.pi - d for d in (1e-1, 1e-2, 1e-3)]
ANGLES = [0.0] + SWEEP + BRACKETS + NEAR_PI
AXES = [np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0), np.array([-2.0, 1.0, 0.5]) / np.sqrt(5.25),
        np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.array([0, 0, 1.0])]
TRANS = [0.0, 1e-3, 1.0, 5.0]
IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])


def is_near_pi(angle):
    return angle > 3.0


def _rng_pose(rng, scale):
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    return np.concatenate([rng.uniform(-scale, scale, size=3), q])


def _offset(angle, axis, size, tdir):
    return np.concatenate([size * tdir, axis * np.sin(0.5 * angle), [np.cos(0.5 * angle)]])


@functools.lru_cache(maxsize=None)
def pose_cases():
    """(name, angle, xi, xj, z): BetweenFactor inputs whose residual Log(z^-1 xi^-1 xj) has rotation angle `angle` about one of AXES and a
    translation of one of TRANS.  Sizes and axes cycle over the plain sweep; 0, the brackets, the angles towards pi and 3e-5 ... 3e-3 get all
    four sizes.  Poses are generic except for
    the first case of all, which is three identities: a residual of exactly zero."""
    rng = np.random.default_rng(20260)
    out = [("identity", 0.0, IDENT.copy(), IDENT.copy(), IDENT.copy())]
    k = 0
    for angle in ANGLES:
        # all four sizes at 0, at the brackets, near pi and over 3e-5 ... 3e-3, where a closed form of se3_dlog that is kept down to 1e-5
        # cancels (eps |v| / theta^2): the errors of the chart scale with the translation
        full = angle == 0.0 or angle in BRACKETS or angle in NEAR_PI or 3e-5 < angle < 4e-3
        for size in (TRANS if full else [TRANS[k % 4]]):
            axis = AXES[k % len(AXES)]
            tdir = rng.normal(size=3); tdir /= np.linalg.norm(tdir)
            xi, xj = _rng_pose(rng, 2.0), _rng_pose(rng, 2.0)
            if k % 3 == 0:
                xi = IDENT.copy()                                # then z^-1 xi^-1 xj is formed without rounding in the rotation
            off = _offset(angle, axis, size, tdir)               # residual = Log(off)
            z = pose_mul(pose_mul(pose_inv(xi), xj), pose_inv(off))
            out.append(("a%.3g_t%g_ax%d" % (angle, size, k % len(AXES)), angle, xi, xj, z))
            k += 1
    return out


@functools.lru_cache(maxsize=None)
def prior_cases():
    """(name, angle, x, mean): PriorFactor inputs, residual Log(mean^-1 x); the first has mean == x bit for bit"""
    rng = np.random.default_rng(20261)
    x0 = _rng_pose(rng, 2.0)
    out = [("mean_is_x", 0.0, x0, x0.copy())]
    k = 1
    for angle in [0.0] + SWEEP[::2] + BRACKETS + NEAR_PI:
        axis = AXES[k % len(AXES)]
        tdir = rng.normal(size=3); tdir /= np.linalg.norm(tdir)
        x = _rng_pose(rng, 2.0)
        mean = pose_mul(x, pose_inv(_offset(angle, axis, TRANS[k % 4], tdir)))
        out.append(("a%.3g_t%g" % (angle, TRANS[k % 4]), angle, x, mean))
        k += 1
    return out


@functools.lru_cache(maxsize=None)
def retract_cases():
    """(name, x, d): steps [omega; v] with the rotation part swept (no near-pi: a step is small) and an O(1) translation part among others"""
    rng = np.random.default_rng(20262)
    out = []
    k = 0
    for angle in [0.0] + SWEEP + BRACKETS:
        for size in ([1.0, TRANS[k % 4]] if angle < 1e-3 else [TRANS[k % 4]]):
            axis = AXES[k % len(AXES)]
            tdir = rng.normal(size=3); tdir /= np.linalg.norm(tdir)
            out.append(("a%.3g_t%g" % (angle, size), _rng_pose(rng, 2.0), np.concatenate([angle * axis, size * tdir])))
            k += 1
    return out


def dexp_cases():
    """rotation vectors for the SO(3) right Jacobian (the preintegrator's gyro x dt and the IMU factor's bias-correction angle)"""
    return [(angle, angle * AXES[k % len(AXES)]) for k, angle in enumerate([0.0] + SWEEP + BRACKETS + NEAR_PI)]


def _unit(v):
    v = np.asarray(v, float)
    return v / np.linalg.norm(v)


# normals: on the axes, ties of two and of three components (unit3_basis breaks them x, then y, then z), a hair off each tie, one generic
NORMALS = [_unit(v) for v in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 0], [0, 1, 1], [1, 0, 1], [1, 1, 1], [-1, 1, -1],
                              [1, 1 + 1e-15, 0.3], [1 + 1e-15, 1, 0.3], [1, 1, 1 + 1e-15], [1, 1 - 1e-15, 1], [2, 1, 1], [0.3, -0.5, 0.8])]
PLANE_ANGLES = [0.0] + [10.0 ** e for e in range(-12, 0)] + [1.5e-8, 3e-8, 0.9e-15, 1.1e-15] + [np.pi - 1e-3]      # 1e-15: unit3_local's cut-off; the last: near antipodal
PLANE_STEPS = [0.0, 0.9e-300, 1e-300, 1.1e-300] + [10.0 ** e for e in range(-12, 1)]      # 1e-300: unit3_retract's switch


def _tilt(n, angle, phi):
    """unit vector at `angle` from n (in float: the tests read the angle back from the vectors, not from here)"""
    a = np.cross(n, [0.3, -0.7, 0.6]); a /= np.linalg.norm(a)
    b = np.cross(n, a)
    y = np.cos(angle) * n + np.sin(angle) * (np.cos(phi) * a + np.sin(phi) * b)
    return y if angle == 0.0 else y / np.linalg.norm(y)


@functools.lru_cache(maxsize=None)
def unit3_cases():
    """(n, y): every plane angle at a cycling normal, and every normal at one tiny and one moderate angle"""
    out = []
    for k, ang in enumerate(PLANE_ANGLES):
        n = NORMALS[k % len(NORMALS)]
        out.append((n, _tilt(n, ang, 0.7 * k)))
    for k, n in enumerate(NORMALS):
        out.append((n, _tilt(n, 1e-7, 0.9 * k))); out.append((n, _tilt(n, 0.3, 0.9 * k)))
    return out


@functools.lru_cache(maxsize=None)
def plane_retract_cases():
    """(plane abcd, v[3])"""
    out = []
    for k, s in enumerate(PLANE_STEPS):
        n = NORMALS[k % len(NORMALS)]
        out.append((np.concatenate([n, [0.5 + k]]), np.array([s * np.cos(1.1 * k), s * np.sin(1.1 * k), 0.25 * s])))
    for k, n in enumerate(NORMALS):
        out.append((np.concatenate([n, [-1.0]]), np.array([0.2, -0.1, 0.05])))
    return out


@functools.lru_cache(maxsize=None)
def plane_factor_cases():
    """(x, plane abcd (world), z abcd (pose frame)): the measured normal at PLANE_ANGLES from the predicted one; the pose is the identity for the
    axis-aligned normals (walls and floors seen from an axis-aligned pose keep their ties), generic otherwise"""
    rng = np.random.default_rng(20263)
    out = []
    for k, ang in enumerate(PLANE_ANGLES + [1e-7, 0.3] * 4):
        n = NORMALS[(3 * k) % len(NORMALS)]
        x = np.concatenate([rng.uniform(-2, 2, size=3), [0, 0, 0, 1.0]]) if k % 2 == 0 else _rng_pose(rng, 2.0)
        d = rng.uniform(-1, 1)
        R = np.array([[float(v) for v in row] for row in p3.pose_mat(x)[0:3, 0:3].tolist()])
        npred = R.T @ n
        z = np.concatenate([_tilt(npred, ang, 0.5 * k), [n @ x[:3] + d + (0.0 if ang == 0.0 else 0.01)]])
        out.append((x, np.concatenate([n, [d]]), z))
    return out


def reproj_cases(calib, bps_list):
    """(x, point, uv, bps, depth): depth q.z in +-{1e-6, 1e-3, 1}; the pixel at the principal point for every other case"""
    from tests.util import quat_rot
    rng = np.random.default_rng(20264)
    out = []
    k = 0
    for bps in bps_list:
        for depth in (1e-6, 1e-3, 1.0, -1e-6, -1e-3, -1.0):
            for centre in (True, False):
                x = _rng_pose(rng, 1.0)
                c = pose_mul(x, bps)
                # lateral offset proportional to the depth: the normalised coordinates stay O(0.1), as for a point in the field of view
                local = np.array([0.0, 0.0, depth]) if centre else np.array([0.13 * abs(depth), -0.07 * abs(depth), depth])
                uv = np.array([calib[3], calib[4]]) if centre else rng.uniform(0, 180, size=2)
                out.append((x, c[:3] + quat_rot(c[3:], local), uv, bps, depth))
                k += 1
    return out


# ------------------------------------------------------------------------------------------------------------ references
def _f(M):
    return np.array([[float(M[r, c]) for c in range(M.cols)] for r in range(M.rows)])


def rotmat(q):
    """float rotation matrix of a quaternion x y z w, through the 40-digit pose_mat"""
    return _f(p3.pose_mat(np.r_[0.0, 0.0, 0.0, np.asarray(q, float)])[0:3, 0:3])


def _unit_twists():
    return [p3.hat([mp.mpf(int(j == k)) for j in range(6)]) for k in range(6)]


def _dexp_se3(r, h=mp.mpf("1e-12")):
    """d vec(top 3 x 4 of Exp(r)) / d r: 12 x 6, central differences of mpmath's matrix exponential"""
    A = mp.zeros(12, 6)
    for k in range(6):
        rp = list(r); rm = list(r)
        rp[k] = rp[k] + h; rm[k] = rm[k] - h
        D = (mp.expm(p3.hat(rp)) - mp.expm(p3.hat(rm))) / (2 * h)
        for i in range(3):
            for j in range(4):
                A[4 * i + j, k] = D[i, j]
    return A


def _vec34(M):
    return mp.matrix([M[i, j] for i in range(3) for j in range(4)])


def _log_se3(M):
    """the real logarithm with rotation angle below pi, and the pseudo-inverse N of dExp/dr there.  mpmath's logm is used where it returns that
    branch; within a few degrees of pi it returns a complex logarithm instead (also a logarithm, but not the chart's), and then the equation
    Exp(r) = M is solved by Newton's method on mpmath's expm from scipy's double-precision logarithm (quadratic: 1e-15, 1e-30, 1e-60)."""
    L = mp.logm(M)
    if max(abs(mp.im(L[i, j])) for i in range(3) for j in range(4)) < mp.mpf("1e-25"):
        r = [mp.re(x) for x in p3.vee(L)]
        A = _dexp_se3(r)
        return r, mp.inverse(A.T * A) * A.T
    import scipy.linalg
    L0 = scipy.linalg.logm(_f(M)).real
    r = [mp.mpf(float(x)) for x in (L0[2, 1], L0[0, 2], L0[1, 0], L0[0, 3], L0[1, 3], L0[2, 3])]
    for _ in range(4):
        A = _dexp_se3(r)
        N = mp.inverse(A.T * A) * A.T
        step = N * _vec34(M - mp.expm(p3.hat(r)))
        r = [r[k] + step[k] for k in range(6)]
    assert mp.norm(M - mp.expm(p3.hat(r))) < mp.mpf("1e-30") and sum(x * x for x in r[:3]) < mp.pi ** 2
    A = _dexp_se3(r)
    return r, mp.inverse(A.T * A) * A.T


def _log_and_jacobians(M, dMs):
    """r = Log(M) and, for each list of six matrices dM/dd_k in dMs, the 6 x 6 Jacobian dr/dd solving (dExp/dr) J = dM/dd in the least-squares sense"""
    r, N = _log_se3(M)
    out = []
    for dM in dMs:
        B = mp.zeros(12, 6)
        for k in range(6):
            for i in range(3):
                for j in range(4):
                    B[4 * i + j, k] = dM[k][i, j]
        out.append(_f(N * B))
    return np.array([float(v) for v in r]), out


def between(xi, xj, z):
    """r, Ji, Jj of BetweenFactor<Pose3>: M(di, dj) = Z^-1 (Xi Exp(di))^-1 Xj Exp(dj)"""
    Xi, Xj, Z = p3.pose_mat(xi), p3.pose_mat(xj), p3.pose_mat(z)
    Zi, H = p3.inv(Z), p3.inv(Xi) * Xj
    M = Zi * H
    G = _unit_twists()
    r, (Ji, Jj) = _log_and_jacobians(M, [[-(Zi * g * H) for g in G], [M * g for g in G]])
    return r, Ji, Jj


def prior(x, mean):
    M = p3.inv(p3.pose_mat(mean)) * p3.pose_mat(x)
    r, (J,) = _log_and_jacobians(M, [[M * g for g in _unit_twists()]])
    return r, J


def _hat3(w):
    return mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def so3_log(R):
    """rotation vector (angle below pi) of an mpmath rotation matrix: mpmath's matrix logarithm where it returns the real branch, otherwise (within
    a few degrees of pi it returns a complex logarithm) Newton's method on mpmath's expm from scipy's double-precision logarithm, as in _log_se3"""
    L = mp.logm(R)
    if max(abs(mp.im(L[i, j])) for i in range(3) for j in range(3)) < mp.mpf("1e-25"):
        return [mp.re(L[2, 1]), mp.re(L[0, 2]), mp.re(L[1, 0])]
    import scipy.linalg
    L0 = scipy.linalg.logm(_f(R)).real
    r = [mp.mpf(float(x)) for x in (L0[2, 1], L0[0, 2], L0[1, 0])]
    h = mp.mpf("1e-12")
    for _ in range(4):
        A = mp.zeros(9, 3)
        for k in range(3):
            rp = list(r); rm = list(r)
            rp[k] += h; rm[k] -= h
            D = (mp.expm(_hat3(rp)) - mp.expm(_hat3(rm))) / (2 * h)
            for i in range(9):
                A[i, k] = D[i // 3, i % 3]
        E = R - mp.expm(_hat3(r))
        step = mp.inverse(A.T * A) * A.T * mp.matrix([E[i // 3, i % 3] for i in range(9)])
        r = [r[k] + step[k] for k in range(3)]
    assert mp.norm(R - mp.expm(_hat3(r))) < mp.mpf("1e-30") and _dot(r, r) < mp.pi ** 2
    return r


def so3_right_jacobian(w, h=mp.mpf("1e-12")):
    """Jr(w) with Exp(w + d) = Exp(w) Exp(Jr d + O(d^2)): column k is vee(R^T dR/dw_k)"""
    w = [mp.mpf(float(x)) for x in w]
    Rt = mp.expm(_hat3(w)).T
    J = np.zeros((3, 3))
    for k in range(3):
        wp = list(w); wm = list(w)
        wp[k] += h; wm[k] -= h
        S = Rt * (mp.expm(_hat3(wp)) - mp.expm(_hat3(wm))) / (2 * h)
        J[:, k] = [float((S[2, 1] - S[1, 2]) / 2), float((S[0, 2] - S[2, 0]) / 2), float((S[1, 0] - S[0, 1]) / 2)]
    return J


# sphere chart ---------------------------------------------------------------------------------------------------------------------------
def _mpv(a):
    return [mp.mpf(float(x)) for x in a]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _normalized(a):
    n = mp.sqrt(_dot(a, a))
    return [x / n for x in a]


def _basis(n):
    """the convention (not a formula under test): b1 along n x (the coordinate axis of smallest |n_i|, first of equals), b2 = n x b1"""
    k = int(np.argmin([abs(float(x)) for x in n]))
    b1 = _normalized(_cross(n, [mp.mpf(int(j == k)) for j in range(3)]))
    return b1, _cross(n, b1)


def _local(n, y, basis=None):
    """n, y: mpmath unit vectors.  Coordinates in `basis` (default: that of n) of the tangent at n whose geodesic ends at y.  The rotation
    about n x y taking n to y is I + [c]x + [c]x^2 / (1 + n.y) with c = n x y; its MATRIX logarithm is the rotation vector w, the tangent w x n."""
    c = _cross(n, y)
    s = 1 + _dot(n, y)
    C = _hat3(c)
    R = mp.eye(3) + C + C * C / s
    w = so3_log(R)
    xi = _cross(w, n)
    b1, b2 = basis or _basis(n)
    return [_dot(b1, xi), _dot(b2, xi)]


def unit3_local(n, y):
    return np.array([float(v) for v in _local(_normalized(_mpv(n)), _normalized(_mpv(y)))])


def _retract(n, v):
    b1, b2 = _basis(n)
    xi = [b1[k] * v[0] + b2[k] * v[1] for k in range(3)]
    R = mp.expm(_hat3(_cross(n, xi)))                        # rotation about n x xi by |xi|
    return [R[k, 0] * n[0] + R[k, 1] * n[1] + R[k, 2] * n[2] for k in range(3)]


def plane_retract(p, v):
    n = _retract(_normalized(_mpv(p[:3])), _mpv(v[:2]))
    return np.array([float(x) for x in n] + [float(mp.mpf(float(p[3])) + mp.mpf(float(v[2])))])


def _transform(X, n, d):
    R, t = X[0:3, 0:3], [X[0, 3], X[1, 3], X[2, 3]]
    return [R[0, k] * n[0] + R[1, k] * n[1] + R[2, k] * n[2] for k in range(3)], _dot(n, t) + d


def plane_factor(x, plane, z, h=mp.mpf("1e-12")):
    """r (3), d r / d [omega; v] of the pose (3 x 6), d r / d [dn; dd] of the plane (3 x 3).  OrientedPlane3Factor as GTSAM 4.0 has it:
    r = [-local_{n'}(n_z); d' - d_z] with (n', d') = plane.transform(pose), and the Jacobians of transform() expressed in the chart at the
    prediction: columns are central differences of [local_{n'(0)}(n'(delta)); d'(delta)]."""
    X = p3.pose_mat(x)
    n, d = _normalized(_mpv(plane[:3])), mp.mpf(float(plane[3]))
    nz, dz = _normalized(_mpv(z[:3])), mp.mpf(float(z[3]))
    n0, d0 = _transform(X, n, d)
    l = _local(n0, nz)
    r = np.array([float(-l[0]), float(-l[1]), float(d0 - dz)])
    B0 = _basis(n0)

    def chart(Xp, np_, dp_):
        a, b = _transform(Xp, np_, dp_)
        return _local(n0, a, B0) + [b]

    Hx, Hp = np.zeros((3, 6)), np.zeros((3, 3))
    for k in range(6):
        e = [mp.mpf(0)] * 6
        e[k] = h
        fp = chart(X * p3.expmap(e), n, d)
        e[k] = -h
        fm = chart(X * p3.expmap(e), n, d)
        Hx[:, k] = [float((a - b) / (2 * h)) for a, b in zip(fp, fm)]
    for k in range(3):
        vp = [mp.mpf(0)] * 3
        vp[k] = h
        fp = chart(X, _retract(n, vp[:2]), d + vp[2])
        fm = chart(X, _retract(n, [-vp[0], -vp[1]]), d - vp[2])
        Hp[:, k] = [float((a - b) / (2 * h)) for a, b in zip(fp, fm)]
    return r, Hx, Hp


# preintegration -------------------------------------------------------------------------------------------------------------------------
def _integrate(acc, gyro, dt, ba, bg, state=None):
    """the definition, sample by sample; constant runs of equal gyro samples reuse the increment's matrix exponential"""
    R, p, v = state or (mp.eye(3), mp.zeros(3, 1), mp.zeros(3, 1))
    last, Rinc = None, None
    for a, w in zip(acc, gyro):
        if last is None or any(x != y for x, y in zip(w, last)):
            Rinc = mp.expm(_hat3([(w[k] - bg[k]) * dt for k in range(3)]))
            last = w
        Ra = R * mp.matrix([a[k] - ba[k] for k in range(3)])
        p = p + v * dt + Ra * (dt * dt / 2)
        v = v + Ra * dt
        R = R * Rinc
    return R, p, v


def preintegrate(acc, gyro, dt, bhat, h=mp.mpf("1e-12")):
    """dict(dR 3 x 3, dp, dv, J_R_bg, J_p_ba, J_p_bg, J_v_ba, J_v_bg) after all samples, bias Jacobians by central differences about bhat
    (the rotation one in the chart at dR: vee of Log(dR^T dR(bg + delta)), which to first order is the antisymmetric part)"""
    acc = [_mpv(a) for a in acc]; gyro = [_mpv(w) for w in gyro]
    dt = mp.mpf(float(dt)); b = _mpv(bhat)
    R, p, v = _integrate(acc, gyro, dt, b[:3], b[3:])
    out = dict(dR=_f(R), dp=_f(p).ravel(), dv=_f(v).ravel())
    J = {k: np.zeros((3, 3)) for k in ("J_R_bg", "J_p_ba", "J_p_bg", "J_v_ba", "J_v_bg")}
    for k in range(6):
        bp = list(b); bm = list(b)
        bp[k] += h; bm[k] -= h
        Rp, pp, vp = _integrate(acc, gyro, dt, bp[:3], bp[3:])
        Rm, pm, vm = _integrate(acc, gyro, dt, bm[:3], bm[3:])
        dpk, dvk = _f((pp - pm) / (2 * h)).ravel(), _f((vp - vm) / (2 * h)).ravel()
        if k < 3:
            J["J_p_ba"][:, k] = dpk; J["J_v_ba"][:, k] = dvk
        else:
            S = R.T * (Rp - Rm) / (2 * h)
            J["J_R_bg"][:, k - 3] = [float((S[2, 1] - S[1, 2]) / 2), float((S[0, 2] - S[2, 0]) / 2), float((S[1, 0] - S[0, 1]) / 2)]
            J["J_p_bg"][:, k - 3] = dpk; J["J_v_bg"][:, k - 3] = dvk
    out.update(J)
    return out


GYRO_DT = [1e-7, 1e-6, 0.9e-5, 1.1e-5, 1e-4, 1e-3]              # rotation per sample of the constant-gyro runs (+ the 0.25 bracket below)
GYRO_DT_CPU = GYRO_DT + [0.0, 0.225, 0.275]


def quat_of(R):
    """unit quaternion x y z w (w >= 0) of a float rotation matrix near enough the identity for the trace branch"""
    w = 0.5 * np.sqrt(1.0 + R[0, 0] + R[1, 1] + R[2, 2])
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


# (bias-correction angle |J_R_bg dbg|, rotation angle of the residual): exactly (0, 0); then the residual angle goes through ANGLES (0, the sweep,
# every bracket, pi - {1e-1, 1e-2, 1e-3}) while the bias-correction angle goes through 0, the sweep and every bracket, shifted so that the two
# angles of a pair differ by orders of magnitude; then pairs with both angles either side of the same switch
_BIAS_ANGLES = [0.0] + SWEEP + BRACKETS
IMU_ANGLES = ([(0.0, 0.0)] + [(_BIAS_ANGLES[(k + 11) % len(_BIAS_ANGLES)], a) for k, a in enumerate(ANGLES)]
              + [(f1 * t, f2 * t) for t in THRESHOLDS for f1, f2 in ((0.9, 1.1), (1.1, 0.9))])


@functools.lru_cache(maxsize=None)
def imu_cases():
    """(xi, vi, xj, vj, bi, bj, pim) per entry of IMU_ANGLES (42 of them): the gyro bias is moved from the integration bias by J_R_bg^-1 (angle x axis), and
    pose j is the prediction turned by the residual angle (the prediction comes from the oracle: it only places the input)"""
    from tests import orc_binding as orc
    rng = np.random.default_rng(20265)
    out = []
    for k, (ab, ar) in enumerate(IMU_ANGLES):
        samples = 20
        t = np.arange(samples) * 0.005
        gyro = np.stack([0.6 * np.sin(2.1 * t + p) for p in rng.uniform(0, 6, 3)], 1)
        acc = np.stack([1.5 * np.cos(1.3 * t + p) for p in rng.uniform(0, 6, 3)], 1) + np.array([0, 0, -9.71])
        bhat = rng.normal(size=6) * 0.01
        pim = orc.Preint(bhat, acc, gyro, 0.005)
        xi = _rng_pose(rng, 1.0); vi = rng.normal(size=3)
        bi = bhat.copy()
        bi[:3] += rng.normal(size=3) * (0.02 if k else 0.0)
        bi[3:] += np.linalg.solve(pim.J_R_bg, ab * AXES[k % len(AXES)])
        xj_pred, vj_pred = pim.predict(xi, vi, bi)
        size = TRANS[k % 4]
        tdir = rng.normal(size=3); tdir /= np.linalg.norm(tdir)
        xj = pose_mul(xj_pred, pose_inv(_offset(ar, AXES[(k + 2) % len(AXES)], size, tdir)))
        vj = vj_pred + (rng.normal(size=3) * 0.2 if k else 0.0)
        bj = bi + (rng.normal(size=6) * 0.01 if k else 0.0)
        out.append((xi, vi, xj, vj, bi, bj, pim))
    return out


def _exp_small(d):
    """Exp of a twist of size 1e-12 by the exponential series up to the fourth power (remainder 1e-60)"""
    A = p3.hat(d)
    A2 = A * A
    return mp.eye(4) + A + A2 / 2 + A2 * A / 6 + A2 * A2 / 24


def imu_factor(xi, vi, xj, vj, bi, bj, pim, g, h=mp.mpf("1e-12")):
    """r (15) and the six Jacobians of the CombinedImuFactor as tests/imu_independent.py defines it (same prose, same 40 digits), by the route
    of `between`: only the base point takes a matrix logarithm; the rotation rows of the Jacobians solve (dExp/dr) J = d(Rj^T Ri dRc)/dd with
    both derivatives central differences (of mpmath's expm, and of the rotation product); the other twelve rows are central differences of
    expressions without a logarithm.  About 0.15 s per factor instead of 3.5 s; held to tests/imu_independent.factor in
    tests/test_chart_edges_cpu.py."""
    Xi0, Xj0 = p3.pose_mat(xi), p3.pose_mat(xj)
    vec = lambda a: mp.matrix([mp.mpf(float(x)) for x in a])
    base = {"vi": vec(vi), "vj": vec(vj), "bi": vec(bi), "bj": vec(bj)}
    bhat, gv, dt = vec(pim.bhat), vec(g), mp.mpf(float(pim.dt))
    q = pim.dR
    dR = p3.pose_mat([0, 0, 0, q[0], q[1], q[2], q[3]])[0:3, 0:3]
    m3 = lambda a: mp.matrix([[mp.mpf(float(np.asarray(a).ravel()[3 * r + c])) for c in range(3)] for r in range(3)])
    JRbg, Jpba, Jpbg, Jvba, Jvbg = (m3(getattr(pim, n)) for n in ("J_R_bg", "J_p_ba", "J_p_bg", "J_v_ba", "J_v_bg"))
    dp0, dv0 = vec(pim.dp), vec(pim.dv)

    def corrected(b_i):
        dba, dbg = (b_i - bhat)[0:3, 0], (b_i - bhat)[3:6, 0]
        w = JRbg * dbg
        return dR * mp.expm(_hat3([w[0], w[1], w[2]])), dp0 + Jpba * dba + Jpbg * dbg, dv0 + Jvba * dba + Jvbg * dbg

    corr0 = corrected(base["bi"])

    def parts(name=None, d=None):
        """E = Rj^T Ri dRc and the twelve residuals that need no logarithm"""
        Xi = Xi0 * _exp_small(d) if name == "xi" else Xi0
        Xj = Xj0 * _exp_small(d) if name == "xj" else Xj0
        v = {k: (a + mp.matrix(d) if k == name else a) for k, a in base.items()}
        dRc, dpc, dvc = corrected(v["bi"]) if name == "bi" else corr0
        Ri, Rj = Xi[0:3, 0:3], Xj[0:3, 0:3]
        pp = Xi[0:3, 3] + v["vi"] * dt + gv * (dt * dt / 2) + Ri * dpc
        vp = v["vi"] + gv * dt + Ri * dvc
        rp, rv, rb = Rj.T * (pp - Xj[0:3, 3]), Rj.T * (vp - v["vj"]), v["bi"] - v["bj"]
        return Rj.T * Ri * dRc, [rp[k] for k in range(3)] + [rv[k] for k in range(3)] + [rb[k] for k in range(6)]

    E0, tail0 = parts()
    r = so3_log(E0)
    A = mp.zeros(9, 3)
    for k in range(3):
        rp_ = list(r); rm_ = list(r)
        rp_[k] += h; rm_[k] -= h
        D = (mp.expm(_hat3(rp_)) - mp.expm(_hat3(rm_))) / (2 * h)
        for i in range(9):
            A[i, k] = D[i // 3, i % 3]
    N = mp.inverse(A.T * A) * A.T
    Js = []
    for name, n in (("xi", 6), ("vi", 3), ("xj", 6), ("vj", 3), ("bi", 6), ("bj", 6)):
        J = np.zeros((15, n))
        for k in range(n):
            d = [mp.mpf(0)] * n
            d[k] = h
            Ep, tp = parts(name, d)
            d[k] = -h
            Em, tm = parts(name, d)
            if name in ("xi", "xj", "bi"):                               # the rotation residual depends on nothing else
                dE = (Ep - Em) / (2 * h)
                c = N * mp.matrix([dE[i // 3, i % 3] for i in range(9)])
                J[:3, k] = [float(c[i]) for i in range(3)]
            J[3:, k] = [float((a - b) / (2 * h)) for a, b in zip(tp, tm)]
        Js.append(J)
    return np.array([float(x) for x in r] + [float(x) for x in tail0]), Js
