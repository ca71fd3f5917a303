"""Reference and case generator of tests/test_ba_reference_cpu.py and tests/test_gpu_ba_forms.py -- CHECKER SIDE ONLY, host only.

The landmark-elimination kernels (csrc/kernels_ba.hip, ba_tables of csrc/structure_ba.cpp) on graphs small enough for a dense system
that shares no formula with the product or the oracle:
  * projection factors: the prose of tests/camera_independent.py again (4x4 matrices, forward-mode dual numbers), here with the dual
    numbers vectorised over the observations and the number format a parameter (reproj_all; test_ba_reference_cpu holds it to reproj_ad);
  * between factors, the pose prior and retract: tests/pose3_independent.py (matrix logarithm / exponential at 40 digits);
  * point priors: 1 / sigma^2 on three rows.
reference(name, extended) accumulates H, b, chi2 and forms, landmark by landmark with closed-form 3x3 inverses,
  S = H_cc - sum_p W_p (H_pp + lambda I)^-1 W_p^T,   g = b_c - sum_p W_p (H_pp + lambda I)^-1 b_p,
together with the scale of every 6x6 block -- |H_blk|max + sum_p max|W_a (H_pp + lambda I)^-1 W_b^T|, the sum of the magnitudes of what
the kernels add up -- and the full damped step (H + lambda I)^-1 b over cameras and landmarks.  Once in numpy.longdouble ("extended")
and once in float64: the difference between the two is what ordinary double arithmetic costs on these sums, and the bounds of the GPU
test are derived from it.

Variables: poses 0 .. K-1, points K .. K+L-1.  Rows / columns of S: the free poses and the free points nobody observes, ids ascending
(`stay`); every other free point is eliminated (it carries projection factors and priors only)."""
import functools

import numpy as np

from tests import pose3_independent as p3
from tests.util import SR4000_CALIB, info_full, pose_inv, pose_mul, quat_mul

BPS = np.array([0.02, -0.01, 0.03, 0.5, 0.5, 0.5, 0.5])           # body x-forward -> camera z-forward, with a lever arm
LAMS = (0.0, 1e-5, 1e3)
LAM0 = 1e-5                                                       # LevenbergMarquardtParams::lambdaInitial
PAIR_SIZES = (1, 9, 10, 11, 19, 20, 21, 39, 40, 41, 79, 80, 81, 159, 160, 161)
COUNTS = (1, 59, 60, 61, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)
GRID_SIZES = (1, 7, 8, 9)
ODOMETRY_SIGMA = (0.002, 0.005)
POSE_PRIOR_SIGMA = 1e-3
MAX_CAMS = 90


# ---------------------------------------------------------------- dual numbers over all observations at once
class VDual:
    """value[n] + partials[n, m], every operation element-wise over the n observations"""
    __slots__ = ("v", "g")
    __array_ufunc__ = None                                        # ndarray op VDual defers to the reflected methods below

    def __init__(self, v, g):
        self.v, self.g = v, g

    def _o(self, o):
        return o if isinstance(o, VDual) else VDual(o, 0.0)

    def __add__(self, o): o = self._o(o); return VDual(self.v + o.v, self.g + o.g)
    __radd__ = __add__
    def __sub__(self, o): o = self._o(o); return VDual(self.v - o.v, self.g - o.g)
    def __rsub__(self, o): o = self._o(o); return VDual(o.v - self.v, o.g - self.g)
    def __neg__(self): return VDual(-self.v, -self.g)

    def __mul__(self, o):
        o = self._o(o)
        return VDual(self.v * o.v, _col(self.v) * o.g + _col(o.v) * self.g)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = self._o(o)
        return VDual(self.v / o.v, (self.g * _col(o.v) - _col(self.v) * o.g) / _col(o.v * o.v))

    def __rtruediv__(self, o): return self._o(o) / self


def _col(v):
    return v[:, None] if isinstance(v, np.ndarray) else v


def _mat_mul(A, B):
    return [[A[r][0] * B[0][c] + A[r][1] * B[1][c] + A[r][2] * B[2][c] + A[r][3] * B[3][c] for c in range(4)] for r in range(4)]


def _pose_mat(p, T):
    """tx ty tz qx qy qz qw [n, 7] -> 4x4 of arrays; the rotation as (w^2 - v.v) I + 2 v v^T + 2 w [v]x"""
    p = np.asarray(p, T)
    q = p[:, 3:] / np.sqrt((p[:, 3:] * p[:, 3:]).sum(1))[:, None]
    v, w = [q[:, 0], q[:, 1], q[:, 2]], q[:, 3]
    vv = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    zero, one = np.zeros(len(p), T), np.ones(len(p), T)
    S = [[zero, -v[2], v[1]], [v[2], zero, -v[0]], [-v[1], v[0], zero]]
    M = [[2 * v[r] * v[c] + 2 * w * S[r][c] + ((w * w - vv) if r == c else zero) for c in range(3)] + [p[:, r]] for r in range(3)]
    return M + [[zero, zero, zero, one]]


def reproj_all(poses, pts, uv, calib, bps, dtype=np.float64):
    """residual [n, 2], d r / d [omega; v] of the pose [n, 2, 6], d r / d point [n, 2, 3] of n projection factors; an observation
    whose point is not in front of its camera: residual 2 fx (1, 1), Jacobians zero"""
    T = dtype
    n = len(poses)
    fx, fy, s, u0, v0, k1, k2, p1, p2 = [T(float(c)) for c in calib]
    eye = np.eye(9, dtype=T)
    zero, one = np.zeros(n, T), np.ones(n, T)
    d = [VDual(zero, np.broadcast_to(eye[k], (n, 9))) for k in range(6)]
    p = [VDual(np.asarray(pts, T)[:, k], np.broadcast_to(eye[6 + k], (n, 9))) for k in range(3)]
    w, v = d[:3], d[3:]
    twist = [[one, -w[2], w[1], v[0]], [w[2], one, -w[0], v[1]], [-w[1], w[0], one, v[2]], [zero, zero, zero, one]]
    cam = _mat_mul(_mat_mul(_pose_mat(poses, T), twist), _pose_mat(np.broadcast_to(bps, (n, 7)), T))
    # the inverse: rotation transposed (first order in the twist, as tests/camera_independent.py), translation -R^T t
    ci = [[cam[c][r] for c in range(3)] + [-(cam[0][r] * cam[0][3] + cam[1][r] * cam[1][3] + cam[2][r] * cam[2][3])] for r in range(3)]
    pc = [ci[r][0] * p[0] + ci[r][1] * p[1] + ci[r][2] * p[2] + ci[r][3] for r in range(3)]
    behind = pc[2].v <= 0
    z = VDual(np.where(behind, one, pc[2].v), pc[2].g)
    xn, yn = pc[0] / z, pc[1] / z
    rr = xn * xn + yn * yn
    g = 1.0 + k1 * rr + k2 * rr * rr
    xd = g * xn + 2.0 * p1 * xn * yn + p2 * (rr + 2.0 * xn * xn)
    yd = g * yn + 2.0 * p2 * xn * yn + p1 * (rr + 2.0 * yn * yn)
    uvT = np.asarray(uv, T)
    u = fx * xd + s * yd + u0 - uvT[:, 0]
    vv = fy * yd + v0 - uvT[:, 1]
    r = np.stack([u.v, vv.v], 1)
    J = np.stack([u.g, vv.g], 1)
    r[behind] = 2 * fx
    J[behind] = 0
    return r, J[:, :, :6], J[:, :, 6:]


# ---------------------------------------------------------------- cases
def _path(n):
    """a short forward-looking path: 2 cm per key frame along x with a gentle weave"""
    k = np.arange(n)
    t = np.stack([0.02 * k, 0.05 * np.sin(0.3 * k), 0.02 * np.cos(0.2 * k)], 1)
    yaw = 0.03 * np.sin(0.25 * k)
    return np.concatenate([t, np.stack([np.zeros(n), np.zeros(n), np.sin(yaw / 2), np.cos(yaw / 2)], 1)], 1)


def _case(name, built_for, K, L, obs_kf, obs_pt, seed, fixed_pose=(), fixed_pt=(), pose_prior=True, no_prior=(), extra_priors=(),
          behind=(), sigmas=None, marks=None, start_noise=1.0):
    """truth, start, measurements and priors of one graph from its observation pattern"""
    rng = np.random.default_rng(seed)
    obs_kf, obs_pt = np.asarray(obs_kf, np.int64), np.asarray(obs_pt, np.int64)
    poses = _path(K)
    x_end = poses[-1, 0]
    pts = np.stack([rng.uniform(x_end + 3.0, x_end + 6.0, L), rng.uniform(-0.6, 0.6, L), rng.uniform(-0.6, 0.6, L)], 1)
    for j in behind:
        pts[j, 0] = -2.0
    r, _, _ = reproj_all(poses[obs_kf], pts[obs_pt], np.zeros((len(obs_kf), 2)), SR4000_CALIB, BPS)
    sig = np.ones(len(obs_kf)) if sigmas is None else np.asarray(sigmas, np.float64)
    uv = r + rng.normal(size=r.shape) * 0.5 * sig[:, None]
    # the start of camera k is the same in every case: the 40-digit between factors are evaluated once per pair of neighbours
    prng = np.random.default_rng(7)
    dt, dr = prng.normal(size=(MAX_CAMS, 3)) * 0.002 * start_noise, prng.normal(size=(MAX_CAMS, 3)) * 0.0005 * start_noise
    poses0 = poses.copy()
    poses0[:, :3] += dt[:K]
    for k in range(K):
        dq = np.concatenate([dr[k], [1.0]])
        poses0[k, 3:] = quat_mul(poses0[k, 3:], dq / np.linalg.norm(dq))
    points0 = pts + rng.normal(size=pts.shape) * 0.01 * start_noise
    fp = np.zeros(K, np.uint8); fp[list(fixed_pose)] = 1
    fl = np.zeros(L, np.uint8); fl[list(fixed_pt)] = 1
    poses0[fp == 1] = poses[fp == 1]
    prior_pt = [j for j in range(L) if j not in set(no_prior) and not fl[j]]
    pp_pt = np.array(prior_pt + [j for j, _ in extra_priors], np.int64)
    pp_sigma = np.array([0.014] * len(prior_pt) + [s for _, s in extra_priors])
    pp_mean = pts[pp_pt] + rng.normal(size=(len(pp_pt), 3)) * 0.005
    bz = np.array([pose_mul(pose_inv(poses[k]), poses[k + 1]) for k in range(K - 1)]).reshape(-1, 7)
    wi = np.zeros(21); wi[[0, 6, 11]] = 1.0 / ODOMETRY_SIGMA[0] ** 2; wi[[15, 18, 20]] = 1.0 / ODOMETRY_SIGMA[1] ** 2
    wp = np.zeros(21); wp[[0, 6, 11, 15, 18, 20]] = 1.0 / POSE_PRIOR_SIGMA ** 2
    return dict(name=name, built_for=built_for, K=K, L=L, poses=poses, points=pts, poses0=poses0, points0=points0, fixed_pose=fp, fixed_pt=fl,
                obs_kf=obs_kf, obs_pt=obs_pt, obs_uv=uv, obs_sigma=sig, between_i=np.arange(K - 1), between_j=np.arange(1, K), between_z=bz,
                between_info=wi, pose_prior=(0, poses[0].copy(), wp) if pose_prior else None, pp_pt=pp_pt, pp_mean=pp_mean, pp_sigma=pp_sigma,
                calib=SR4000_CALIB.copy(), bps=BPS.copy(), marks=dict(marks or {}))


def _pairs_pattern(sizes, first_cam=0):
    kf, pt, j = [], [], 0
    for k, m in enumerate(sizes):
        for _ in range(m):
            kf += [first_cam + 2 * k, first_cam + 2 * k + 1]; pt += [j, j]; j += 1
    return kf, pt, j


def case_pairs():
    kf, pt, L = _pairs_pattern(PAIR_SIZES)
    return _case("pairs", "cameras (2k, 2k+1) share exactly PAIR_SIZES[k] landmarks and nothing else: pair-list lengths either side of every "
                 "stride of k_ba_schur at one and four waves and of the ba_small switch", 2 * len(PAIR_SIZES), L, kf, pt, seed=101)


def case_counts():
    """cameras 0..13 with exactly COUNTS[i] observations; every landmark is also seen by one of the partner cameras 14 / 15, so every
    count camera has row blocks besides its own"""
    kf, pt, j = [], [], 0
    for i, n in enumerate(COUNTS):
        for _ in range(n):
            kf += [i, 14 + (j & 1)]; pt += [j, j]; j += 1
    return _case("counts", "cameras with exactly COUNTS[i] observations and >= 2 blocks each: the steps of k_ba_cameras (64 per wave, 256 per "
                 "step) and the staging batches of k_ba_schur_cam (256), a batch ending inside the pair window included", 16, j, kf, pt, seed=102)


def case_clique90():
    kf, pt = [], []
    for c in range(90):
        for j in range(12):
            kf.append(c); pt.append(j)
    for c in range(12):
        for j in range(12, 112):
            kf.append(c); pt.append(j)
    return _case("clique90", "90 cameras see the same 12 landmarks, cameras 0..11 another 100: column cameras with 90, 89, .., 1 row blocks (the ten "
                 "widest block by block, k_ba_schur_cam at every nT 80 .. 1); blocks among cameras 0..11 carry 112 pairs, all others 12",
                 90, 112, kf, pt, seed=103)


def case_hub():
    kf, pt = [], []
    for c in range(41):
        for j in range(260):
            kf.append(c); pt.append(j)
    return _case("hub", "41 mutually co-visible cameras (G = 1 in k_ba_schur_cam) sharing 260 landmarks: per-slice lists across two staging batches",
                 41, 260, kf, pt, seed=104)


def case_grid(n):
    """n free cameras in a chain, two landmarks per neighbouring pair (a single camera: two landmarks of its own)"""
    kf, pt, j = [], [], 0
    for k in range(max(n - 1, 1)):
        for _ in range(2):
            kf += [k] + ([k + 1] if n > 1 else []); pt += [j] * (2 if n > 1 else 1); j += 1
    return _case("grid%d" % n, "%d free cameras that see landmarks: the grids of the per-camera launches and the XCD remap around 8" % n,
                 n, j, kf, pt, seed=110 + n)


ODD_FIXED_CAM = 3


def case_odd():
    M, kf, pt, sg = {}, [], [], []

    def lm(mark, cams):
        j = len(M)
        M[j] = mark
        for c in cams:
            kf.append(c); pt.append(j); sg.append(0.5 + 1.5 * ((7 * len(sg)) % 11) / 10.0)      # 0.5 .. 2 px
        return j
    for k in range(6):
        lm("regular", [k, k + 1] if k % 2 else [k, ODD_FIXED_CAM, (k + 2) % 7])
    lm("fixed_camera_only", [ODD_FIXED_CAM])
    for k in range(3):
        lm("no_prior", [0, 1, 2, 4 + k % 3, ODD_FIXED_CAM][:3 + k])
    two = lm("two_priors", [4, 5])
    lm("seen_once", [5])
    lm("pair_twice", [1, 1, 2])
    behind = lm("behind_its_camera", [6])
    lm("unobserved", [])
    fixed = lm("fixed_landmark", [0, 1])
    no_prior = [j for j, m in M.items() if m == "no_prior"]
    return _case("odd", "a fixed camera that sees eliminated landmarks, a landmark of the fixed camera only, landmarks without a prior seen by >= 3 "
                 "cameras, two priors of different sigma, a landmark seen once, a pair observed twice, a landmark behind its camera, pixel sigmas "
                 "0.5 .. 2, a free landmark nobody observes, a fixed landmark that is observed", 7, len(M), kf, pt, seed=105,
                 fixed_pose=[ODD_FIXED_CAM], fixed_pt=[fixed], no_prior=no_prior, extra_priors=[(two, 0.05)], behind=[behind], sigmas=sg, marks=M)


NO_PRIORS_SIZES = (1, 21, 81)


def case_no_priors():
    """as `pairs`, three pairs: pose 0 is FIXED instead of carrying a prior and sees every landmark (a third view, and no block of
    the reduced system), no landmark has a prior: n_priors == 0"""
    kf, pt, L = _pairs_pattern(NO_PRIORS_SIZES, first_cam=1)
    kf += [0] * L; pt += list(range(L))
    return _case("no_priors", "as pairs, cut to three pairs; pose 0 fixed instead of a prior, no prior anywhere: the plan has n_priors == 0",
                 1 + 2 * len(NO_PRIORS_SIZES), L, kf, pt, seed=106, fixed_pose=[0], pose_prior=False, no_prior=range(L))


def case_underdetermined():
    """grid7 plus one landmark without a prior that is seen once: H_pp of that landmark has rank 2"""
    g = case_grid(7)
    kf, pt = list(g["obs_kf"]) + [3], list(g["obs_pt"]) + [g["L"]]
    return _case("underdetermined", "grid7 plus a landmark without a prior, seen once", 7, g["L"] + 1, kf, pt, seed=117, no_prior=[g["L"]])


CASES = dict(pairs=case_pairs, counts=case_counts, clique90=case_clique90, hub=case_hub, grid1=lambda: case_grid(1), grid7=lambda: case_grid(7),
             grid8=lambda: case_grid(8), grid9=lambda: case_grid(9), odd=case_odd, no_priors=case_no_priors)
CASE_NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    return case_underdetermined() if name == "underdetermined" else CASES[name]()


def layout(c):
    """stay: ids of the rows / columns of the reduced system; elim: point numbers of the eliminated landmarks"""
    K, L = c["K"], c["L"]
    seen = np.bincount(c["obs_pt"], minlength=L)
    free_pt = c["fixed_pt"] == 0
    elim = np.nonzero(free_pt & (seen > 0))[0]
    stay = np.concatenate([np.nonzero(c["fixed_pose"] == 0)[0], K + np.nonzero(free_pt & (seen == 0))[0]])
    return stay, elim


def obs_per_camera(c):
    return np.bincount(c["obs_kf"], minlength=c["K"])


def shared_landmarks(c):
    """[K, K]: number of distinct landmarks two cameras both see"""
    V = np.zeros((c["K"], c["L"]), np.int64)
    V[c["obs_kf"], c["obs_pt"]] = 1
    return V @ V.T


# ---------------------------------------------------------------- the dense reference
@functools.lru_cache(maxsize=None)
def _between(xi, xj, z):
    return p3.between(*(np.frombuffer(a) for a in (xi, xj, z)))


@functools.lru_cache(maxsize=None)
def _pose_factors(name):
    """between factors and the pose prior of a case: (r, Ji, Jj) / (r, J) as floats, exact to double (40-digit arithmetic)"""
    c = case(name)
    bt = [_between(c["poses0"][i].tobytes(), c["poses0"][j].tobytes(), z.tobytes()) for i, j, z in zip(c["between_i"], c["between_j"], c["between_z"])]
    pr = p3.prior(c["poses0"][c["pose_prior"][0]], c["pose_prior"][1]) if c["pose_prior"] else None
    return bt, pr


def _inv3(A):
    """closed-form inverses of symmetric 3x3 matrices [n, 3, 3]: adjugate over determinant"""
    a, b, c_, d, e, f = A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2]
    c00, c01, c02 = d * f - e * e, c_ * e - b * f, b * e - c_ * d
    c11, c12, c22 = a * f - c_ * c_, b * c_ - a * e, a * d - b * b
    det = a * c00 + b * c01 + c_ * c02
    out = np.stack([np.stack([c00, c01, c02], 1), np.stack([c01, c11, c12], 1), np.stack([c02, c12, c22], 1)], 1)
    return out / det[:, None, None]


def _solve_refined(A, b):
    """A x = b in the precision of A: double LU, residuals in A's precision until they stop shrinking"""
    A64 = np.asarray(A, np.float64)
    x = np.linalg.solve(A64, np.asarray(b, np.float64)).astype(A.dtype)
    if A.dtype == np.float64:
        return x
    for _ in range(6):
        r = b - A @ x
        x = x + np.linalg.solve(A64, np.asarray(r, np.float64)).astype(A.dtype)
    return x


@functools.lru_cache(maxsize=None)
def reference(name, extended=True):
    """dense H_cc, b_c, chi2 at the start of a case and, per lambda of LAMS, S, g, their block scales and (lambda = LAM0) the damped step"""
    T = np.longdouble if extended else np.float64
    c = case(name)
    K, L = c["K"], c["L"]
    stay, elim = layout(c)
    n = len(stay)
    row = np.full(K + L, -1); row[stay] = np.arange(n)
    eidx = np.full(L, -1); eidx[elim] = np.arange(len(elim))
    H = np.zeros((n, 6, n, 6), T); b = np.zeros((n, 6), T)
    chi = T(0)
    for k in stay[stay >= K]:                                           # identity on the padding of a 3-dof variable that stays
        for q in range(3, 6):
            H[row[k], q, row[k], q] = 1
    bt, pr = _pose_factors(name)
    Wb = np.asarray(info_full(c["between_info"]), T)
    for (r, Ji, Jj), i, j in zip(bt, c["between_i"], c["between_j"]):
        r, J = np.asarray(r, T), {i: np.asarray(Ji, T), j: np.asarray(Jj, T)}
        chi += r @ Wb @ r
        for u in (i, j):
            if row[u] < 0:
                continue
            b[row[u]] -= J[u].T @ Wb @ r
            for v in (i, j):
                if row[v] >= 0:
                    H[row[u], :, row[v], :] += J[u].T @ Wb @ J[v]
    if pr is not None:
        r, J = np.asarray(pr[0], T), np.asarray(pr[1], T)
        Wp = np.asarray(info_full(c["pose_prior"][2]), T)
        chi += r @ Wp @ r
        u = row[c["pose_prior"][0]]
        H[u, :, u, :] += J.T @ Wp @ J; b[u] -= J.T @ Wp @ r
    # projection factors
    ok, op = c["obs_kf"], c["obs_pt"]
    r, Jx, Jp = reproj_all(c["poses0"][ok], c["points0"][op], c["obs_uv"], c["calib"], c["bps"], T)
    w = 1 / np.asarray(c["obs_sigma"], T) ** 2
    chi += (w * (r * r).sum(1)).sum()
    Hpp = np.zeros((len(elim), 3, 3), T); bp = np.zeros((len(elim), 3), T)
    Wo = w[:, None, None] * np.einsum("oki,okj->oij", Jx, Jp)            # [obs, 6, 3]
    Hxx = w[:, None, None] * np.einsum("oki,okj->oij", Jx, Jx)
    bx = -w[:, None] * np.einsum("oki,ok->oi", Jx, r)
    Hll = w[:, None, None] * np.einsum("oki,okj->oij", Jp, Jp)
    bl = -w[:, None] * np.einsum("oki,ok->oi", Jp, r)
    for o in range(len(ok)):
        u = row[ok[o]]
        if u >= 0:
            H[u, :, u, :] += Hxx[o]; b[u] += bx[o]
        if eidx[op[o]] >= 0:
            Hpp[eidx[op[o]]] += Hll[o]; bp[eidx[op[o]]] += bl[o]
    # point priors
    for j, mean, s in zip(c["pp_pt"], c["pp_mean"], c["pp_sigma"]):
        wj = 1 / T(s) ** 2
        d = np.asarray(c["points0"][j], T) - np.asarray(mean, T)
        chi += wj * (d @ d)
        if eidx[j] >= 0:
            Hpp[eidx[j]] += wj * np.eye(3, dtype=T); bp[eidx[j]] -= wj * d
        elif row[K + j] >= 0:
            u = row[K + j]
            H[u, :3, u, :3] += wj * np.eye(3, dtype=T); b[u, :3] -= wj * d
    # observations of every eliminated landmark from cameras with a column
    views = [[] for _ in elim]
    for o in range(len(ok)):
        if eidx[op[o]] >= 0 and row[ok[o]] >= 0:
            views[eidx[op[o]]].append(o)
    Hmax = np.abs(H).max(axis=(1, 3))
    bmax = np.abs(b).max(axis=1)
    touched = np.zeros((n, n), bool)
    out = dict(stay=stay, elim=elim, H=H.reshape(6 * n, 6 * n), b=b.reshape(-1), chi2=chi, S={}, g={}, S_scale={}, g_scale={}, touched=touched,
               delta_stay={}, delta_lm={})
    for lam in (LAMS[1:] if name == "underdetermined" else LAMS):       # (H_pp of its extra landmark is singular without damping)
        A = _inv3(Hpp + T(lam) * np.eye(3, dtype=T)) if len(elim) else Hpp
        S, g = H.copy(), b.copy()
        Ss, gs = Hmax.astype(T), bmax.astype(T)
        for p, vs in enumerate(views):
            if not vs:
                continue
            cams = row[ok[vs]]
            Wp_ = Wo[vs]                                                 # [v, 6, 3]
            WA = Wp_ @ A[p]
            M = np.einsum("aik,bjk->abij", WA, Wp_)                      # W_a A W_b^T
            Mm = np.abs(M).max(axis=(2, 3))
            t = WA @ bp[p]                                               # [v, 6]
            tm = np.abs(t).max(axis=1)
            if len(set(cams)) == len(cams):
                S[cams[:, None], :, cams[None, :], :] -= M
                Ss[cams[:, None], cams[None, :]] += Mm
                g[cams] -= t; gs[cams] += tm
            else:                                                        # a camera sees the landmark twice
                for x, cx in enumerate(cams):
                    g[cx] -= t[x]; gs[cx] += tm[x]
                    for y, cy in enumerate(cams):
                        S[cx, :, cy, :] -= M[x, y]; Ss[cx, cy] += Mm[x, y]
            touched[cams[:, None], cams[None, :]] = True
        out["S"][lam], out["g"][lam] = S.reshape(6 * n, 6 * n), g.reshape(-1)
        out["S_scale"][lam], out["g_scale"][lam] = Ss, gs
        if lam != LAM0:
            continue
        if extended:                                                     # through the reduced system, then landmark by landmark
            dc = _solve_refined(out["S"][lam] + T(lam) * np.eye(6 * n, dtype=T), out["g"][lam]).reshape(n, 6)
            dl = np.zeros((len(elim), 3), T)
            for p, vs in enumerate(views):
                t = bp[p].copy()
                for o in vs:
                    t -= Wo[o].T @ dc[row[ok[o]]]
                dl[p] = A[p] @ t
        else:                                                            # numpy's own double solve of the whole system
            m = 6 * n + 3 * len(elim)
            F = np.zeros((m, m)); F[:6 * n, :6 * n] = out["H"]
            rhs = np.concatenate([out["b"], bp.reshape(-1)])
            for p, vs in enumerate(views):
                q = 6 * n + 3 * p
                F[q:q + 3, q:q + 3] = Hpp[p]
                for o in vs:
                    u = 6 * row[ok[o]]
                    F[u:u + 6, q:q + 3] += Wo[o]; F[q:q + 3, u:u + 6] += Wo[o].T
            x = np.linalg.solve(F + lam * np.eye(m), rhs)
            dc, dl = x[:6 * n].reshape(n, 6), x[6 * n:].reshape(-1, 3)
        out["delta_stay"][lam], out["delta_lm"][lam] = dc, dl
    return out


def block_rel(diff, scale):
    """diff / scale per block; a block nothing is added to (scale 0) must not differ at all"""
    diff, scale = np.asarray(diff, np.float64), np.asarray(scale, np.float64)
    return np.where(scale > 0, diff / np.where(scale > 0, scale, 1.0), np.where(diff == 0, 0.0, np.inf))


def conditioning(name):
    """what double arithmetic costs on a case: worst |float64 - extended| of S and g relative to the block scales (over LAMS), and of
    the damped step at LAM0 (absolute, with the step's own size)"""
    e, d = reference(name, True), reference(name, False)
    n = len(e["stay"])
    s_rel = g_rel = 0.0
    for lam in LAMS:
        dS = np.abs(np.asarray(d["S"][lam], np.longdouble) - e["S"][lam]).reshape(n, 6, n, 6).max(axis=(1, 3))
        s_rel = max(s_rel, float(block_rel(dS, e["S_scale"][lam]).max()))
        dg = np.abs(np.asarray(d["g"][lam], np.longdouble) - e["g"][lam]).reshape(n, 6).max(axis=1)
        g_rel = max(g_rel, float(block_rel(dg, e["g_scale"][lam]).max()))
    de = np.concatenate([e["delta_stay"][LAM0].reshape(-1), e["delta_lm"][LAM0].reshape(-1)])
    dd = np.concatenate([d["delta_stay"][LAM0].reshape(-1), d["delta_lm"][LAM0].reshape(-1)])
    return dict(S=s_rel, g=g_rel, step_diff=float(np.abs(dd - de).max()), step=float(np.abs(de).max()))


EPS = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def bounds():
    """the GPU bounds: S and g 10 x the worst float64-vs-extended figure over all cases (never below 2^-53, never above 1e-10), relative
    to the block scales; the LM step per case 10 x |delta_float64 - delta_extended|_inf (floor 1e-13 max(1, |delta|_inf), cap 1e-8)"""
    fig = {name: conditioning(name) for name in CASE_NAMES}
    clamp = lambda v: min(max(10.0 * v, EPS), 1e-10)
    step = {name: min(max(10.0 * f["step_diff"], 1e-13 * max(1.0, f["step"])), 1e-8) for name, f in fig.items()}
    return dict(figures=fig, S=clamp(max(f["S"] for f in fig.values())), g=clamp(max(f["g"] for f in fig.values())), step=step)
