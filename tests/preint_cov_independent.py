"""The preintegrated 15 x 15 covariance and its inverse a second time -- CHECKER SIDE ONLY.  mpmath at 40 digits, no formula shared with
csrc/imu_preint.cpp, csrc/preint_kernel.hip, csrc/fgo_core.cpp (fgo_preint_information) or oracle/orc_imu.h: no closed-form SO(3) Jacobian, no
quaternion, no hand-written transition matrix.

  state        (R, p, v, ba, bg)
  step         a = acc - ba, w = gyro - bg:   R' = R expm(hat(w dt)),  p' = p + v dt + R a dt^2 / 2,  v' = v + R a dt   (the step of
               tests/chart_edges._integrate; the biases stay)
  error state  R Exp(dtheta), p + R dp, v + R dv, ba + dba, bg + dbg   (order theta p v ba bg: the chart the payload documents)
  F            15 x 15 per sample, column k the central difference of d -> local(step(x (+) d), step(x)) along e_k, step 1e-14 (truncation
               1e-28).  The rotation part of `local` is the antisymmetric part of R0^T R1 = Exp(phi): sin|phi| / |phi| phi, which is phi up to
               O(phi^3), an error of O(step^2) in the difference; it spares the matrix logarithm.
  recursion    Sigma <- F Sigma F^T + Q from Sigma = 0

THE ONE THING SHARED WITH THE PRODUCT is the noise convention, GTSAM 4.0's "optimised" G Q G^T / dt of PreintegratedCombinedMeasurements as
DESIGN.md and oracle/orc_imu.h document it, because a convention cannot be derived.  Every matrix in it is taken from the differentiated F:
  theta theta  (gyro_cov + bias_acc_omega_int) / dt  (F_theta,bg) (F_theta,bg)^T
  v v          (acc_cov + bias_acc_omega_int) / dt   (F_v,ba) (F_v,ba)^T
  p p          dt integ_cov I          ba ba   dt bias_acc_cov I          bg bg   dt bias_gyro_cov I
Parameter order: acc, gyro, integration, bias acc, bias gyro, biasAccOmegaInt (fgo_imu_params, orc.Preint(variances=...)).

cases() is the one list of inputs that tests/test_preint_cov_cpu.py (host, oracle) and tests/test_gpu_preint_cov.py (device) share: 115 samples
in all, about 0.05 s each."""
import functools

import mpmath as mp
import numpy as np

mp.mp.dps = 40

DT = 0.005
STEP = mp.mpf("1e-14")


def vn100():
    """the reference's VN100 variances (gtsam/imu_vn100.cpp:24-67), restated from the data sheet figures"""
    d2r = np.pi / 180
    return ((0.14e-3 * 9.81) ** 2, (0.0035 * d2r) ** 2, 1e-4, ((0.04e-3 * 9.81) * np.sqrt(200)) ** 2, ((10 * d2r / 3600) * np.sqrt(200)) ** 2, 1e-3)


SPREAD_A = (1e-2, 1e-8, 1e-2, 1e-12, 1e-14, 0.0)         # cond(cov) 1e12, 1.0 after diagonal scaling (8 samples); biasAccOmegaInt = 0
SPREAD_B = (1e-6, 1e-6, 1e-10, 1e-3, 1e-3, 1e-3)         # cond(cov) 9e3, 12 after diagonal scaling (8 samples)
BHAT = (0.02, -0.01, 0.03, 0.002, -0.001, 0.0015)
SWITCHES = (1e-10, 0.25)                                   # quat_exp; right_jacobian (enters F and Q)


# ---------------------------------------------------------------------------------------------------------------- inputs
def _smooth(rng, n, scale_w, scale_a=1.5):
    t = np.arange(n) * DT
    w = np.stack([scale_w * np.sin(2.1 * t + p) for p in rng.uniform(0, 6, 3)], 1).reshape(n, 3)
    a = np.stack([scale_a * np.cos(1.3 * t + p) for p in rng.uniform(0, 6, 3)], 1).reshape(n, 3) + np.array([0, 0, -9.71])
    return a, w


def _constant(rng, n, angle, axis, bhat):
    """n samples whose rotation per sample |(gyro - bg) dt| is `angle` about `axis`"""
    a, _ = _smooth(rng, n, 0.0)
    bg = np.zeros(3) if bhat is None else np.asarray(bhat[3:])
    return a, np.tile(angle / DT * np.asarray(axis) + bg, (n, 1))


@functools.lru_cache(maxsize=None)
def cases():
    """tuple of dict(name, acc n x 3, gyro n x 3, dt, bhat (None or 6), params (6))"""
    rng = np.random.default_rng(20266)
    ax1, ax2 = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0), np.array([-2.0, 1.0, 0.5]) / np.sqrt(5.25)
    out = []

    def add(name, acc, gyro, bhat, params):
        out.append(dict(name=name, acc=np.ascontiguousarray(acc), gyro=np.ascontiguousarray(gyro), dt=DT,
                        bhat=None if bhat is None else np.array(bhat), params=tuple(params)))

    for n in (0, 1, 2, 3, 8, 16, 40):                                       # 70 samples
        a, w = _smooth(rng, n, 0.4)
        add("n%d" % n, a, w, BHAT if n % 2 else None, vn100())
    add("gyro_zero", *_constant(rng, 3, 0.0, ax1, None), None, vn100())                         # 3
    for f in (0.9, 1.1):                                                                        # 4 + 6
        add("exp_%.1f" % f, *_constant(rng, 2, f * SWITCHES[0], ax2, None), None, vn100())
        add("jr_%.1f" % f, *_constant(rng, 3, f * SWITCHES[1], ax1, BHAT), BHAT, vn100())
    add("past_pi", *_constant(rng, 8, 0.45, ax2, BHAT), BHAT, vn100())                          # 8: 3.6 rad about one axis
    a, w = _smooth(rng, 8, 60.0)                                                                # 8: 0.3 rad per sample, the axis moves
    add("fast", a, w, None, vn100())
    a, w = _smooth(rng, 8, 0.4)                                                                 # 8 + 8
    add("spread_a", a, w, BHAT, SPREAD_A)
    a, w = _smooth(rng, 8, 0.4)
    add("spread_b", a, w, None, SPREAD_B)
    assert sum(len(c["acc"]) for c in out) <= 120
    return tuple(out)


def angle_per_sample(case):
    """|(gyro - bg) dt| of every sample, as the code under test forms it"""
    bg = np.zeros(3) if case["bhat"] is None else case["bhat"][3:]
    return np.array([np.sqrt((((w - bg) * case["dt"]) ** 2).sum()) for w in case["gyro"]])


# ------------------------------------------------------------------------------------------------------------- reference
def _hat(w):
    return mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def _step(x, acc, gyro, dt, cache):
    R, p, v, ba, bg = x
    w = tuple((gyro[k] - bg[k]) * dt for k in range(3))
    if w not in cache:
        cache[w] = mp.expm(_hat(w))
    Ra = R * (acc - ba)
    return R * cache[w], p + v * dt + Ra * (dt * dt / 2), v + Ra * dt, ba, bg


def _oplus(x, k, h):
    """x (+) h e_k"""
    R, p, v, ba, bg = x
    e = mp.zeros(3, 1)
    e[k % 3] = h
    b = k // 3
    if b == 0: return R * mp.expm(_hat(e)), p, v, ba, bg
    if b == 1: return R, p + R * e, v, ba, bg
    if b == 2: return R, p, v + R * e, ba, bg
    if b == 3: return R, p, v, ba + e, bg
    return R, p, v, ba, bg + e


def _local(x1, x0):
    E = x0[0].T * x1[0]
    th = [(E[2, 1] - E[1, 2]) / 2, (E[0, 2] - E[2, 0]) / 2, (E[1, 0] - E[0, 1]) / 2]
    dp, dv, dba, dbg = x0[0].T * (x1[1] - x0[1]), x0[0].T * (x1[2] - x0[2]), x1[3] - x0[3], x1[4] - x0[4]
    return th + [u[k] for u in (dp, dv, dba, dbg) for k in range(3)]


def transition(x, acc, gyro, dt, h=STEP):
    """(F 15 x 15, step(x)) of one sample at state x"""
    cache = {}
    x1 = _step(x, acc, gyro, dt, cache)
    F = mp.zeros(15, 15)
    for k in range(15):
        lp = _local(_step(_oplus(x, k, h), acc, gyro, dt, cache), x1)
        lm = _local(_step(_oplus(x, k, -h), acc, gyro, dt, cache), x1)
        for r in range(15):
            F[r, k] = (lp[r] - lm[r]) / (2 * h)
    return F, x1


def noise(F, dt, params):
    pa, pg, pi, pba, pbg, pint = (mp.mpf(float(v)) for v in params)
    Q = mp.zeros(15, 15)
    Tb, Vb = F[0:3, 12:15], F[6:9, 9:12]
    Q[0:3, 0:3] = (pg + pint) / dt * (Tb * Tb.T)
    Q[6:9, 6:9] = (pa + pint) / dt * (Vb * Vb.T)
    for k in range(3):
        Q[3 + k, 3 + k] = dt * pi; Q[9 + k, 9 + k] = dt * pba; Q[12 + k, 12 + k] = dt * pbg
    return Q


def covariance_mp(acc, gyro, dt, bhat, params, h=STEP):
    """the 40-digit covariance after all samples (mpmath 15 x 15)"""
    v3 = lambda a: mp.matrix([mp.mpf(float(u)) for u in a])
    b = np.zeros(6) if bhat is None else np.asarray(bhat, float)
    x = (mp.eye(3), mp.zeros(3, 1), mp.zeros(3, 1), v3(b[:3]), v3(b[3:]))
    dt = mp.mpf(float(dt))
    S = mp.zeros(15, 15)
    for a, w in zip(np.asarray(acc, float).reshape(-1, 3), np.asarray(gyro, float).reshape(-1, 3)):
        F, x = transition(x, v3(a), v3(w), dt, h)
        S = F * S * F.T + noise(F, dt, params)
    return S


def _f(M):
    return np.array([[float(M[r, c]) for c in range(M.cols)] for r in range(M.rows)])


def covariance(acc, gyro, dt, bhat, params):
    return _f(covariance_mp(acc, gyro, dt, bhat, params))


def information(C):
    """40-digit inverse of C (numpy array, read exactly, or mpmath matrix) as floats"""
    if not isinstance(C, mp.matrix):
        C = mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.asarray(C)])
    return _f(mp.inverse(C))


@functools.lru_cache(maxsize=None)
def reference(k):
    """(covariance as floats, its 40-digit inverse as floats or None for the empty case) of cases()[k]"""
    c = cases()[k]
    S = covariance_mp(c["acc"], c["gyro"], c["dt"], c["bhat"], c["params"])
    return _f(S), (information(S) if len(c["acc"]) else None)


def scaled_error(C, Cref):
    """max_ij |C - C*|_ij / sqrt(C*_ii C*_jj); where C* is exactly zero the entry must be below 1e-30 in absolute value (returned as inf if not)"""
    d = np.sqrt(np.abs(np.diag(Cref)))
    zero = Cref == 0.0
    if np.any(np.abs(C[zero]) > 1e-30):
        return np.inf
    s = np.outer(d, d)
    if zero.all():
        return 0.0
    return float((np.abs(C - Cref)[~zero] / s[~zero]).max())


def params9(case):
    """fgo_imu_params as the doubles it is made of: the six variances and the reference's gravity"""
    return np.array(list(case["params"]) + [0.0, 0.0, 9.71])


@functools.lru_cache(maxsize=None)
def oracle_error(k):
    """scaled_error of oracle/orc_imu.h's covariance on cases()[k]: the yardstick of the host's and the device's bound"""
    from tests import orc_binding as orc
    c = cases()[k]
    o = orc.Preint(np.zeros(6) if c["bhat"] is None else c["bhat"], c["acc"], c["gyro"], c["dt"], variances=c["params"])
    return scaled_error(o.cov, reference(k)[0])


def product_bound(k):
    """16 x the oracle's own error on the case (two implementations of one recursion differ by FMA contraction and summation order, not by
    more than the recursion's own rounding), and no less than one unit in the last place of an entry the size of its diagonal.  The
    oracle's error counts only up to the oracle's own bound, 64 eps max(1, n): an error that product and oracle share must not widen this."""
    n = len(cases()[k]["acc"])
    return max(16.0 * min(oracle_error(k), 64 * EPS * max(1, n)), EPS)


def scaled_cond(C):
    """2-norm condition number of the diagonally equilibrated C"""
    d = 1.0 / np.sqrt(np.diag(C))
    return float(np.linalg.cond(C * np.outer(d, d)))


EPS = 2.0 ** -52
INFO_BOUND = 8.0          # in units of EPS * scaled_cond: a Cholesky inverse of the equilibrated matrix errs by a small multiple of that


def information_error(W, C):
    """(max_ij |W - W*|_ij / sqrt(W*_ii W*_jj), scaled_cond(C)) with W* the 40-digit inverse of the float matrix C"""
    Wr = information(C)
    d = np.sqrt(np.diag(Wr))
    return float((np.abs(np.asarray(W) - Wr) / np.outer(d, d)).max()), scaled_cond(np.asarray(C))


# ------------------------------------------------------------------------------------------- raw samples -> H: one graph of IMU factors
FREE = ("n16", "n40", "jr_1.1")         # three factors on variables of their own
CHAIN = ("n8", "n3")                    # two factors through one middle key frame; the chain's first pose is fixed
N_KEY = 9                               # poses 0 .. 8 (2 f, 2 f + 1 of free factor f; 6, 7, 8 the chain), velocities 9 .. 17, biases 18 .. 26
FIXED_POSE = 6


@functools.lru_cache(maxsize=None)
def reference_preint(k):
    """orc.Preint as a container of the reference's numbers for cases()[k]: deltas and bias Jacobians from tests.chart_edges.preintegrate,
    the covariance from this module"""
    from tests import chart_edges as ce
    from tests import orc_binding as orc
    c = cases()[k]
    bhat = np.zeros(6) if c["bhat"] is None else c["bhat"]
    ref = ce.preintegrate(c["acc"], c["gyro"], c["dt"], bhat)
    buf = np.concatenate([[len(c["acc"]) * c["dt"]], ce.quat_of(ref["dR"]), ref["dp"], ref["dv"]] +
                         [ref[n].ravel() for n in ("J_R_bg", "J_p_ba", "J_p_bg", "J_v_ba", "J_v_bg")] + [bhat, reference(k)[0].ravel()])
    return orc.Preint.from_buf(buf)


@functools.lru_cache(maxsize=None)
def imu_only_graph():
    """dict(ks: case of every factor, ids: its six variables X_i V_i X_j V_j B_i B_j, poses / vels / bias (N_KEY each), fixed (poses), states:
    (xi, vi, xj, vj, bi, bj) per factor, a way off the prediction as tests.test_independent_imu._case places them; the prediction only places
    the input)"""
    from tests.util import noisy, random_pose
    rng = np.random.default_rng(316)
    names = [c["name"] for c in cases()]
    ks = [names.index(n) for n in FREE + CHAIN]
    assert all(cases()[k]["params"] == vn100() for k in ks)
    pims = [reference_preint(k) for k in ks]

    def state(pim, xi=None, vi=None, bi=None):
        xi = random_pose(rng, 1.0) if xi is None else xi
        vi = rng.normal(size=3) if vi is None else vi
        bi = pim.bhat + rng.normal(size=6) * 0.02 if bi is None else bi
        xp, vp = pim.predict(xi, vi, bi)
        return xi, vi, noisy(rng, xp, 0.1, 0.15), vp + rng.normal(size=3) * 0.2, bi, bi + rng.normal(size=6) * 0.01

    nf = len(FREE)
    states = [state(pims[f]) for f in range(nf)]
    s0 = state(pims[nf])
    s1 = state(pims[nf + 1], xi=s0[2], vi=s0[3], bi=s0[5])
    states += [s0, s1]
    pick = lambda a, b: np.array([p for s in states[:nf] for p in (s[a], s[b])] + [s0[a], s0[b], s1[b]])
    ids = [[2 * f, 9 + 2 * f, 2 * f + 1, 10 + 2 * f, 18 + 2 * f, 19 + 2 * f] for f in range(nf)] + [[6, 15, 7, 16, 24, 25], [7, 16, 8, 17, 25, 26]]
    fixed = np.zeros(N_KEY, np.uint8); fixed[FIXED_POSE] = 1
    return dict(ks=ks, ids=ids, poses=pick(0, 2), vels=pick(1, 3), bias=pick(4, 5), fixed=fixed, states=states)


def _col(v):
    """first dense column of variable v: the order the variables were added in, six scalars each, the fixed pose left out"""
    return None if v == FIXED_POSE else 6 * (v if v < FIXED_POSE else v - 1)


@functools.lru_cache(maxsize=None)
def reference_system():
    """(H, b, chi2) of imu_only_graph(): r and J of every factor from tests.imu_independent.factor read through reference_preint, W the
    40-digit inverse of the 40-digit covariance; J^T W J, -J^T W r, r^T W r with the fixed pose's columns dropped"""
    from tests import imu_independent as imu
    from tests import orc_binding as orc
    g = imu_only_graph()
    m = 6 * (3 * N_KEY - 1)
    H, b, chi = np.zeros((m, m)), np.zeros(m), 0.0
    for f, k in enumerate(g["ks"]):
        r, Js = imu.factor(*g["states"][f], reference_preint(k), orc.GRAVITY)
        W = reference(k)[1]
        J = np.zeros((15, m))
        for v, Jk in zip(g["ids"][f], Js):
            if _col(v) is not None:
                J[:, _col(v):_col(v) + Jk.shape[1]] = Jk
        H += J.T @ W @ J; b -= J.T @ W @ r; chi += r @ W @ r
    return H, b, chi


def system_errors(chi, H, b):
    """per connected component of imu_only_graph() (the three free factors, the chain): (largest |H - H*| over the largest |H*| of the
    component, largest |b - b*| over max(1, largest |b*|)) as tests/test_gpu_independent.py scales them; then the relative error of chi2.
    Asserts that nothing couples two components.  The padding rows of the 3-dof velocities are left out."""
    g = imu_only_graph()
    Href, bref, cref = reference_system()
    assert H.shape == Href.shape and b.shape == bref.shape
    pad = np.zeros(len(b), bool)
    for v in range(N_KEY, 2 * N_KEY):
        pad[_col(v) + 3:_col(v) + 6] = True
    nf = len(FREE)
    comps = [sorted(g["ids"][f]) for f in range(nf)] + [sorted(set(g["ids"][nf] + g["ids"][nf + 1]) - {FIXED_POSE})]
    member = np.full(len(b), -1)
    out = []
    for q, comp in enumerate(comps):
        sel = np.concatenate([np.arange(_col(v), _col(v) + 6) for v in comp])
        member[sel] = q
        sel = sel[~pad[sel]]
        sub = np.ix_(sel, sel)
        out.append((float(np.abs(H[sub] - Href[sub]).max() / np.abs(Href[sub]).max()),
                    float(np.abs(b[sel] - bref[sel]).max() / max(1.0, np.abs(bref[sel]).max()))))
    assert np.all(member >= 0) and not H[member[:, None] != member[None, :]].any()
    return out, abs(chi - cref) / cref
