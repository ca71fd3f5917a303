"""GPU: the device's manifold arithmetic (csrc/pose3_device.hpp, imu_device.hpp, factors_device.hpp, preint_kernel.hip; host imu_preint.cpp) at its
branch points, read back through the C-ABI and held to the 40-digit references of tests/chart_edges.py -- the inputs of
tests/test_chart_edges_cpu.py (exactly zero, 1e-12 ... 1, either side of every switch, towards pi, tied plane normals, small depths) through
the kernels: k_linearize_gtsam, k_imu_eval, k_preint_batch, the retraction of k_isam2_estimate and the two-view kernel.

Bounds of the H, b, chi2 comparisons: every test runs a control group of random inputs through the same context and prints its worst error
relative to max |H_k|; the edge inputs must stay within 10 x that (input-to-input variation) and never looser than the 1e-9 max |H_k| of
tests/test_gpu_independent.py.  Residual rotations within 0.1 of pi get NEAR_PI times more: measured on the CPU (fixed oracle, same formulas,
against mpmath) the Jacobian error there is 1.1e-14 at pi - 1e-3 against 3.1e-15 for the worst other input, conditioning growing like
1 / (pi - theta).  The measured figures are in profiles/NOTES.md ("Chart arithmetic at its branch points").

Where the time goes: nearly all of this file's run time is checker cost on the CPU -- the 40-digit references, about 0.2 s each, computed once per
process (lru_cache) and shared by the parametrised tests -- not kernel time: every launch and read-back here takes milliseconds."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import graph_slam_amd as G
from tests import chart_edges as ce
from tests import orc_binding as orc
from tests import pose3_independent as p3
from tests import se3_independent as ind
from tests.util import random_info, info_ut, SR4000_CALIB

NEAR_PI = 4.0
# the sphere chart at pi - 1e-3 from the prediction: the direction of the step comes from an orthogonal component of length 1e-3 that carries the
# rounding of unit vectors, i.e. conditioning 1 / (pi - theta) = 1e3 against about 3 for the control group (angles up to 0.3); measured on the
# CPU 7.0e-14 in b against 2.4e-16 for the worst other plane input
NEAR_ANTIPODE = 300.0
CAP = 1e-9


def _bound(control_worst):
    """10 x the control group's worst, at most the 1e-9 of tests/test_gpu_independent.py -- and at least 2^-53: an H block whose every entry is
    the correctly rounded double of the exact value is already that far from it, relative to its largest entry, so no arithmetic can be held
    below it.  (The floor matters for the IMU blocks alone: their largest entries come from the bias rows, whose Jacobian is +-I, and the
    control group's worst is 5e-18 there, a twentieth of one rounding of those entries.)"""
    return min(max(10.0 * control_worst, 2.0 ** -53), CAP)


# ------------------------------------------------------------------------------------------------------- between / prior
@functools.lru_cache(maxsize=None)
def _between_inputs():
    """edge cases first, then the control group of tests/test_gpu_independent.py (24 random triples); references computed once"""
    from tests.test_independent_pose3 import _triples
    edge = [(name, angle, xi, xj, z) for name, angle, xi, xj, z in ce.pose_cases()]
    ctrl = [("control%d" % k, None, xi, xj, z) for k, (xi, xj, z) in enumerate(_triples(np.random.default_rng(4712), 24))]
    cases = edge + ctrl
    return cases, [ce.between(xi, xj, z) for _, _, xi, xj, z in cases]


@functools.lru_cache(maxsize=None)
def _prior_inputs():
    from tests.util import random_pose, pose_mul, noisy
    rng = np.random.default_rng(4713)
    ctrl = []
    for k in range(12):
        x = random_pose(rng, 2.0)
        ctrl.append(("control%d" % k, None, x, pose_mul(x, noisy(rng, ce.IDENT, 0.3, 0.3))))
    cases = list(ce.prior_cases()) + ctrl
    return cases, [ce.prior(x, m) for _, _, x, m in cases]


def _err_H(name, angle, got, want):
    return name, angle, np.abs(got - want).max(), np.abs(want).max(), np.abs(want).max()


def _err_b(name, angle, got, want, JtW):
    """two scales: max(1, |b|), the one of tests/test_gpu_independent.py, for the 1e-9 cap; and for the comparison with the control group the
    larger of that and max |J^T W|: the variables are O(1), so a residual carries an absolute rounding error of a few eps however small it is,
    and b = -J^T W r inherits it times J^T W -- relative to |b| alone an input whose residual is (nearly) zero would compare noise with noise"""
    cap_scale = max(1.0, np.abs(want).max())
    return name, angle, np.abs(got - want).max(), cap_scale, max(cap_scale, np.abs(JtW).max())


def _judge(what, errs, near_pi=NEAR_PI):
    """errs: list of (name, angle or None for control, absolute error, scale of the existing 1e-9 bound, scale for the control comparison)"""
    for n, a, e, cap_scale, _ in errs:
        assert e <= CAP * cap_scale, (what, n, e, cap_scale)
    ctrl = max(e / sc for _, a, e, _, sc in errs if a is None)
    edge = [(e / sc / (near_pi if ce.is_near_pi(a) else 1.0), n) for n, a, e, _, sc in errs if a is not None]
    worst, name = max(edge)
    raw = max([e / sc for _, a, e, _, sc in errs if a is not None and ce.is_near_pi(a)] or [0.0])
    print("%s: control worst %.2e, edge worst %.2e (%s), near pi %.2e (allowed %g x), bound %.2e" % (what, ctrl, worst, name, raw, near_pi, _bound(ctrl)))
    assert worst <= _bound(ctrl), (what, name, worst, ctrl)


@pytest.mark.parametrize("weight", ["unit", "spd"])
def test_between_and_prior_blocks_at_the_branch_points(weight):
    bc, bref = _between_inputs()
    pc, pref = _prior_inputs()
    rng = np.random.default_rng(91)
    W = np.eye(6) if weight == "unit" else ind.info_full(info_ut(random_info(rng)))
    Wp = np.eye(6) if weight == "unit" else ind.info_full(info_ut(random_info(rng)))
    n = 2 * len(bc)
    poses = np.array([p for _, _, xi, xj, _ in bc for p in (xi, xj)] + [x for _, _, x, _ in pc])
    ei = np.arange(0, n, 2, dtype=np.int64)
    gr = G.Graph()
    gr.add_poses(poses, np.zeros(len(poses), np.uint8))
    gr.add_edges(ei, ei + 1, np.array([z for *_, z in bc]), np.tile(info_ut(W), (len(bc), 1)), tangent_order=G.FGO_TANGENT_GTSAM)
    for k, (_, _, x, m) in enumerate(pc):
        gr.add_prior(n + k, m, info_ut(Wp))
    chi, H, b = gr.linearize(dense=True)
    gr.close()
    assert H.shape == (6 * len(poses),) * 2
    eH, eb, chi_ref = [], [], 0.0
    for k, ((name, angle, *_), (e, Ji, Jj)) in enumerate(zip(bc, bref)):
        J = np.hstack([Ji, Jj])
        Hk, bk = J.T @ W @ J, -J.T @ W @ e
        chi_ref += e @ W @ e
        idx = np.r_[12 * k:12 * k + 12]
        eH.append(_err_H(name, angle, H[np.ix_(idx, idx)], Hk))
        eb.append(_err_b(name, angle, b[idx], bk, J.T @ W))
    for k, ((name, angle, *_), (e, J)) in enumerate(zip(pc, pref)):
        Hk, bk = J.T @ Wp @ J, -J.T @ Wp @ e
        chi_ref += e @ Wp @ e
        idx = np.r_[6 * (n + k):6 * (n + k) + 6]
        eH.append(_err_H("prior " + name, angle, H[np.ix_(idx, idx)], Hk))
        eb.append(_err_b("prior " + name, angle, b[idx], bk, J.T @ Wp))
    off = H.copy()
    for k in range(len(bc)):
        off[12 * k:12 * k + 12, 12 * k:12 * k + 12] = 0
    for k in range(len(pc)):
        off[6 * (n + k):6 * (n + k) + 6, 6 * (n + k):6 * (n + k) + 6] = 0
    assert not off.any()                                       # disjoint pairs: nothing outside the blocks
    _judge("between/prior H (%s)" % weight, eH)
    _judge("between/prior b (%s)" % weight, eb)
    print("chi2 relative error %.2e" % (abs(chi - chi_ref) / chi_ref))
    assert abs(chi - chi_ref) <= 1e-12 * chi_ref


# ---------------------------------------------------------------------------------------------------------------- planes
@functools.lru_cache(maxsize=None)
def _plane_inputs():
    rng = np.random.default_rng(4714)
    ctrl = []
    for k in range(24):
        x = ce._rng_pose(rng, 2.0)
        n = ce._unit(rng.normal(size=3)); d = rng.uniform(-1, 1)
        npred = ce.rotmat(x[3:]).T @ n
        ctrl.append((None, x, np.r_[n, d], np.r_[ce._tilt(npred, rng.uniform(0.01, 0.3), rng.uniform(0, 6)), n @ x[:3] + d + rng.normal() * 0.05]))
    edge = [(float(np.arccos(np.clip(ce.rotmat(x[3:]).T @ pl[:3] @ z[:3], -1, 1))), x, pl, z) for x, pl, z in ce.plane_factor_cases()]
    cases = edge + ctrl
    return cases, [ce.plane_factor(x, pl, z) for _, x, pl, z in cases]


@pytest.mark.parametrize("weight", ["unit", "spd"])
def test_plane_factor_blocks_on_tied_normals_and_tiny_angles(weight):
    cases, ref = _plane_inputs()
    rng = np.random.default_rng(92)
    if weight == "unit":
        S = np.eye(3)
    else:
        A = rng.normal(size=(3, 3)); S = A @ A.T * 1e-2 + np.eye(3) * 1e-2          # Gaussian::Covariance(S)
    W = np.linalg.inv(S)
    n = len(cases)
    gr = G.Graph()
    gr.add_poses(np.array([x for _, x, _, _ in cases]), np.zeros(n, np.uint8))
    for k, (_, x, pl, z) in enumerate(cases):
        gr.add_plane(n + k, pl)
        gr.add_plane_factor(k, n + k, z, [S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2]])
    chi, H, b = gr.linearize(dense=True)
    gr.close()
    eH, eb, chi_ref = [], [], 0.0
    for k, ((angle, x, pl, z), (r, Hx, Hp)) in enumerate(zip(cases, ref)):
        J = np.hstack([Hx, Hp])
        Hk, bk = J.T @ W @ J, -J.T @ W @ r
        chi_ref += r @ W @ r
        idx = np.r_[6 * k:6 * k + 6, 6 * (n + k):6 * (n + k) + 3]
        name = "plane%d" % k
        eH.append(_err_H(name, angle, H[np.ix_(idx, idx)], Hk))
        eb.append(_err_b(name, angle, b[idx], bk, J.T @ W))
    _judge("plane H (%s)" % weight, eH, NEAR_ANTIPODE)
    _judge("plane b (%s)" % weight, eb, NEAR_ANTIPODE)
    assert abs(chi - chi_ref) <= 1e-12 * chi_ref


# ------------------------------------------------------------------------------------------------------------------ IMU
@functools.lru_cache(maxsize=None)
def _imu_inputs():
    """every case of ce.imu_cases() (exactly zero, both angles swept over 1e-12 ... 1, every bracket, towards pi), then the control group:
    twelve random cases of tests/test_independent_imu.py"""
    from tests.test_independent_imu import _case
    rng = np.random.default_rng(315)
    cases = [(ce.IMU_ANGLES[k], c) for k, c in enumerate(ce.imu_cases())] + [(None, _case(rng)) for _ in range(12)]
    return cases, [ce.imu_factor(*c[:6], c[6], orc.GRAVITY) for _, c in cases]


def test_combined_imu_factor_blocks_with_swept_bias_correction_and_residual_angles():
    """one context of disjoint one-factor groups (X_i, X_j, V_i, V_j, B_i, B_j added in that order, so group c owns columns 36 c ... 36 c + 35);
    the existing bound of tests/test_gpu_independent.py is 1e-8 max |H|, the cap here stays 1e-9"""
    cases, ref = _imu_inputs()
    gr = G.Graph()
    gr.set_gravity(orc.GRAVITY)
    for c, (_, (xi, vi, xj, vj, bi, bj, pim)) in enumerate(cases):
        o = 6 * c
        gr.add_poses(np.array([xi, xj]), ids=[o, o + 1])
        gr.add_vec3(o + 2, vi); gr.add_vec3(o + 3, vj)
        gr.add_bias(o + 4, bi); gr.add_bias(o + 5, bj)
        gr.add_imu([o, o + 2, o + 1, o + 3, o + 4, o + 5], pim.buf)          # X(i) V(i) X(j) V(j) B(i) B(j)
    chi, H, b = gr.linearize(dense=True)
    gr.close()
    assert H.shape == (36 * len(cases),) * 2
    eH, eb, chi_ref = [], [], 0.0
    keep = np.ones(36, bool); keep[15:18] = False; keep[21:24] = False          # the padding of the two velocities
    for c, ((angles, (*_, pim)), (r, Js)) in enumerate(zip(cases, ref)):
        W = G.preint_information(pim.buf)
        J = np.zeros((15, 36))
        for c0, Jk in zip((0, 12, 6, 18, 24, 30), Js):                          # Jacobians come as xi vi xj vj bi bj
            J[:, c0:c0 + Jk.shape[1]] = Jk
        Href, bref = J.T @ W @ J, -J.T @ W @ r
        chi_ref += r @ W @ r
        idx = np.arange(36 * c, 36 * c + 36)[keep]
        name, angle = str(angles), None if angles is None else angles[1]
        eH.append(_err_H(name, angle, H[np.ix_(idx, idx)], Href[np.ix_(keep, keep)]))
        eb.append(_err_b(name, angle, b[idx], bref[keep], J.T @ W))
    _judge("imu H", eH)
    _judge("imu b", eb)
    print("chi2 relative error %.2e" % (abs(chi - chi_ref) / chi_ref))
    assert abs(chi - chi_ref) <= 1e-9 * chi_ref


# ---------------------------------------------------------------------------------------------------------- reprojection
def test_reprojection_blocks_at_small_depth():
    """H blocks and both pieces of b on the scale tests/test_gpu_independent.py uses for this factor, max(1, max |J|^2).
    tests/camera_independent.py is in double precision, so the bound carries the conditioning term derived in tests/test_chart_edges_cpu.py
    (relative error 16 eps s / |depth| of the normalised coordinates, twice that in H's factors J); the control group (depth 1 ... 6, where that
    term is 1e-14) sets the base as elsewhere"""
    from tests import camera_independent as cam
    from tests.util import random_pose, pose_mul, quat_rot
    rng = np.random.default_rng(2029)
    bps = random_pose(rng, 0.1)
    cases = [(depth, x, pw, uv, b) for x, pw, uv, b, depth in ce.reproj_cases(SR4000_CALIB, [ce.IDENT, bps])]
    errs = {}
    for b_ in (ce.IDENT, bps):
        sub = [c for c in cases if c[4] is b_]
        for k in range(12):                                                        # control: points well in front of the camera
            x = random_pose(rng, 1.0); c = pose_mul(x, b_)
            sub.append((None, x, c[:3] + quat_rot(c[3:], np.array([rng.normal() * 0.4, rng.normal() * 0.4, rng.uniform(1, 6)])), rng.uniform(0, 180, size=2), b_))
        n = len(sub)
        gr = G.Graph()
        gr.add_poses(np.array([c[1] for c in sub]), np.zeros(n, np.uint8))
        gr.set_calibration(SR4000_CALIB, b_)
        for k, (_, x, pw, uv, _) in enumerate(sub):
            gr.add_point(n + k, pw)
            gr.add_reproj(k, n + k, uv, 1.0)
        chi, H, b = gr.linearize(dense=True)
        gr.close()
        chi_ref = 0.0
        for k, (depth, x, pw, uv, _) in enumerate(sub):
            r, Hx, Hp = cam.reproj_ad(x, pw, uv, SR4000_CALIB, b_)
            chi_ref += r @ r
            J = np.hstack([Hx, Hp])
            Hk, bk = J.T @ J, -J.T @ r
            idx = np.r_[6 * k:6 * k + 6, 6 * (n + k):6 * (n + k) + 3]
            if not J.any():                                                        # behind the camera: zero blocks, exactly
                assert not H[np.ix_(idx[:6], idx)].any() and not b[idx[:6]].any()
                continue
            cond = 0.0 if depth is None else 16 * np.finfo(float).eps * max(1.0, np.abs(x[:3]).max(), np.abs(pw).max()) / abs(depth)
            sc = max(1.0, np.abs(J).max() ** 2)
            eH = np.abs(H[np.ix_(idx, idx)] - Hk).max() / sc
            eb = np.abs(b[idx] - bk).max() / sc
            errs.setdefault("control" if depth is None else "edge", []).append((max(eH, eb), cond, depth))
        assert abs(chi - chi_ref) <= 1e-9 * chi_ref
    ctrl = max(e for e, _, _ in errs["control"])
    print("reprojection: control worst %.2e; edge (error, conditioning term, depth): %s" % (ctrl, ["%.1e %.1e %g" % t for t in errs["edge"]]))
    for e, cond, depth in errs["edge"]:
        assert e <= min(_bound(ctrl) + 4 * cond, CAP), (e, cond, depth)


# ------------------------------------------------------------------------------------------------------- preintegration
def test_preintegration_of_constant_gyro_runs_across_the_switch():
    """k_preint_batch and the host's fgo_preint_integrate: 200 samples at constant rate, rotation per sample 1e-7 ... 1e-3 with 0.9e-5 and 1.1e-5
    (where so3_dexp switched) and either side of 0.25 (where it switches now); dR, dp, dv and the bias Jacobians against the definition at 40
    digits.  Absolute bounds as on the CPU: 1e-12 on the state, 1e-10 on the Jacobians, times max(1, |dp|, |dv|)."""
    dt, ns = 0.005, 200
    rates = ce.GYRO_DT + [0.225, 0.275]
    acc = np.tile([0.4, -0.3, 9.5], (ns * len(rates), 1))
    gyro = np.concatenate([np.tile(a / dt * ce.AXES[k % 5], (ns, 1)) for k, a in enumerate(rates)])
    bhat = np.tile([0.01, -0.02, 0.015, 0.0, 0.0, 0.0], (len(rates), 1))
    out = G.preint_batch(np.arange(len(rates) + 1) * ns, acc, gyro, dt, bias_hat=bhat)
    for k, a in enumerate(rates):
        ref = ce.preintegrate(acc[:ns], gyro[k * ns:(k + 1) * ns], dt, bhat[k])
        s = max(1.0, np.abs(ref["dp"]).max(), np.abs(ref["dv"]).max())
        host = G.Preintegrator(bias_hat=bhat[k])
        for i in range(ns):
            host.integrate(acc[i], gyro[k * ns + i], dt)
        for who, buf in (("device", out[k]), ("host", host.buf)):
            pim = orc.Preint.from_buf(buf)                                                    # the payload layout is the oracle's
            np.testing.assert_allclose(ce.rotmat(pim.dR), ref["dR"], atol=1e-12, rtol=0, err_msg="%s %g" % (who, a))
            np.testing.assert_allclose(pim.dp, ref["dp"], atol=1e-12 * s, rtol=0, err_msg="%s %g" % (who, a))
            np.testing.assert_allclose(pim.dv, ref["dv"], atol=1e-12 * s, rtol=0, err_msg="%s %g" % (who, a))
            for name in ("J_R_bg", "J_p_ba", "J_p_bg", "J_v_ba", "J_v_bg"):
                np.testing.assert_allclose(getattr(pim, name), ref[name], atol=1e-10 * s, rtol=0, err_msg="%s %s %g" % (who, name, a))


# -------------------------------------------------------------------------------------------------------------- retract
def test_retract_on_the_device_with_tiny_rotation_steps():
    """pairs (A, B): A carries a prior whose mean is A Exp(xi), B a prior at itself, and one between factor ties them at the means, so the first
    ISAM2 update solves a step of about xi for A (tiny rotation, O(1) translation) and about zero for B.  With a huge relinearisation threshold
    (A context without a single binary factor is a configuration that neither the drivers nor any other test build; the pair keeps the update on
    the path every GTSAM-semantics graph takes, and the step of B, pulled by A's, is checked as well.)  theta stays put and get_poses() is theta (+) delta as k_isam2_estimate retracts it: held to X Exp(delta) at 40 digits with the DEVICE's own
    theta and delta, 1e-13 max(1, translation) as on the CPU, so only the retraction is under test."""
    from tests.util import pose_mul, pose_inv
    cases = ce.retract_cases()
    rng = np.random.default_rng(93)
    poses, means = [], []
    for _, x, d in cases:
        b = ce._rng_pose(rng, 2.0)
        poses += [x, b]; means += [p3.retract(x, d), b]
    n = len(poses)
    W = info_ut(np.diag([1e4] * 6))
    gr = G.Graph()
    gr.add_poses(np.array(poses), np.zeros(n, np.uint8))
    ei = np.arange(0, n, 2, dtype=np.int64)
    gr.add_edges(ei, ei + 1, np.array([pose_mul(pose_inv(means[i]), means[i + 1]) for i in ei]), np.tile(W, (len(ei), 1)), tangent_order=G.FGO_TANGENT_GTSAM)
    for v in range(n):
        gr.add_prior(v, means[v], W)
    gr.isam2_update(1e9)
    est = gr.get_poses()
    tiny = 0
    for v in range(n):
        th, de = gr.isam2_state(v)
        want = p3.retract(th, de)
        if want[3:] @ est[v, 3:] < 0:
            want[3:] *= -1
        np.testing.assert_allclose(est[v], want, atol=1e-13 * max(1.0, np.abs(th[:3]).max(), np.abs(de[3:]).max()), rtol=0, err_msg=str(cases[v // 2][0]))
        tiny += np.linalg.norm(de[:3]) < 1e-8 and np.linalg.norm(de[3:]) > 0.1
    gr.close()
    assert tiny >= 10, tiny                                     # steps with a tiny rotation and an O(1) translation part were part of it


# ------------------------------------------------------------------------------------------------------------- two-view
def test_two_view_pair_restarted_where_its_own_lm_ended():
    """pose j of a record is restarted where the kernel's LM ended, twice over (the record's points always start at their measured xyz and pose i
    at the identity: the entry point takes no other start).  Pose j is then at the joint optimum, its Gauss-Newton steps are the second-order
    remainder, and the third run moves it by less than 1e-8 rad in all (asserted; the oracle's own third run moves it by 6e-14): retract_pose3
    inside the kernel with rotation parts that small.  Iterations, trials, lambda, errors and poses against the oracle as in
    tests/test_gpu_two_view.py."""
    from tests.test_gpu_two_view import make_pair, run_oracle, run_batch, _check_vs_oracle
    start = None
    for _ in range(2):
        start = run_batch([make_pair(105, 20, 1.0, pose_j0=start)])["pose_j"][0]
    pr = make_pair(105, 20, 1.0, pose_j0=start)
    out = run_batch([pr])
    _check_vs_oracle(out, 0, run_oracle(pr))
    qa, qb = start[3:], out["pose_j"][0][3:]
    moved = 2.0 * np.linalg.norm(qa * np.sign(qa @ qb) - qb)
    print("pose j moved by %.2e rad, %.2e in translation over %d iterations" % (moved, np.abs(start[:3] - out["pose_j"][0][:3]).max(), out["iterations"][0]))
    assert out["iterations"][0] >= 1 and moved < 1e-8


def test_plane_retract_on_the_device():
    """a pose held by a prior sees a plane whose measurement is the transform of the plane RETRACTED by v, so the first ISAM2 update solves a
    step of about v for the plane (lengths 0, 1e-300, 1e-12 ... 1; axis-aligned and tied normals); the estimate is held to the 40-digit
    retraction of the device's own theta by the device's own delta"""
    cases = ce.plane_retract_cases()
    n = len(cases)
    rng = np.random.default_rng(94)
    poses = np.array([ce._rng_pose(rng, 1.0) for _ in range(n)])
    gr = G.Graph()
    gr.add_poses(poses, np.zeros(n, np.uint8))
    for k, (pl, v) in enumerate(cases):
        gr.add_prior(k, poses[k], info_ut(np.diag([1e8] * 6)))
        gr.add_plane(n + k, pl)
        target = ce.plane_retract(pl, v)
        z = orc.plane_transform(orc.plane(*target), poses[k])              # only places the measurement
        gr.add_plane_factor(k, n + k, z, [1e-4, 0, 0, 1e-4, 0, 1e-4])
    gr.isam2_update(1e9)
    est = gr.get_poses(ids=np.arange(n, 2 * n))
    moved = 0
    for k, (pl, v) in enumerate(cases):
        th, de = gr.isam2_state(n + k)
        want = ce.plane_retract(th[:4], de[:3])
        np.testing.assert_allclose(est[k, :4], want, atol=1e-13 * max(1.0, abs(th[3]), abs(de[2])), rtol=0, err_msg="%s %s" % (pl, v))
        moved += np.linalg.norm(de[:2]) > 0
    gr.close()
    assert moved >= n - 4, moved
