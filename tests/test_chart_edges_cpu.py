"""CPU: the oracle's manifold arithmetic at its branch points -- exactly zero, 1e-12 ... 1, either side of every series / closed-form switch, towards
pi, axis-aligned and tied plane normals, small depths -- against the 40-digit references of tests/chart_edges.py, which share no formula with it.
The oracle restates the product's formulas (oracle/orc_pose3.h, orc_imu.h, orc_plane.h == csrc/pose3_device.hpp, imu_device.hpp,
factors_device.hpp), so what fails here is wrong on the device too; tests/test_gpu_chart_edges.py runs the same inputs through the kernels.

Bounds are the ones tests/test_independent_pose3.py uses for random inputs: residual 1e-12, Jacobian 1e-10, retract 1e-13, each times
max(1, largest translation in the case)."""
import numpy as np

from tests import orc_binding as orc
from tests import chart_edges as ce
from tests import pose3_independent as p3

R_TOL, J_TOL, RETRACT_TOL = 1e-12, 1e-10, 1e-13


def _scale(*poses_or_vectors):
    return max(1.0, max(np.abs(np.asarray(a)[:3]).max() for a in poses_or_vectors))


def test_exponential_route_agrees_with_the_all_differences_route():
    """tests/chart_edges.between (Jacobians from the differentiated matrix exponential) against tests/pose3_independent.between (differences of
    matrix logarithms): two routes, both at 40 digits, agree far below double precision"""
    cases = {c[0]: c for c in ce.pose_cases()}
    picked = [n for n in cases if n.startswith(("a1.1e-05_t5_", "a0.275_t1_", "a1_t", "a3.16e-09_t"))]
    assert len(picked) == 4
    for n in picked:
        _, _, xi, xj, z = cases[n]
        r, Ji, Jj = ce.between(xi, xj, z)
        r2, Ji2, Jj2 = p3.between(xi, xj, z)
        assert max(np.abs(r - r2).max(), np.abs(Ji - Ji2).max(), np.abs(Jj - Jj2).max()) < 1e-20


def test_between_factor_at_the_branch_points():
    """Near pi (the last twelve cases) Logmap is ill conditioned like 1 / (pi - theta); measured there, fixed oracle against mpmath, scaled as
    below: residual 3.4e-16, Jacobians 1.7e-15 (pi - 1e-1), 3.3e-15 (pi - 1e-2), 1.1e-14 (pi - 1e-3).  Ten times that is still below the bounds
    for random inputs, so the same bounds hold for every case."""
    worst = {}
    for name, angle, xi, xj, z in ce.pose_cases():
        e, Ji, Jj = orc.between(xi, xj, z)
        e2, Ji2, Jj2 = ce.between(xi, xj, z)
        s = _scale(xi, xj, z, e2[3:])
        k = "near pi" if ce.is_near_pi(angle) else "rest"
        w = worst.setdefault(k, [0.0, 0.0])
        w[0] = max(w[0], np.abs(e - e2).max() / s); w[1] = max(w[1], np.abs(Ji - Ji2).max() / s, np.abs(Jj - Jj2).max() / s)
        np.testing.assert_allclose(e, e2, atol=R_TOL * s, rtol=0, err_msg=name)
        np.testing.assert_allclose(Ji, Ji2, atol=J_TOL * s, rtol=0, err_msg=name)
        np.testing.assert_allclose(Jj, Jj2, atol=J_TOL * s, rtol=0, err_msg=name)
    print("between: worst scaled error (residual, Jacobian)", worst)


def test_prior_factor_at_the_branch_points():
    for name, angle, x, mean in ce.prior_cases():
        e, J = orc.prior(x, mean)
        e2, J2 = ce.prior(x, mean)
        s = _scale(x, mean, e2[3:])
        np.testing.assert_allclose(e, e2, atol=R_TOL * s, rtol=0, err_msg=name)
        np.testing.assert_allclose(J, J2, atol=J_TOL * s, rtol=0, err_msg=name)


def test_retract_with_tiny_rotation_and_large_translation_steps():
    for name, x, d in ce.retract_cases():
        a, b = orc.retract(x, d), p3.retract(x, d)
        if a[3:] @ b[3:] < 0:
            b[3:] *= -1
        np.testing.assert_allclose(a, b, atol=RETRACT_TOL * _scale(x, d[3:]), rtol=0, err_msg=name)


def test_right_jacobian_and_one_preintegration_step():
    """one sample from rest: J_R_bg = -Jr(w dt) dt, so the oracle's SO(3) right Jacobian is read off it (dt a power of two: the division is exact)
    and held to the differentiated matrix exponential; dR, dp, dv and the other bias Jacobians of that step to the definition"""
    dt = 2.0 ** -8
    for angle, w in ce.dexp_cases():
        acc = np.array([[0.3, -0.2, 9.6]]); gyro = np.array([w / dt])
        pim = orc.Preint(np.zeros(6), acc, gyro, dt)
        Jr = ce.so3_right_jacobian(gyro[0] * dt)
        np.testing.assert_allclose(-pim.J_R_bg / dt, Jr, atol=J_TOL, rtol=0, err_msg=str(angle))
        ref = ce.preintegrate(acc, gyro, dt, np.zeros(6))
        np.testing.assert_allclose(ce.rotmat(pim.dR), ref["dR"], atol=R_TOL, rtol=0, err_msg=str(angle))
        np.testing.assert_allclose(pim.dp, ref["dp"], atol=R_TOL, rtol=0, err_msg=str(angle))
        np.testing.assert_allclose(pim.dv, ref["dv"], atol=R_TOL, rtol=0, err_msg=str(angle))
        for name in ("J_p_ba", "J_p_bg", "J_v_ba", "J_v_bg"):
            np.testing.assert_allclose(getattr(pim, name), ref[name], atol=J_TOL, rtol=0, err_msg="%s %g" % (name, angle))


def test_preintegration_of_constant_gyro_runs_across_the_switch():
    """200 samples at constant rate, rotation per sample 0, 1e-7 ... 1e-3 and either side of 1e-5 and 0.25: dR, dp, dv and the five bias Jacobians
    against the definition integrated at 40 digits"""
    dt, n = 0.005, 200
    for k, a in enumerate(ce.GYRO_DT_CPU):
        gyro = np.tile(a / dt * ce.AXES[k % 5], (n, 1)); acc = np.tile([0.4, -0.3, 9.5], (n, 1))
        bhat = np.array([0.01, -0.02, 0.015, 0.0, 0.0, 0.0])
        pim = orc.Preint(bhat, acc, gyro, dt)
        ref = ce.preintegrate(acc, gyro, dt, bhat)
        s = max(1.0, np.abs(ref["dp"]).max(), np.abs(ref["dv"]).max())
        np.testing.assert_allclose(ce.rotmat(pim.dR), ref["dR"], atol=R_TOL, rtol=0, err_msg=str(a))
        np.testing.assert_allclose(pim.dp, ref["dp"], atol=R_TOL * s, rtol=0, err_msg=str(a))
        np.testing.assert_allclose(pim.dv, ref["dv"], atol=R_TOL * s, rtol=0, err_msg=str(a))
        for name in ("J_R_bg", "J_p_ba", "J_p_bg", "J_v_ba", "J_v_bg"):
            np.testing.assert_allclose(getattr(pim, name), ref[name], atol=J_TOL * s, rtol=0, err_msg="%s %g" % (name, a))


def test_imu_exponential_route_agrees_with_the_all_differences_route():
    """tests/chart_edges.imu_factor against tests/imu_independent.factor (every column a difference of matrix logarithms) on a pair of tiny
    angles and a pair of large ones"""
    from tests import imu_independent as imu
    for k in (3, 30):
        c = ce.imu_cases()[k]
        r, Js = ce.imu_factor(*c[:6], c[6], orc.GRAVITY)
        r2, Js2 = imu.factor(*c[:6], c[6], orc.GRAVITY)
        assert np.abs(r - r2).max() < 1e-20, ce.IMU_ANGLES[k]
        for J, J2 in zip(Js, Js2):
            assert np.abs(J - J2).max() < 1e-18 * max(1.0, np.abs(J2).max()), ce.IMU_ANGLES[k]


def test_combined_imu_factor_with_swept_bias_correction_and_residual_angles():
    """bounds: those of tests/test_independent_imu.py (residual 1e-11, Jacobians 1e-9 max(1, |J|))"""
    for k, (xi, vi, xj, vj, bi, bj, pim) in enumerate(ce.imu_cases()):
        r, Js = pim.factor(xi, vi, xj, vj, bi, bj, g=orc.GRAVITY)
        r2, Js2 = ce.imu_factor(xi, vi, xj, vj, bi, bj, pim, orc.GRAVITY)
        np.testing.assert_allclose(r, r2, atol=1e-11, rtol=0, err_msg=str(ce.IMU_ANGLES[k]))
        for J, J2 in zip(Js, Js2):
            np.testing.assert_allclose(J, J2, atol=1e-9 * max(1.0, np.abs(J2).max()), rtol=0, err_msg=str(ce.IMU_ANGLES[k]))


def test_sphere_local_coordinates_from_zero_to_the_antipode():
    for n, y in ce.unit3_cases():
        got = orc.plane_local(np.r_[n, 0.0], np.r_[y, 0.0])[:2]
        np.testing.assert_allclose(got, ce.unit3_local(n, y), atol=R_TOL, rtol=0, err_msg="%s %s" % (n, y))
    n = ce.NORMALS[4]
    assert np.all(orc.plane_local(np.r_[n, 0.0], np.r_[n, 0.0]) == 0)
    np.testing.assert_array_equal(orc.plane_local(np.r_[n, 0.0], np.r_[-n, 0.0])[:2], [np.pi, 0.0])      # the antipodal convention


def test_sphere_local_coordinates_have_no_dead_zone():
    """the angle read back from the oracle's coordinates is the angle of the input to 1e-3 relative all the way down to 1e-12 (taking acos of the
    dot product returned exactly 0 below 1.5e-8)"""
    n = ce.NORMALS[-1]
    for ang in ce.PLANE_ANGLES[1:13]:
        y = ce._tilt(n, ang, 0.4)
        want = np.linalg.norm(ce.unit3_local(n, y))
        got = np.linalg.norm(orc.plane_local(np.r_[n, 0.0], np.r_[y, 0.0])[:2])
        assert abs(got - want) <= 1e-3 * want + 1e-16, (ang, got, want)


def test_plane_retract_steps_from_zero_to_one():
    for p, v in ce.plane_retract_cases():
        np.testing.assert_allclose(orc.plane_retract(p, v), ce.plane_retract(p, v), atol=RETRACT_TOL * max(1.0, abs(p[3])), rtol=0, err_msg="%s %s" % (p, v))


def test_plane_factor_on_axis_aligned_and_tied_normals():
    for x, pl, z in ce.plane_factor_cases():
        r, Hx, Hp = orc.plane_factor(x, pl, z)
        r2, Hx2, Hp2 = ce.plane_factor(x, pl, z)
        s = _scale(x)
        np.testing.assert_allclose(r, r2, atol=R_TOL * s, rtol=0, err_msg="%s %s" % (pl, z))
        np.testing.assert_allclose(Hx, Hx2, atol=J_TOL * s, rtol=0, err_msg="%s %s" % (pl, z))
        np.testing.assert_allclose(Hp, Hp2, atol=J_TOL * s, rtol=0, err_msg="%s %s" % (pl, z))


def test_reprojection_at_small_depth_on_both_sides_of_the_camera():
    """tests/camera_independent.py is in double precision (automatic differentiation), so both sides round.  The point in the camera frame comes
    out of a handful (say 16) of operations on numbers of size s = max(1, |t|, |p|), i.e. with an absolute error of 16 eps s; the division by the
    depth turns that into a RELATIVE error c = 16 eps s / |depth| of the normalised coordinates (3.6e-9 at depth 1e-6), hence fx c (1 + |xn|) in
    the residual, and twice that relative error in the Jacobians, whose entries go like 1 / depth^2.  Those terms are added to the usual bounds."""
    from tests import camera_independent as cam
    from tests.util import SR4000_CALIB
    bps = np.array([0.05, -0.02, 0.1, 0.1, -0.05, 0.02, 0.0]); bps[6] = np.sqrt(1 - bps[3:6] @ bps[3:6])
    behind = 0
    for x, pw, uv, b, depth in ce.reproj_cases(SR4000_CALIB, [ce.IDENT, bps]):
        r, Hx, Hp = orc.reproj(x, pw, uv, SR4000_CALIB, b)
        r2, Hx2, Hp2 = cam.reproj_ad(x, pw, uv, SR4000_CALIB, b)
        c = 16 * np.finfo(float).eps * max(1.0, np.abs(x[:3]).max(), np.abs(pw).max()) / abs(depth)
        np.testing.assert_allclose(r, r2, atol=R_TOL + 2 * SR4000_CALIB[0] * c, rtol=0, err_msg=str(depth))
        np.testing.assert_allclose(Hx, Hx2, atol=(J_TOL + 2 * c) * max(1.0, np.abs(Hx2).max()), rtol=0, err_msg=str(depth))
        np.testing.assert_allclose(Hp, Hp2, atol=(J_TOL + 2 * c) * max(1.0, np.abs(Hp2).max()), rtol=0, err_msg=str(depth))
        behind += not Hx2.any()
    assert behind == 12                                        # every negative depth took the cheirality branch, none of the positive ones
