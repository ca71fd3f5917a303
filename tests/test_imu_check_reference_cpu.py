"""Pins the numpy restatement of the IMU check (tests/imu_check_reference.py) before the kernel is held to it:
  J_imu, J_vro   against central differences of dw under right perturbations of either rotation (step 1e-6: truncation about
                 step^2 = 1e-12 and rounding about 1e-16 / step = 1e-10, bound 1e-8)
  dw             against the 40-digit matrix logarithm of tests/pose3_independent.py, bound 1e-13
  Lth            against the block of numpy.linalg.inv of the covariance as stored, and against the Schur complement
  calibrated d2  is chi-square with 3 degrees of freedom when both rotations carry noise from the covariances the check is told:
                 over N = 20000 draws the mean lies within 3 +- 4 sqrt(6 / N) (the variance of chi-square(3) is 6) and the share above
                 chi2_quantile(3, 0.95) within 0.05 +- 4 sqrt(0.05 * 0.95 / N) -- four standard deviations of either estimate
  reference d2   (gtsam/test_vro_imu_graph.cpp:724-743) is NOT: the same draws give a mean outside that band (measured 4.6 .. 4.7:
                 DESIGN.md section 7 says why)"""
import functools

import mpmath as mp
import numpy as np

import graph_slam_amd as G
from tests import imu_check_reference as ref
from tests import pose3_independent as ind

ANGLES = (1e-3, 0.05, 0.2, 0.3, 1.0, 3.0)


def _cases():
    rng = np.random.default_rng(11)
    pres = [ref.make_preint(rng, n, bias_hat=1e-2 * rng.normal(size=6)) for n in (3, 40)]
    out = []
    for i, a in enumerate(ANGLES + ANGLES):                      # with and without a bias, with and without an extrinsic
        q_uc = ref.random_unit(rng, 4) if i % 2 == 0 else None
        r = ref.draw_record(rng, pres, i % 2, a, i % 3 != 0, configs=((q_uc, True),))
        out.append((r, ref.record_args(r, pres, q_uc, i % 3 != 0)))
    return out


def test_jacobians_against_central_differences():
    h, worst = 1e-6, [0.0, 0.0]
    for _, a in _cases():
        R_imu, R_vro, _ = ref.rotations(**a)
        _, J_imu, J_vro = ref.residual(R_imu, R_vro, True)
        for which, J in enumerate((J_imu, J_vro)):
            num = np.zeros((3, 3))
            for k in range(3):
                d = np.zeros(3); d[k] = h
                if which == 0:
                    num[:, k] = (ref.residual(R_imu @ ref.rot_exp(d), R_vro) - ref.residual(R_imu @ ref.rot_exp(-d), R_vro)) / (2 * h)
                else:
                    num[:, k] = (ref.residual(R_imu, R_vro @ ref.rot_exp(d)) - ref.residual(R_imu, R_vro @ ref.rot_exp(-d))) / (2 * h)
            worst[which] = max(worst[which], np.abs(num - J).max())
    print("largest deviation from central differences: J_imu %.2e, J_vro %.2e" % tuple(worst))
    assert max(worst) <= 1e-8


def test_dw_against_the_40_digit_matrix_logarithm():
    worst = 0.0
    for _, a in _cases():
        R_imu, R_vro, _ = ref.rotations(**a)
        Rw = R_imu.T @ R_vro
        T = mp.eye(4)
        for a in range(3):
            for b in range(3):
                T[a, b] = mp.mpf(float(Rw[a, b]))
        want = np.array([float(x) for x in ind.logmap(T)[:3]])
        worst = max(worst, np.abs(ref.residual(R_imu, R_vro) - want).max())
    print("largest deviation of dw from the 40-digit logarithm: %.2e" % worst)
    assert worst <= 1e-13


def test_information_block_against_the_inverse_and_the_schur_complement():
    for r, a in _cases():
        w = ref.check_record(cov=r["cov"], **a)
        C = a["pre"][ref.COV].reshape(15, 15)
        inv = np.linalg.inv(C)[:3, :3]
        assert np.abs(w["Lth"] - inv).max() <= 1e-11 * w["cond_cov15"] * np.abs(inv).max()
        schur = C[:3, :3] - C[:3, 3:] @ np.linalg.solve(C[3:, 3:], C[3:, :3])
        assert np.abs(w["Lth"] @ schur - np.eye(3)).max() <= 1e-11 * w["cond_cov15"]
        assert w["status"] == ref.IC_OK and abs(w["d2_ref"] - w["dw"] @ w["J_imu"] @ inv @ w["J_imu"].T @ w["dw"]) <= 1e-11 * w["cond_cov15"] * w["d2_ref"]


def test_statuses_of_the_restatement():
    rng = np.random.default_rng(5)
    pres = [ref.make_preint(rng, 0), ref.make_preint(rng, 1)]
    r = ref.record_args(ref.draw_record(rng, pres, 1, 0.05, False), pres)
    r.update(cov=ref.pose_cov(rng, ref.random_rot_cov(rng)))
    r["info"] = ref.info_ut21(np.linalg.inv(r["cov"]))
    assert ref.check_record(r["pose"], pres[0], cov=r["cov"])["status"] == ref.IC_NUM               # no samples: the covariance is 0
    assert ref.check_record(r["pose"], pres[1], cov=r["cov"])["status"] == ref.IC_OK
    failed = ref.sentinel_info(r["info"])                       # information (0, 0) == 10000: a failed VO record
    w = ref.check_record(r["pose"], pres[1], info=failed)
    assert w["status"] == ref.IC_SKIPPED and w["d2"] == 0 and not w["cov_dw"].any()
    assert ref.check_record(r["pose"], pres[1], info=failed, failed_info00=0.0)["status"] == ref.IC_OK
    bad = np.diag([1.0, 1, 1, 1, 1, -1])
    assert ref.check_record(r["pose"], pres[1], info=ref.info_ut21(bad))["status"] == ref.IC_NUM


N_DRAWS = 20000


@functools.lru_cache(maxsize=None)
def monte_carlo():
    """d2 and d2_ref of N_DRAWS consistent records on one 40-sample preintegration: the rotation the IMU reports is the true one
    times Exp(N(0, Sth)), the one the record reports (camera frame) the true one times Exp(N(0, Sij[0:3, 0:3]))"""
    rng = np.random.default_rng(2024)
    pre = ref.make_preint(rng, 40)
    q_true = pre[ref.DR].copy()
    C = pre[ref.COV].reshape(15, 15)
    L_imu = np.linalg.cholesky(0.5 * (C[:3, :3] + C[:3, :3].T))
    Sww = ref.random_rot_cov(rng, 1e-5)
    S = ref.pose_cov(rng, Sww)
    L_vro = np.linalg.cholesky(S[:3, :3])
    q_uc = ref.random_unit(rng, 4)
    d2 = np.zeros(N_DRAWS); d2_ref = np.zeros(N_DRAWS)
    pose_true = ref.record_pose(pre, np.zeros(3), None, q_uc)          # the true rotation in the camera frame: no noise, no bias
    for k in range(N_DRAWS):
        noisy = pre.copy()
        noisy[ref.DR] = ref.qmul(q_true, ref.qexp(L_imu @ rng.normal(size=3)))
        pose = np.concatenate([np.zeros(3), ref.qmul(pose_true[3:], ref.qexp(L_vro @ rng.normal(size=3)))])
        w = ref.check_record(pose, noisy, cov=S, imu_q_cam=q_uc, conds=False)
        assert w["status"] == ref.IC_OK
        d2[k] = w["d2"]; d2_ref[k] = w["d2_ref"]
    return d2, d2_ref


def test_calibrated_form_follows_the_chi_square_law():
    d2, _ = monte_carlo()
    mean, share = d2.mean(), (d2 > G.chi2_quantile(3, 0.95)).mean()
    band_mean, band_share = 4 * np.sqrt(6.0 / N_DRAWS), 4 * np.sqrt(0.05 * 0.95 / N_DRAWS)
    print("calibrated form: mean d2 %.4f (3 +- %.4f), share above the 95 %% quantile %.4f (0.05 +- %.4f)" % (mean, band_mean, share, band_share))
    assert abs(mean - 3.0) <= band_mean
    assert abs(share - 0.05) <= band_share


def test_reference_form_does_not():
    _, d2_ref = monte_carlo()
    mean = d2_ref.mean()
    print("reference form: mean d2_ref %.4f" % mean)
    assert abs(mean - 3.0) > 4 * np.sqrt(6.0 / N_DRAWS)
