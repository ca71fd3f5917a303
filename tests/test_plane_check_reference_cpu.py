"""The yardstick of the plane check (tests/plane_check_reference.py, the numpy restatement of include/fgo.h
fgo_plane_check_vro_batch) is itself held to what does not depend on it: the golden errorVector regression the reference carries
(gtsam/test/testOrientedPlane3.cpp:143-149), the oracle's OrientedPlane3::transform, central differences of every Jacobian, the
chi-square law of the distance on consistent data, hand-built plane lists for the matching rule and the sdj formula."""
import numpy as np

from tests import orc_binding as orc
from tests import plane_check_reference as ref

IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])


def test_golden_error_vector():
    p1, p2 = ref.normalize([-1, 0.1, 0.2, 5]), ref.normalize([-1.1, 0.2, 0.3, 5.4])
    np.testing.assert_allclose(ref.error_vector(p1, p2), [-0.0677674148, -0.0760543588, -0.4], atol=1e-9)
    np.testing.assert_allclose(ref.error_vector(p1, p1), 0, atol=1e-15)
    np.testing.assert_allclose(ref.error_vector(p1, p2), orc.plane_error_vector(p1, p2), atol=1e-15)


def _central(f, k, dim, h=1e-6):
    v = np.zeros(dim); v[k] = h
    return (f(v) - f(-v)) / (2 * h)


def test_jacobians_against_central_differences():
    """200 random planes; every normal whose basis is differentiated keeps its two smallest |n_i| 1e-2 apart, so no sample sits on
    the basis rule's axis switch.  H1, H2 of errorVector and D_pose, D_plane of transform to 1e-8 (h = 1e-6)."""
    rng = np.random.default_rng(11)
    worst = 0.0
    for _ in range(200):
        while True:
            pose = ref.random_pose(rng, 1.0, 1.0)
            P = np.append(ref.random_unit(rng), rng.uniform(0.5, 3))
            pe = ref.transform(P, pose)
            if ref.axis_margin(pe[:3]) >= 1e-2:
                break
        # transform: the restatement agrees with the oracle, and both with central differences in the tangent of the result
        out, Dx, Dp = ref.transform(P, pose, True)
        o_out, o_Dx, o_Dp = orc.plane_transform(P, pose, True)
        np.testing.assert_allclose(out, o_out, atol=1e-14)
        np.testing.assert_allclose(Dx, o_Dx, atol=1e-13)
        np.testing.assert_allclose(Dp, o_Dp, atol=1e-13)
        for k in range(6):
            num = _central(lambda v: orc.plane_local(pe, ref.transform(P, ref.pose_retract(pose, v))), k, 6)
            worst = max(worst, np.abs(num - Dx[:, k]).max())
        for k in range(3):
            num = _central(lambda v: orc.plane_local(pe, ref.transform(ref.plane_retract(P, v), pose)), k, 3)
            worst = max(worst, np.abs(num - Dp[:, k]).max())
        # errorVector against a plane within reach of a match (10 deg, 0.2 m) of pe
        pj = ref.plane_retract(pe, np.append(rng.uniform(-0.17, 0.17, 2), rng.uniform(-0.2, 0.2)))
        e, H1, H2 = ref.error_vector(pe, pj, True)
        for k in range(3):
            worst = max(worst, np.abs(_central(lambda v: ref.error_vector(ref.plane_retract(pe, v), pj), k, 3) - H1[:, k]).max())
            worst = max(worst, np.abs(_central(lambda v: ref.error_vector(pe, ref.plane_retract(pj, v)), k, 3) - H2[:, k]).max())
    print("largest deviation from central differences: %.3g" % worst)
    assert worst <= 1e-8


def test_retractions_agree_with_the_oracle():
    rng = np.random.default_rng(5)
    for _ in range(50):
        pose = ref.random_pose(rng, 1.0, 1.0); xi = rng.normal(size=6) * 0.2
        a, b = ref.pose_retract(pose, xi), orc.retract(pose, xi)
        np.testing.assert_allclose(a[:3], b[:3], atol=1e-14)
        np.testing.assert_allclose(a[3:] * np.sign(a[3:] @ b[3:]), b[3:], atol=1e-14)
        P = np.append(ref.random_unit(rng), 1.0); v = rng.normal(size=3) * 0.2
        np.testing.assert_allclose(ref.plane_retract(P, v), orc.plane_retract(P, v), atol=1e-14)


def test_distance_is_chi_square_on_consistent_data():
    """4000 consistent samples (ref.draw_record: plane i, the pose and plane j each carry noise drawn from the covariance the
    check is told): d2 is chi-square with 3 degrees of freedom, so its mean is 3 +- 4 sqrt(6 / 4000) = 3 +- 0.16 and the share
    above the 95 % quantile 7.815 is 0.05 +- 4 sqrt(0.05 * 0.95 / 4000) = 0.05 +- 0.014."""
    rng = np.random.default_rng(2024)
    d2 = np.zeros(4000); cond = 0.0
    for k in range(len(d2)):
        r = ref.draw_record(rng, [0], [0])
        out = ref.check_record(r["pose"], r["pi"], r["ci"], r["pj"], r["cj"], cov=r["cov"])
        assert out["match"][0] == 0 and out["n_bad"] == 0 and out["best_i"] == 0
        d2[k] = out["err"]; cond = max(cond, out["cond_e"][0])
    print("mean %.4f, share above 7.815 %.4f, largest cond(S_e) %.1f" % (d2.mean(), (d2 > 7.815).mean(), cond))
    assert abs(d2.mean() - 3) <= 0.16
    assert abs((d2 > 7.815).mean() - 0.05) <= 0.014


def _lists(pi, pj, **kw):
    """hand-built plane lists under the identity pose with a small, well-conditioned covariance everywhere"""
    C = np.diag([1e-4, 1e-4, 1e-4, 1e-4]).reshape(16)
    pi, pj = np.array(pi, np.float64).reshape(-1, 4), np.array(pj, np.float64).reshape(-1, 4)
    return ref.check_record(IDENT, pi, np.tile(C, (len(pi), 1)), pj, np.tile(C, (len(pj), 1)), cov=1e-4 * np.eye(6), **kw)


def test_matching_rule_on_hand_built_lists():
    z = [0, 0, 1.0]
    tilt = lambda deg: [np.sin(np.deg2rad(deg)), 0, np.cos(np.deg2rad(deg))]
    # first match wins: j = 1 and j = 2 both qualify, j = 0 fails on the angle; the later, closer j = 2 is not taken
    out = _lists([z + [1.0]], [tilt(30) + [1.0], tilt(4) + [1.05], z + [1.0]])
    assert list(out["match"]) == [1] and out["best_j"] == 1 and out["n_matched"] == 1
    # the offset gates too (0.25 > 0.2), and the antipodal normal counts as parallel (|cos|)
    out = _lists([z + [1.0]], [z + [1.25], [0, 0, -1.0, 1.1]])
    assert list(out["match"]) == [1]
    # two i take the same j; the larger distance is the record's
    out = _lists([tilt(2) + [1.0], tilt(5) + [1.0]], [tilt(40) + [1.0], z + [1.0]])
    assert list(out["match"]) == [1, 1] and out["best_i"] == 1 and out["err"] == out["d2"][1] > out["d2"][0] > 0
    assert out["err_raw"] == out["raw"][1]
    # strict > on a tie: two identical planes i, the first stays
    out = _lists([tilt(3) + [1.0], tilt(3) + [1.0], tilt(1) + [1.0]], [z + [1.0]])
    assert out["d2"][0] == out["d2"][1] > out["d2"][2] and out["best_i"] == 0 and out["n_matched"] == 3
    # nothing matched
    out = _lists([z + [1.0], tilt(3) + [2.0]], [tilt(30) + [1.0], z + [1.5]])
    assert list(out["match"]) == [-1, -1] and (out["best_i"], out["best_j"], out["err"], out["err_raw"]) == (-1, -1, 0, 0)
    assert not out["d2"].any() and not out["raw"].any() and out["n_matched"] == 0
    # empty lists on either side
    assert _lists([], [z + [1.0]])["best_i"] == -1 and _lists([z + [1.0]], [])["match"][0] == -1
    # thresholds are parameters
    assert list(_lists([z + [1.0]], [tilt(30) + [1.0]], cos_min=0.8)["match"]) == [0]
    assert list(_lists([z + [1.0]], [z + [1.25]], d_max=0.3)["match"]) == [0]


def test_record_status_and_degenerate_covariances():
    z = np.array([[0, 0, 1.0, 1.0]]); zj = np.array([[0.02, 0, 1.0, 1.01]]); C = np.full((1, 16), 0.0)
    info = 1e4 * np.eye(6)
    out = ref.check_record(IDENT, z, C, zj, C, info=ref.info_ut21(info))                    # the failed-VO sentinel
    assert out["status"] == ref.PC_SKIPPED and out["err"] == 0 and out["match"][0] == -1
    out = ref.check_record(IDENT, z, C, zj, C, info=ref.info_ut21(info), failed_info00=0)   # ... disabled
    assert out["status"] == ref.PC_OK and out["match"][0] == 0 and out["err"] > 0
    bad = np.eye(6); bad[5, 5] = -1
    assert ref.check_record(IDENT, z, C, zj, C, info=ref.info_ut21(bad))["status"] == ref.PC_NUM
    # all covariances zero: the pair matches, S_e = 0 is not positive definite
    out = ref.check_record(IDENT, z, C, zj, C, cov=np.zeros((6, 6)))
    assert (out["n_matched"], out["n_bad"], out["err"], out["best_i"]) == (1, 1, 0, -1) and np.isinf(out["d2"][0]) and np.isinf(out["raw"][0])


def test_sdj_formula():
    rng = np.random.default_rng(3)
    for _ in range(20):
        r = ref.draw_record(rng, [0, 1], [0])
        out = ref.check_record(r["pose"], r["pi"], r["ci"], r["pj"], r["cj"], info=r["info"])
        S = np.linalg.inv(ref.info_full(r["info"]))
        for i in range(2):
            n, t, C = r["pi"][i, :3], r["pose"][:3], r["ci"][i].reshape(4, 4)
            g = t - n * (n @ t)
            want = C[3, 3] + n @ S[3:, 3:] @ n + g @ C[:3, :3] @ g
            assert abs(out["sdj"][i] - want) <= 1e-14 * want
