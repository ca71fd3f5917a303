"""CPU: the preintegrated covariance of the host (csrc/imu_preint.cpp, G.Preintegrator) and of the oracle (oracle/orc_imu.h, orc.Preint), and the
information matrix fgo_preint_information derives from it, against tests/preint_cov_independent.py: 40 digits, F by differentiating the step,
only the noise convention shared.  Host and oracle were written from one derivation (the same F, Q from the same Jr and IncT, the same 0.25
switch), so their agreement (tests/test_host_preint.py) cannot see an error in it, and tests/test_oracle_imu.py holds the covariance to
symmetry and positivity only.

Measured (x86-64, scaled error max_ij |C - C*|_ij / sqrt(C*_ii C*_jj) over tests.preint_cov_independent.cases()):
  oracle   largest 1.35e-15 (n40: 0.15 eps n); largest in units of eps n: 1.5 (n1)                       bound 64 eps max(1, n)
  host     largest 1.61e-15 (n40); largest relative to the oracle's error on the same case: 1.66 (past_pi)   bound 16 x the oracle's,
           the oracle's error counted up to its own bound only, and no less than 2^-52
  fgo_preint_information, error / (eps kappa_s): largest 1.79 (n2, n3, jr_1.1; kappa_s 1.1), n40 0.36, SPREAD_A 1.66, SPREAD_B 0.75, 200 samples 0.39      bound 8"""
import mpmath as mp
import numpy as np
import pytest

import graph_slam_amd as G
from tests import orc_binding as orc
from tests import preint_cov_independent as pc
from tests.test_oracle_imu import imu_samples

CASES = pc.cases()
IDS = [c["name"] for c in CASES]


def host_payload(c):
    pim = G.Preintegrator(c["bhat"], params=pc.params9(c))
    for a, w in zip(c["acc"], c["gyro"]):
        pim.integrate(a, w, c["dt"])
    return pim.buf


# ---------------------------------------------------------------------------------------------------- a. the reference itself
def test_reference_one_sample_from_zero_is_the_noise_term():
    c = CASES[IDS.index("jr_1.1")]
    v3 = lambda a: mp.matrix([mp.mpf(float(u)) for u in a])
    x = (mp.eye(3), mp.zeros(3, 1), mp.zeros(3, 1), v3(c["bhat"][:3]), v3(c["bhat"][3:]))
    dt = mp.mpf(float(c["dt"]))
    F, _ = pc.transition(x, v3(c["acc"][0]), v3(c["gyro"][0]), dt)
    Q = pc.noise(F, dt, c["params"])
    S = pc.covariance_mp(c["acc"][:1], c["gyro"][:1], c["dt"], c["bhat"], c["params"])
    assert all(S[r, k] == Q[r, k] for r in range(15) for k in range(15))
    assert all(Q[k, k] > 0 for k in range(15))


@pytest.mark.parametrize("name", ["n3", "jr_1.1", "spread_a"])
def test_reference_does_not_depend_on_the_differentiation_step(name):
    """steps 1e-12 and 1e-14: truncation 1e-24 against 1e-28, rounding 1e-40 / step"""
    c = CASES[IDS.index(name)]
    Sa = pc.covariance_mp(c["acc"][:3], c["gyro"][:3], c["dt"], c["bhat"], c["params"], h=mp.mpf("1e-12"))
    Sb = pc.covariance_mp(c["acc"][:3], c["gyro"][:3], c["dt"], c["bhat"], c["params"], h=mp.mpf("1e-14"))
    err = max(abs(Sa[r, k] - Sb[r, k]) / mp.sqrt(Sb[r, r] * Sb[k, k]) for r in range(15) for k in range(15))
    print("step 1e-12 against 1e-14: %.2e" % float(err))
    assert err < mp.mpf("1e-20")


def test_reference_is_symmetric_and_zero_without_samples():
    c = CASES[IDS.index("n8")]
    S = pc.covariance_mp(c["acc"], c["gyro"], c["dt"], c["bhat"], c["params"])
    assert max(abs(S[r, k] - S[k, r]) / mp.sqrt(S[r, r] * S[k, k]) for r in range(15) for k in range(15)) < mp.mpf("1e-35")
    for k, c in enumerate(CASES):
        C, W = pc.reference(k)
        assert np.array_equal(C, C.T), c["name"]
        if len(c["acc"]) == 0:
            assert not C.any() and W is None
        else:
            assert np.linalg.eigvalsh(C).min() > 0


# ---------------------------------------------------------------------------------------------------- d. no silent skip
def test_case_list_covers_what_it_claims():
    ang = {c["name"]: pc.angle_per_sample(c) for c in CASES}
    assert sum(len(c["acc"]) for c in CASES) <= 120
    assert {0, 1, 2, 3, 16, 40} <= {len(c["acc"]) for c in CASES}
    assert len(ang["gyro_zero"]) and np.all(ang["gyro_zero"] == 0.0)
    for name, t in (("exp", 1e-10), ("jr", 0.25)):
        below, above = ang[name + "_0.9"], ang[name + "_1.1"]
        assert len(below) and len(above)
        assert np.all(below < t) and np.all(below > 0.85 * t), (name, below)          # the code under test compares t < threshold
        assert np.all(above >= t) and np.all(above < 1.15 * t), (name, above)
    assert ang["past_pi"].sum() > np.pi and np.ptp(CASES[IDS.index("past_pi")]["gyro"], axis=0).max() == 0.0       # one axis: the angles add
    assert np.all(ang["fast"] >= 0.25) and np.ptp(CASES[IDS.index("fast")]["gyro"], axis=0).min() > 0.0            # closed form, moving axis
    assert any(c["bhat"] is None for c in CASES) and any(c["bhat"] is not None and np.all(c["bhat"] != 0) for c in CASES)
    params = {c["params"] for c in CASES}
    assert params == {pc.vn100(), pc.SPREAD_A, pc.SPREAD_B} and pc.SPREAD_A[5] == 0.0
    p = np.zeros(G.IMU_PARAM_DOUBLES); G.lib.fgo_imu_params_vn100(G._dp(p))
    np.testing.assert_allclose(p[:6], pc.vn100(), rtol=1e-14)                       # the module's restatement is the product's default
    np.testing.assert_array_equal(p[6:], pc.params9(CASES[0])[6:])


# ---------------------------------------------------------------------------------------------------- b. the covariance
@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_oracle_covariance_vs_differentiated_step(k):
    n = len(CASES[k]["acc"])
    err = pc.oracle_error(k)
    print("%s: oracle %.3e = %.2f eps max(1, n)" % (IDS[k], err, err / pc.EPS / max(1, n)))
    assert err <= 64 * pc.EPS * max(1, n)


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_host_covariance_vs_differentiated_step(k):
    buf = host_payload(CASES[k])
    err = pc.scaled_error(buf[62:].reshape(15, 15), pc.reference(k)[0])
    print("%s: host %.3e, oracle %.3e, bound %.3e" % (IDS[k], err, pc.oracle_error(k), pc.product_bound(k)))
    assert err <= pc.product_bound(k)


def test_parameters_reach_the_covariance():
    """the reference's covariances under the three parameter sets differ by more than half in most diagonal entries (VN100 and SPREAD_B share
    biasAccOmegaInt, which dominates theta and v): a code under test that ignored `params` could not pass the cases above"""
    Ca, Cb = pc.reference(IDS.index("spread_a"))[0], pc.reference(IDS.index("spread_b"))[0]
    Cv = pc.reference(IDS.index("n8"))[0]
    for C1, C2 in ((Ca, Cb), (Ca, Cv), (Cb, Cv)):
        assert (np.abs(np.diag(C1) / np.diag(C2) - 1) > 0.5).sum() >= 9


# ---------------------------------------------------------------------------------------------------- c. the information matrix
def _check_information(buf, what):
    W = G.preint_information(buf)
    np.testing.assert_array_equal(W, W.T)
    err, ks = pc.information_error(W, buf[62:].reshape(15, 15))
    print("%s: error %.3e = %.2f eps kappa_s, kappa_s %.2f" % (what, err, err / (pc.EPS * ks), ks))
    assert err <= pc.INFO_BOUND * pc.EPS * ks, (what, err / (pc.EPS * ks))


@pytest.mark.parametrize("k", [k for k in range(len(CASES)) if len(CASES[k]["acc"])], ids=[n for n, c in zip(IDS, CASES) if len(c["acc"])])
def test_information_is_the_inverse_of_the_payload_covariance(k):
    """against the 40-digit inverse of the float covariance in the same payload: bound 8 eps kappa_s, kappa_s the condition number of the
    diagonally equilibrated covariance (the Cholesky factorisation is invariant under that scaling up to rounding; the unscaled condition
    number, 5e3 for the VN100 settings and 1e12 for SPREAD_A, does not enter)"""
    _check_information(host_payload(CASES[k]), IDS[k])


def test_information_of_a_200_sample_payload():
    acc, gyro = imu_samples(np.random.default_rng(7), 200)
    pim = G.Preintegrator(np.array(pc.BHAT))
    for a, w in zip(acc, gyro):
        pim.integrate(a, w, 0.005)
    _check_information(pim.buf, "200 samples")


def test_information_refuses_the_empty_payload():
    with pytest.raises(G.FgoError):
        G.preint_information(host_payload(CASES[IDS.index("n0")]))


# ---------------------------------------------------------------------------------------------------- raw samples -> H, the oracle's leg
def test_oracle_raw_samples_to_H_vs_independent_references():
    """tests.preint_cov_independent.imu_only_graph() assembled by the oracle from its own preintegration of the raw samples and
    numpy.linalg.inv of its own covariance, the chain's first pose fixed: the system tests/test_gpu_preint_cov.py holds the device to, at
    the same bounds (H 1e-8 of the component's largest entry, b 1e-8, chi2 1e-9).  Measured: H 1.8e-16, b 2.3e-16, chi2 4.3e-16."""
    g = pc.imu_only_graph()
    N = 3 * pc.N_KEY
    values = np.zeros((N, 7)); vkind = np.zeros(N, np.int32); fixed = np.zeros(N, np.uint8)
    values[:pc.N_KEY] = g["poses"]; values[pc.N_KEY:2 * pc.N_KEY, :3] = g["vels"]; values[2 * pc.N_KEY:, :6] = g["bias"]
    vkind[pc.N_KEY:2 * pc.N_KEY] = orc.VK_VEC3; vkind[2 * pc.N_KEY:] = orc.VK_BIAS
    fixed[:pc.N_KEY] = g["fixed"]
    pre = []
    for k in g["ks"]:
        c = CASES[k]
        pre.append(orc.Preint(np.zeros(6) if c["bhat"] is None else c["bhat"], c["acc"], c["gyro"], c["dt"]))
    po = orc.Problem(values, fixed, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 7)), np.zeros((0, 21)))
    po.set_kinds(vkind, np.zeros(0, np.int32))
    po.add_imu_factors(g["ids"], pre, [np.linalg.inv(p.cov) for p in pre])
    H, b = po.dense_system()
    figures, ec = pc.system_errors(po.chi2(), H, b)
    print("H, b per component:", " ".join("(%.3e, %.3e)" % f for f in figures), " chi2 %.3e" % ec)
    assert max(e for e, _ in figures) <= 1e-8 and max(e for _, e in figures) <= 1e-8, figures
    assert ec <= 1e-9
