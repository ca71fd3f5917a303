"""Pins tests/gate_reference.py, the numpy evaluation the GPU gate tests compare against, so that a wrong sign or transpose in
the cross term cannot hide in it: its e / J against the independent forward-mode derivation, its two algebraic forms of d2 against
each other, and its statistics by Monte Carlo -- d2 of a correct candidate that is not in the graph is chi-square with 6 degrees
of freedom, and is not once the cross-covariance term is dropped."""
import numpy as np

from tests import gate_reference as R
from tests import orc_binding as orc
from tests import se3_independent as ind
from tests.util import pose_inv, pose_mul, random_info, small_graph


def _sigma(g):
    po = orc.Problem(g["poses"], g["fixed"], g["ei"].astype(np.int32), g["ej"].astype(np.int32), g["meas"], g["info"])
    return np.linalg.inv(po.dense_system()[0])


def test_reference_jacobians_and_both_forms_of_d2():
    g = small_graph(np.random.default_rng(31), n=150, extra=12)
    Sigma, pos = _sigma(g), R.free_positions(g["fixed"])
    a, b, meas, info = R.candidates(np.random.default_rng(32), g["poses"], R.SMALL_PAIRS)
    worst_j = worst_d = 0.0
    for k, ref in enumerate(R.gate_many(Sigma, pos, g["poses"], a, b, meas, info)):
        e, Ja, Jb = ind.edge_se3_ad(g["poses"][a[k]], g["poses"][b[k]], meas[k])
        worst_j = max(worst_j, np.abs(ref["e"] - e).max(), np.abs(ref["Ja"] - Ja).max(), np.abs(ref["Jb"] - Jb).max())
        worst_d = max(worst_d, abs(ref["d2"] - ref["d2w"]) / ref["d2"])
        assert 0 <= ref["d2"] <= ref["chi2"]
    print("e / J against the independent derivation: %.1e; direct against whitened d2: %.1e" % (worst_j, worst_d))
    assert worst_j < 1e-12
    assert worst_d < 1e-12


def test_d2_is_chi_square_6_only_with_the_cross_term():
    """delta ~ N(0, Sigma) moves the true poses away from the estimate, the candidate measures the TRUE relative pose with noise
    n ~ N(0, W^-1): Z = (Xa^-1 Xb) fromVector(n)^-1.  Gated at the estimate, d2 has mean 6; N = 4000 draws: standard error of the
    mean sqrt(12 / 4000) = 0.055, the band 6 +- 0.2 is 3.6 sigma."""
    rng = np.random.default_rng(41)
    g = small_graph(rng, n=12, extra=6, noise=0.003)
    g["info"] = g["info"] * 1e3
    Sigma, pos = _sigma(g), R.free_positions(g["fixed"])
    est = g["poses"]
    Ls = np.linalg.cholesky(Sigma)
    N = 4000
    for (a, b) in [(2, 11), (0, 9), (7, 3)]:
        W = 1e3 * random_info(rng)
        Ln = np.linalg.cholesky(np.linalg.inv(W))
        blocks = R.sigma_blocks(Sigma, pos, a, b)
        d2 = np.zeros(N); d2_nocross = np.zeros(N)
        for k in range(N):
            delta = Ls @ rng.normal(size=Sigma.shape[0])
            xa = est[a] if pos[a] is None else orc.oplus(est[a], delta[6 * pos[a]:6 * pos[a] + 6])
            xb = est[b] if pos[b] is None else orc.oplus(est[b], delta[6 * pos[b]:6 * pos[b] + 6])
            nz = Ln @ rng.normal(size=6)
            fv = np.concatenate([nz, [np.sqrt(1.0 - nz[3:] @ nz[3:])]])
            z = pose_mul(pose_mul(pose_inv(xa), xb), pose_inv(fv))
            e, Ja, Jb = orc.edge_se3(est[a], est[b], z)
            d2[k] = R.d2_direct(e, R.predicted_cov(Ja, Jb, *blocks), W)
            d2_nocross[k] = R.d2_direct(e, R.predicted_cov(Ja, Jb, *blocks, cross=False), W)
        print("pair (%d, %d): mean d2 %.3f, without the cross term %.3f" % (a, b, d2.mean(), d2_nocross.mean()))
        assert abs(d2.mean() - 6.0) < 0.2, (a, b, d2.mean())
        if pos[a] is not None and pos[b] is not None:
            assert abs(d2_nocross.mean() - 6.0) > 0.2, (a, b, d2_nocross.mean())
