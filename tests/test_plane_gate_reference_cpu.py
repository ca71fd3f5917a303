"""Pins tests/plane_gate_reference.py, the numpy evaluation the GPU plane-gate tests compare against, so that a wrong sign or
transpose in the cross term cannot hide in it: its Jacobians against central differences of the oracle's plane factor, and its
statistics by Monte Carlo -- d2 of a correct association is chi-square with 3 degrees of freedom, and is not once the pose/plane
cross-covariance is dropped (the form the reference has commented out, gtsam/gtsam_graph.cpp:1429-1476)."""
import numpy as np

from tests import orc_binding as orc
from tests import plane_gate_reference as R
from tests.util import mixed_graph, mixed_oracle


def _graph():
    g = mixed_graph(np.random.default_rng(22), 10, 3, 14)
    return g, np.linalg.inv(mixed_oracle(g).dense_system()[0]), list(range(len(g["values"])))


def test_reference_jacobians_against_central_differences():
    """The GTSAM 4.0 factor takes d r / d predicted = I, which is exact where the residual vanishes (tests/test_plane_golden.py):
    the comparison is made there, with that file's step and tolerance (h = 1e-6, 1e-8 absolute)."""
    g, Sigma, pos = _graph()
    V, h, worst = g["values"], 1e-6, 0.0
    for x in range(1, 10):
        for p in range(10, 13):
            z = orc.plane_transform(V[p][:4], V[x])
            ref = R.gate(Sigma, pos, V, x, p, z, 1e-4 * np.eye(3))
            Nx = np.zeros((3, 6)); Np = np.zeros((3, 3))
            for k in range(6):
                d = np.zeros(6); d[k] = h
                Nx[:, k] = (orc.plane_factor(orc.retract(V[x], d), V[p][:4], z, jac=False)
                            - orc.plane_factor(orc.retract(V[x], -d), V[p][:4], z, jac=False)) / (2 * h)
            for k in range(3):
                d = np.zeros(3); d[k] = h
                Np[:, k] = (orc.plane_factor(V[x], orc.plane_retract(V[p][:4], d), z, jac=False)
                            - orc.plane_factor(V[x], orc.plane_retract(V[p][:4], -d), z, jac=False)) / (2 * h)
            worst = max(worst, np.abs(ref["Jx"] - Nx).max(), np.abs(ref["Jp"] - Np).max())
            np.testing.assert_allclose(ref["Jx"], Nx, atol=1e-8)
            np.testing.assert_allclose(ref["Jp"], Np, atol=1e-8)
            assert abs(ref["cos"] - 1) < 1e-12 and ref["d2"] <= ref["chi2"] < 1e-20
    print("Jx / Jp against central differences: %.1e" % worst)


def test_d2_is_chi_square_3_only_with_the_cross_term():
    """Linearised draws: (dx, dp) ~ N(0, Sigma) moves the true pose and plane away from the estimate, the observation sees the TRUE
    plane with noise n ~ N(0, S), so gated at the estimate e = Jx dx + Jp dp + n with J at the zero-residual point.  d2 has mean 3
    and variance 6: with N draws the mean lies within 4 sqrt(6 / N) of 3 (4 sigma); without the cross term it lies outside that band
    on every pair.  S = 1e-4 I, the covariance of the graph's own plane factors."""
    g, Sigma, pos = _graph()
    V, N = g["values"], 20000
    rng = np.random.default_rng(43)
    band = 4 * np.sqrt(6.0 / N)
    S = 1e-4 * np.eye(3)
    lo, hi, lo_nc, hi_nc = np.inf, -np.inf, np.inf, -np.inf
    for x in range(1, 10):
        for p in range(10, 13):
            z = orc.plane_transform(V[p][:4], V[x])
            _, Jx, Jp = orc.plane_factor(V[x], V[p][:4], z)
            Sxx, Sxp, Spp = R.sigma_blocks(Sigma, pos, x, p)
            joint = np.block([[Sxx, Sxp], [Sxp.T, Spp]])
            draws = rng.normal(size=(N, 9)) @ np.linalg.cholesky(joint).T
            E = draws @ np.hstack([Jx, Jp]).T + 1e-2 * rng.normal(size=(N, 3))
            mean = {}
            for cross in (True, False):
                M = np.linalg.inv(R.predicted_cov(Jx, Jp, Sxx, Sxp, Spp, cross) + S)
                mean[cross] = float(np.einsum("ni,ij,nj->n", E, M, E).mean())
            lo, hi = min(lo, mean[True]), max(hi, mean[True])
            lo_nc, hi_nc = min(lo_nc, mean[False]), max(hi_nc, mean[False])
            assert abs(mean[True] - 3.0) <= band, (x, p, mean[True])
            assert abs(mean[False] - 3.0) > band, (x, p, mean[False])
    print("mean d2 over the 27 pairs: %.3f .. %.3f; without the cross term %.3f .. %.3f (band 3 +- %.3f)" % (lo, hi, lo_nc, hi_nc, band))
