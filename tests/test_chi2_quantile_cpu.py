"""fgo_chi2_quantile (csrc/chi2_quantile.cpp; the reference's utils::chi2, gtsam/chi2.h:17-26) against scipy: the quantile itself
against scipy.stats.chi2.ppf, the probability at the quantile against scipy.special.gammainc, both to the project's per-value
tolerance, relative 1e-11, and the edge returns."""
import math

import pytest
from scipy.special import gammainc
from scipy.stats import chi2

import graph_slam_amd as G

TOL = 1e-11
PS = (1e-3, 0.1, 0.5, 0.9, 0.95, 0.99, 0.999)


@pytest.mark.parametrize("dof", range(1, 16))
def test_quantile_against_scipy(dof):
    for p in PS:
        x, want = G.chi2_quantile(dof, p), chi2.ppf(p, dof)
        assert abs(x - want) <= TOL * want, (dof, p, x, want)
        back = gammainc(0.5 * dof, 0.5 * x)
        assert abs(back - p) <= TOL * p, (dof, p, x, back)


def test_edge_returns():
    for dof in (0, -1, -100):
        for p in (0.5, 0.0, 1.0, float("nan")):
            assert G.chi2_quantile(dof, p) == 0.0, (dof, p)                        # as the reference returns
    for p in (0.0, -0.5, -math.inf):
        assert G.chi2_quantile(3, p) == 0.0, p
    for p in (1.0, 1.5, math.inf):
        assert G.chi2_quantile(3, p) == math.inf, p
    assert math.isnan(G.chi2_quantile(3, float("nan")))


def test_the_gates_the_library_documents():
    assert abs(G.chi2_quantile(3, 0.95) - 7.814727903251179) <= TOL * 7.814727903251179
    assert abs(G.chi2_quantile(6, 0.95) - chi2.ppf(0.95, 6)) <= TOL * 12.59 and round(G.chi2_quantile(6, 0.95), 2) == 12.59
