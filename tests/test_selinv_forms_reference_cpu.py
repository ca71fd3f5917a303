"""The dense references of tests/test_gpu_selinv_forms.py, checked without a device: for every graph of
tests/selinv_forms_child.py the information matrix H of the independent oracle is symmetric positive definite, no 6x6 block of
its inverse is exactly zero (every graph stays connected without its fixed vertex, so every covariance block the GPU test asks
for is compared with something), and the reference's own attainable error leaves the GPU test's bound below the 1e-8 of the
existing marginal tests:  16 * max(d_ref, n eps) <= 1e-8.

d_ref compares two independent double-precision inverses, numpy.linalg.inv (LU) and Li^T Li with Li = solve(cholesky(H), I),
block by block: the largest max|R_blk - C_blk| / max|R_blk|.  Measured with these builders: chains of 2 / 43 / 44 / 86 poses at
spread 0.3 about 1e-16 / 1e-12, the star of 600 poses 4e-11 (cond(H) 5e9), the hub graph 1e-12, the complete graphs 1e-14.  The
86-pose chain at the default spread 3.0 gives 5e-10, too close to the cap: hence the chains' spread."""
import numpy as np
import pytest

from tests import orc_binding as orc
from tests import selinv_forms_child as child

EPS = 2.0 ** -53
CAP = 1e-8            # the tolerance of tests/test_gpu_marginals_all.py
MARGIN = 16.0         # over two backward-stable dense inverses: covers a recursion that accumulates along the elimination tree and
                      # sums in another order.  Not measured on the device.


def block_max(A):
    """max |.| of every 6x6 block"""
    nb = A.shape[0] // 6
    return np.abs(A).reshape(nb, 6, nb, 6).max(axis=(1, 3))


class Reference:
    """R = numpy.linalg.inv(H), its blockwise distance d_ref from the Cholesky inverse, and the bound a device block is held to:
    max|D - R_blk| / max|R_blk| <= min(CAP, MARGIN * max(d_ref, n eps)).
    real: the rows of H that belong to a variable's own dimensions (a 3-dof variable is padded to 6 with a unit diagonal: its padding
    would put a 1 into every block maximum of its diagonal block, so the maxima, d_ref and the device's errors are taken over the real
    rows and columns only, and the padding is held to the same figure absolutely)"""

    def __init__(self, H, real=None):
        self.n = n = H.shape[0]
        real = np.ones(n, bool) if real is None else np.asarray(real, bool)
        self.sym = float(np.abs(H - H.T).max() / np.abs(H).max())
        self.R = np.linalg.inv(H)
        L = np.linalg.cholesky(H)                                     # raises unless H is positive definite
        Li = np.linalg.solve(L, np.eye(n))
        C = Li.T @ Li
        M = np.outer(real, real).astype(np.float64)
        self.rmax = block_max(self.R * M)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.d_ref = float(np.nanmax(block_max((self.R - C) * M) / self.rmax))
        self.pad_ref = float(np.abs((self.R - C) * (1.0 - M)).max())
        self.raw_bound = MARGIN * max(self.d_ref, n * EPS)
        self.bound = min(CAP, self.raw_bound)
        self.R4 = self.R.reshape(n // 6, 6, n // 6, 6)
        self.M4 = M.reshape(n // 6, 6, n // 6, 6)

    def errors(self, D, pa, pb):
        """device blocks D[k] against blocks (pa[k], pb[k]) of R: (largest relative error over the real entries, largest absolute
        error of the padding)"""
        E = np.abs(np.asarray(D) - self.R4[pa, :, pb, :])
        Mk = self.M4[pa, :, pb, :]
        rel = (E * Mk).max(axis=(1, 2)) / self.rmax[pa, pb]
        return float(rel.max()), float((E * (1.0 - Mk)).max())


def g2o_dense(g):
    po = orc.Problem(g["poses"], g["fixed"], np.asarray(g["ei"], np.int32), np.asarray(g["ej"], np.int32), g["meas"], g["info"])
    return po.dense_system()[0]


def ba_dense():
    """(H, real rows) of the independent oracle's system: poses, then points padded from 3 to 6 dimensions"""
    from graph_slam_amd import scenarios
    from tests.test_gpu_ba_oracle import ba_oracle
    n_kf, n_pts = child.BA_SHAPE
    real = np.concatenate([np.ones(6 * n_kf, bool), np.tile([True, True, True, False, False, False], n_pts)])
    return ba_oracle(scenarios.ba_problem(n_kf, n_pts)).dense_system()[0], real


def _check(name, H, real=None):
    ref = Reference(H, real)
    print("[selinv reference] %-24s n %5d  d_ref %.2e  n eps %.2e  16 max %.2e  smallest block max %.2e" % (
        name, ref.n, ref.d_ref, ref.n * EPS, ref.raw_bound, ref.rmax.min()))
    assert ref.sym <= 1e-15, ref.sym
    assert np.all(np.isfinite(ref.R))
    assert ref.rmax.min() > 0.0, "a 6x6 block of the inverse is exactly zero"
    assert ref.raw_bound <= CAP, (ref.d_ref, ref.raw_bound)
    assert ref.pad_ref == 0.0                                         # (padding decouples: both inverses return it exactly)


@pytest.mark.parametrize("name", [g[0] for g in child.G2O_GRAPHS if g[0] != "complete200_w1_nopanels"])     # (the same graph as complete200)
def test_g2o_reference(name):
    make = {g[0]: g[1] for g in child.G2O_GRAPHS}[name]
    _check(name, g2o_dense(make()))


def test_ba_reference():
    _check(child.BA_GRAPH, *ba_dense())
