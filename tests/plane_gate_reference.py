"""numpy evaluation of the plane gate (fgo_gate_plane_factors, fgo_associate_planes) from a dense covariance: for a candidate
observation z = (n_z, d_z), covariance S, of plane p from pose x at the current estimate,
    e, Jx, Jp   from the oracle's factor function (orc.plane_factor: 3 rows, [w; v] pose tangent, 3-dof plane tangent)
    chi2 = e' S^-1 e
    P    = Jx Sxx Jx' + Jx Sxp Jp' + Jp Sxp' Jx' + Jp Spp Jp'    (S.. blocks of Sigma = H^-1; zero for a fixed endpoint)
    d2   = e' (P + S)^-1 e
    cos  = n' . n_z                                              (n' = the plane's normal seen from the pose)
and the association rule on a matrix of d2 / cos values."""
import numpy as np

from tests import orc_binding as orc


def cov_full(ut6):
    s = ut6
    return np.array([[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]], float)


def cov_ut(S):
    return np.array([S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2]])


def predicted_cov(Jx, Jp, Sxx, Sxp, Spp, cross=True):
    """P (3x3); Sxx 6x6, Sxp 6x3, Spp 3x3; a block that is None counts as zero (fixed endpoint); cross=False drops the Sxp terms
    (the deliberately wrong form the reference has commented out)"""
    P = np.zeros((3, 3))
    if Sxx is not None:
        P += Jx @ Sxx @ Jx.T
    if Spp is not None:
        P += Jp @ Spp @ Jp.T
    if cross and Sxp is not None:
        C = Jx @ Sxp @ Jp.T
        P += C + C.T
    return P


def sigma_blocks(Sigma, pos, x, p):
    """(Sxx, Sxp, Spp) of the dense Sigma of padded 6-blocks; pos[v] = block index of variable v among the free ones, None if fixed.
    Only the leading three rows / columns of the plane's block are taken: its padding is never read."""
    ix, ip = pos[x], pos[p]
    Sxx = None if ix is None else Sigma[6 * ix:6 * ix + 6, 6 * ix:6 * ix + 6]
    Spp = None if ip is None else Sigma[6 * ip:6 * ip + 3, 6 * ip:6 * ip + 3]
    Sxp = None if ix is None or ip is None else Sigma[6 * ix:6 * ix + 6, 6 * ip:6 * ip + 3]
    return Sxx, Sxp, Spp


def d2_direct(e, P, S):
    return float(e @ np.linalg.solve(P + S, e))


def gate_blocks(values, x, p, z, S, Sxx, Sxp, Spp, cross=True):
    """dict(e, Jx, Jp, chi2, P, d2, cos, cond) of one candidate from its three covariance blocks"""
    e, Jx, Jp = orc.plane_factor(values[x], values[p][:4], z)
    P = predicted_cov(Jx, Jp, Sxx, Sxp, Spp, cross)
    n_pred = orc.plane_transform(values[p][:4], values[x])[:3]
    return dict(e=e, Jx=Jx, Jp=Jp, chi2=float(e @ np.linalg.solve(S, e)), P=P, d2=d2_direct(e, P, S), cos=float(n_pred @ z[:3]),
                cond=float(np.linalg.cond(P + S)))


def gate(Sigma, pos, values, x, p, z, S, cross=True):
    return gate_blocks(values, x, p, z, S, *sigma_blocks(Sigma, pos, x, p), cross=cross)


def associate(D2, COS, pd, d2_gate, cos_min):
    """The association rule on k x m arrays of d2, cos and `pd` (both covariances positive definite): a candidate with
    cos < cos_min or not pd is excluded (+inf); per observation the smallest and second smallest d2 going through the planes from
    the first to the last, a tie to the earlier one; match = position of the smallest if it is < d2_gate, else -1.
    Returns (match positions[k], best2[k, 2], matrix[k, m])."""
    k, m = D2.shape
    M = np.where(pd & (COS >= cos_min), D2, np.inf)
    match = np.full(k, -1, np.int64); best2 = np.full((k, 2), np.inf)
    for i in range(k):
        for j in range(m):
            d = M[i, j]
            if d < best2[i, 0]:
                best2[i, 1] = best2[i, 0]; best2[i, 0] = d; match[i] = j
            elif d < best2[i, 1]:
                best2[i, 1] = d
        if not best2[i, 0] < d2_gate:
            match[i] = -1
    return match, best2, M


def random_cov(rng, lo=1e-4, hi=1e-2):
    """dense random SPD 3x3 with eigenvalues in [lo, hi]"""
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return Q @ np.diag(rng.uniform(lo, hi, size=3)) @ Q.T


def perturbed_view(rng, values, x, p, lo=0.05, hi=0.3):
    """the predicted plane in the pose frame retracted by a tangent vector of norm lo .. hi"""
    v = rng.normal(size=3)
    v *= rng.uniform(lo, hi) / np.linalg.norm(v)
    return orc.plane_retract(orc.plane_transform(values[p][:4], values[x]), v)
