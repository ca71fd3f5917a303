"""numpy evaluation of the edge gate (fgo_gate_edges_se3) from a dense covariance: for a candidate edge between a and b with
measurement Z and information W at the current estimate,
    e, Ja, Jb   from the oracle's factor functions (orc.edge_se3: g2o [t; q] tangent, orc.between: GTSAM [w; v] tangent)
    chi2 = e' W e
    P    = Ja Saa Ja' + Ja Sab Jb' + Jb Sab' Ja' + Jb Sbb Jb'      (S.. blocks of Sigma = H^-1; zero for a fixed endpoint)
    d2   = e' (P + W^-1)^-1 e
and, as a cross-check of the algebra, the whitened form d2 = w' (I + L' P L)^-1 w with W = L L', w = L' e."""
import numpy as np

from tests import orc_binding as orc
from tests.util import info_full, info_ut, noisy, pose_inv, pose_mul, random_info


def predicted_cov(Ja, Jb, Saa, Sab, Sbb, cross=True):
    """P; a block that is None counts as zero (fixed endpoint); cross=False drops the Sab terms (a deliberately wrong variant)"""
    P = np.zeros((6, 6))
    if Saa is not None:
        P += Ja @ Saa @ Ja.T
    if Sbb is not None:
        P += Jb @ Sbb @ Jb.T
    if cross and Sab is not None:
        C = Ja @ Sab @ Jb.T
        P += C + C.T
    return P


def d2_direct(e, P, W):
    return float(e @ np.linalg.solve(P + np.linalg.inv(W), e))


def d2_whitened(e, P, W):
    L = np.linalg.cholesky(W)
    w = L.T @ e
    return float(w @ np.linalg.solve(np.eye(6) + L.T @ P @ L, w))


def sigma_blocks(Sigma, pos, a, b):
    """(Saa, Sab, Sbb) of the dense Sigma; pos[v] = block index of variable v among the free ones, None if v is fixed"""
    def blk(u, v):
        if pos[u] is None or pos[v] is None:
            return None
        return Sigma[6 * pos[u]:6 * pos[u] + 6, 6 * pos[v]:6 * pos[v] + 6]
    return blk(a, a), blk(a, b), blk(b, b)


def gate(Sigma, pos, values, a, b, z, W, gtsam=False, cross=True):
    """dict(e, Ja, Jb, chi2, P, d2, d2w, cond) of one candidate"""
    e, Ja, Jb = (orc.between if gtsam else orc.edge_se3)(values[a], values[b], z)
    Saa, Sab, Sbb = sigma_blocks(Sigma, pos, a, b)
    P = predicted_cov(Ja, Jb, Saa, Sab, Sbb, cross)
    return dict(e=e, Ja=Ja, Jb=Jb, chi2=float(e @ W @ e), P=P, d2=d2_direct(e, P, W), d2w=d2_whitened(e, P, W),
                cond=float(np.linalg.cond(P + np.linalg.inv(W))))


def free_positions(fixed):
    pos, k = [], 0
    for f in fixed:
        pos.append(None if f else k)
        k += 0 if f else 1
    return pos


# the candidates of the small g2o scenario (small_graph(default_rng(31), n=150, extra=12), vertex 0 fixed): neighbours on the factor's
# pattern, far pairs off it, fixed endpoints
SMALL_PAIRS = [(5, 6), (6, 5), (30, 31), (1, 149), (149, 2), (10, 120), (75, 3), (77, 141), (0, 149), (120, 0), (0, 1)]


def candidates(rng, values, pairs, st=0.05, sq=0.02):
    """(a, b, meas[n, 7], info[n, 21]): the current relative pose of every pair, perturbed, with a random dense information"""
    a = np.array([p[0] for p in pairs], np.int64); b = np.array([p[1] for p in pairs], np.int64)
    meas = np.array([noisy(rng, pose_mul(pose_inv(values[i]), values[j]), st, sq) for i, j in pairs])
    info = np.array([info_ut(random_info(rng)) for _ in pairs])
    return a, b, meas, info


def gate_many(Sigma, pos, values, a, b, meas, info, gtsam=False):
    return [gate(Sigma, pos, values, int(a[k]), int(b[k]), meas[k], info_full(info[k]), gtsam) for k in range(len(a))]
