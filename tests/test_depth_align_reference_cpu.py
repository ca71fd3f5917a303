"""tests/depth_align_reference.py, the yardstick of tests/test_gpu_depth_align.py, pinned without a GPU: against a per-pixel brute
force written from include/fgo_dense.h with Python floats and loops on 16 x 12 frames, its analytic Jacobian against central
differences, and the conditions the GPU test leans on --
  * every gate margin of the restatement exceeds 1e-6 (pixels or metres, as the gate is stated; the two thresholds of the solve
    relatively, 1e-3) at every evaluation of every pair of the two test scenes, in f64 and in longdouble: two implementations whose
    per-sample numbers differ by rounding alone then associate the same samples and take the same decisions;
  * the f64-against-longdouble difference of the restatement, norm-wise (max |difference| / max |value| of a block, absolute for
    the pose), stays inside the record depth_align_reference.YARDSTICK.  Measured over the 16 pairs at this commit: H 4.1e-16,
    g 5.4e-15, chi2 3.2e-15 at the first evaluation; pose 2.7e-16, info 2.3e-16 after the full run.  The GPU test allows 16 x the record;
  * the restatement recovers the ground truth of every pair within half the bound the GPU test holds the kernel to."""
import math

import numpy as np
import pytest

from tests import depth_align_reference as ref

TINY = ref.default_params(fx=23.0, fy=23.0, cx=8.0, cy=6.0, n_levels=1, skip=(1, 1, 1), normal_step=1, normal_jump=0.3505,
                          max_dist=0.3003, min_pairs=6)


def _tiny_frames():
    ci = ref.camera()
    cj = ref.camera(yaw=25.6, pitch=15.3, roll=1.5, pos=(0.02, -0.01, 0.015))
    return ref.render(ci, TINY, 16, 12), ref.render(cj, TINY, 16, 12), ref.relative_pose(ci, cj)


# ---- the brute force: one pixel at a time, the target's point and normal recomputed from the words at every look-up ----------------
def _point(P, u, v, word):
    z = float(word) * P["z_scale"]
    if not (z > P["z_min"] and z < P["z_max"]):
        return None
    return [((u - P["cx"]) * z) / P["fx"], ((v - P["cy"]) * z) / P["fy"], z]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _target(P, D, u, v):
    H, W = D.shape
    s = P["normal_step"]
    if u - s < 0 or u + s >= W or v - s < 0 or v + s >= H:
        return None
    p = _point(P, u, v, D[v, u])
    nb = [_point(P, u - s, v, D[v, u - s]), _point(P, u + s, v, D[v, u + s]), _point(P, u, v - s, D[v - s, u]), _point(P, u, v + s, D[v + s, u])]
    if p is None or any(x is None for x in nb):
        return None
    if any(abs(x[2] - p[2]) > P["normal_jump"] for x in nb):
        return None
    a = [nb[1][k] - nb[0][k] for k in range(3)]; b = [nb[3][k] - nb[2][k] for k in range(3)]
    c = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    l = math.sqrt(_dot(c, c))
    if not l > 0:
        return None
    n = [x / l for x in c]
    if _dot(n, p) > 0:
        n = [-x for x in n]
    return p, n


def _sigma2(P, n, p):
    z = p[2]
    sz = P["sigma_z"][0] + z * (P["sigma_z"][1] + z * P["sigma_z"][2])
    gx = (n[0] * z) / P["fx"]; gy = (n[1] * z) / P["fy"]
    nr = (n[0] * (p[0] / z) + n[1] * (p[1] / z)) + n[2]
    return (P["sigma_px"] * P["sigma_px"]) * (gx * gx + gy * gy) + (sz * sz) * (nr * nr)


def brute_evaluate(P, Di, Dj, t, q, k):
    H, W = Dj.shape
    R = ref.qmat([float(c) for c in q])
    Hm = [0.0] * 21; g = [0.0] * 6; chi2 = ss = 0.0
    used = []
    for v in range(0, H, k):
        for u in range(0, W, k):
            pj = _point(P, u, v, Dj[v, u])
            if pj is None:
                continue
            qv = [((R[c][0] * pj[0] + R[c][1] * pj[1]) + R[c][2] * pj[2]) + float(t[c]) for c in range(3)]
            if not qv[2] > 0:
                continue
            ud = float(np.rint((P["fx"] * qv[0]) / qv[2] + P["cx"])); vd = float(np.rint((P["fy"] * qv[1]) / qv[2] + P["cy"]))
            if not (0 <= ud <= W - 1 and 0 <= vd <= H - 1):
                continue
            tg = _target(P, Di, int(ud), int(vd))
            if tg is None:
                continue
            pi, n = tg
            e = [qv[c] - pi[c] for c in range(3)]
            if math.sqrt(_dot(e, e)) > P["max_dist"]:
                continue
            if abs(_dot(n, qv)) < P["min_cos"] * math.sqrt(_dot(qv, qv)):
                continue
            r = _dot(n, e)
            m = [(R[0][c] * n[0] + R[1][c] * n[1]) + R[2][c] * n[2] for c in range(3)]
            J = [pj[1] * m[2] - pj[2] * m[1], pj[2] * m[0] - pj[0] * m[2], pj[0] * m[1] - pj[1] * m[0], m[0], m[1], m[2]]
            w = 1.0 / (_sigma2(P, n, pi) + _sigma2(P, m, pj))
            for a in range(6):
                for b in range(a, 6):
                    Hm[ref.ut6(a, b)] += (w * J[a]) * J[b]
                g[a] += (w * J[a]) * r
            chi2 += (w * r) * r; ss += r * r
            used.append((u, v))
    return np.array(Hm), np.array(g), chi2, ss, used


@pytest.mark.parametrize("k", [1, 2])
def test_restatement_equals_the_per_pixel_brute_force(k):
    Di, Dj, truth = _tiny_frames()
    for pose in (np.array([0, 0, 0, 0, 0, 0, 1.0]), truth):
        ev = ref.evaluate(ref.frame(Dj, TINY), ref.frame(Di, TINY), pose[:3], pose[3:], k, TINY)
        Hm, g, chi2, ss, used = brute_evaluate(TINY, Di, Dj, pose[:3], pose[3:], k)
        assert ev["count"] == len(used) >= (40 if k == 1 else 10)
        assert list(zip(ev["u"].tolist(), ev["v"].tolist())) == used              # the same samples, in pixel order
        assert ref.rel_diff(ev["H"], Hm) < 1e-14 and ref.rel_diff(ev["g"], g) < 1e-13
        assert abs(ev["chi2"] - chi2) < 1e-13 * chi2 and abs(ev["ss"] - ss) < 1e-13 * ss


def test_the_gates_reject_what_the_header_says():
    """the brute force and the restatement agree where samples ARE rejected: a tight max_dist, a steep min_cos and a small
    normal_jump each remove associations, and remove the same ones"""
    Di, Dj, truth = _tiny_frames()
    full = ref.evaluate(ref.frame(Dj, TINY), ref.frame(Di, TINY), truth[:3], truth[3:], 1, TINY)["count"]
    for kw in (dict(max_dist=0.0503), dict(min_cos=0.8), dict(normal_jump=0.1005), dict(z_max=2.9), dict(normal_step=2)):
        P = dict(TINY, **kw)
        ev = ref.evaluate(ref.frame(Dj, P), ref.frame(Di, P), truth[:3], truth[3:], 1, P)
        used = brute_evaluate(P, Di, Dj, truth[:3], truth[3:], 1)[4]
        assert 0 < ev["count"] < full, kw
        assert list(zip(ev["u"].tolist(), ev["v"].tolist())) == used, kw


def test_analytic_jacobian_against_central_differences():
    """r(xi) = n . (T Exp(xi) p_j - p_i) with the association held fixed: dr/dxi = J = [p_j x m; m], m = R^T n"""
    Di, Dj, truth = _tiny_frames()
    src, tgt = ref.frame(Dj, TINY), ref.frame(Di, TINY)
    t, q = list(truth[:3]), list(truth[3:])
    ev = ref.evaluate(src, tgt, t, q, 1, TINY)
    assert ev["count"] > 40
    h = 1e-6
    for s in range(0, ev["count"], 7):
        u, v = ev["u"][s], ev["v"][s]
        pj = src["pts"][:, v, u]
        R = np.array(ref.qmat(q))
        qv = R @ pj + t
        ui, vi = int(np.rint(TINY["fx"] * qv[0] / qv[2] + TINY["cx"])), int(np.rint(TINY["fy"] * qv[1] / qv[2] + TINY["cy"]))
        pi, n = tgt["pts"][:, vi, ui], tgt["n"][:, vi, ui]

        def resid(xi):
            t2, q2 = ref.retract(t, q, list(xi), np.float64)
            return float(n @ (np.array(ref.qmat(q2)) @ pj + np.array(t2) - pi))

        assert abs(resid(np.zeros(6)) - ev["r"][s]) < 1e-14
        for c in range(6):
            d = np.zeros(6); d[c] = h
            assert abs((resid(d) - resid(-d)) / (2 * h) - ev["J"][c, s]) < 1e-8, (s, c)


def test_the_solve_is_a_solve_and_the_covariance_the_inverse():
    S = ref.scene("small")
    ev = ref.evaluate(ref.frame(S["depth"][1], S["P"]), ref.frame(S["depth"][0], S["P"]), [0, 0, 0], [0, 0, 0, 1], 1, S["P"])
    st, piv, s, M = ref.factor(ev, S["P"])
    assert st == ref.OK and piv > S["P"]["min_pivot"]
    Hf = np.zeros((6, 6))
    for r in range(6):
        for c in range(r, 6):
            Hf[r, c] = Hf[c, r] = ev["H"][ref.ut6(r, c)]
    d = np.array(ref.step(ev, s, M))
    assert np.allclose(Hf @ d, ev["g"], rtol=1e-9, atol=1e-9 * np.abs(ev["g"]).max())
    cov = ref.covariance(s, M)
    assert np.array_equal(cov, cov.T) and np.allclose(cov @ Hf, np.eye(6), atol=1e-9)


# ---- the conditions the GPU test leans on -----------------------------------------------------------------------------------------
CASES = [(kind, pair) for kind in ("big", "small") for pair in range(8)]


def test_longdouble_is_wider_than_f64():
    assert np.finfo(np.longdouble).eps < 1e-18          # the yardstick below needs an extended type


@pytest.mark.parametrize("kind,pair", CASES)
def test_scene_keeps_clear_of_every_gate_and_yardstick(kind, pair):
    S = ref.scene(kind)
    a, b = ref.scene_run(kind, pair), ref.scene_run(kind, pair, np.longdouble)
    for run in (a, b):
        assert run["status"] == ref.OK and run["converged"] == 1 and run["n_pairs_used"] >= S["P"]["min_pairs"]
        assert set(run["margins"]) == {"z_range", "normal_jump", "cross", "flip", "qz", "rint", "max_dist", "min_cos", "eps_rel", "pivot_rel"}
        for k, m in run["margins"].items():
            assert m > (ref.MARGIN_REL if k.endswith("_rel") else ref.MARGIN), (k, m)
    for k in ("status", "iterations", "converged", "n_pairs_used", "evaluations"):
        assert a[k] == b[k], k
    ne, nl = a["normal_eq"], b["normal_eq"]
    measured = {"H": ref.rel_diff(ne[:21], nl[:21]), "g": ref.rel_diff(ne[21:27], nl[21:27]), "chi2": ref.rel_diff(ne[27:], nl[27:]),
                "pose": float(np.max(np.abs(a["pose_ij"] - b["pose_ij"]))), "info": ref.rel_diff(a["info"], b["info"])}
    print(kind, pair, {k: "%.2e" % v for k, v in measured.items()})
    for k, v in measured.items():
        assert v <= ref.YARDSTICK[k], (k, v)
    # the start is "about 5 cm / 3 degrees off", and the restatement alone gets to the truth within half the GPU test's bound
    dt0, dr0 = ref.pose_error([0, 0, 0, 0, 0, 0, 1], S["truth"][pair])
    assert 0.015 < dt0 < 0.06 and math.radians(2.2) < dr0 < math.radians(3.2)
    dt, dr = ref.pose_error(a["pose_ij"], S["truth"][pair])
    bt, br = ref.truth_bound(kind)
    assert dt <= bt / 2 and dr <= br / 2 and dr < dr0
    assert dt < dt0 or kind == "small"          # a 40 x 30 pixel is 4.4 cm wide at 2.5 m: a start 3 cm off is below what those frames resolve


def test_truth_bound_is_the_restatements_own_error_times_two():
    for kind, (lim_t, lim_r) in (("big", (5e-4, 3e-4)), ("small", (8e-2, 2e-2))):
        bt, br = ref.truth_bound(kind)
        errs = [ref.pose_error(ref.scene_run(kind, p)["pose_ij"], ref.scene(kind)["truth"][p]) for p in range(8)]
        assert bt == 2 * max(e[0] for e in errs) and br == 2 * max(e[1] for e in errs)
        assert 0 < bt < lim_t and 0 < br < lim_r          # depth quantisation and nothing else: under a tenth of a pixel's width at 176 x 144, under two pixels at 40 x 30 (4.4 cm each)


def test_failure_statuses_of_the_restatement():
    P = ref.small_params()
    wall = np.full((30, 40), 2000, np.uint16)
    o = ref.align(wall, wall, None, P)
    assert o["status"] == ref.DEGENERATE and o["min_pivot"] < P["min_pivot"] and o["iterations"] == 0
    assert np.array_equal(o["pose_ij"], [0, 0, 0, 0, 0, 0, 1]) and o["info"][ref.ut6(3, 3)] == 10000.0 and not o["cov"].any()
    for empty in (np.zeros((30, 40), np.uint16), np.full((30, 40), 6000, np.uint16)):
        o = ref.align(empty, empty, None, P)
        assert o["status"] == ref.TOO_FEW and o["n_pairs_used"] == 0
    S = ref.scene("small")
    o = ref.align(S["depth"][0], S["depth"][0], None, P)
    assert o["status"] == ref.OK and o["converged"] == 1 and o["iterations"] == P["n_levels"]
    assert np.array_equal(o["pose_ij"], [0, 0, 0, 0, 0, 0, 1]) and o["chi2"] == 0 and o["rmse"] == 0
