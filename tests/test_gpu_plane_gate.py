"""Gating and association of plane observations on the device (fgo_gate_plane_factors, fgo_associate_planes;
kernels_plane_gate.hip): the squared Mahalanobis distance of a candidate observation's innovation under the map's covariance,
against tests/plane_gate_reference.py evaluated on numpy.linalg.inv of the oracle's dense information matrix."""
import numpy as np
import pytest

import graph_slam_amd as G
from tests import gate_reference as RE
from tests import orc_binding as orc
from tests import plane_gate_reference as R
from tests.test_gpu_factors import mixed_gpu
from tests.util import SR4000_CALIB, info_ut, mixed_graph, mixed_oracle, noisy, pose_inv, pose_mul, small_graph

pytestmark = pytest.mark.gpu

S_OBS = np.array([1e-4, 0, 0, 1e-4, 0, 1e-4])                                    # 1e-4 I, the covariance of the graphs' own plane factors
COS10 = float(np.cos(np.deg2rad(10.0)))
_cache = {}


def _mixed():
    """the small mixed graph (10 poses, planes 10..12, 14 points; nothing fixed) and its dense covariance, computed once"""
    if "mixed" not in _cache:
        g = mixed_graph(np.random.default_rng(22), n_poses=10, n_planes=3, n_points=14)
        Sigma = np.linalg.inv(mixed_oracle(g).dense_system()[0])
        Sigma.setflags(write=False)
        _cache["mixed"] = (g, Sigma, list(range(len(g["values"]))))
    return _cache["mixed"]


def _candidates(rng, V, pairs):
    x = np.array([p[0] for p in pairs], np.int64); p = np.array([p[1] for p in pairs], np.int64)
    z = np.array([R.perturbed_view(rng, V, i, j) for i, j in pairs])
    S = np.array([R.random_cov(rng) for _ in pairs])
    return x, p, z, S, np.array([R.cov_ut(s) for s in S])


def _check(refs, S, d2, chi2, cos, P, e, tol_sigma, label):
    """chi2, e, cos to 1e-11 relative (the per-edge tolerance); P to tol_sigma x max|P| (the bound the marginal
    tests hold blocks of Sigma to); d2 against the full reference to tol_sigma x cond(P + S), the first-order effect of that bound;
    d2 against e'(P_device + S)^-1 e in numpy to 1e-9 (the kernel's own factorisation and solve)"""
    worst = dict(chi2=0.0, e=0.0, cos=0.0, P=0.0, d2_over_cond=0.0, d2_own=0.0)
    for k, ref in enumerate(refs):
        worst["chi2"] = max(worst["chi2"], abs(chi2[k] - ref["chi2"]) / ref["chi2"])
        worst["e"] = max(worst["e"], np.abs(e[k] - ref["e"]).max() / np.abs(ref["e"]).max())
        worst["cos"] = max(worst["cos"], abs(cos[k] - ref["cos"]) / abs(ref["cos"]))
        scale = np.abs(ref["P"]).max()
        if scale > 0:
            worst["P"] = max(worst["P"], np.abs(P[k] - ref["P"]).max() / scale)
        else:
            assert np.all(P[k] == 0)
        worst["d2_over_cond"] = max(worst["d2_over_cond"], abs(d2[k] - ref["d2"]) / ref["d2"] / ref["cond"])
        worst["d2_own"] = max(worst["d2_own"], abs(d2[k] - R.d2_direct(ref["e"], P[k], S[k])) / d2[k])
        assert 0 <= d2[k] <= chi2[k] * (1 + 1e-12), (k, d2[k], chi2[k])
    print("%s: largest errors chi2 %.1e, e %.1e, cos %.1e, P / max|P| %.1e, d2 / cond %.1e (cond <= %.1e), d2 against its own P %.1e"
          % (label, worst["chi2"], worst["e"], worst["cos"], worst["P"], worst["d2_over_cond"], max(r["cond"] for r in refs), worst["d2_own"]))
    assert worst["chi2"] <= 1e-11 and worst["e"] <= 1e-11 and worst["cos"] <= 1e-11
    assert worst["P"] <= tol_sigma
    assert worst["d2_over_cond"] <= tol_sigma
    assert worst["d2_own"] <= 1e-9


def test_every_pose_plane_pair_of_the_mixed_graph():
    g, Sigma, pos = _mixed()
    gr = mixed_gpu(g)
    pairs = [(x, 10 + p) for x in range(10) for p in range(3)]                    # 12 of them share a plane factor, 18 do not
    shared = {(int(i), int(j)) for i, j, kd in zip(g["ei"], g["ej"], g["kind"]) if kd == orc.FK_PLANE}
    assert 0 < len(shared & set(pairs)) < len(pairs)
    x, p, z, S, S6 = _candidates(np.random.default_rng(51), g["values"], pairs)
    d2, chi2, cos, P, e = gr.gate_plane_factors(x, p, z, S6, want_cov=True, want_resid=True)
    refs = [R.gate(Sigma, pos, g["values"], int(x[k]), int(p[k]), z[k], S[k]) for k in range(len(pairs))]
    _check(refs, S, d2, chi2, cos, P, e, 1e-7, "mixed graph, 30 pairs")          # (1e-7: the level this graph's marginal test holds)
    d2b, chi2b, cosb = gr.gate_plane_factors(x, p, z, S6)                         # without P: the same numbers
    assert np.array_equal(d2, d2b) and np.array_equal(chi2, chi2b) and np.array_equal(cos, cosb)
    # the form without the cross term is a different number: the device has it in
    nocross = np.array([R.gate(Sigma, pos, g["values"], int(x[k]), int(p[k]), z[k], S[k], cross=False)["d2"] for k in range(len(pairs))])
    assert np.abs(nocross / d2 - 1).max() > 1e-2


def test_exact_measurement_gives_zero():
    g, _, _ = _mixed()
    gr = mixed_gpu(g)
    pairs = [(0, 10), (3, 11), (9, 12), (5, 10), (7, 12)]
    z = np.array([orc.plane_transform(g["values"][j][:4], g["values"][i]) for i, j in pairs])
    S6 = np.array([R.cov_ut(R.random_cov(np.random.default_rng(52))) for _ in pairs])
    d2, chi2, cos = gr.gate_plane_factors([q[0] for q in pairs], [q[1] for q in pairs], z, S6)
    assert np.all(chi2 < 1e-20) and np.all(d2 < 1e-20) and np.all(d2 >= 0), (chi2, d2)
    assert np.all(np.abs(cos - 1) < 1e-12)


def chain_graph(rng, n_poses=80, n_planes=3, seen_from=(0, 1, 2, 3), noise=0.01):
    """A chain of poses (odometry only) whose planes are seen from the first few poses only, in the layout of tests.util.mixed_graph
    (no points): a late pose shares no factor with a plane and is far from it in the elimination tree."""
    g0 = small_graph(rng, n=n_poses, extra=0, noise=noise, fixed_first=False)
    truth = [np.array([0, 0, 0, 0, 0, 0, 1.0])]
    for k in range(n_poses - 1):
        truth.append(pose_mul(truth[-1], g0["meas"][k]))
    truth = np.array(truth)
    N = n_poses + n_planes
    values = np.zeros((N, 7)); vkind = np.zeros(N, np.int32)
    values[:n_poses] = [noisy(rng, t, 0.05, 0.02) for t in truth]
    values[0] = truth[0]
    ei, ej, kind, meas, info = [], [], [], [], []
    Wb = np.diag([1 / 0.01 ** 2] * 3 + [1 / 0.02 ** 2] * 3)
    for k in range(n_poses - 1):
        z = pose_mul(pose_inv(truth[k]), truth[k + 1])
        ei.append(k); ej.append(k + 1); kind.append(orc.FK_BETWEEN); meas.append(noisy(rng, z, noise, noise * 0.5)); info.append(info_ut(Wb))
    for p in range(n_planes):
        vid = n_poses + p
        n = rng.normal(size=3); n /= np.linalg.norm(n)
        pl = np.array([n[0], n[1], n[2], rng.uniform(2.0, 6.0)])
        values[vid, :4] = orc.plane_retract(pl, rng.normal(size=3) * 0.05)
        vkind[vid] = orc.VK_PLANE
        for k in seen_from:
            m = np.zeros(7); m[:4] = orc.plane_retract(orc.plane_transform(pl, truth[k]), rng.normal(size=3) * noise)
            ei.append(int(k)); ej.append(vid); kind.append(orc.FK_PLANE); meas.append(m)
            w = np.zeros(21); w[:6] = [1e4, 0, 0, 1e4, 0, 1e4]; info.append(w)
    return dict(values=values, vkind=vkind, ei=np.array(ei, np.int32), ej=np.array(ej, np.int32), kind=np.array(kind, np.int32),
                meas=np.array(meas), info=np.array(info), prior_ids=np.array([0], np.int32), prior_mean=np.array([truth[0]]),
                prior_info=np.array([info_ut(np.diag([1e14] * 6))]), calib=SR4000_CALIB.copy(), bps=np.array([0, 0, 0, 0, 0, 0, 1.0]),
                n_poses=n_poses, n_planes=n_planes, n_points=0)


def test_off_pattern_pairs_go_through_column_solves():
    """80 poses in a chain, planes 80..82 seen from poses 0..3.  The candidates are poses 60..79 against those planes: no
    such pair shares a factor, and a late pose is eliminated in a sub-tree that never reaches the planes' neighbourhood, so its
    cross-covariance block is off the factor's pattern.  The reference takes its blocks from marginal_cov_pairs (which solves for
    the planes' columns; the gate solves for whichever side has fewer), each held to 1e-7 x max|block| against the dense inverse
    here, the level the other GTSAM-semantics graphs' marginals are held to."""
    g = chain_graph(np.random.default_rng(53))
    gr = mixed_gpu(g)
    V, n0 = g["values"], g["n_poses"]
    pairs = [(x, n0 + (x + t) % 3) for x in range(n0 - 20, n0) for t in range(2)]
    x, p, z, S, S6 = _candidates(np.random.default_rng(54), V, pairs)
    d2, chi2, cos, P, e = gr.gate_plane_factors(x, p, z, S6, want_cov=True, want_resid=True)
    st = gr.gate_stats()
    print("chain graph:", st)
    assert st["off_pattern"] >= 1 and st["column_groups"] >= 1, st
    Sxx, Spp, Sxp = gr.marginal_cov_pairs(x, x), gr.marginal_cov_pairs(p, p), gr.marginal_cov_pairs(x, p)
    Sigma = np.linalg.inv(mixed_oracle(g).dense_system()[0])
    for k, (i, j) in enumerate(pairs):
        for blk, (a, b) in ((Sxx[k], (i, i)), (Spp[k], (j, j)), (Sxp[k], (i, j))):
            ref = Sigma[6 * a:6 * a + 6, 6 * b:6 * b + 6]
            np.testing.assert_allclose(blk, ref, rtol=0, atol=1e-7 * np.abs(ref).max())
    refs = [R.gate_blocks(V, i, j, z[k], S[k], Sxx[k], Sxp[k][:, :3], Spp[k][:3, :3]) for k, (i, j) in enumerate(pairs)]
    _check(refs, S, d2, chi2, cos, P, e, 1e-7, "chain graph, 40 late pairs")
    # the association form from one late pose: one group of six solves (the pose's columns) serves all planes
    planes, late = np.arange(n0, n0 + 3), n0 - 3
    rk = np.random.default_rng(55)
    zk = np.array([R.perturbed_view(rk, V, late, n0 + t % 3, 0.01, 0.03) for t in range(5)])
    match, best2, D = gr.associate_planes(late, zk, np.tile(S_OBS, (5, 1)), planes, want_matrix=True)
    st = gr.gate_stats()
    assert st["column_groups"] == 1 and st["off_pattern"] >= 5, st
    xs = np.full(15, late); ps = np.tile(planes, 5)
    dd = gr.gate_plane_factors(xs, ps, np.repeat(zk, 3, axis=0), np.tile(S_OBS, (15, 1)))[0]
    blocks = gr.marginal_cov_pairs([late] * 3, [late] * 3), gr.marginal_cov_pairs([late] * 3, planes), gr.marginal_cov_pairs(planes, planes)
    for i in range(5):
        for j in range(3):
            ref = R.gate_blocks(V, late, n0 + j, zk[i], R.cov_full(S_OBS), blocks[0][j], blocks[1][j][:, :3], blocks[2][j][:3, :3])
            assert abs(D[i, j] - ref["d2"]) <= 1e-7 * ref["cond"] * ref["d2"]
            assert abs(dd[3 * i + j] - ref["d2"]) <= 1e-7 * ref["cond"] * ref["d2"]


def test_fixed_pose_contributes_nothing():
    g, _, _ = _mixed()
    gr = mixed_gpu(g)
    gr._chk(G.lib.fgo_set_fixed(gr._h, 4, 1))
    fixed = np.zeros(len(g["values"]), np.uint8); fixed[4] = 1
    po = orc.Problem(g["values"], fixed, g["ei"], g["ej"], g["meas"], g["info"])
    po.set_kinds(g["vkind"], g["kind"]); po.set_calibration(g["calib"], g["bps"])
    po.add_priors(g["prior_ids"], g["prior_mean"], g["prior_info"])
    Sigma, pos = np.linalg.inv(po.dense_system()[0]), RE.free_positions(fixed)
    assert Sigma.shape[0] == 6 * (len(fixed) - 1) and pos[4] is None
    pairs = [(4, 10), (4, 11), (4, 12), (3, 11), (5, 12)]
    x, p, z, S, S6 = _candidates(np.random.default_rng(56), g["values"], pairs)
    d2, chi2, cos, P, e = gr.gate_plane_factors(x, p, z, S6, want_cov=True, want_resid=True)
    refs = [R.gate(Sigma, pos, g["values"], int(x[k]), int(p[k]), z[k], S[k]) for k in range(len(pairs))]
    _check(refs, S, d2, chi2, cos, P, e, 1e-7, "pose 4 fixed")
    for k in range(3):                                                            # P = Jp Spp Jp' alone
        Jp, Spp = refs[k]["Jp"], Sigma[6 * pos[p[k]]:6 * pos[p[k]] + 3, 6 * pos[p[k]]:6 * pos[p[k]] + 3]
        np.testing.assert_allclose(refs[k]["P"], Jp @ Spp @ Jp.T, rtol=0, atol=1e-15 * np.abs(refs[k]["P"]).max())
    # and the device's P is that of its own plane marginal alone.  J of the device and of the oracle agree to the per-edge 1e-11 and P is
    # bilinear in J: 1e-10 x max|P| with margin
    Spp_dev = gr.marginal_cov_pairs(p[:3], p[:3])
    for k in range(3):
        Pk = refs[k]["Jp"] @ Spp_dev[k][:3, :3] @ refs[k]["Jp"].T
        np.testing.assert_allclose(P[k], Pk, rtol=0, atol=1e-10 * np.abs(Pk).max())


def _association_scenario():
    """pose 5 of the mixed graph against planes 10, 11, 12: (z[4, 4], S6[4, 6]) and the reference's k x m arrays"""
    g, Sigma, pos = _mixed()
    V, x, planes = g["values"], 5, np.array([10, 11, 12], np.int64)
    rng = np.random.default_rng(57)
    pred = [orc.plane_transform(V[j][:4], V[x]) for j in planes]
    z = [orc.plane_retract(pred[0], rng.normal(size=3) * 0.01), orc.plane_retract(pred[2], rng.normal(size=3) * 0.01)]
    while True:                                                                   # a normal more than 30 degrees from all three
        n = rng.normal(size=3); n /= np.linalg.norm(n)
        if max(float(n @ q[:3]) for q in pred) < np.cos(np.deg2rad(30.0)):
            break
    z.append(np.array([n[0], n[1], n[2], 3.0]))
    z.append(pred[1] + np.array([0, 0, 0, 0.08]))
    z = np.array(z)
    refs = [[R.gate(Sigma, pos, V, x, int(j), z[i], R.cov_full(S_OBS)) for j in planes] for i in range(4)]
    D2 = np.array([[r["d2"] for r in row] for row in refs]); COS = np.array([[r["cos"] for r in row] for row in refs])
    return g, x, planes, z, np.tile(S_OBS, (4, 1)), refs, D2, COS


def test_association_of_four_observations():
    g, x, planes, z, S6, refs, D2, COS = _association_scenario()
    rmatch, rbest2, RM = R.associate(D2, COS, np.ones_like(D2, bool), 7.815, COS10)
    # the scenario's character, on the reference itself
    assert rmatch[0] == 0 and rmatch[1] == 2
    assert np.all(np.isinf(RM[2])) and rmatch[2] == -1
    assert rmatch[3] == -1 and COS[3, 1] >= COS10 and abs(refs[3][1]["e"][2]) <= 0.2      # the coarse test accepts it
    assert np.isfinite(RM[3, 1]) and RM[3, 1] >= 7.815
    gr = mixed_gpu(g)
    match, best2, D = gr.associate_planes(x, z, S6, planes, d2_gate=7.815, cos_min=COS10, want_matrix=True)
    print("association: match", match, "best2", best2.tolist(), "reference", rbest2.tolist())
    np.testing.assert_array_equal(match, np.where(rmatch >= 0, planes[np.maximum(rmatch, 0)], -1))
    np.testing.assert_array_equal(np.isinf(D), np.isinf(RM))
    for i in range(4):
        for j in range(3):
            if np.isfinite(RM[i, j]):
                assert abs(D[i, j] - RM[i, j]) <= 1e-7 * refs[i][j]["cond"] * RM[i, j], (i, j)
        for t in range(2):
            if np.isfinite(rbest2[i, t]):
                assert abs(best2[i, t] - rbest2[i, t]) <= 1e-7 * max(r["cond"] for r in refs[i]) * rbest2[i, t], (i, t)
            else:
                assert np.isinf(best2[i, t])
    # the matrix is gate_plane_factors on the expanded list, bit for bit; best2 / match follow from it by the rule
    d2, chi2, cos = gr.gate_plane_factors(np.full(12, x), np.tile(planes, 4), np.repeat(z, 3, axis=0), np.repeat(S6, 3, axis=0))
    assert np.array_equal(D, np.where(cos >= COS10, d2, np.inf).reshape(4, 3))
    dmatch, dbest2, _ = R.associate(d2.reshape(4, 3), cos.reshape(4, 3), np.ones((4, 3), bool), 7.815, COS10)
    assert np.array_equal(best2, dbest2) and np.array_equal(match, np.where(dmatch >= 0, planes[np.maximum(dmatch, 0)], -1))
    m2, b2 = gr.associate_planes(x, z, S6, planes, d2_gate=7.815, cos_min=COS10)      # without the matrix: the same
    assert np.array_equal(m2, match) and np.array_equal(b2, best2)
    # cos_min = -1 disables the exclusion; an indefinite S excludes the observation's candidates instead of failing
    ma, ba, Da = gr.associate_planes(x, z, S6, planes, want_matrix=True)
    assert np.array_equal(Da, d2.reshape(4, 3)) and np.all(np.isfinite(ba))       # (the runner-up is reduced too)
    amatch, abest2, _ = R.associate(d2.reshape(4, 3), cos.reshape(4, 3), np.ones((4, 3), bool), 7.815, -1.0)
    assert np.array_equal(ba, abest2) and np.array_equal(ma, np.where(amatch >= 0, planes[np.maximum(amatch, 0)], -1))
    bad = S6.copy(); bad[1] = [1e-4, 0, 0, -1e-4, 0, 1e-4]
    mb, bb, Db = gr.associate_planes(x, z, bad, planes, want_matrix=True)
    assert mb[1] == -1 and np.all(np.isinf(Db[1])) and np.all(np.isinf(bb[1])) and np.all(np.isfinite(Db[[0, 2, 3]]))
    # a duplicated observation gets identical rows; another order of the planes permutes the columns
    zz = np.vstack([z, z[:1]]); SS = np.vstack([S6, S6[:1]])
    m5, b5, D5 = gr.associate_planes(x, zz, SS, planes, d2_gate=7.815, cos_min=COS10, want_matrix=True)
    assert np.array_equal(D5[4], D5[0]) and np.array_equal(b5[4], b5[0]) and m5[4] == m5[0] and np.array_equal(D5[:4], D)
    mr, br, Dr = gr.associate_planes(x, z, S6, planes[::-1].copy(), d2_gate=7.815, cos_min=COS10, want_matrix=True)
    assert np.array_equal(Dr[:, ::-1], D) and np.array_equal(mr, match) and np.array_equal(br, best2)


def test_a_tie_goes_to_the_earlier_entry():
    """Two planes with identical values, the pose and both planes fixed: P = 0, so both candidates get the same bits, and the match
    is whichever of the two comes first in plane_ids."""
    ident = np.array([0, 0, 0, 0, 0, 0, 1.0])
    gr = G.Graph()
    gr.add_poses(np.array([ident, [1.0, 0, 0, 0, 0, 0, 1.0]]))
    gr.add_prior(0, ident, info_ut(np.eye(6) * 1e6))
    gr.add_edges([0], [1], np.array([[1.0, 0, 0, 0, 0, 0, 1.0]]), np.array([info_ut(np.eye(6) * 1e4)]), tangent_order=G.FGO_TANGENT_GTSAM)
    for pid in (7, 8):
        gr.add_plane(pid, [0.0, 0.6, 0.8, 3.0])
        gr.add_plane_factor(1, pid, [0.0, 0.6, 0.8, 3.0], S_OBS)
        gr._chk(G.lib.fgo_set_fixed(gr._h, pid, 1))
    gr._chk(G.lib.fgo_set_fixed(gr._h, 0, 1))
    z = np.array([[0.0, 0.6, 0.8, 3.01]])
    for ids in ([7, 8], [8, 7]):
        match, best2, D = gr.associate_planes(0, z, S_OBS[None], ids, want_matrix=True)
        assert D[0, 0] == D[0, 1] and best2[0, 0] == best2[0, 1] == D[0, 0], D
        assert abs(D[0, 0] - 1.0) < 1e-9                                           # (0.01)^2 / 1e-4
        assert match[0] == ids[0]
    d2, chi2, cos, P = gr.gate_plane_factors([0], [7], z, S_OBS[None], want_cov=True)
    assert d2[0] == chi2[0] and np.all(P == 0)                                    # both endpoints fixed


def test_determinism_and_residency():
    g, _, _ = _mixed()
    pairs = [(x, 10 + p) for x in range(10) for p in range(3)]
    x, p, z, S, S6 = _candidates(np.random.default_rng(58), g["values"], pairs)
    gr1, gr2 = mixed_gpu(g), mixed_gpu(g)
    o1 = gr1.gate_plane_factors(x, p, z, S6, want_cov=True, want_resid=True)
    si = gr1.selinv_stats()
    o2 = gr2.gate_plane_factors(x, p, z, S6, want_cov=True, want_resid=True)
    o1b = gr1.gate_plane_factors(x, p, z, S6, want_cov=True, want_resid=True)
    for a, b, c in zip(o1, o2, o1b):
        assert np.array_equal(a, b) and np.array_equal(a, c)                      # bit-equal across contexts and on repeat
    perm = np.random.default_rng(59).permutation(len(pairs))
    for a, b in zip(o1, gr1.gate_plane_factors(x[perm], p[perm], z[perm], S6[perm], want_cov=True, want_resid=True)):
        assert np.array_equal(a[perm], b)                                         # a candidate's bits do not depend on its position
    one = gr1.gate_plane_factors(x[17:18], p[17:18], z[17:18], S6[17:18])
    assert one[0][0] == o1[0][17] and one[1][0] == o1[1][17]
    gr1.associate_planes(3, z[:4], S6[:4], [10, 11, 12])
    # the repeats ran no factorisation and no selected inversion: the figures of the last one (HIP event times) are untouched
    assert gr1.selinv_stats() == si and si["ms_factor"] > 0 and si["ms_sweep"] > 0


def test_the_context_is_untouched():
    g, _, _ = _mixed()
    pairs = [(1, 10), (7, 12), (4, 11)]
    x, p, z, S, S6 = _candidates(np.random.default_rng(60), g["values"], pairs)
    ga, gb = mixed_gpu(g), mixed_gpu(g)
    ga.chi2(); gb.chi2()
    a, b, meas, info = RE.candidates(np.random.default_rng(61), g["values"], [(1, 7), (8, 2), (0, 5)])
    se3_before = gb.gate_edges(a, b, meas, info, tangent_order=G.FGO_TANGENT_GTSAM, want_cov=True)
    gb.gate_plane_factors(x, p, z, S6, want_cov=True)
    gb.associate_planes(6, z, S6, [10, 11, 12], want_matrix=True)
    for u, v in zip(se3_before, gb.gate_edges(a, b, meas, info, tangent_order=G.FGO_TANGENT_GTSAM, want_cov=True)):
        assert np.array_equal(u, v)                                               # the SE3 gate around a plane call: the same bits
    assert G.lib.fgo_num_edges(gb._h) == G.lib.fgo_num_edges(ga._h)              # nothing was added
    ga.optimize_gtsam(2); gb.optimize_gtsam(2)
    assert np.array_equal(ga.get_poses(), gb.get_poses())
    for u, v in zip(ga.trace(), gb.trace()):
        assert np.array_equal(u, v)
    assert np.array_equal(gb.gate_plane_factors(x, p, z, S6)[0], ga.gate_plane_factors(x, p, z, S6)[0])           # and at the new estimate


def test_errors_and_empty_requests():
    g, _, _ = _mixed()
    gr = mixed_gpu(g)
    pairs = [(1, 10), (7, 12), (4, 11)]
    x, p, z, S, S6 = _candidates(np.random.default_rng(62), g["values"], pairs)
    gr.gate_plane_factors(x, p, z, S6)
    with pytest.raises(G.FgoError, match="candidate 1"):
        gr.gate_plane_factors([1, 1000, 4], p, z, S6)                             # unknown id
    with pytest.raises(G.FgoError, match="candidate 2"):
        gr.gate_plane_factors([1, 7, 11], p, z, S6)                               # a plane where the pose goes
    with pytest.raises(G.FgoError, match="candidate 0"):
        gr.gate_plane_factors(x, [3, 12, 11], z, S6)                              # a pose where the plane goes
    with pytest.raises(G.FgoError, match="candidate 1"):
        gr.gate_plane_factors(x, [10, 13, 11], z, S6)                             # a point where the plane goes
    zz = z.copy(); zz[2, :3] = 0
    with pytest.raises(G.FgoError, match="candidate 2"):
        gr.gate_plane_factors(x, p, zz, S6)                                       # zero normal
    bad = S6.copy(); bad[1] = R.cov_ut(np.diag([1e-4, 1e-4, -1e-4]))
    with pytest.raises(G.FgoError, match="candidate 1"):
        gr.gate_plane_factors(x, p, z, bad)                                       # indefinite S
    # the codes themselves: FGO_ENUM -5, FGO_EINVAL -1, FGO_ESTATE -4
    assert G.lib.fgo_gate_plane_factors(gr._h, 3, G._i64p(x), G._i64p(p), G._dp(z), G._dp(bad), G._dp(np.zeros(3)), None, None, None, None) == -5
    assert G.lib.fgo_gate_plane_factors(gr._h, 3, G._i64p(x), G._i64p(np.array([10, 13, 11])), G._dp(z), G._dp(S6), G._dp(np.zeros(3)), None, None, None,
                                        None) == -1
    with pytest.raises(G.FgoError):
        gr.associate_planes(1, z, S6, [10, 11, 10])                               # a plane listed twice
    with pytest.raises(G.FgoError):
        gr.associate_planes(10, z, S6, [10, 11])                                  # not a pose
    with pytest.raises(G.FgoError):
        gr.associate_planes(1, z, S6, [10, 2])                                    # not a plane
    with pytest.raises(G.FgoError):
        gr.associate_planes(1, z, S6, [10, 999])                                  # unknown id
    with pytest.raises(G.FgoError):
        gr.associate_planes(1, zz, S6, [10, 11])                                  # zero normal
    # empty sizes
    assert gr.gate_plane_factors([], [], np.zeros((0, 4)), np.zeros((0, 6)))[0].shape == (0,)
    m0, b0 = gr.associate_planes(1, np.zeros((0, 4)), np.zeros((0, 6)), [10, 11])
    assert m0.shape == (0,) and b0.shape == (0, 2)
    m1, b1, D1 = gr.associate_planes(1, z, S6, [], want_matrix=True)
    assert np.all(m1 == -1) and np.all(np.isinf(b1)) and D1.shape == (3, 0)
    gr.gate_plane_factors(x, p, z, S6)                                            # the context is still good
    # a g2o-semantics context has no planes and refuses; so does distributed mode
    g2 = small_graph(np.random.default_rng(63), n=20, extra=5)
    gg = G.Graph(); gg.add_poses(g2["poses"], g2["fixed"]); gg.add_edges(g2["ei"], g2["ej"], g2["meas"], g2["info"])
    assert G.lib.fgo_gate_plane_factors(gg._h, 1, G._i64p(np.array([1])), G._i64p(np.array([2])), G._dp(z), G._dp(S6), G._dp(np.zeros(1)), None, None,
                                        None, None) == -1
    gs = mixed_gpu(g)
    gs.set_shard(0, 2, lambda ptr, n: 0)
    assert G.lib.fgo_gate_plane_factors(gs._h, 3, G._i64p(x), G._i64p(p), G._dp(z), G._dp(S6), G._dp(np.zeros(3)), None, None, None, None) == -4
    with pytest.raises(G.FgoError):
        gs.associate_planes(1, z, S6, [10, 11])
