"""Gating of candidate SE3 edges on the device (fgo_gate_edges_se3, fgo_edge_chi2_se3; kernels_gate.hip): the squared Mahalanobis
distance of a candidate's innovation under the map's covariance, against tests/gate_reference.py evaluated on numpy.linalg.inv of
the oracle's dense information matrix."""
import numpy as np
import pytest

import graph_slam_amd as G
from graph_slam_amd import scenarios as S
from tests import gate_reference as R
from tests import orc_binding as orc
from tests.util import info_full, info_ut, mixed_graph, mixed_oracle, pose_inv, pose_mul, random_info, small_graph

pytestmark = pytest.mark.gpu


def _g2o_gpu(g, **kw):
    gr = G.Graph(**kw)
    gr.add_poses(g["poses"], g["fixed"])
    gr.add_edges(g["ei"], g["ej"], g["meas"], g["info"])
    return gr


def _synth(n, seed):
    g = G.synth_manhattan3d(n, 5, 4, seed=seed)
    g["fixed"] = np.zeros(n, np.uint8); g["fixed"][0] = 1
    return g


def _dense_inverse(g):
    po = orc.Problem(g["poses"], g["fixed"], g["ei"].astype(np.int32), g["ej"].astype(np.int32), g["meas"], g["info"])
    return np.linalg.inv(po.dense_system()[0])


def _d2_from_P(e, P, W):
    return float(e @ np.linalg.solve(P + np.linalg.inv(W), e))


def _check(refs, info, d2, chi2, P, tol_sigma, label):
    """chi2 to 1e-12; P to tol_sigma x max|P| (the bound the marginal tests hold blocks of Sigma to); d2 against the full reference
    to tol_sigma x cond(P + W^-1), the first-order effect of that bound; d2 against e'(P_device + W^-1)^-1 e in numpy to 1e-9 (the
    kernel's own factorisation and solve: eps x cond, with margin)"""
    worst = dict(chi2=0.0, P=0.0, d2_over_cond=0.0, d2_own=0.0)
    for k, ref in enumerate(refs):
        W = info_full(info[k])
        worst["chi2"] = max(worst["chi2"], abs(chi2[k] - ref["chi2"]) / ref["chi2"])
        scale = np.abs(ref["P"]).max()
        if scale > 0:
            worst["P"] = max(worst["P"], np.abs(P[k] - ref["P"]).max() / scale)
        else:
            assert np.all(P[k] == 0)
        worst["d2_over_cond"] = max(worst["d2_over_cond"], abs(d2[k] - ref["d2"]) / ref["d2"] / ref["cond"])
        worst["d2_own"] = max(worst["d2_own"], abs(d2[k] - _d2_from_P(ref["e"], P[k], W)) / d2[k])
        assert 0 <= d2[k] <= chi2[k] * (1 + 1e-12), (k, d2[k], chi2[k])
    print("%s: largest errors chi2 %.1e, P / max|P| %.1e, d2 / cond %.1e (cond <= %.1e), d2 against its own P %.1e"
          % (label, worst["chi2"], worst["P"], worst["d2_over_cond"], max(r["cond"] for r in refs), worst["d2_own"]))
    assert worst["chi2"] <= 1e-12
    assert worst["P"] <= tol_sigma
    assert worst["d2_over_cond"] <= tol_sigma
    assert worst["d2_own"] <= 1e-9
    return worst


def test_small_g2o_graph_every_path():
    g = small_graph(np.random.default_rng(31), n=150, extra=12)             # vertex 0 fixed; unoptimised
    gr = _g2o_gpu(g)
    Sigma, pos = _dense_inverse(g), R.free_positions(g["fixed"])
    a, b, meas, info = R.candidates(np.random.default_rng(32), g["poses"], R.SMALL_PAIRS)
    d2, chi2, P = gr.gate_edges(a, b, meas, info, want_cov=True)
    st = gr.gate_stats()
    assert st["off_pattern"] >= 3 and st["column_groups"] >= 1, st
    _check(R.gate_many(Sigma, pos, g["poses"], a, b, meas, info), info, d2, chi2, P, 1e-8, "small g2o graph")
    d2b, chi2b = gr.gate_edges(a, b, meas, info)                              # without P: the same numbers
    assert np.array_equal(d2, d2b) and np.array_equal(chi2, chi2b)
    assert gr.gate_edges([], [], np.zeros((0, 7)), np.zeros((0, 21)))[0].shape == (0,)   # n = 0 is fine


def test_grouping_follows_the_side_with_fewer_columns():
    n = 2000
    g = _synth(n, 6)
    gr = _g2o_gpu(g)
    rng = np.random.default_rng(33)
    old = rng.choice(np.arange(1, 1500), 32, replace=False)
    new = np.full(32, n - 1)
    pairs = list(zip(old.tolist(), new.tolist()))
    a, b, meas, info = R.candidates(rng, g["poses"], pairs)
    meas_rev = np.array([pose_inv(z) for z in meas])
    # the reference from the blocks marginal_cov_pairs returns.  Those come by b's columns in either orientation, the gate's by
    # the newest pose's: two solve routes, each within the 1e-8 x max|Sigma| the marginal tests hold -> d2 to 1e-8 x cond(P + W^-1)
    Saa, Sbb, Sab = gr.marginal_cov_pairs(a, a), gr.marginal_cov_pairs(b, b), gr.marginal_cov_pairs(a, b)
    for (ia, ib, mz, fwd) in ((a, b, meas, True), (b, a, meas_rev, False)):
        d2, chi2, P = gr.gate_edges(ia, ib, mz, info, want_cov=True)
        st = gr.gate_stats()
        assert st["column_groups"] == 1 and st["off_pattern"] >= 1, st
        for k in range(32):
            e, Ja, Jb = orc.edge_se3(g["poses"][ia[k]], g["poses"][ib[k]], mz[k])
            W = info_full(info[k])
            Pr = R.predicted_cov(Ja, Jb, Saa[k], Sab[k], Sbb[k]) if fwd else R.predicted_cov(Ja, Jb, Sbb[k], Sab[k].T, Saa[k])
            np.testing.assert_allclose(P[k], Pr, rtol=0, atol=1e-8 * np.abs(Pr).max())
            assert abs(d2[k] - R.d2_direct(e, Pr, W)) <= 1e-8 * np.linalg.cond(Pr + np.linalg.inv(W)) * d2[k]
            assert abs(d2[k] - _d2_from_P(e, P[k], W)) <= 1e-9 * d2[k]
            assert abs(chi2[k] - e @ W @ e) <= 1e-12 * chi2[k]


def test_exact_measurement_gives_zero():
    g = small_graph(np.random.default_rng(31), n=150, extra=12)
    gr = _g2o_gpu(g)
    pairs = [(5, 6), (1, 149), (0, 149), (120, 0), (77, 141)]
    a = np.array([p[0] for p in pairs]); b = np.array([p[1] for p in pairs])
    meas = np.array([pose_mul(pose_inv(g["poses"][i]), g["poses"][j]) for i, j in pairs])
    info = np.array([info_ut(random_info(np.random.default_rng(34))) for _ in pairs])
    d2, chi2 = gr.gate_edges(a, b, meas, info)
    assert np.all(chi2 < 1e-20) and np.all(d2 < 1e-20) and np.all(d2 >= 0), (chi2, d2)


def test_gtsam_semantics_on_a_mixed_graph():
    from tests.test_gpu_factors import mixed_gpu
    g = mixed_graph(np.random.default_rng(22), n_poses=10, n_planes=3, n_points=14)
    gr = mixed_gpu(g)
    Sigma = np.linalg.inv(mixed_oracle(g).dense_system()[0])
    pos = list(range(len(g["values"])))                                       # nothing is fixed (pose 0 carries a prior)
    pairs = [(1, 7), (8, 2), (0, 5), (3, 4), (9, 0), (6, 1)]
    a, b, meas, info = R.candidates(np.random.default_rng(35), g["values"], pairs)
    d2, chi2, P = gr.gate_edges(a, b, meas, info, tangent_order=G.FGO_TANGENT_GTSAM, want_cov=True)
    refs = R.gate_many(Sigma, pos, g["values"], a, b, meas, info, gtsam=True)
    _check(refs, info, d2, chi2, P, 1e-7, "mixed GTSAM graph")              # (1e-7: the level this graph's marginal test holds)
    with pytest.raises(G.FgoError):
        gr.gate_edges([1], [g["n_poses"]], meas[:1], info[:1], tangent_order=G.FGO_TANGENT_GTSAM)     # a plane
    with pytest.raises(G.FgoError):
        gr.gate_edges(a, b, meas, info, tangent_order=G.FGO_TANGENT_G2O)


def test_bundle_adjustment_stays_in_the_eliminated_form(monkeypatch):
    p = S.ba_problem(300, 8000)
    monkeypatch.setenv("FGO_BA_SCHUR", "0")              # (read when the structure is built: each context is built under its setting)
    g0 = S.ba_graph(p)
    g0.chi2()
    monkeypatch.setenv("FGO_BA_SCHUR", "1")
    g1 = S.ba_graph(p)
    g1.chi2()
    nnz0, nnz1 = g0.stats().nnz_L_blocks, g1.stats().nnz_L_blocks
    assert nnz1 < nnz0 / 2, (nnz1, nnz0)
    pairs = [(1, 2), (5, 290), (250, 3), (120, 121), (299, 17), (40, 200)]
    a, b, meas, info = R.candidates(np.random.default_rng(36), g0.get_poses(300), pairs, 0.01, 0.005)
    info = info * 1e3                                    # (information of the order of the cameras' own: P matters in d2)
    r1 = g1.gate_edges(a, b, meas, info, tangent_order=G.FGO_TANGENT_GTSAM, want_cov=True)
    assert g1.stats().nnz_L_blocks == nnz1               # cameras only: the context still factors the reduced camera system
    r0 = g0.gate_edges(a, b, meas, info, tangent_order=G.FGO_TANGENT_GTSAM, want_cov=True)
    assert g0.stats().nnz_L_blocks == nnz0
    for k in range(len(pairs)):
        np.testing.assert_allclose(r1[2][k], r0[2][k], rtol=1e-6, atol=1e-9 * np.abs(r0[2][k]).max())
    np.testing.assert_allclose(r1[0], r0[0], rtol=1e-6)
    np.testing.assert_allclose(r1[1], r0[1], rtol=1e-12)


def test_edge_chi2_of_the_edges_in_the_graph():
    """The sum against chi2() to 1e-12 relative; each value against the oracle's to 1e-12 relative plus what the rounding of e
    itself allows.  small_graph chains its poses from the odometry measurements, so the n - 1 chain edges have a residual that is
    zero but for rounding (chi2 of the order of 1e-30) and no relative bound can hold for them; a loop closure's translation
    residual Rz'(Ri'(tj - ti) - tz) is what cancellation leaves of operands of size |tj - ti| and |tz|.  Two rotations by a unit
    quaternion and one subtraction are some 20 roundings per component, each of eps x (1 + |tj - ti| + |tz|) at the most (the 1
    for the quaternion part), so two implementations' e differ by de <= 64 eps (1 + |tj - ti| + |tz|) with margin, and
    e'We by ||W||_2 de (2 ||e|| + de)."""
    g = small_graph(np.random.default_rng(37), n=60, extra=25)
    gr = _g2o_gpu(g)
    c = gr.edge_chi2()
    assert len(c) == len(g["ei"])
    assert abs(c.sum() - gr.chi2()) <= 1e-12 * gr.chi2()
    eps, worst = np.finfo(np.float64).eps, 0.0
    for k in range(len(c)):
        xi, xj, z = g["poses"][g["ei"][k]], g["poses"][g["ej"][k]], g["meas"][k]
        e = orc.edge_se3(xi, xj, z, jac=False)
        W = info_full(g["info"][k])
        ref = e @ W @ e
        de = 64 * eps * (1 + np.linalg.norm(xj[:3] - xi[:3]) + np.linalg.norm(z[:3]))
        tol = 1e-12 * ref + np.linalg.norm(W, 2) * de * (2 * np.linalg.norm(e) + de)
        worst = max(worst, abs(c[k] - ref) / tol)
        assert abs(c[k] - ref) <= tol, (k, c[k], ref, tol)
    print("edge_chi2: largest |difference| / bound %.2e" % worst)
    loops = slice(len(g["poses"]) - 1, None)                                   # the loop closures carry nearly all of chi2
    assert c[loops].sum() > 0.999 * c.sum() and np.all(c[loops] > 1e-6)
    assert np.array_equal(gr.edge_chi2(7, 20), c[7:27])
    assert len(gr.edge_chi2(len(c), 0)) == 0
    with pytest.raises(G.FgoError):
        gr.edge_chi2(len(c) - 3, 4)
    gr.optimize(2)
    assert abs(gr.edge_chi2().sum() - gr.chi2()) <= 1e-12 * gr.chi2()       # follows the estimate


def test_state_and_determinism():
    n = 1200
    g = _synth(n, 5)
    rng = np.random.default_rng(38)
    pairs = [(5, 6), (6, 700), (1, 1100), (0, 1199), (900, 0), (1199, 3), (400, 401)]
    a, b, meas, info = R.candidates(rng, g["poses"], pairs)

    def gate(gr):
        return gr.gate_edges(a, b, meas, info, want_cov=True)
    gr1, gr2 = _g2o_gpu(g), _g2o_gpu(g)
    o1, o2 = gate(gr1), gate(gr2)
    for x, y, z in zip(o1, o2, gate(gr1)):
        assert np.array_equal(x, y) and np.array_equal(x, z)                  # bit-equal across contexts and on repeat
    gr1.optimize(1)
    assert not np.array_equal(gate(gr1)[0], o1[0])
    # a gate call between the build and the optimisation leaves no trace in it
    ga, gb = _g2o_gpu(g), _g2o_gpu(g)
    ga.chi2(); gb.chi2()
    gate(gb)
    ga.optimize(2); gb.optimize(2)
    assert np.array_equal(ga.get_poses(), gb.get_poses())
    for x, y in zip(ga.trace(), gb.trace()):
        assert np.array_equal(x, y)
    grg = G.Graph()
    grg.set_growth(40, 16)                               # growth reserve: another elimination order, phantom slots are not variables
    grg.add_poses(g["poses"], g["fixed"])
    grg.add_edges(g["ei"], g["ej"], g["meas"], g["info"])
    og = gate(grg)
    for k in range(len(pairs)):
        W = info_full(info[k])
        np.testing.assert_allclose(og[2][k], o1[2][k], rtol=0, atol=1e-8 * np.abs(o1[2][k]).max())
        assert abs(og[0][k] - o1[0][k]) <= 1e-8 * np.linalg.cond(o1[2][k] + np.linalg.inv(W)) * o1[0][k]
        assert abs(og[1][k] - o1[1][k]) <= 1e-12 * o1[1][k]


def test_errors():
    g = small_graph(np.random.default_rng(39), n=30, extra=10)
    gr = _g2o_gpu(g)
    a, b, meas, info = R.candidates(np.random.default_rng(40), g["poses"], [(3, 9), (4, 20), (7, 2)])
    gr.gate_edges(a, b, meas, info)
    with pytest.raises(G.FgoError, match="candidate 1"):
        gr.gate_edges([3, 1000, 7], b, meas, info)                            # unknown id
    with pytest.raises(G.FgoError, match="candidate 2"):
        gr.gate_edges(a, [9, 20, 7], meas, info)                              # a == b
    bad = info.copy(); bad[1] = info_ut(np.diag([1.0, 1, 1, 1, 1, -1]))
    with pytest.raises(G.FgoError, match="candidate 1"):
        gr.gate_edges(a, b, meas, bad)                                        # indefinite information
    with pytest.raises(G.FgoError):
        gr.gate_edges(a, b, meas, info, tangent_order=G.FGO_TANGENT_GTSAM)
    gr.gate_edges(a, b, meas, info)                                           # the context is still good
    gs = _g2o_gpu(small_graph(np.random.default_rng(26), n=30, extra=10))
    gs.set_shard(0, 2, lambda ptr, n: 0)
    with pytest.raises(G.FgoError):
        gs.gate_edges(a, b, meas, info)
