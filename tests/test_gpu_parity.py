"""GPU parity tests: the HIP path, called through the C-ABI (libfgo.so), against the CPU oracle on the
same seeded inputs.  Floating point (f64): tolerances are stated per test; BASELINE.json's north star asks
for final chi2 within 1e-6 relative and these tests hold it to much tighter bounds where the maths allows.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import graph_slam_amd as G
from tests import orc_binding as orc
from tests.util import small_graph, pose_mul, pose_inv, random_pose, info_ut, random_info


def make_gpu(g, **kw):
    gr = G.Graph(**kw)
    gr.add_poses(g["poses"], g["fixed"])
    gr.add_edges(g["ei"], g["ej"], g["meas"], g["info"])
    return gr


def make_orc(g):
    return orc.Problem(g["poses"], g["fixed"], g["ei"], g["ej"], g["meas"], g["info"])


def synth(n, lookback, n_loop, seed=42):
    g = G.synth_manhattan3d(n, lookback, n_loop, seed)
    g["fixed"] = np.zeros(n, np.uint8); g["fixed"][0] = 1    # CGraphG2O::firstNode: vertex 0 fixed
    return g


def test_library_loaded_is_in_tree():
    import os
    assert os.path.samefile(G.LIB_PATH, os.path.join(os.path.dirname(G.__file__), "libfgo.so"))
    assert G.lib.fgo_device_count() >= 1


@pytest.mark.parametrize("seed,n,extra", [(0, 5, 3), (1, 30, 40), (2, 200, 400)])
def test_linearize_matches_oracle(seed, n, extra):
    """H, b (dense read-back) and chi2: tolerance 1e-11 relative to the largest entry."""
    rng = np.random.default_rng(seed)
    g = small_graph(rng, n=n, extra=extra)
    gr = make_gpu(g)
    chi, H, b = gr.linearize()
    Ho, bo = make_orc(g).dense_system()
    chio = make_orc(g).chi2()
    assert abs(chi - chio) <= 1e-12 * chio
    np.testing.assert_allclose(H, Ho, rtol=0, atol=1e-11 * np.abs(Ho).max())
    np.testing.assert_allclose(b, bo, rtol=0, atol=1e-11 * np.abs(bo).max())
    assert abs(gr.chi2() - chio) <= 1e-12 * chio


@pytest.mark.parametrize("seed,n,extra", [(3, 6, 4), (4, 60, 90), (5, 400, 700)])
def test_damped_solve_matches_dense_numpy(seed, n, extra):
    """(H + lambda I) d = b: block Cholesky + triangular solves vs numpy.linalg.solve, 1e-9 relative."""
    rng = np.random.default_rng(seed)
    g = small_graph(rng, n=n, extra=extra)
    gr = make_gpu(g)
    Ho, bo = make_orc(g).dense_system()
    lam = 1e-5 * np.abs(np.diag(Ho)).max()
    d = gr.solve_step(lam)
    ref = np.linalg.solve(Ho + lam * np.eye(len(bo)), bo)
    np.testing.assert_allclose(d, ref, rtol=0, atol=1e-9 * np.abs(ref).max())
    rc, do = make_orc(g).solve_step(lam)
    np.testing.assert_allclose(d, do, rtol=0, atol=1e-9 * np.abs(ref).max())


def test_duplicate_and_reversed_edges():
    """the same vertex pair measured twice and once in the opposite direction (shared H block)"""
    rng = np.random.default_rng(11)
    g = small_graph(rng, n=12, extra=10)
    ei, ej = list(g["ei"]), list(g["ej"])
    meas, info = list(g["meas"]), list(g["info"])
    for a, b in [(2, 5), (5, 2), (2, 5), (0, 3), (3, 0)]:
        z = pose_mul(pose_inv(g["poses"][a]), g["poses"][b])
        ei.append(a); ej.append(b); meas.append(z); info.append(info_ut(random_info(rng)))
    g2 = dict(g, ei=np.array(ei, np.int32), ej=np.array(ej, np.int32), meas=np.array(meas), info=np.array(info))
    gr = make_gpu(g2)
    chi, H, b = gr.linearize()
    Ho, bo = make_orc(g2).dense_system()
    np.testing.assert_allclose(H, Ho, rtol=0, atol=1e-11 * np.abs(Ho).max())
    np.testing.assert_allclose(b, bo, rtol=0, atol=1e-11 * np.abs(bo).max())


def test_fixed_vertices_anywhere():
    rng = np.random.default_rng(12)
    g = small_graph(rng, n=25, extra=30)
    g["fixed"][:] = 0
    g["fixed"][[7, 19]] = 1
    gr, po = make_gpu(g), make_orc(g)
    chi, H, b = gr.linearize()
    Ho, bo = po.dense_system()
    np.testing.assert_allclose(H, Ho, rtol=0, atol=1e-11 * np.abs(Ho).max())
    rc, st = gr.optimize(3)
    po.optimize(3)
    out = gr.get_poses()
    np.testing.assert_array_equal(out[[7, 19]], g["poses"][[7, 19]])
    np.testing.assert_allclose(out, po.get_poses(), atol=1e-8)


def _run_schedule(obj, calls=10, iters=2):
    """CGraphG2O::optimizeGraph: 10 x optimize(2) (g2o/g2o_graph.cpp:244-250)"""
    chis, lams, total = [], [], 0
    for _ in range(calls):
        rc, st = obj.optimize(iters)
        assert rc >= 1
        total += rc
        c, l = obj.trace()
        chis += list(c); lams += list(l)
    return np.array(chis), np.array(lams), total


def test_config1_manhattan_1k_full_schedule():
    """BASELINE config 1: 1k poses / ~5k edges, the reference's 20-iteration schedule.
    chi2 trajectory within 1e-9 relative per iteration, lambda within 1e-7, poses within 1e-7."""
    g = synth(1000, 4, 0)
    gr, po = make_gpu(g), make_orc(g)
    c0 = gr.chi2()
    assert abs(c0 - po.chi2()) <= 1e-12 * po.chi2()
    cg, lg, tg = _run_schedule(gr)
    co, lo, to = _run_schedule(po)
    assert tg == to == 20
    np.testing.assert_allclose(cg, co, rtol=1e-9)
    np.testing.assert_allclose(lg, lo, rtol=1e-7)
    assert abs(gr.chi2() - po.chi2()) <= 1e-9 * po.chi2()
    P, Q = gr.get_poses(), po.get_poses()
    sgn = np.sign(np.sum(P[:, 3:] * Q[:, 3:], axis=1))[:, None]     # q and -q are the same rotation
    assert np.abs(P[:, :3] - Q[:, :3]).max() < 1e-7
    assert np.abs(P[:, 3:] * sgn - Q[:, 3:]).max() < 1e-7
    assert cg[-1] < 0.3 * c0


def test_manhattan_10k_with_loop_closures():
    """10k poses / 100k edges with loop closures: 3 x optimize(2); final chi2 within 1e-8 relative
    (north star: 1e-6)."""
    g = synth(10000, 5, 4)
    gr, po = make_gpu(g), make_orc(g)
    cg, lg, _ = _run_schedule(gr, calls=3)
    co, lo, _ = _run_schedule(po, calls=3)
    np.testing.assert_allclose(cg, co, rtol=1e-8)
    assert abs(gr.chi2() - po.chi2()) <= 1e-8 * po.chi2()


def test_second_lap_graph_large_separators():
    """A second lap along the same corridor: every 10th pose also sees the pose 1 500 key frames earlier, so loop closures span every
    index cut of the time dissection (csrc/ordering_cuts.cpp split_by_index) and the top separators are an order of magnitude larger than
    the look-back band (tools/symstats FGO_LAPS: 5 x the fill of the plain graph) -- wide row structures, long update lists and hub-like
    targets on a pose graph.  3 x optimize(2) against the oracle: chi2 trajectory 1e-8, lambda 1e-6, final chi2 1e-8."""
    g = synth(6000, 5, 0, seed=5)
    i = np.arange(1500, 6000, 10)
    j = i - 1500
    rng = np.random.default_rng(2)
    meas = np.array([pose_mul(pose_mul(pose_inv(g["truth"][a]), g["truth"][b]), random_pose(rng, 0.01)) for a, b in zip(j, i)])
    g["ei"] = np.concatenate([g["ei"], j]); g["ej"] = np.concatenate([g["ej"], i])
    g["meas"] = np.concatenate([g["meas"], meas]); g["info"] = np.concatenate([g["info"], np.tile(g["info"][0], (len(i), 1))])
    gr, po = make_gpu(g), make_orc(g)
    assert abs(gr.chi2() - po.chi2()) <= 1e-12 * po.chi2()
    cg, lg, _ = _run_schedule(gr, calls=3)
    co, lo, _ = _run_schedule(po, calls=3)
    np.testing.assert_allclose(cg, co, rtol=1e-8)
    np.testing.assert_allclose(lg, lo, rtol=1e-6)
    assert abs(gr.chi2() - po.chi2()) <= 1e-8 * po.chi2()
    st = gr.stats()
    assert st.nnz_L_blocks > 3 * st.nnz_H_blocks            # (the plain 6 000-pose graph: 2.0 x)


def test_rejected_trial_keeps_state():
    """A graph started far from the optimum forces rejected trials (lambda *= nu); the device must roll
    back exactly like g2o's pop()."""
    rng = np.random.default_rng(21)
    g = small_graph(rng, n=40, extra=60, noise=0.02)
    g["poses"][1:, :3] += rng.normal(size=(39, 3)) * 3.0           # scramble the initial guess
    for v in range(1, 40):
        g["poses"][v, 3:] = random_pose(rng)[3:]
    gr, po = make_gpu(g), make_orc(g)
    tr_g = tr_o = 0
    for _ in range(6):
        rg, sg = gr.optimize(3); ro, so = po.optimize(3)
        tr_g += sg.trials; tr_o += so.trials
        assert rg == ro
        assert abs(sg.chi2_final - so.chi2_final) <= 1e-7 * max(1.0, so.chi2_final)
    assert tr_g == tr_o
    assert tr_g > 18        # at least one rejected trial happened


def test_determinism_bitwise():
    g = synth(3000, 5, 4, seed=7)
    outs = []
    for _ in range(2):
        gr = make_gpu(g)
        gr.optimize(4)
        outs.append((gr.get_poses().copy(), gr.chi2()))
    assert outs[0][1] == outs[1][1]
    np.testing.assert_array_equal(outs[0][0], outs[1][0])


def test_graph_mode_equals_eager(monkeypatch):
    g = synth(2000, 5, 4, seed=9)
    res = []
    for mode in ("1", "0"):
        monkeypatch.setenv("FGO_GRAPH", mode)
        gr = make_gpu(g)
        gr.optimize(3)
        res.append(gr.get_poses().copy())
    np.testing.assert_array_equal(res[0], res[1])


def test_incremental_add_rebuilds_structure():
    """optimise, add more vertices/edges (as the online driver does between optimizeGraph calls), optimise again"""
    g = synth(600, 4, 0, seed=3)
    half = 300
    keep = g["ej"] < half
    gr = G.Graph()
    gr.add_poses(g["poses"][:half], g["fixed"][:half])
    gr.add_edges(g["ei"][keep], g["ej"][keep], g["meas"][keep], g["info"][keep])
    gr.optimize(2)
    first = gr.get_poses()
    # new vertices initialised by chaining from the optimised estimate (g2o_graph.cpp:118)
    poses = list(first)
    odo = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(g["ei"], g["ej"]))}
    for v in range(half, 600):
        poses.append(pose_mul(poses[v - 1], g["meas"][odo[(v - 1, v)]]))
    gr.add_poses(np.array(poses[half:]), np.zeros(600 - half, np.uint8), ids=np.arange(half, 600))
    gr.add_edges(g["ei"][~keep], g["ej"][~keep], g["meas"][~keep], g["info"][~keep])
    rc, st = gr.optimize(2)
    assert st.structure_rebuilt == 1
    po = orc.Problem(np.array(poses), g["fixed"], np.concatenate([g["ei"][keep], g["ei"][~keep]]).astype(np.int32),
                     np.concatenate([g["ej"][keep], g["ej"][~keep]]).astype(np.int32),
                     np.concatenate([g["meas"][keep], g["meas"][~keep]]), np.concatenate([g["info"][keep], g["info"][~keep]]))
    po.optimize(2)
    assert abs(gr.chi2() - po.chi2()) <= 1e-9 * po.chi2()


def test_error_conventions():
    gr = G.Graph()
    with pytest.raises(G.FgoError):
        gr.add_edges([0], [1], np.array([[0, 0, 0, 0, 0, 0, 1.0]]), np.zeros((1, 21)))   # unknown ids
    gr.add_poses(np.array([[0, 0, 0, 0, 0, 0, 1.0]]), np.array([1], np.uint8))
    assert gr.chi2() == 0.0
    st = G.FgoStats()
    import ctypes as C
    assert G.lib.fgo_optimize(gr._h, 2, C.byref(st)) == -4      # FGO_ESTATE: g2o's optimize() == -1
    with pytest.raises(G.FgoError):
        gr.add_poses(np.array([[0, 0, 0, 0, 0, 0, 1.0]]), ids=np.array([0]))             # duplicate id
    with pytest.raises(G.FgoError):
        gr.set_pose(99, np.array([0, 0, 0, 0, 0, 0, 1.0]))


def test_set_get_pose_roundtrip():
    g = synth(100, 4, 0)
    gr = make_gpu(g)
    gr.optimize(1)
    p = gr.get_poses()
    newp = random_pose(np.random.default_rng(0))
    gr.set_pose(17, newp)
    q = gr.get_poses()
    np.testing.assert_allclose(q[17], newp, atol=1e-15)
    np.testing.assert_array_equal(np.delete(q, 17, 0), np.delete(p, 17, 0))
    po = orc.Problem(q, g["fixed"], g["ei"].astype(np.int32), g["ej"].astype(np.int32), g["meas"], g["info"])
    assert abs(gr.chi2() - po.chi2()) <= 1e-12 * po.chi2()


@pytest.mark.parametrize("n,lookback,n_loop", [(100000, 5, 4)])
def test_full_size_properties(n, lookback, n_loop):
    """BASELINE config 2 (100k poses / 1M edges), size-independent properties:
    chi2 from the fused linearise pass == chi2 from the stand-alone kernel; accepted iterations decrease
    chi2; the damped step solves the normal equations (residual check through a second linearisation);
    the initial chi2 equals the oracle's (one pass over the edges is cheap on the CPU)."""
    g = synth(n, lookback, n_loop)
    gr = make_gpu(g)
    po = make_orc(g)
    c0 = gr.chi2()
    assert abs(c0 - po.chi2()) <= 1e-11 * po.chi2()
    rc, st = gr.optimize(2)
    assert rc == 2 and st.n_edges == len(g["ei"]) and st.n_free == n - 1
    c, l = gr.trace()
    assert c[0] < c0 and c[1] < c[0]
    c_fused = st.chi2_final
    po.set_poses(gr.get_poses())
    assert abs(c_fused - po.chi2()) <= 1e-10 * po.chi2()
    # Newton-step property: with lambda large the step is ~ b / lambda  (checks factor+solve at full size)
    chi, _, _ = gr.linearize(dense=False)
    lam = 1e12
    d = gr.solve_step(lam)
    assert np.isfinite(d).all() and np.abs(d).max() < 1.0


def rot_angle_between(qa, qb):
    """rotation angle (rad) of qa^-1 qb, quaternions x y z w"""
    d = np.abs(np.sum(qa * qb, axis=1)).clip(0, 1)
    return 2 * np.arccos(d)


def test_config2_full_schedule_vs_oracle():
    """BASELINE config 2 (100k poses / 999 944 edges) through the reference's WHOLE schedule -- CGraphG2O::optimizeGraph =
    10 x optimize(2) (g2o/g2o_graph.cpp:241-252) -- HIP path vs the CPU oracle, same graph, same start.
    Per optimize() call: iterations done equal, chi2 1e-8 relative.  After the 20 iterations: final chi2 1e-8 relative
    (north star: 1e-6), poses |dt|_inf <= 1e-6 m and rotation-angle inf-norm <= 1e-6 rad (SURVEY §8d asks for both; they
    are reported).  The oracle needs about a minute for this (single thread, simplicial LL^T)."""
    g = synth(100000, 5, 4)
    gr, po = make_gpu(g), make_orc(g)
    trials_g = trials_o = 0
    for call in range(10):
        rg, sg = gr.optimize(2)
        ro, so = po.optimize(2)
        assert rg == ro == 2, (call, rg, ro)
        trials_g += sg.trials; trials_o += so.trials
        assert abs(sg.chi2_final - so.chi2_final) <= 1e-8 * so.chi2_final, (call, sg.chi2_final, so.chi2_final)
    assert trials_g == trials_o
    pg, pq = gr.get_poses(), po.get_poses()
    dt = np.abs(pg[:, :3] - pq[:, :3]).max()
    da = rot_angle_between(pg[:, 3:], pq[:, 3:]).max()
    rel = abs(gr.chi2() - po.chi2()) / po.chi2()
    print("cfg2 20 iterations: final chi2 %.9e (oracle %.9e, rel %.2e), |dt|_inf %.3e m, rot-angle inf %.3e rad, trials %d"
          % (gr.chi2(), po.chi2(), rel, dt, da, trials_g))
    assert rel <= 1e-8
    assert dt <= 1e-6 and da <= 1e-6


def test_config5_size_single_gpu():
    """BASELINE config 5's graph (1M poses / 10M edges, generator seed 45) on ONE MI355X (it fits: about 20 GB of the
    288 GB).  Size-independent properties, as test_full_size_properties does for config 2: chi2 of the start equals the
    oracle's (one edge pass is cheap on the CPU) to 1e-11; two LM iterations are accepted and decrease chi2; the chi2
    the fused linearisation reports equals the oracle's chi2 at the GPU's poses to 1e-10; a heavily damped step is
    finite and small (factor + solves at full size)."""
    n = 1000000
    g = synth(n, 5, 4, seed=45)
    assert 9.9e6 < len(g["ei"]) < 10.1e6
    gr, po = make_gpu(g), make_orc(g)
    c0 = gr.chi2()
    assert abs(c0 - po.chi2()) <= 1e-11 * po.chi2()
    rc, st = gr.optimize(2)
    assert rc == 2 and st.n_edges == len(g["ei"]) and st.n_free == n - 1
    c, l = gr.trace()
    assert c[0] < c0 and c[1] < c[0]
    po.set_poses(gr.get_poses())
    assert abs(st.chi2_final - po.chi2()) <= 1e-10 * po.chi2()
    d = gr.solve_step(1e12)
    assert np.isfinite(d).all() and np.abs(d).max() < 1.0
    print("cfg5 on one GPU: chi2 %.6e -> %.6e, nnz(L) %d blocks, %d levels" % (c0, st.chi2_final, st.nnz_L_blocks, st.n_levels))


def test_ordering_candidates_pick_by_predicted_cost_and_change_nothing_but_speed():
    """fgo_config.order_candidates = 4: four orderings (balance weight / leaf size variants) are built and the one with the
    lowest predicted sweep time is kept.  The ordering changes fill and schedule only, never the solution: the LM run of the
    reference's schedule equals the oracle's exactly as with one candidate, and the kept structure is predicted no slower."""
    g = synth(3000, 5, 4, seed=11)
    po = make_orc(g)

    def run(n_cand):
        gr = G.Graph(order_candidates=n_cand)
        gr.add_poses(g["poses"], g["fixed"])
        gr.add_edges(g["ei"], g["ej"], g["meas"], g["info"])
        tr = []
        for _ in range(3):
            rc, st = gr.optimize(2)
            tr += list(gr.trace()[0])
        return np.array(tr), gr.get_poses(), gr.stats()
    t1, x1, s1 = run(1)
    t4, x4, s4 = run(4)
    to = []
    for _ in range(3):
        po.optimize(2); to += list(po.trace()[0])
    np.testing.assert_allclose(t1, to, rtol=1e-9)
    np.testing.assert_allclose(t4, to, rtol=1e-9)
    assert np.abs(x4[:, :3] - x1[:, :3]).max() < 1e-8
    cost = lambda s: 76.0 * s.n_levels + 0.051e-3 * s.n_update_ops
    assert cost(s4) <= cost(s1) * (1 + 1e-12)
