"""Marginal covariances of every variable and of variable pairs by selected inversion of the resident undamped factor
(fgo_marginal_cov_all / fgo_marginal_cov_pairs; g2o SparseOptimizer::computeMarginals, GTSAM Marginals and
jointMarginalCovariance) against numpy.linalg.inv of the dense information matrix and against fgo_marginal_cov."""
import ctypes as C
import re

import numpy as np
import pytest

import graph_slam_amd as G
from graph_slam_amd import scenarios as S
from tests import orc_binding as orc
from tests.util import small_graph, mixed_graph, mixed_oracle, vio_graph

pytestmark = pytest.mark.gpu


def _close(a, b, tol):
    np.testing.assert_allclose(a, b, rtol=0, atol=tol * np.abs(b).max())


def _g2o_gpu(g, **kw):
    gr = G.Graph(**kw)
    gr.add_poses(g["poses"], g["fixed"])
    gr.add_edges(g["ei"], g["ej"], g["meas"], g["info"])
    return gr


def _dense_inverse(g):
    po = orc.Problem(g["poses"], g["fixed"], g["ei"].astype(np.int32), g["ej"].astype(np.int32), g["meas"], g["info"])
    return np.linalg.inv(po.dense_system()[0])


def _check_against_inverse(gr, Hinv, free_ids, pairs, tol=1e-8):
    """every block of marginal_cov_all and the given pairs against the dense inverse (free-variable order = free_ids)"""
    pos = {int(v): k for k, v in enumerate(free_ids)}
    ids, cov = gr.marginal_cov_all()
    np.testing.assert_array_equal(ids, free_ids)
    for k, v in enumerate(ids):
        r = 6 * pos[int(v)]
        _close(cov[k], Hinv[r:r + 6, r:r + 6], tol)
    a = np.array([p[0] for p in pairs], np.int64); b = np.array([p[1] for p in pairs], np.int64)
    cp = gr.marginal_cov_pairs(a, b)
    for k in range(len(a)):
        ra, rb = 6 * pos[int(a[k])], 6 * pos[int(b[k])]
        _close(cp[k], Hinv[ra:ra + 6, rb:rb + 6], tol)
    return ids, cov


def _edge_pairs(ei, ej, free):
    out = []
    for i, j in zip(ei, ej):
        if int(i) in free and int(j) in free:
            out.append((int(i), int(j)))
            out.append((int(j), int(i)))
    return out


def test_small_g2o_graph_all_blocks_and_pairs():
    g = small_graph(np.random.default_rng(21), n=150, extra=12)            # vertex 0 fixed; a long chain: far pairs are off the pattern
    gr = _g2o_gpu(g)
    Hinv = _dense_inverse(g)
    free_ids = np.arange(1, 150)
    pairs = _edge_pairs(g["ei"], g["ej"], set(free_ids.tolist()))
    far = [(1, 149), (149, 2), (10, 120), (75, 3), (40, 40), (77, 141)]     # far apart: the column-solve fallback
    _check_against_inverse(gr, Hinv, free_ids, pairs + far)
    assert gr.selinv_stats()["fallback_pairs"] >= 3                           # some of them really were off the pattern of L
    assert len(pairs) > 0
    gr.marginal_cov_pairs([p[0] for p in pairs], [p[1] for p in pairs])
    assert gr.selinv_stats()["fallback_pairs"] == 0                           # pairs that share a factor never are
    J = gr.joint_marginal_cov([3, 90, 17])
    sel = np.concatenate([np.arange(6 * (v - 1), 6 * v) for v in (3, 90, 17)])
    _close(J, Hinv[np.ix_(sel, sel)], 1e-8)


def test_whole_schedule_leaf_and_panel_levels(capfd):
    n = 1800
    g = G.synth_manhattan3d(n, 2, 2, seed=3)             # (lookback 2: the bottom tasks are sub-trees, not paths -> a leaf level)
    g["fixed"] = np.zeros(n, np.uint8); g["fixed"][0] = 1
    gr = _g2o_gpu(g, verbose=1)
    capfd.readouterr()
    free_ids = np.arange(1, n)
    Hinv = _dense_inverse(g)
    pairs = _edge_pairs(g["ei"], g["ej"], set(free_ids.tolist()))
    _check_against_inverse(gr, Hinv, free_ids, pairs)
    err = capfd.readouterr().err
    m = re.search(r"selected inversion: prep .* levels (\d+) \(leaf (\d+), panel (\d+)\), widest (\d+) tasks", err)
    assert m, err
    n_levels, n_leaf, n_panel, widest = (int(x) for x in m.groups())
    assert n_leaf >= 1 and n_panel >= 1 and widest >= 4, m.group(0)      # the sweep ran through both kinds of level, several tasks wide


def _check_gtsam_graph(gr, po, n_vars, tol=1e-7):
    Hinv = np.linalg.inv(po.dense_system()[0])
    ids, cov = gr.marginal_cov_all()
    np.testing.assert_array_equal(ids, np.arange(n_vars))
    for v in range(n_vars):
        _close(cov[v], Hinv[6 * v:6 * v + 6, 6 * v:6 * v + 6], tol)
        _close(cov[v], gr.marginal_cov(v), 1e-9)
    return Hinv


def test_mixed_and_gtsam_semantics():
    from tests.test_gpu_factors import mixed_gpu
    from tests.test_gpu_imu import vio_gpu
    g = mixed_graph(np.random.default_rng(22), n_poses=10, n_planes=3, n_points=14)
    gr = mixed_gpu(g)
    Hinv = _check_gtsam_graph(gr, mixed_oracle(g), len(g["values"]))
    pairs = [(int(i), int(j)) for i, j in zip(g["ei"], g["ej"])]
    cp = gr.marginal_cov_pairs([p[0] for p in pairs], [p[1] for p in pairs])
    for k, (i, j) in enumerate(pairs):
        _close(cp[k], Hinv[6 * i:6 * i + 6, 6 * j:6 * j + 6], 1e-7)
    gv = vio_graph(np.random.default_rng(23), n_kf=8, with_planes=True)     # Vec3 / bias variables: 3-dof padding
    grv = vio_gpu(gv)
    Hv = _check_gtsam_graph(grv, mixed_oracle(gv), len(gv["values"]), 1e-6)   # (X0's prior: sigma 1e-7)
    K = gv["n_kf"]
    a = [0, 1, K + 2, 2 * K + 3, 5]; b = [K, 2 * K + 1, 2, 3 * K - 1, 2 * K + 5]
    cp = grv.marginal_cov_pairs(a, b)
    for k in range(len(a)):
        _close(cp[k], Hv[6 * a[k]:6 * a[k] + 6, 6 * b[k]:6 * b[k] + 6], 1e-6)


def test_bundle_adjustment_cameras_from_the_reduced_factor(monkeypatch):
    p = S.ba_problem(300, 8000)
    monkeypatch.setenv("FGO_BA_SCHUR", "0")              # (read when the structure is built: each context is built under its setting)
    g0 = S.ba_graph(p)
    g0.chi2()
    monkeypatch.setenv("FGO_BA_SCHUR", "1")
    g1 = S.ba_graph(p)
    g1.chi2()
    nnz0, nnz1 = g0.stats().nnz_L_blocks, g1.stats().nnz_L_blocks
    assert nnz1 < nnz0 / 2, (nnz1, nnz0)                 # g1 factors the reduced camera system, g0 the whole one
    a = np.concatenate([np.arange(1, 299), [5, 17, 250, 120]])
    b = np.concatenate([np.arange(2, 300), [5, 290, 3, 121]])
    c1 = g1.marginal_cov_pairs(a, b)                     # cameras only: the BA context stays in the eliminated form
    assert g1.stats().nnz_L_blocks == nnz1               # ... and still did for the pairs
    c0 = g0.marginal_cov_pairs(a, b)
    assert g0.stats().nnz_L_blocks == nnz0
    for k in range(len(a)):
        np.testing.assert_allclose(c1[k], c0[k], rtol=1e-6, atol=1e-9 * np.abs(c0[k]).max())
    np.testing.assert_allclose(c1[-4], g0.marginal_cov(5), rtol=1e-6, atol=1e-9 * np.abs(c1[-4]).max())   # (5, 5): the marginal
    ids1, all1 = g1.marginal_cov_all()                   # landmarks included: the generic form
    ids0, all0 = g0.marginal_cov_all()
    np.testing.assert_array_equal(ids1, ids0)
    assert 300 + 17 in ids0 and len(ids0) > 8000
    for k in range(len(ids0)):
        np.testing.assert_allclose(all1[k], all0[k], rtol=1e-6, atol=1e-9 * np.abs(all0[k]).max())
    _close(all0[list(ids0).index(300 + 17)], g0.marginal_cov(300 + 17), 1e-9)


def test_full_size_cfg2_against_column_solves():
    n = 100000
    g = G.synth_manhattan3d(n, 5, 4, seed=42)
    g["fixed"] = np.zeros(n, np.uint8); g["fixed"][0] = 1
    gr = _g2o_gpu(g)
    ids, cov = gr.marginal_cov_all()
    np.testing.assert_array_equal(ids, np.arange(1, n))
    assert np.all(np.diagonal(cov, axis1=1, axis2=2) > 0)
    rng = np.random.default_rng(24)
    pick = np.unique(np.concatenate([rng.choice(np.arange(1, n), 60, replace=False), [1, n // 2, n - 2, n - 1]]))
    many = gr.marginal_cov_many(pick)
    for k, v in enumerate(pick):
        np.testing.assert_allclose(cov[v - 1], many[k], rtol=1e-7, atol=1e-7 * np.abs(many[k]).max())


def test_cache_determinism_refresh_and_growth():
    n = 1200
    g = G.synth_manhattan3d(n, 5, 4, seed=5)
    g["fixed"] = np.zeros(n, np.uint8); g["fixed"][0] = 1
    gr1, gr2 = _g2o_gpu(g), _g2o_gpu(g)
    ids1, a1 = gr1.marginal_cov_all()
    ids2, a2 = gr2.marginal_cov_all()
    assert np.array_equal(ids1, ids2) and np.array_equal(a1, a2)           # bit-equal across contexts
    _, a1b = gr1.marginal_cov_all()
    assert np.array_equal(a1, a1b)                                          # and on repeat
    pc = gr1.marginal_cov_pairs([5, 6], [6, 700])
    assert np.array_equal(pc, gr2.marginal_cov_pairs([5, 6], [6, 700]))

    def requests():
        return gr1.marginal_cov_all()[1], gr1.marginal_cov_many([29, 1, 7, 7, 700]), gr1.marginal_cov_pairs([5, 6, 1], [6, 700, 1100])
    before = requests()
    assert np.array_equal(before[1][2], before[1][3])                         # a repeated id
    delta = np.zeros(6 * n)
    # calls that write the resident factor (a damped one) or the linearisation at the same estimate: the next requests
    # factor again and give the same bits
    for call in (lambda: gr1._chk(G.lib.fgo_solve_step(gr1._h, 1e-3, delta.ctypes.data_as(C.POINTER(C.c_double)))),
                 lambda: gr1.bench_phase(1, 1), lambda: gr1.linearize(dense=False)):
        call()
        for a, b in zip(before, requests()):
            assert np.array_equal(a, b)
    gr1.optimize(1)
    _, a3 = gr1.marginal_cov_all()
    assert not np.array_equal(a3, a1)
    g3 = dict(g); g3["poses"] = gr1.get_poses()
    _, a4 = _g2o_gpu(g3).marginal_cov_all()
    for k in range(len(a3)):
        _close(a3[k], a4[k], 1e-9)
    grg = G.Graph()
    grg.set_growth(40, 16)                               # growth reserve: phantom slots are not variables
    grg.add_poses(g["poses"], g["fixed"])
    grg.add_edges(g["ei"], g["ej"], g["meas"], g["info"])
    idsg, ag = grg.marginal_cov_all()
    np.testing.assert_array_equal(idsg, ids1)
    for k in range(len(ag)):
        _close(ag[k], a1[k], 1e-8)


def test_errors():
    g = small_graph(np.random.default_rng(25), n=30, extra=10)
    gr = _g2o_gpu(g)
    with pytest.raises(G.FgoError):
        gr.marginal_cov_pairs([0], [3])                  # fixed vertex
    with pytest.raises(G.FgoError):
        gr.marginal_cov_pairs([3], [1000])               # unknown id
    n = G.lib.fgo_marginal_cov_all(gr._h, 0, None, None)
    assert n == 29
    ids = np.zeros(n, np.int64); out = np.zeros((n, 36))
    assert G.lib.fgo_marginal_cov_all(gr._h, n - 1, ids.ctypes.data_as(C.POINTER(C.c_int64)),
                                      out.ctypes.data_as(C.POINTER(C.c_double))) == -1      # FGO_EINVAL: cap too small
    assert G.lib.fgo_marginal_cov_all(gr._h, n, ids.ctypes.data_as(C.POINTER(C.c_int64)),
                                      out.ctypes.data_as(C.POINTER(C.c_double))) == n
    gs = _g2o_gpu(small_graph(np.random.default_rng(26), n=30, extra=10))
    gs.set_shard(0, 2, lambda ptr, n: 0)
    with pytest.raises(G.FgoError):
        gs.marginal_cov_all()
    with pytest.raises(G.FgoError):
        gs.marginal_cov_pairs([3], [4])
