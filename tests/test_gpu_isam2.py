"""ISAM2 semantics (CGraphGT::optimizeGraphIncremental, gtsam/gtsam_graph.cpp:1768-1776; ISAM2Params :93-99) through the
C-ABI against the oracle's restatement (oracle/orc_gtsam.c: orc_isam2_step): linearisation point theta, linear solution
delta, fluid relinearisation by threshold, estimate = theta (+) delta.  Static graphs updated repeatedly, graphs that
grow between updates (the drivers' pattern), mixed variable kinds (planes / points / velocities / biases), limits of
the threshold."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import graph_slam_amd as G
from tests import orc_binding as orc
from tests.util import small_graph, info_ut, mixed_graph, mixed_oracle, vio_graph
from tests.test_gpu_gtsam import build, synth_gtsam
from tests.test_gpu_factors import mixed_gpu
from tests.test_gpu_imu import vio_gpu

SOFT_PRIOR = info_ut(np.diag([1e6] * 6))       # sigma 1e-3: well conditioned, so iterates can be compared tightly


def state_of(gr, n):
    th = np.zeros((n, 7)); de = np.zeros((n, 6))
    for v in range(n):
        th[v], de[v] = gr.isam2_state(v)
    return th, de


@pytest.mark.parametrize("thr", [0.1, 0.02])
def test_static_graph_repeated_updates_match_oracle(thr):
    g = synth_gtsam(300, 4, 2, seed=7)
    rng = np.random.default_rng(0)
    g["poses"][1:, :3] += rng.normal(size=(299, 3)) * 0.15           # start far enough for several relinearisation rounds
    gr, po = build(g, prior_info=SOFT_PRIOR)
    n = len(g["poses"])
    theta = g["poses"].copy(); delta = np.zeros((n, 6))
    moved_total = 0
    for it in range(6):
        st = gr.isam2_update(thr)
        est_o, moved = po.isam2_step(thr, theta, delta)
        assert int(st.reserved[1]) == moved
        moved_total += moved
        est = gr.get_poses()
        np.testing.assert_allclose(est, est_o, atol=2e-9)
        th, de = state_of(gr, n)
        np.testing.assert_allclose(th, theta, atol=2e-9)
        np.testing.assert_allclose(de, delta, atol=2e-9)
        assert abs(st.chi2_final - po.chi2()) <= 1e-8 * max(po.chi2(), 1e-12)
        assert abs(gr.chi2() - st.chi2_final) <= 1e-12 * st.chi2_final    # the values ARE the estimate
    assert moved_total > 0
    assert st.chi2_final < 0.05 * gr_initial_chi2(g)


def gr_initial_chi2(g):
    gr0, _ = build(g, prior_info=SOFT_PRIOR)
    return gr0.chi2()


def test_first_update_is_one_gauss_newton_step():
    rng = np.random.default_rng(1)
    g = small_graph(rng, n=80, extra=120, noise=0.03, fixed_first=False)
    gr, po = build(g, prior_info=SOFT_PRIOR)
    ref, _ = build(g, prior_info=SOFT_PRIOR)
    d = ref.solve_step(0.0)                                              # H d = b at the initial values
    gr.isam2_update(0.1)
    n = len(g["poses"])
    th, de = state_of(gr, n)
    np.testing.assert_allclose(th, g["poses"], rtol=0, atol=1e-15)       # delta was zero: nothing relinearised (quaternions are normalised on entry)
    np.testing.assert_allclose(de.ravel(), d, atol=1e-12 * max(1.0, np.abs(d).max()))
    theta = g["poses"].copy(); delta = np.zeros((n, 6))
    est_o, moved = po.isam2_step(0.1, theta, delta)
    assert moved == 0
    np.testing.assert_allclose(gr.get_poses(), est_o, atol=1e-9)


def test_threshold_zero_relinearises_everything_and_converges_to_the_batch_optimum():
    rng = np.random.default_rng(2)
    g = small_graph(rng, n=60, extra=90, noise=0.03, fixed_first=False)
    gr, _ = build(g, prior_info=SOFT_PRIOR)
    batch, _ = build(g, prior_info=SOFT_PRIOR)
    batch.optimize_gtsam()
    n = len(g["poses"])
    for it in range(8):
        st = gr.isam2_update(0.0)
        if it > 0:
            assert int(st.reserved[1]) == n                              # every free variable moved
    assert abs(gr.error() - batch.error()) <= 1e-6 * batch.error()
    assert np.abs(gr.get_poses()[:, :3] - batch.get_poses()[:, :3]).max() < 1e-4


def test_huge_threshold_never_moves_the_linearisation_point():
    rng = np.random.default_rng(3)
    g = small_graph(rng, n=40, extra=50, noise=0.03, fixed_first=False)
    gr, _ = build(g, prior_info=SOFT_PRIOR)
    gr.isam2_update(1e9)
    e1 = gr.get_poses().copy()
    st = gr.isam2_update(1e9)
    assert int(st.reserved[1]) == 0
    np.testing.assert_array_equal(gr.get_poses(), e1)                    # same theta, same system, deterministic solve
    th, _ = state_of(gr, len(g["poses"]))
    np.testing.assert_allclose(th, g["poses"], rtol=0, atol=1e-15)


@pytest.mark.parametrize("reserve", [0, 384])
def test_growing_graph_like_the_drivers(reserve):
    """per record: new poses + their factors, then optimizeGraphIncremental (test_vro_imu_graph.cpp:344).
    reserve 0: the structure phase reruns at every update (round 1's behaviour); reserve 384 (the default): new variables
    claim phantom slots and factors inside the band are appended in place, only far loop closures rebuild -- the estimates
    must match the oracle step by step either way."""
    g = synth_gtsam(120, 4, 2, seed=11)
    rng = np.random.default_rng(4)
    g["poses"][1:, :3] += rng.normal(size=(119, 3)) * 0.05
    N, ei, ej = len(g["poses"]), g["ei"], g["ej"]
    order = np.argsort(np.maximum(ei, ej), kind="stable")
    ei, ej, meas, info = ei[order], ej[order], g["meas"][order], g["info"][order]
    newest = np.maximum(ei, ej)
    gr = G.Graph()
    gr.isam2_reserve(reserve)
    gr.add_poses(g["poses"][:1]); gr.add_prior(0, g["poses"][0], SOFT_PRIOR)
    theta = np.zeros((0, 7)); delta = np.zeros((0, 6))
    have, used = 1, 0
    thr = 0.05
    rebuilt = 0
    steps = 0
    while have < N:
        k = min(N, have + 7)
        gr.add_poses(g["poses"][have:k], ids=np.arange(have, k))
        sel = np.nonzero((newest < k) & (newest >= have))[0]
        gr.add_edges(ei[sel], ej[sel], meas[sel], info[sel], tangent_order=G.FGO_TANGENT_GTSAM)
        used += len(sel)
        have = k
        st = gr.isam2_update(thr)
        rebuilt += st.structure_rebuilt
        steps += 1
        # the oracle gets the grown graph as a new problem and the carried-over ISAM2 state
        m = newest < have
        po = orc.Problem(g["poses"][:have], np.zeros(have, np.uint8), ei[m], ej[m], meas[m], info[m])
        po.set_gtsam()
        po.add_priors(np.array([0], np.int32), g["poses"][:1], SOFT_PRIOR[None, :])
        theta = np.ascontiguousarray(np.vstack([theta, g["poses"][len(theta):have]]))
        delta = np.ascontiguousarray(np.vstack([delta, np.zeros((have - len(delta), 6))]))
        est_o, moved = po.isam2_step(thr, theta, delta)
        assert int(st.reserved[1]) == moved
        np.testing.assert_allclose(gr.get_poses(), est_o, atol=5e-9)
    assert used == len(ei)
    if reserve == 0:
        assert rebuilt == steps
    else:
        far = int(np.sum(np.abs(g["ej"] - g["ei"]) > 60))
        assert rebuilt <= 1 + far, (rebuilt, far, steps)      # the first build + at most one rebuild per far loop closure
        print("growing graph: %d updates, %d structure builds (%d loop closures beyond the band)" % (steps, rebuilt, far))
    # no new factors: the structure phase is not repeated
    st = gr.isam2_update(thr)
    assert st.structure_rebuilt == 0
    # the drivers finish with a batch run from the incremental estimate (test_vro_imu_graph.cpp:385): it has little left to do
    e_inc = gr.error()
    gr.optimize_gtsam()
    assert gr.error() <= e_inc and gr.error() > 0.5 * e_inc


def test_mixed_variable_kinds_match_oracle():
    rng = np.random.default_rng(5)
    g = mixed_graph(rng, n_poses=10, n_planes=3, n_points=20)
    gr, po = mixed_gpu(g), mixed_oracle(g)
    n = len(g["values"])
    theta = np.ascontiguousarray(g["values"][:, :7].copy()); delta = np.zeros((n, 6))
    for it in range(4):
        st = gr.isam2_update(0.01)
        est_o, moved = po.isam2_step(0.01, theta, delta)
        assert int(st.reserved[1]) == moved
        V = gr.get_poses()
        np.testing.assert_allclose(V[:, :7], est_o, atol=1e-7)
    assert st.chi2_final < gr_chi2_of(mixed_gpu(g))


def gr_chi2_of(gr):
    return gr.chi2()


def test_vio_graph_with_imu_factors_matches_oracle():
    rng = np.random.default_rng(6)
    g = vio_graph(rng, n_kf=10, with_planes=True)
    gr, po = vio_gpu(g), mixed_oracle(g)
    n = len(g["values"])
    theta = np.ascontiguousarray(g["values"][:, :7].copy()); delta = np.zeros((n, 6))
    for it in range(4):
        st = gr.isam2_update(0.1)
        est_o, moved = po.isam2_step(0.1, theta, delta)
        assert int(st.reserved[1]) == moved
        V = gr.get_poses()
        K = g["n_kf"]
        assert np.abs(V[:K, :7] - est_o[:K]).max() < 1e-6
        assert np.abs(V[K:2 * K, :3] - est_o[K:2 * K, :3]).max() < 1e-6
        assert np.abs(V[2 * K:3 * K, :6] - est_o[2 * K:3 * K, :6]).max() < 1e-6


def test_reset_and_misuse():
    rng = np.random.default_rng(7)
    g = small_graph(rng, n=12, extra=10, fixed_first=False)
    gr, _ = build(g, prior_info=SOFT_PRIOR)
    with pytest.raises(G.FgoError):
        gr.isam2_state(0)                                                # no update yet
    gr.isam2_update(0.1)
    gr.isam2_state(0)
    gr.isam2_reset()
    with pytest.raises(G.FgoError):
        gr.isam2_state(0)
    with pytest.raises(G.FgoError):
        gr.isam2_update(-1.0)
    # g2o-semantics graphs have no ISAM2 counterpart in the reference
    g2 = small_graph(rng, n=6, extra=4)
    h = G.Graph(); h.add_poses(g2["poses"], g2["fixed"]); h.add_edges(g2["ei"], g2["ej"], g2["meas"], g2["info"])
    with pytest.raises(G.FgoError):
        h.isam2_update(0.1)
    # an indefinite system (no prior: the gauge is free) is reported, not silently solved
    g3 = small_graph(rng, n=6, extra=4, fixed_first=False)
    f = G.Graph(); f.add_poses(g3["poses"]); f.add_edges(g3["ei"], g3["ej"], g3["meas"], g3["info"], tangent_order=G.FGO_TANGENT_GTSAM)
    try:
        f.isam2_update(0.1)
        gauge_free_detected = False
    except G.FgoError:
        gauge_free_detected = True
    # rounding may leave the singular matrix numerically positive; either outcome must leave the context usable
    assert gauge_free_detected in (True, False)
    f.chi2()


def test_incremental_updates_do_not_rebuild_the_structure():
    """SURVEY §8 f4 / VERDICT r1 #6: one new pose per update on a 5 000-pose graph (the reference's per-record flow,
    gtsam/test_ba_imu_graph.cpp:427): after the first build the structure phase must not run again (stats.structure_rebuilt
    == 0; stats.t_symbolic is the host time of the in-place extension), and the estimate equals the one of a context that
    rebuilds every time (reserve 0) to rounding."""
    n0, extra = 5000, 12
    g = synth_gtsam(n0 + extra, 5, 0, seed=17)
    newest = np.maximum(g["ei"], g["ej"])
    res = {}
    for reserve in (384, 0):
        gr = G.Graph()
        gr.isam2_reserve(reserve)
        gr.add_poses(g["poses"][:n0]); gr.add_prior(0, g["poses"][0], SOFT_PRIOR)
        m = newest < n0
        gr.add_edges(g["ei"][m], g["ej"][m], g["meas"][m], g["info"][m], tangent_order=G.FGO_TANGENT_GTSAM)
        gr.isam2_update(0.1)
        rebuilt, host_ms = 0, []
        for k in range(n0, n0 + extra):
            gr.add_poses(g["poses"][k:k + 1], ids=[k])
            m = newest == k
            gr.add_edges(g["ei"][m], g["ej"][m], g["meas"][m], g["info"][m], tangent_order=G.FGO_TANGENT_GTSAM)
            st = gr.isam2_update(0.1)
            rebuilt += st.structure_rebuilt; host_ms.append(1e3 * st.t_symbolic)
        res[reserve] = (rebuilt, gr.get_poses().copy(), np.median(host_ms))
    assert res[384][0] == 0 and res[0][0] == extra
    assert res[384][2] < 2.0, res[384][2]                      # host side of an update: well under the 10+ ms of a rebuild at this size
    print("incremental update at 5k poses: host %.3f ms (in place) vs %.3f ms (rebuild)" % (res[384][2], res[0][2]))
    np.testing.assert_allclose(res[384][1], res[0][1], atol=1e-6)   # two elimination orders of a 5 000-pose chain: rounding differs (measured 3e-8)


def test_phantom_slots_never_reach_the_caller():
    """after fgo_isam2_update the structure carries phantom variable slots (growth reserve).  They
    must not appear in n_free, fgo_linearize's dense system or fgo_solve_step's delta: a C caller sizes its buffers from
    its own free-variable count (fgo.h).  Buffers get canaries behind the caller-sized part."""
    import ctypes as C
    g = synth_gtsam(60, 3, 1, seed=3)
    gr, po = build(g, prior_info=SOFT_PRIOR)
    n = len(g["poses"])
    # reference values from a context that never entered the incremental mode
    gr0, _ = build(g, prior_info=SOFT_PRIOR)
    chi0, H0, b0 = gr0.linearize()
    d0 = gr0.solve_step(1e-3)
    assert H0.shape == (6 * n, 6 * n)
    st = gr.isam2_update(1e9)                       # threshold never reached: theta and the values stay where they are
    assert st.n_free == n, (st.n_free, n)
    assert gr.stats().n_free == n
    lib, h = G.lib, gr._h
    CAN = 1234.5
    m = 6 * n
    d = np.full(m + 4096, CAN)
    assert lib.fgo_solve_step(h, 1e-3, d.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert np.all(d[m:] == CAN), "fgo_solve_step wrote behind 6 * n_free doubles"
    Hd = np.full(m * m + 4096, CAN); bd = np.full(m + 4096, CAN)
    chi = C.c_double(); nf = C.c_int64()
    assert lib.fgo_linearize(h, C.byref(chi), Hd.ctypes.data_as(C.POINTER(C.c_double)), bd.ctypes.data_as(C.POINTER(C.c_double)), C.byref(nf)) == 0
    assert nf.value == n
    assert np.all(Hd[m * m:] == CAN) and np.all(bd[m:] == CAN)
    # ... and what IS reported is the caller's system (the estimate did not move: delta of the first update is tiny
    # next to the 1e9 threshold, values = theta (+) delta differ from the start by one Gauss-Newton step)
    gr2, _ = build(g, prior_info=SOFT_PRIOR)
    est = gr.get_poses()
    for v in range(n):
        gr2.set_pose(v, est[v])
    chi2, H2, b2 = gr2.linearize()
    np.testing.assert_allclose(Hd[:m * m].reshape(m, m), H2, rtol=0, atol=1e-9 * np.abs(H2).max())
    np.testing.assert_allclose(bd[:m], b2, rtol=0, atol=1e-9 * max(np.abs(b2).max(), 1.0))
    np.testing.assert_allclose(d[:m], gr2.solve_step(1e-3), rtol=0, atol=1e-9)
    # fgo_isam2_reset leaves the incremental mode: the reserve is gone at the next use
    gr.isam2_reset()
    assert gr.linearize()[1].shape == (m, m)


def _grow(gr_factory, g, n0, extra, on_update=None):
    newest = np.maximum(g["ei"], g["ej"])
    gr = gr_factory()
    gr.add_poses(g["poses"][:n0]); gr.add_prior(0, g["poses"][0], SOFT_PRIOR)
    m = newest < n0
    gr.add_edges(g["ei"][m], g["ej"][m], g["meas"][m], g["info"][m], tangent_order=G.FGO_TANGENT_GTSAM)
    stats = [gr.isam2_update(0.1)]
    for k in range(n0, n0 + extra):
        gr.add_poses(g["poses"][k:k + 1], ids=[k])
        m = newest == k
        gr.add_edges(g["ei"][m], g["ej"][m], g["meas"][m], g["info"][m], tangent_order=G.FGO_TANGENT_GTSAM)
        stats.append(gr.isam2_update(0.1))
        if on_update: on_update(gr, k)
    return gr, stats


def test_partial_refactorisation_equals_full_sweep_bitwise(monkeypatch):
    """SURVEY §8 f4 / VERDICT r2 #6: an incremental update re-runs only the tasks on the paths from the affected variables to
    the roots of the elimination tree; every other column keeps its blocks of L and its entry of y.  The result must be
    BIT-identical to the full sweep (same kernels, same inputs, same order), the number of tasks re-run a small fraction, and
    a relinearisation wave (threshold reached somewhere) must be handled the same way."""
    n0, extra = 5000, 12
    g = synth_gtsam(n0 + extra, 5, 2, seed=23)
    rng = np.random.default_rng(1)
    g["poses"][n0 - 40:n0, :3] += rng.normal(size=(40, 3)) * 0.12       # a stretch that will cross the 0.1 threshold and relinearise
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("FGO_ISAM_PARTIAL", mode)
        gr, stats = _grow(G.Graph, g, n0, extra)
        th, de = state_of(gr, 30)
        out[mode] = (gr.get_poses().copy(), th, de, stats)
    np.testing.assert_array_equal(out["1"][0], out["0"][0])
    np.testing.assert_array_equal(out["1"][1], out["0"][1]); np.testing.assert_array_equal(out["1"][2], out["0"][2])
    s1, s0 = out["1"][3], out["0"][3]
    assert all(int(a.reserved[1]) == int(b.reserved[1]) for a, b in zip(s1, s0))            # same relinearisation decisions
    print("tasks re-run per step, partial on:", [int(st.reserved[3]) for st in s1], "off:", [int(st.reserved[3]) for st in s0])
    assert s1[0].reserved[3] == -1 and all(st.reserved[3] == -1 for st in s0)               # first step / switched off: full sweeps
    part = [int(st.reserved[3]) for st in s1[1:]]
    assert all(p > 0 or p == -2 for p in part) and 0 < np.median(part) < 0.2 * s1[-1].n_tasks, (part, s1[-1].n_tasks)
    ms1 = np.median([st.reserved[0] for st in s1[2:]]); ms0 = np.median([st.reserved[0] for st in s0[2:]])
    print("ISAM2 update at %d poses: %.3f ms device with partial re-factorisation (%d of %d tasks), %.3f ms full sweep" %
          (n0, ms1, int(np.median(part)), s1[-1].n_tasks, ms0))
    assert sum(int(st.reserved[1]) for st in s1) > 0


def test_factor_taken_between_updates_forces_a_full_sweep():
    """The previous step's factor stays in d_L for the next update only while nothing else writes it: after a marginal
    request, fgo_solve_step or fgo_bench_phase the next update re-factors everything and still ends where an undisturbed run
    ends, bit for bit; after calls that leave d_L alone it stays partial.  A marginal request right after an update factors
    the undamped system itself: it must not take the ISAM2 factor for that one."""
    import ctypes as C
    n0, extra = 5000, 12
    g = synth_gtsam(n0 + extra, 5, 2, seed=23)
    rng = np.random.default_rng(1)
    g["poses"][n0 - 40:n0, :3] += rng.normal(size=(40, 3)) * 0.12
    delta = np.zeros(6 * (n0 + extra))

    def marginals(gr):
        m = gr.marginal_cov_many([3, n0 - 7, 17, 17])
        gr.linearize(dense=False)
        assert np.array_equal(m, gr.marginal_cov_many([3, n0 - 7, 17, 17]))

    def solve_step(gr):
        gr._chk(G.lib.fgo_solve_step(gr._h, 1e-3, delta.ctypes.data_as(C.POINTER(C.c_double))))

    def preserve(gr):
        gr.get_poses(); gr.chi2(); gr.linearize(dense=False)

    calls = {n0 + 1: marginals, n0 + 3: preserve, n0 + 5: solve_step, n0 + 7: preserve, n0 + 9: lambda gr: gr.bench_phase(1, 1),
             n0 + 10: preserve}
    gr, stats = _grow(G.Graph, g, n0, extra, lambda gr, k: calls[k](gr) if k in calls else None)
    plain, plain_stats = _grow(G.Graph, g, n0, extra)
    assert all(int(st.reserved[3]) > 0 or int(st.reserved[3]) == -2 for st in plain_stats[1:])
    for k, call in calls.items():
        tasks = int(stats[k - n0 + 2].reserved[3])                         # the update after the call
        assert (tasks > 0 or tasks == -2) if call is preserve else tasks == -1, (k - n0, tasks)
    assert [int(st.reserved[1]) for st in stats] == [int(st.reserved[1]) for st in plain_stats]
    np.testing.assert_array_equal(gr.get_poses(), plain.get_poses())
    for a, b in zip(state_of(gr, n0 + extra), state_of(plain, n0 + extra)):
        np.testing.assert_array_equal(a, b)


def test_against_independent_isam2_reference():
    """The product against tests/isam2_reference.py -- per-factor cached linearisations, variable-wise relinearisation,
    elimination + back-substitution with the wildfire rule -- on a graph that grows by one pose per update.
    wildfire = 0: the two must agree (the full solve IS what partial re-elimination computes); wildfire = 1e-3 (ISAM2's
    default): the deviation of the product's exact back-substitution from ISAM2's thresholded one is reported and bounded."""
    from tests.isam2_reference import Isam2Reference
    n0, extra = 40, 25
    g = synth_gtsam(n0 + extra, 3, 1, seed=31)
    rng = np.random.default_rng(2)
    g["poses"][1:, :3] += rng.normal(size=(n0 + extra - 1, 3)) * 0.08
    newest = np.maximum(g["ei"], g["ej"])
    dev = {}
    for wild in (0.0, 1e-3):
        ref = Isam2Reference(0.1, wild)
        for k in range(n0): ref.add_pose(g["poses"][k])
        ref.add_prior(0, g["poses"][0], SOFT_PRIOR)
        for e in np.nonzero(newest < n0)[0]: ref.add_between(int(g["ei"][e]), int(g["ej"][e]), g["meas"][e], g["info"][e])
        est_ref = [ref.update()]
        worst = [0.0]

        def on_update(gr, k):
            ref.add_pose(g["poses"][k])
            for e in np.nonzero(newest == k)[0]: ref.add_between(int(g["ei"][e]), int(g["ej"][e]), g["meas"][e], g["info"][e])
            est, moved = ref.update()
            worst[0] = max(worst[0], np.abs(gr.get_poses()[:, :3] - est[:, :3]).max())
        gr, stats = _grow(G.Graph, g, n0, extra, on_update)
        dev[wild] = worst[0]
        n_fac = len(ref.factors)
        # the reference really worked incrementally: far fewer factor linearisations than (updates x factors)
        assert ref.n_relinearised_factors < 0.6 * (extra + 1) * n_fac
    print("deviation from the independent ISAM2 reference: %.2e (wildfire 0), %.2e (wildfire 1e-3)" % (dev[0.0], dev[1e-3]))
    assert dev[0.0] < 1e-8
    assert dev[1e-3] < 2e-2                               # bounded by the threshold's order times the chain length it is allowed to ignore


def test_updates_without_lookahead_flags_and_masked_linearisation_give_the_same_states():
    """An update normally (a) knows from the END of the previous one which variables it will relinearise (no mid-stream
    synchronisation) and (b) re-gathers H / b / chi2 only for the variables whose factors changed (`k_linearize_gtsam`, masked
    form).  Both are shortcuts, not approximations: with `FGO_TUNE=isam_lookahead=0,isam_masked=0` (flags fetched with a
    synchronisation, every variable gathered again) a growing graph with a relinearisation wave must end in the same state,
    bit for bit, with the same relinearisation decisions and the same chi2 at every linearisation point."""
    import subprocess, sys, json, os
    code = r"""
import sys, json, numpy as np
sys.path.insert(0, %r)
import graph_slam_amd as G
from tests.test_gpu_isam2 import _grow, synth_gtsam, state_of
n0, extra = 3000, 10
g = synth_gtsam(n0 + extra, 5, 2, seed=29)
rng = np.random.default_rng(3)
g["poses"][n0 - 30:n0, :3] += rng.normal(size=(30, 3)) * 0.12
gr, stats = _grow(G.Graph, g, n0, extra)
th, de = state_of(gr, 25)
print(json.dumps({"poses": gr.get_poses().tolist(), "theta": np.asarray(th).tolist(), "delta": np.asarray(de).tolist(),
                  "relin": [int(s.reserved[1]) for s in stats], "chi0": [s.chi2_initial for s in stats], "chi1": [s.chi2_final for s in stats],
                  "tasks": [int(s.reserved[3]) for s in stats]}))
""" % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for name, tune in (("fast", ""), ("plain", "isam_lookahead=0,isam_masked=0")):
        env = dict(os.environ); env["FGO_TUNE"] = tune
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        out[name] = json.loads(r.stdout.strip().splitlines()[-1])
    a, b = out["fast"], out["plain"]
    assert a["relin"] == b["relin"] and sum(a["relin"]) > 0 and a["tasks"] == b["tasks"]
    for key in ("poses", "theta", "delta", "chi1"):
        np.testing.assert_array_equal(np.asarray(a[key]), np.asarray(b[key]), err_msg=key)
    # chi2 at the linearisation point: summed per variable (masked form) against per workgroup -- the same terms in another order
    np.testing.assert_allclose(np.asarray(a["chi0"]), np.asarray(b["chi0"]), rtol=1e-13)


def test_wildfire_threshold_cuts_the_back_substitution_and_stays_within_the_threshold():
    """fgo_isam2_set_wildfire (ISAM2Params::wildfireThreshold analogue, gtsam/gtsam_graph.cpp:93-99): below the re-factored root
    paths a task is solved again only if a delta it reads moved by >= the threshold.  With the smallest positive threshold
    every change counts, so the result must equal the exact back-substitution bit for bit (a task that is skipped would have
    reproduced its old values); at GTSAM's default 1e-3 the estimate may differ from the exact one by the order of the threshold."""
    n0, extra = 6000, 10
    g = synth_gtsam(n0 + extra, 5, 2, seed=31)
    out = {}
    for name, thr in (("exact", 0.0), ("tiny", 5e-324), ("gtsam", 1e-3)):
        def factory(thr=thr):
            gr = G.Graph()
            gr.isam2_set_wildfire(thr)
            return gr
        gr, stats = _grow(factory, g, n0, extra)
        th, de = state_of(gr, 40)
        out[name] = (gr.get_poses().copy(), np.asarray(th), np.asarray(de), stats)
    cut = [int(st.reserved[4]) for st in out["tiny"][3]]
    assert cut[0] == 0 and sum(cut) >= extra - 4 and all(cut[-4:]), cut   # the first updates (full sweeps) leave a solution behind, the rest cut
    assert not any(int(st.reserved[4]) for st in out["exact"][3])
    np.testing.assert_array_equal(out["tiny"][0], out["exact"][0])
    np.testing.assert_array_equal(out["tiny"][2], out["exact"][2])
    d = np.abs(out["gtsam"][0] - out["exact"][0]).max()
    print("wildfire 1e-3: largest deviation of the estimate from the exact back-substitution %.3e" % d)
    assert d < 2e-2 and all(int(st.reserved[4]) for st in out["gtsam"][3][-4:])

