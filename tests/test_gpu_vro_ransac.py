"""The batched RANSAC registration of visual-odometry records (csrc/kernels_vro_ransac.hip, fgo_vro_ransac_batch: one workgroup per
pair, all pairs in one launch) against its numpy restatement (tests/vro_ransac_reference.py, itself pinned by
tests/test_vro_ransac_reference_cpu.py).  The VRO library's arithmetic is not in the reference tree: the restatement is the yardstick.

ONE batch of 46 pairs (vro_ransac_reference.gpu_cases): M in {0, 2, 3, 4, 7, 8, 63, 64, 65, 127, 128, 129, 130, 300} three times
(the empty pair, the smallest samples, either side of a wave and of the 128-match LDS chunk, multi-chunk pairs) with outlier
shares 0 / 30 % / 60 % and rotations 0 / 0.1 / 1 / pi - 1e-3 rad cycling against each other, and four status pairs in the middle
(too few matches, collinear points, inliers below min_inliers, an inlier with z <= 0).  The number of hypotheses belongs to a
call, so the batch runs with hypotheses = 1, 100 and 256 (one hypothesis, a partial last round, full rounds) at the default
min_inliers = 8, and once more with 256 / min_inliers = 3 so that the smallest pairs register too; the results are shared.

Tolerances: the project's per-value tolerance, relative 1e-11, times the condition numbers the
restatement computes at run time.  With g = min(1, fit_gap) (the rotation of the fit is determined to rounding / fit_gap):
  q      1e-11 / g                                       t     1e-11 (1 + p_max) / g      (t = c_i - R c_j, |c_j| <= p_max)
  info   1e-11 cond_S / g x its largest entry            cov   the same x cond(info), of its largest entry
  rmse   1e-11 (1 + p_max) / g, absolute                 (a residual moves by |dR| |p_j| + |dt|)
Counts, the winner, the statuses, the masks and the void records are compared exactly."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import graph_slam_amd as G
from tests import vro_ransac_reference as ref

TOL = 1e-11
CONFIGS = ((1, 8), (100, 8), (256, 8), (256, 3))               # (hypotheses, min_inliers)
FIELDS = ("pose_ij", "status", "n_inliers", "best_hypothesis", "best_count", "n_valid", "rounds", "rmse", "info", "cov", "inliers",
          "hyp_counts")


def run(ptr, xi, xj, K, min_inliers, **kw):
    return G.vro_ransac_batch(ptr, xi, xj, params=G.vro_params(hypotheses=K, min_inliers=min_inliers), want_hyp_counts=True, **kw)


@functools.lru_cache(maxsize=None)
def cases():
    pairs = ref.gpu_cases()
    ptr, xi, xj = ref.pack(pairs)
    want, got = {}, {}
    for K, mi in CONFIGS:
        want[K, mi] = [ref.ransac_pair(p["xi"], p["xj"], hypotheses=K, min_inliers=mi) for p in pairs]
        got[K, mi] = run(ptr, xi, xj, K, mi)
    return pairs, ptr, xi, xj, want, got


def _ut_to_full(u):
    A = np.zeros((6, 6)); A[np.triu_indices(6)] = u
    return A + np.triu(A, 1).T


@pytest.mark.parametrize("K,min_inliers", CONFIGS)
def test_counts_winner_status_and_mask_equal_the_reference(K, min_inliers):
    pairs, ptr, xi, xj, want, got = cases()
    g = got[K, min_inliers]
    n_dec = 0
    for k, w in enumerate(want[K, min_inliers]):
        d = w["decided"]
        n_dec += int(d.sum())
        assert np.array_equal(g["hyp_counts"][k][d], w["hyp_counts"][d]), (k, np.nonzero(g["hyp_counts"][k] != w["hyp_counts"])[0][:5])
        if d.all():
            for f in ("best_hypothesis", "best_count", "n_valid"):
                assert g[f][k] == w[f], (k, f, g[f][k], w[f])
        assert g["status"][k] == w["status"], (k, pairs[k]["kind"], g["status"][k], w["status"])
        assert g["n_inliers"][k] == w["n_inliers"] and g["rounds"][k] == w["rounds"], (k, g["n_inliers"][k], w["n_inliers"], g["rounds"][k])
        assert np.array_equal(g["inliers"][ptr[k]:ptr[k + 1]].astype(bool), w["mask"]), k
    st = g["status"]
    print("K = %d, min_inliers = %d: %d hypotheses decided and equal; %d OK, %d too few, %d numerical" % (
        K, min_inliers, n_dec, (st == 0).sum(), (st == 1).sum(), (st == 2).sum()))
    if K > 1:
        kinds = {p["kind"]: st[k] for k, p in enumerate(pairs)}
        assert (kinds["too_few"], kinds["collinear"], kinds["z_nonpositive"]) == (G.FGO_VRO_TOO_FEW, G.FGO_VRO_TOO_FEW, G.FGO_VRO_NUM)
        assert kinds["below_min"] == (G.FGO_VRO_TOO_FEW if min_inliers == 8 else G.FGO_VRO_OK)
        assert (st == 0).sum() >= 20


@pytest.mark.parametrize("K,min_inliers", CONFIGS)
def test_pose_information_covariance_and_rmse_against_the_reference(K, min_inliers):
    pairs, ptr, xi, xj, want, got = cases()
    g = got[K, min_inliers]
    worst, n_ok = {}, 0
    for k, w in enumerate(want[K, min_inliers]):
        if w["status"] != ref.VRO_OK:
            continue
        n_ok += 1
        gap = min(1.0, w["fit_gap"])
        pose, info, cov = g["pose_ij"][k], _ut_to_full(g["info"][k]), g["cov"][k]
        assert pose[6] >= 0 and abs(pose[3:] @ pose[3:] - 1) <= 1e-14
        err = dict(q=np.abs(pose[3:] - w["pose"][3:]).max() / (TOL / gap),
                   t=np.abs(pose[:3] - w["pose"][:3]).max() / (TOL * (1 + w["p_max"]) / gap),
                   info=np.abs(info - w["info"]).max() / (TOL * w["cond_S"] / gap * np.abs(w["info"]).max()),
                   cov=np.abs(cov - w["cov"]).max() / (TOL * w["cond_S"] * w["cond_info"] / gap * np.abs(w["cov"]).max()),
                   rmse=abs(g["rmse"][k] - w["rmse"]) / (TOL * (1 + w["p_max"]) / gap))
        for f, e in err.items():
            assert e <= 1.0, (k, len(pairs[k]["xi"]), f, e, w["fit_gap"], w["cond_S"], w["cond_info"])
        worst = {f: max(e, worst.get(f, 0.0)) for f, e in err.items()}
        assert np.array_equal(cov, cov.T), k
    print("K = %d, min_inliers = %d, %d OK pairs: largest error as a share of its bound: %s" % (
        K, min_inliers, n_ok, ", ".join("%s %.1e" % fe for fe in worst.items())))
    assert n_ok >= (20 if K > 1 else 1)


@pytest.mark.parametrize("K,min_inliers", CONFIGS)
def test_failed_pairs_carry_the_void_record_bit_for_bit(K, min_inliers):
    pairs, ptr, xi, xj, want, got = cases()
    g = got[K, min_inliers]
    void_info = ref.ut21(10000.0 * np.eye(6))
    failed = np.nonzero(g["status"] != G.FGO_VRO_OK)[0]
    assert len(failed) >= 4
    for k in failed:
        assert g["pose_ij"][k].tobytes() == np.array([0, 0, 0, 0, 0, 0, 1.0]).tobytes(), k
        assert g["info"][k].tobytes() == void_info.tobytes() and not g["cov"][k].any(), k
        assert not g["inliers"][ptr[k]:ptr[k + 1]].any() and g["n_inliers"][k] == 0 and g["rmse"][k] == 0, k


def test_two_calls_and_both_workgroup_shapes_are_bit_identical():
    pairs, ptr, xi, xj, want, got = cases()
    for K, mi in ((100, 8), (256, 3)):
        again = run(ptr, xi, xj, K, mi)
        for f in FIELDS:
            assert again[f].tobytes() == got[K, mi][f].tobytes(), (K, f)
        default = G.lib.fgo_debug_vro_waves(0)
        try:
            for waves in (1, 4):
                assert G.lib.fgo_debug_vro_waves(waves) == waves
                o = run(ptr, xi, xj, K, mi)
                for f in FIELDS:
                    assert o[f].tobytes() == got[K, mi][f].tobytes(), (K, waves, f)
        finally:
            assert G.lib.fgo_debug_vro_waves(0) == default


def test_a_pair_alone_equals_the_pair_in_the_batch_and_outputs_are_optional():
    pairs, ptr, xi, xj, want, got = cases()
    K, mi = 256, 8
    g = got[K, mi]
    sizes = np.diff(ptr)
    picks = [int(np.nonzero(sizes == m)[0][-1]) for m in (0, 8, 65, 129, 300)] + [k for k, p in enumerate(pairs) if p["kind"] != "general"]
    for k in picks:
        a, b = ptr[k], ptr[k + 1]
        one = run([0, b - a], xi[a:b], xj[a:b], K, mi)
        for f in FIELDS:
            whole = g[f][a:b] if f == "inliers" else g[f][k]
            assert one[f].reshape(whole.shape).tobytes() == whole.tobytes(), (k, f)
    bare = run(ptr, xi, xj, K, mi, want_info=False, want_cov=False, want_inliers=False)
    assert "info" not in bare and "cov" not in bare and "inliers" not in bare
    for f in bare:
        assert bare[f].tobytes() == g[f].tobytes(), f
    empty = G.vro_ransac_batch([0], np.zeros((0, 3)), np.zeros((0, 3)))          # FGO_OK: nothing raised
    assert len(empty["status"]) == 0


def test_other_parameters_reach_the_kernel():
    """refine_rounds = 0 reports the winner's own pose and inliers; the seed moves the samples; sigma_z is a polynomial"""
    pairs, ptr, xi, xj, want, got = cases()
    keep = [k for k, p in enumerate(pairs) if len(p["xi"]) in (64, 130)]
    sp, sxi, sxj = ref.pack([pairs[k] for k in keep])
    for kw in (dict(refine_rounds=0), dict(seed=12345), dict(sigma_z=(0.01, 0.003, 0.002), fx=300.0, sigma_px=0.7), dict(max_dist=0.01, rigid_tol=0.0)):
        o = G.vro_ransac_batch(sp, sxi, sxj, params=G.vro_params(hypotheses=100, **kw), want_hyp_counts=True)
        for n, k in enumerate(keep):
            w = ref.ransac_pair(pairs[k]["xi"], pairs[k]["xj"], hypotheses=100, **kw)
            assert np.array_equal(o["hyp_counts"][n][w["decided"]], w["hyp_counts"][w["decided"]]), (kw, k)
            assert (o["status"][n], o["n_inliers"][n], o["rounds"][n]) == (w["status"], w["n_inliers"], w["rounds"]), (kw, k)
            if w["status"] == ref.VRO_OK:
                gap = min(1.0, w["fit_gap"])
                assert np.abs(o["pose_ij"][n][3:] - w["pose"][3:]).max() <= TOL / gap, (kw, k)
                assert np.abs(_ut_to_full(o["info"][n]) - w["info"]).max() <= TOL * w["cond_S"] / gap * np.abs(w["info"]).max(), (kw, k)


def test_the_records_feed_the_imu_check():
    """pose_ij7 and info_ut21 go to imu_check_vro_batch as they are: the failed pairs are skipped, the others are checked"""
    pairs, ptr, xi, xj, want, got = cases()
    g = got[256, 8]
    pre = G.Preintegrator()
    for _ in range(20):
        pre.integrate([0.1, -0.2, 9.7], [0.05, 0.02, -0.03], 0.005)
    n = len(pairs)
    o = G.imu_check_vro_batch(g["pose_ij"], pre.buf[None], np.zeros(n, np.int64), info=g["info"])
    failed = g["status"] != G.FGO_VRO_OK
    assert failed.any() and (~failed).any()
    assert np.array_equal(o["status"], np.where(failed, G.FGO_IC_SKIPPED, G.FGO_IC_OK)), (o["status"], g["status"])
