"""Batched two-view bundle adjustment (csrc/kernels_two_view.hip, fgo_two_view_ba_batch: one wave per pair, the whole LM run of a
pair in one launch) against the oracle and against the context-per-pair path.
Reference: CGraphGT::bundleAdjust, gtsam/gtsam_graph.cpp:500-610 -- PriorFactor<Pose3> sigma 1e-7 on the first pose, one Point3 per
match with PriorFactor<Point3> sigma 0.014, two GenericProjectionFactor sigma 1 px per match, LevenbergMarquardtOptimizer, then
Marginals::marginalCovariance of the second pose and its inverse.

Problems: camera SR4000, base twist XI scaled by s (s = 1: a visual-odometry step, the oracle's LM accepts every trial; s = 5 from
an identity start: rejected trials, and for some seeds LM gives up at the lambda bound), points in front of camera i, 0.3 px pixel
noise, (5, 5, 10) mm noise on the 3-D feature.  Every expected count is the ORACLE's, taken at run time; the bounds are the ones the
bundle-adjustment path already answers to (tests/test_gpu_ba_oracle.py:55-67, tests/test_gpu_marginals_all.py:115)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import graph_slam_amd as G
import graph_slam_amd.scenarios as S
from tests import orc_binding as orc
from tests.util import info_ut

CALIB = np.array([250.5773, 250.5773, 0, 90, 70, -0.8466, 0.5370, 0, 0])
XI = np.array([0.02, -0.03, 0.015, 0.10, -0.05, 0.04])
IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])
POSE_SIGMA, POINT_SIGMA, PIXEL_SIGMA = 1e-7, 0.014, 1.0


def _rotvec_quat(w):
    th = np.linalg.norm(w)
    return np.concatenate([np.sin(0.5 * th) / th * w, [np.cos(0.5 * th)]]) if th > 0 else IDENT[3:].copy()


def _conj(q):
    return q * np.array([-1, -1, -1, 1.0])


def make_pair(seed, n, s, bps=None, pose_j0=None):
    """one visual-odometry record: xyz (feature in body frame i, noisy), uv_i / uv_j (its pixels), the start of pose j"""
    rng = np.random.default_rng(seed)
    b = IDENT if bps is None else np.asarray(bps, np.float64)
    Tj = np.concatenate([s * XI[3:], _rotvec_quat(s * XI[:3])])
    pc = np.stack([0.35 * rng.uniform(-1, 1, n), 0.25 * rng.uniform(-1, 1, n), 1.5 + 0.8 * rng.uniform(-1, 1, n)], 1)
    pw = b[:3] + S._quat_rot(b[None, 3:], pc)                                   # body i = world
    cam_q = S._quat_mul(Tj[3:], b[3:]); cam_t = Tj[:3] + S._quat_rot(Tj[None, 3:], b[None, :3])[0]
    pj = S._quat_rot(_conj(cam_q)[None], pw - cam_t)
    uv_i = S._project(pc, CALIB) + 0.3 * rng.normal(size=(n, 2))
    uv_j = S._project(pj, CALIB) + 0.3 * rng.normal(size=(n, 2))
    xyz = pw + rng.normal(size=(n, 3)) * np.array([0.005, 0.005, 0.010])
    return {"n": n, "xyz": xyz, "uv_i": uv_i, "uv_j": uv_j, "bps": bps, "pose_j0": IDENT.copy() if pose_j0 is None else np.asarray(pose_j0, np.float64),
            "truth_j": Tj}


def pair_oracle(pr):
    """the graph bundleAdjust builds for the record, handed to the oracle: X0, X1, then the points"""
    n = pr["n"]
    vals = np.zeros((2 + n, 7)); vals[0] = IDENT; vals[1] = pr["pose_j0"]; vals[2:, :3] = pr["xyz"]
    vk = np.zeros(2 + n, np.int32); vk[2:] = orc.VK_POINT
    ei = np.repeat([0, 1], n).astype(np.int32); ej = np.tile(2 + np.arange(n), 2).astype(np.int32)
    meas = np.zeros((2 * n, 7)); meas[:n, :2] = pr["uv_i"]; meas[n:, :2] = pr["uv_j"]
    info = np.zeros((2 * n, 21)); info[:, 0] = 1.0 / PIXEL_SIGMA ** 2
    po = orc.Problem(vals, np.zeros(2 + n, np.uint8), ei, ej, meas, info)
    po.set_kinds(vk, np.full(2 * n, orc.FK_REPROJ, np.int32))
    po.set_calibration(CALIB, IDENT if pr["bps"] is None else np.asarray(pr["bps"], np.float64))
    w = np.zeros(21); w[[0, 6, 11, 15, 18, 20]] = 1.0 / POSE_SIGMA ** 2
    pw6 = np.zeros((6, 6)); pw6[:3, :3] = np.eye(3) / POINT_SIGMA ** 2
    infos = np.tile(info_ut(pw6), (1 + n, 1)); infos[0] = w
    po.add_priors(np.concatenate([[0], 2 + np.arange(n)]).astype(np.int32), np.concatenate([IDENT[None], vals[2:]]), infos)
    return po


def run_oracle(pr):
    po = pair_oracle(pr)
    e0 = po.error_gtsam()
    _, st = po.optimize_gtsam(100)
    return {"po": po, "e0": e0, "e1": po.error_gtsam(), "iterations": st.iterations, "trials": st.trials, "lambda": st.lambda_final,
            "vals": po.get_poses()}


def batch_arrays(pairs):
    mp = np.concatenate([[0], np.cumsum([p["n"] for p in pairs])]).astype(np.int64)
    cat = lambda k, w: np.concatenate([p[k].reshape(-1, w) for p in pairs]) if pairs else np.zeros((0, w))
    return mp, cat("xyz", 3), cat("uv_i", 2), cat("uv_j", 2), np.array([p["pose_j0"] for p in pairs]).reshape(-1, 7)


def run_batch(pairs, **kw):
    mp, xyz, uvi, uvj, p0 = batch_arrays(pairs)
    return G.two_view_ba_batch(mp, xyz, uvi, uvj, CALIB, pose_j0=p0, **kw)


def _rejecting(o):
    return o["trials"] > o["iterations"] and o["lambda"] < 1e5


def _at_bound(o):
    return o["lambda"] >= 1e5


@functools.lru_cache(maxsize=None)
def cases():
    """the ragged batch of test 1: N below, at and above a lane pass and several passes at s = 1, then the s = 5 records whose LM
    rejects trials / gives up at the lambda bound.  Oracle and GPU run once; the tests share the results and leave them alone."""
    pairs = [make_pair(100 + n, n, 1.0) for n in (5, 8, 63, 64, 65, 130)] + [make_pair(1, 8, 5.0), make_pair(3, 8, 5.0)]
    ref = [run_oracle(p) for p in pairs]
    for want in (_rejecting, _at_bound):                                        # coverage of the reject path cannot disappear silently
        if not any(want(o) for o in ref):
            for seed in range(1, 21):
                p = make_pair(seed, 8, 5.0); o = run_oracle(p)
                if want(o):
                    pairs.append(p); ref.append(o)
                    break
            else:
                pytest.fail("no s = 5 record in seeds 1..20 whose oracle LM %s" % ("rejects a trial and converges" if want is _rejecting else "ends at the lambda bound"))
    return pairs, ref, run_batch(pairs)


def _pose_diff(a, b):
    sgn = 1.0 if np.dot(a[3:], b[3:]) >= 0 else -1.0
    return max(np.abs(a[:3] - b[:3]).max(), np.abs(a[3:] * sgn - b[3:]).max())


def _check_vs_oracle(out, k, o):
    print("pair %d: it %d/%d trials %d/%d lambda %.3e/%.3e e0 rel %.2e e1 rel %.2e pose_i %.2e pose_j %.2e" % (
        k, out["iterations"][k], o["iterations"], out["trials"][k], o["trials"], out["lambda_final"][k], o["lambda"],
        abs(out["error_initial"][k] - o["e0"]) / o["e0"], abs(out["error_final"][k] - o["e1"]) / o["e1"],
        _pose_diff(out["pose_i"][k], o["vals"][0]), _pose_diff(out["pose_j"][k], o["vals"][1])))
    assert out["status"][k] == G.FGO_TV_OK
    assert out["iterations"][k] == o["iterations"] and out["trials"][k] == o["trials"]
    assert abs(out["lambda_final"][k] - o["lambda"]) <= 1e-12 * o["lambda"]
    assert abs(out["error_initial"][k] - o["e0"]) <= 1e-11 * o["e0"]
    assert abs(out["error_final"][k] - o["e1"]) <= 1e-8 * o["e1"]
    assert _pose_diff(out["pose_i"][k], o["vals"][0]) < 1e-7
    assert _pose_diff(out["pose_j"][k], o["vals"][1]) < 1e-7


def test_lm_against_the_oracle():
    """iterations, trials, lambda, start and final error, both poses of every pair of the ragged batch"""
    pairs, ref, out = cases()
    assert any(_rejecting(o) for o in ref) and any(_at_bound(o) for o in ref)
    for k, o in enumerate(ref):
        _check_vs_oracle(out, k, o)
    for k in range(6):                                                          # s = 1: pose j found from an identity start
        assert _pose_diff(out["pose_j"][k], pairs[k]["truth_j"]) < 0.05


def _ut_full(ut):
    M = np.zeros((6, 6)); M[np.triu_indices(6)] = ut
    return M + np.triu(M, 1).T


def test_covariance_and_information():
    """cov = block [6:12, 6:12] of the inverse of the oracle's dense undamped system at the batch's own poses (the oracle's final
    points: they agree with the batch's to the 1e-7 of test 1), 1e-6 of the largest entry -- the allowance graphs with the sigma-1e-7
    prior have (tests/test_gpu_marginals_all.py:115); info = cov^-1 to the same bound, positive definite"""
    pairs, ref, out = cases()
    worst = 0.0
    for k, (pr, o) in enumerate(zip(pairs, ref)):
        vals = o["vals"].copy(); vals[0] = out["pose_i"][k]; vals[1] = out["pose_j"][k]
        po = pair_oracle(pr)
        po.set_poses(vals)
        H, _ = po.dense_system()
        rows = np.concatenate([np.arange(12), (6 * (2 + np.arange(pr["n"]))[:, None] + np.arange(3)[None, :]).ravel()])
        want = np.linalg.inv(H[np.ix_(rows, rows)])[6:12, 6:12]
        cov = out["cov"][k]
        rel = np.abs(cov - want).max() / np.abs(want).max()
        worst = max(worst, rel)
        info = _ut_full(out["info"][k])
        rel_i = np.abs(info - np.linalg.inv(cov)).max() / np.abs(info).max()
        print("pair %d: cov rel %.2e info rel %.2e" % (k, rel, rel_i))
        assert rel <= 1e-6
        assert np.array_equal(cov, cov.T)
        assert rel_i <= 1e-6
        assert np.linalg.eigvalsh(info).min() > 0
    print("covariance agreement, worst pair: %.2e of the largest entry" % worst)


def _context_path(pr):
    n = pr["n"]
    gr = G.Graph()
    gr.add_poses(np.array([IDENT, pr["pose_j0"]]))
    w = np.zeros(21); w[[0, 6, 11, 15, 18, 20]] = 1.0 / POSE_SIGMA ** 2
    gr.add_prior(0, IDENT, w)
    ids = (2 + np.arange(n)).astype(np.int64)
    gr._chk(G.lib.fgo_add_points3(gr._h, n, S._i64p(ids), S._dp(np.ascontiguousarray(pr["xyz"])), POINT_SIGMA))
    gr.set_calibration(CALIB, pr["bps"])
    pid = np.repeat([0, 1], n).astype(np.int64); qid = np.tile(ids, 2)
    uv = np.ascontiguousarray(np.concatenate([pr["uv_i"], pr["uv_j"]]))
    gr._chk(G.lib.fgo_add_reprojs(gr._h, 2 * n, S._i64p(pid), S._i64p(qid), S._dp(uv), PIXEL_SIGMA))
    _, st = gr.optimize_gtsam(100)
    return st, gr.get_poses(2), gr.marginal_cov(1)


@pytest.mark.parametrize("k", [0, 3, 6])
def test_against_the_context_path(k):
    """one fgo_ctx per pair (what host/examples/run_bundle_adjust.cpp does): same counts, estimate 1e-7, covariance 1e-6 of the largest entry"""
    pairs, _, out = cases()
    st, V, cov = _context_path(pairs[k])
    assert (out["iterations"][k], out["trials"][k]) == (st.iterations, st.trials)
    assert _pose_diff(out["pose_i"][k], V[0]) < 1e-7 and _pose_diff(out["pose_j"][k], V[1]) < 1e-7
    assert abs(out["error_final"][k] - 0.5 * st.chi2_final) <= 1e-8 * 0.5 * st.chi2_final
    assert np.abs(out["cov"][k] - cov).max() <= 1e-6 * np.abs(cov).max()


KEYS = ("pose_j", "pose_i", "cov", "info", "status", "iterations", "trials", "error_initial", "error_final", "lambda_final")


def _same_bits(a, ka, b, kb):
    for key in KEYS:
        x, y = np.ascontiguousarray(a[key][ka]), np.ascontiguousarray(b[key][kb])
        assert x.tobytes() == y.tobytes(), (key, ka, kb)


def test_a_pair_does_not_depend_on_its_batch():
    """every pair alone, and the batch reversed: bit-identical outputs"""
    pairs, _, out = cases()
    for k, pr in enumerate(pairs):
        _same_bits(run_batch([pr]), 0, out, k)
    rev = run_batch(pairs[::-1])
    for k in range(len(pairs)):
        _same_bits(rev, len(pairs) - 1 - k, out, k)


def test_edge_cases_in_one_batch():
    """no matches, too few matches and a NaN pixel between ordinary pairs: their own status, the neighbours untouched"""
    start = np.concatenate([[0.1, -0.05, 0.04], _rotvec_quat(np.array([0.02, -0.03, 0.015]))])
    ordinary = [make_pair(200 + q, n, 1.0) for q, n in enumerate((9, 70, 6, 33))]
    empty = make_pair(300, 0, 1.0, pose_j0=start)
    few = make_pair(301, 4, 1.0, pose_j0=start)
    nan = make_pair(302, 12, 1.0)
    nan["uv_j"][7, 1] = np.nan
    out = run_batch([ordinary[0], empty, ordinary[1], few, ordinary[2], nan, ordinary[3]])       # (a failure of the call raises FgoError)
    clean = run_batch(ordinary)
    for q, k in enumerate((0, 2, 4, 6)):
        assert out["status"][k] == G.FGO_TV_OK
        _same_bits(out, k, clean, q)
    for k in (1, 3):
        assert out["status"][k] == G.FGO_TV_TOO_FEW and out["iterations"][k] == 0 and out["trials"][k] == 0
        assert np.array_equal(out["pose_j"][k], start) and np.array_equal(out["pose_i"][k], IDENT)
        assert not out["cov"][k].any() and not out["info"][k].any()
    assert out["status"][5] == G.FGO_TV_NUM
    assert not out["cov"][5].any() and not out["info"][5].any()
    assert np.isfinite(out["pose_j"][5]).all()                                   # no trial of a NaN problem is accepted: the start
    # min_matches is a parameter: 4 matches are enough when the caller says so
    assert run_batch([few], params=G.two_view_params(min_matches=4))["status"][0] == G.FGO_TV_OK


def test_one_pair_and_no_pair():
    pairs, _, out = cases()
    _same_bits(run_batch(pairs[3:4]), 0, out, 3)
    none = run_batch([])
    assert none["pose_j"].shape == (0, 7) and none["cov"].shape == (0, 6, 6) and none["status"].shape == (0,)


def test_start_pose_and_body_P_sensor_against_the_oracle():
    """a start of pose j that is not the identity and a camera that is not at the body origin"""
    bps = np.concatenate([[0.05, -0.02, 0.10], _rotvec_quat(np.array([0.3, -0.2, 0.1]))])
    start = np.concatenate([0.8 * XI[3:], _rotvec_quat(0.8 * XI[:3])])
    pr = make_pair(400, 40, 1.0, bps=bps, pose_j0=start)
    o = run_oracle(pr)
    out = run_batch([pr], body_P_sensor=bps)
    _check_vs_oracle(out, 0, o)
    assert _pose_diff(out["pose_j"][0], pr["truth_j"]) < 0.05
