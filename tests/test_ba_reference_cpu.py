"""tests/ba_reference.py on the CPU: every case has the property it is built for (so that a later edit cannot quietly lose the edge the
GPU test needs), the vectorised dual numbers equal tests/camera_independent.reproj_ad, and the dense reference agrees with the oracle
-- orc.Problem fed with the same factors, dense_system(), numpy's Schur complement as tests/test_gpu_ba_oracle.py forms it -- to 1e-10 of
every block's own scale (chi2: 1e-12).  Prints the float64-vs-extended figures the bounds of tests/test_gpu_ba_forms.py are derived from."""
import numpy as np
import pytest

from tests import ba_reference as R
from tests import camera_independent as cam
from tests import orc_binding as orc
from tests.util import info_ut


def oracle_problem(c):
    K, L = c["K"], c["L"]
    N = K + L
    values = np.zeros((N, 7)); values[:K] = c["poses0"]; values[K:, :3] = c["points0"]
    vkind = np.zeros(N, np.int32); vkind[K:] = orc.VK_POINT
    no, nb = len(c["obs_kf"]), len(c["between_i"])
    meas = np.zeros((no + nb, 7)); meas[:no, :2] = c["obs_uv"]; meas[no:] = c["between_z"]
    info = np.zeros((no + nb, 21)); info[:no, 0] = 1.0 / c["obs_sigma"] ** 2; info[no:] = c["between_info"]
    ei = np.concatenate([c["obs_kf"], c["between_i"]]).astype(np.int32)
    ej = np.concatenate([K + c["obs_pt"], c["between_j"]]).astype(np.int32)
    kind = np.concatenate([np.full(no, orc.FK_REPROJ), np.full(nb, orc.FK_BETWEEN)]).astype(np.int32)
    po = orc.Problem(values, np.concatenate([c["fixed_pose"], c["fixed_pt"]]).astype(np.uint8), ei, ej, meas, info)
    po.set_kinds(vkind, kind)
    po.set_calibration(c["calib"], c["bps"])
    ids, mean, infos = [], [], []
    if c["pose_prior"]:
        ids.append(c["pose_prior"][0]); mean.append(c["pose_prior"][1]); infos.append(c["pose_prior"][2])
    for j, m, s in zip(c["pp_pt"], c["pp_mean"], c["pp_sigma"]):
        pw6 = np.zeros((6, 6)); pw6[:3, :3] = np.eye(3) / s ** 2
        m7 = np.zeros(7); m7[:3] = m
        ids.append(K + j); mean.append(m7); infos.append(info_ut(pw6))
    if ids:
        po.add_priors(np.array(ids, np.int32), np.array(mean), np.array(infos))
    return po


def oracle_schur(c, lam):
    """numpy's Schur complement of the oracle's dense system onto the rows that stay (tests/test_gpu_ba_oracle._schur_of_oracle)"""
    po = oracle_problem(c)
    Ho, bo = po.dense_system()
    stay, elim = R.layout(c)
    free = np.nonzero(np.concatenate([c["fixed_pose"], c["fixed_pt"]]) == 0)[0]
    pos = np.full(c["K"] + c["L"], -1); pos[free] = np.arange(len(free))
    keep = (6 * pos[stay][:, None] + np.arange(6)[None, :]).ravel()
    lm3 = (6 * pos[c["K"] + elim][:, None] + np.arange(3)[None, :]).ravel()
    Hcc, Hcp, Hpp = Ho[np.ix_(keep, keep)], Ho[np.ix_(keep, lm3)], Ho[np.ix_(lm3, lm3)] + lam * np.eye(len(lm3))
    X = np.linalg.solve(Hpp, np.concatenate([Hcp.T, bo[lm3, None]], 1))
    return Hcc - Hcp @ X[:, :-1], bo[keep] - Hcp @ X[:, -1], po.chi2()


def test_pairs_share_exactly_the_listed_landmarks():
    c = R.case("pairs")
    sh = R.shared_landmarks(c)
    assert c["K"] == 2 * len(R.PAIR_SIZES) and set(R.PAIR_SIZES) >= {1, 9, 10, 11, 19, 20, 21, 39, 40, 41, 79, 80, 81, 159, 160, 161}
    want = np.zeros_like(sh)
    for k, m in enumerate(R.PAIR_SIZES):
        want[2 * k:2 * k + 2, 2 * k:2 * k + 2] = m
    np.testing.assert_array_equal(sh, want)
    assert len(np.unique(c["obs_kf"] * c["L"] + c["obs_pt"])) == len(c["obs_kf"])


def test_counts_cameras_have_exactly_the_listed_observations():
    c = R.case("counts")
    n = R.obs_per_camera(c)
    assert tuple(n[:len(R.COUNTS)]) == R.COUNTS == (1, 59, 60, 61, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)
    sh = R.shared_landmarks(c)
    for i in range(c["K"]):
        assert (sh[i] > 0).sum() >= 2, i                                 # its own block and at least one more


def test_clique90_degrees_and_pair_counts():
    c = R.case("clique90")
    sh = R.shared_landmarks(c)
    assert c["K"] == 90 and (sh > 0).all()                               # in ANY elimination order the columns have 90, 89, .., 1 row blocks
    assert (sh[:12, :12] == 112).all() and (sh[12:, :] == 12).all() and (sh[:, 12:] == 12).all()
    assert 112 > 80 >= 12                                                # four waves / one wave at the default ba_small


def test_hub_is_a_clique_of_more_than_40_cameras_over_more_than_one_batch():
    c = R.case("hub")
    sh = R.shared_landmarks(c)
    assert c["K"] >= 41 and 80 // c["K"] == 1 and (sh > 256).all()


@pytest.mark.parametrize("n", R.GRID_SIZES)
def test_grids_have_the_listed_number_of_free_cameras(n):
    c = R.case("grid%d" % n)
    assert int(((c["fixed_pose"] == 0) & (R.obs_per_camera(c) > 0)).sum()) == n
    sh = R.shared_landmarks(c)
    for k in range(n - 1):
        assert sh[k, k + 1] == 2
    assert np.count_nonzero(np.triu(sh, 2)) == 0


def test_odd_holds_every_marked_landmark():
    c = R.case("odd")
    K, F = c["K"], R.ODD_FIXED_CAM
    by = {}
    for j, m in c["marks"].items():
        by.setdefault(m, []).append(j)
    cams = lambda j: sorted(c["obs_kf"][c["obs_pt"] == j])
    npri = lambda j: int((c["pp_pt"] == j).sum())
    stay, elim = R.layout(c)
    assert c["fixed_pose"][F] and 0 < F < K - 1 and any(F in cams(j) and j in elim for j in by["regular"])
    (j,) = by["fixed_camera_only"]; assert cams(j) == [F] and npri(j) == 1 and j in elim
    for j in by["no_prior"]:
        assert npri(j) == 0 and len(set(cams(j))) >= 3 and j in elim
    (j,) = by["two_priors"]; assert npri(j) == 2 and len(set(c["pp_sigma"][c["pp_pt"] == j])) == 2
    (j,) = by["seen_once"]; assert len(cams(j)) == 1 and cams(j) != [F] and npri(j) == 1
    (j,) = by["pair_twice"]; assert len(cams(j)) == len(set(cams(j))) + 1
    (j,) = by["behind_its_camera"]
    o = np.nonzero(c["obs_pt"] == j)[0]
    r, Jx, Jp = R.reproj_all(c["poses0"][c["obs_kf"][o]], c["points0"][[j] * len(o)], c["obs_uv"][o], c["calib"], c["bps"])
    assert np.all(Jx == 0) and np.all(Jp == 0) and np.all(r == 2 * c["calib"][0])
    (j,) = by["unobserved"]; assert cams(j) == [] and K + j in stay and not c["fixed_pt"][j] and npri(j) == 1
    (j,) = by["fixed_landmark"]; assert c["fixed_pt"][j] and len(cams(j)) >= 1 and j not in elim
    assert c["obs_sigma"].min() == 0.5 and c["obs_sigma"].max() == 2.0 and len(set(c["obs_sigma"])) > 5
    # every other intended observation is in front of its camera
    r, Jx, _ = R.reproj_all(c["poses0"][c["obs_kf"]], c["points0"][c["obs_pt"]], c["obs_uv"], c["calib"], c["bps"])
    assert (np.abs(Jx).max(axis=(1, 2)) > 0).sum() == len(c["obs_kf"]) - 1


def test_no_priors_has_no_prior_at_all():
    c = R.case("no_priors")
    assert c["pose_prior"] is None and len(c["pp_pt"]) == 0 and c["fixed_pose"][0] == 1 and c["fixed_pose"][1:].sum() == 0
    sh = R.shared_landmarks(c)[1:, 1:]
    want = np.zeros_like(sh)
    for k, m in enumerate(R.NO_PRIORS_SIZES):
        want[2 * k:2 * k + 2, 2 * k:2 * k + 2] = m
    np.testing.assert_array_equal(sh, want)
    assert (np.bincount(c["obs_pt"]) >= 3).all()                          # lambda = 0 is fine: three views of every landmark


def test_every_intended_observation_is_in_front_of_its_camera():
    for name in R.CASE_NAMES:
        if name == "odd":
            continue
        c = R.case(name)
        _, Jx, _ = R.reproj_all(c["poses0"][c["obs_kf"]], c["points0"][c["obs_pt"]], c["obs_uv"], c["calib"], c["bps"])
        assert (np.abs(Jx).max(axis=(1, 2)) > 0).all(), name


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_vectorised_dual_numbers_equal_reproj_ad(dtype):
    c = R.case("odd")
    r, Jx, Jp = R.reproj_all(c["poses0"][c["obs_kf"]], c["points0"][c["obs_pt"]], c["obs_uv"], c["calib"], c["bps"], dtype)
    for o in range(len(c["obs_kf"])):
        r1, Jx1, Jp1 = cam.reproj_ad(c["poses0"][c["obs_kf"][o]], c["points0"][c["obs_pt"][o]], c["obs_uv"][o], c["calib"], c["bps"])
        sc = max(1.0, np.abs(Jx1).max())
        np.testing.assert_allclose(np.asarray(r[o], np.float64), r1, rtol=0, atol=1e-12 * max(1.0, np.abs(r1).max()))
        np.testing.assert_allclose(np.asarray(Jx[o], np.float64), Jx1, rtol=0, atol=1e-12 * sc)
        np.testing.assert_allclose(np.asarray(Jp[o], np.float64), Jp1, rtol=0, atol=1e-12 * sc)


@pytest.mark.parametrize("name", R.CASE_NAMES + ["underdetermined"])
def test_reference_agrees_with_the_oracle(name):
    c = R.case(name)
    ref = R.reference(name, True)
    n = len(ref["stay"])
    for lam in R.LAMS:
        if name == "underdetermined" and lam == 0.0:
            continue                                                     # H_pp of its extra landmark is singular without damping
        So, go, chio = oracle_schur(c, lam)
        assert So.shape == ref["S"][lam].shape
        dS = np.abs(So - np.asarray(ref["S"][lam], np.float64)).reshape(n, 6, n, 6).max(axis=(1, 3))
        dg = np.abs(go - np.asarray(ref["g"][lam], np.float64)).reshape(n, 6).max(axis=1)
        relS = float(R.block_rel(dS, ref["S_scale"][lam]).max())
        relg = float(R.block_rel(dg, ref["g_scale"][lam]).max())
        print("[ba reference] %-10s lambda %-6g oracle vs extended: S %.2e  g %.2e of the block scales" % (name, lam, relS, relg))
        assert relS <= 1e-10 and relg <= 1e-10, (name, lam, relS, relg)
        # blocks the reference says receive no landmark term are the linearised blocks themselves
        H4, S4 = ref["H"].reshape(n, 6, n, 6), ref["S"][lam].reshape(n, 6, n, 6)
        for a, b in zip(*np.nonzero(~ref["touched"])):
            assert np.array_equal(H4[a, :, b, :], S4[a, :, b, :])
    assert abs(chio - float(ref["chi2"])) <= 1e-12 * chio


def test_float64_against_extended_figures():
    """the figures the GPU bounds come from (profiles/NOTES.md "Landmark elimination at small shapes")"""
    B = R.bounds()
    for name, f in B["figures"].items():
        print("[ba reference] %-10s float64 vs extended: S %.3e  g %.3e of the block scales; step %.3e (|step| %.3e) -> step bound %.3e" % (
            name, f["S"], f["g"], f["step_diff"], f["step"], B["step"][name]))
    print("[ba reference] bounds: S %.3e  g %.3e" % (B["S"], B["g"]))
    assert R.EPS <= B["S"] <= 1e-10 and R.EPS <= B["g"] <= 1e-10
    for name in R.CASE_NAMES:
        assert 1e-13 <= B["step"][name] <= 1e-8
