"""The batched plane extraction (csrc/kernels_plane_extract.hip, fgo_plane_extract_batch: one workgroup per frame, all frames in one
launch) against its numpy restatement (tests/plane_extract_reference.py, itself pinned by tests/test_plane_extract_reference_cpu.py).
The plane package's arithmetic is not in the reference tree: the restatement is the yardstick.

W and H belong to a call, and so do the hypotheses and max_planes, so there are a few small calls (plane_extract_reference.gpu_cases):
16 x 12 (fewer pixels than lanes), 48 x 40, 23 x 89 / 64 x 32 / 683 x 3 (2047, 2048 and 2049 pixels: the kernel's 2048-point staging
chunk - 1, the chunk, the chunk + 1), each with five frames (all-zero depth, valid pixels below min_pixels, one wall, a corner with
three walls, a wall with 30 % of the pixels at random depths) at max_planes = 4 and the corner alone at max_planes = 1 (more walls
than it allows), and one call of three frames at 176 x 144; each with hypotheses = 1, 100 (a partial pass), 512 (exactly one pass
of the kernel's 512 hypotheses) and 520 (one pass and a bit).  min_pixels = W H / 8.  Every case is well posed
(test_plane_extract_reference_cpu.py): no decision within 1e-9 of its threshold and no plane through the camera, whose orientation
would hang on rounding -- which is why the calls of one hypothesis run with seed 1.

Compared exactly: the counts of the decided hypotheses (at most 1 % of a frame's may be undecided), the winner and n_valid_hyp of a
plane whose round was decided throughout, status, n_planes, rounds_run, n_valid_pixels, n_pixels, fits and the label image.
Tolerances: the project's per-value tolerance, relative 1e-11, times the condition numbers the restatement
computes at run time.  With g = min(1, (l1 - l0) / l2) of the plane's scatter matrix:
  n      1e-11 / g                          d, centroid, rmse   1e-11 (1 + p_max) / g
  C, cov16   1e-11 cond(A) / g of their largest entry"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import graph_slam_amd as G
from tests import plane_check_reference as pcr
from tests import plane_extract_reference as ref

TOL = 1e-11
FIELDS = ("status", "n_planes", "n_valid_pixels", "rounds_run", "abcd_all", "cov16_all", "cov_ut6_all", "n_pixels", "best_hypothesis",
          "best_count", "n_valid_hyp", "fits", "rmse", "centroid", "ptr", "abcd", "cov16", "cov_ut6", "labels", "hyp_counts")


def run(c, depth=None, **kw):
    return G.plane_extract_batch(c["depth"] if depth is None else depth, params=G.plane_extract_params(**ref.call_params(c)),
                                 want_labels=True, want_hyp_counts=True, **kw)


@functools.lru_cache(maxsize=None)
def calls():
    return ref.gpu_cases()


@functools.lru_cache(maxsize=None)
def case(i):
    """call i: the restatement's frames and the entry point's output, computed once and shared"""
    c = calls()[i]
    return c, [ref.extract_frame(f, **ref.call_params(c)) for f in c["depth"]], run(c)


IDS = ["%dx%d-K%d-P%d" % (c["W"], c["H"], c["hypotheses"], c["max_planes"]) for c in ref.gpu_cases()]


@pytest.mark.parametrize("i", range(len(IDS)), ids=IDS)
def test_counts_winners_statuses_and_labels_equal_the_reference(i):
    c, want, g = case(i)
    n_dec = n_all = 0
    for f, w in enumerate(want):
        rr = w["rounds_run"]
        d = w["decided"]
        n_dec += int(d[:rr].sum()); n_all += d[:rr].size
        assert rr == 0 or 1.0 - d[:rr].mean() <= 0.01, (f, c["kinds"][f])
        assert np.array_equal(g["hyp_counts"][f][d], w["hyp_counts"][d]), (f, np.argwhere(g["hyp_counts"][f] != w["hyp_counts"])[:5])
        for k in ("status", "n_planes", "n_valid_pixels", "rounds_run"):
            assert g[k][f] == w[k], (f, c["kinds"][f], k, g[k][f], w[k])
        assert np.array_equal(g["n_pixels"][f], w["n_pixels"]) and np.array_equal(g["fits"][f], w["fits"]), (f, g["n_pixels"][f], w["n_pixels"])
        assert np.array_equal(g["labels"][f], w["labels"]), (f, c["kinds"][f], int(np.sum(g["labels"][f] != w["labels"])))
        for k in range(w["n_planes"]):
            if d[w["round"][k]].all():                            # the round that found the plane was decided throughout
                for fld in ("best_hypothesis", "best_count", "n_valid_hyp"):
                    assert g[fld][f][k] == w[fld][k], (f, k, fld, g[fld][f][k], w[fld][k])
    print("%s: %d of %d hypotheses decided and equal; planes per frame %s" % (IDS[i], n_dec, n_all, list(g["n_planes"])))
    assert np.array_equal(g["ptr"], np.concatenate([[0], np.cumsum(g["n_planes"])]))


@pytest.mark.parametrize("i", range(len(IDS)), ids=IDS)
def test_planes_and_covariances_against_the_reference(i):
    c, want, g = case(i)
    worst = {}
    for f, w in enumerate(want):
        mp = c["max_planes"]
        for k in range(w["n_planes"], mp):                        # the slots past the last plane are zero
            assert not g["abcd_all"][f][k].any() and not g["cov16_all"][f][k].any() and not g["cov_ut6_all"][f][k].any(), (f, k)
            assert g["n_pixels"][f][k] == 0 and g["rmse"][f][k] == 0 and not g["centroid"][f][k].any(), (f, k)
        for k in range(w["n_planes"]):
            gg, pm = w["g"][k], 1 + w["p_max"]
            abcd, S, C6 = g["abcd_all"][f][k], g["cov16_all"][f][k], g["cov_ut6_all"][f][k]
            assert abs(abcd[:3] @ abcd[:3] - 1) <= 1e-14 and abcd[3] >= 0 and np.array_equal(S, S.T), (f, k)
            ctol = TOL * w["cond_A"][k] / gg
            err = dict(n=np.abs(abcd[:3] - w["abcd"][k][:3]).max() / (TOL / gg),
                       d=abs(abcd[3] - w["abcd"][k][3]) / (TOL * pm / gg),
                       centroid=np.abs(g["centroid"][f][k] - w["centroid"][k]).max() / (TOL * pm / gg),
                       rmse=abs(g["rmse"][f][k] - w["rmse"][k]) / (TOL * pm / gg),
                       C=np.abs(C6 - w["cov_ut6"][k]).max() / (ctol * np.abs(w["cov_ut6"][k]).max()),
                       cov16=np.abs(S - w["cov16"][k]).max() / (ctol * np.abs(w["cov16"][k]).max()))
            for name, e in err.items():
                assert e <= 1.0, (f, c["kinds"][f], k, name, e, gg, w["cond_A"][k])
            worst = {name: max(e, worst.get(name, 0.0)) for name, e in err.items()}
    print("%s: largest error as a share of its bound: %s" % (IDS[i], ", ".join("%s %.1e" % ne for ne in worst.items())))
    # the packed form is the kept slots in order
    keep = np.arange(c["max_planes"])[None, :] < g["n_planes"][:, None]
    assert g["abcd"].tobytes() == g["abcd_all"][keep].tobytes() and g["cov16"].tobytes() == g["cov16_all"][keep].tobytes()
    assert g["cov_ut6"].tobytes() == g["cov_ut6_all"][keep].tobytes()


def _pick(W, H, K, P):
    return IDS.index("%dx%d-K%d-P%d" % (W, H, K, P))


def test_two_calls_are_bit_identical_and_outputs_are_optional():
    for i in (_pick(683, 3, 520, 4), _pick(176, 144, 100, 4)):
        c, want, g = case(i)
        again = run(c)
        for f in FIELDS:
            assert again[f].tobytes() == g[f].tobytes(), (IDS[i], f)
    c, want, g = case(_pick(48, 40, 100, 4))
    bare = G.plane_extract_batch(c["depth"], params=G.plane_extract_params(**ref.call_params(c)))
    assert "labels" not in bare and "hyp_counts" not in bare
    for f in bare:
        assert bare[f].tobytes() == g[f].tobytes(), f
    assert G.lib.fgo_debug_plane_extract_kernel_ms() > 0


def test_a_frame_alone_equals_the_frame_in_the_batch():
    for i in (_pick(64, 32, 512, 4), _pick(176, 144, 100, 4)):
        c, want, g = case(i)
        for f in range(len(c["depth"])):
            one = run(c, depth=c["depth"][f:f + 1])
            for fld in FIELDS:
                if fld in ("ptr", "abcd", "cov16", "cov_ut6"):
                    whole = g[fld][g["ptr"][f]:g["ptr"][f + 1]] if fld != "ptr" else np.array([0, g["n_planes"][f]], np.int64)
                    assert one[fld].tobytes() == whole.tobytes(), (IDS[i], f, fld)
                else:
                    assert one[fld][0].tobytes() == g[fld][f].tobytes(), (IDS[i], f, fld)
    # the place in the batch does not matter either
    c, want, g = case(_pick(48, 40, 100, 4))
    back = run(c, depth=c["depth"][::-1])
    for fld in ("status", "n_planes", "abcd_all", "cov16_all", "labels", "hyp_counts", "rmse"):
        assert back[fld][::-1].tobytes() == g[fld].tobytes(), fld


def test_other_parameters_reach_the_kernel():
    """refine_rounds = 0 keeps the winner's set; the seed moves the samples; sigma_z is a polynomial; z_min / z_max cut the frame"""
    c, want, g = case(_pick(48, 40, 100, 4))
    for kw in (dict(refine_rounds=0), dict(seed=12345), dict(sigma_z=(0.01, 0.003, 0.002), sigma_px=0.7), dict(max_dist=0.03, min_area=0.05),
               dict(z_min=1.0, z_max=2.4), dict(z_scale=0.0011, cx=20.0, cy=25.0)):
        P = dict(ref.call_params(c), **kw)
        o = G.plane_extract_batch(c["depth"], params=G.plane_extract_params(**P), want_labels=True, want_hyp_counts=True)
        for f, frame in enumerate(c["depth"]):
            w = ref.extract_frame(frame, **P)
            assert w["margin"] >= 1e-9 and w["g_min"] >= 1e-3 and w["d_min"] >= 1e-6, (kw, f)
            assert np.array_equal(o["hyp_counts"][f][w["decided"]], w["hyp_counts"][w["decided"]]), (kw, f)
            assert (o["status"][f], o["n_planes"][f], o["rounds_run"][f]) == (w["status"], w["n_planes"], w["rounds_run"]), (kw, f)
            assert np.array_equal(o["labels"][f], w["labels"]) and np.array_equal(o["fits"][f], w["fits"]), (kw, f)
            for k in range(w["n_planes"]):
                assert np.abs(o["abcd_all"][f][k][:3] - w["abcd"][k][:3]).max() <= TOL / w["g"][k], (kw, f, k)
                assert np.abs(o["cov_ut6_all"][f][k] - w["cov_ut6"][k]).max() <= TOL * w["cond_A"][k] / w["g"][k] * np.abs(w["cov_ut6"][k]).max(), (kw, f, k)


def test_the_planes_feed_the_plane_check():
    """two renders of one room from poses i and j go through plane_extract_batch, the packed output goes straight into
    plane_check_vro_batch with the true relative pose and a small pose covariance: the pairing equals what plane_check_reference
    gives on the restatement's planes (only the geometric pairing is asserted, not the size of d2)"""
    W, H = 48, 40
    rng = np.random.default_rng(7)
    cam = ref.camera(W, H)
    lo, hi = np.array([-40.0, -40.0, -40.0]), np.array([1.6, 1.1, 2.2])
    Ri = ref.rot_y(np.deg2rad(40.0)) @ ref.rot_x(np.deg2rad(-25.0)); ti = np.zeros(3)
    Rj = ref.rot_y(np.deg2rad(46.0)) @ ref.rot_x(np.deg2rad(-22.0)); tj = np.array([0.05, -0.03, 0.1])
    depth = np.stack([ref.render(ref.room_planes(lo, hi, R, t), W, H, cam, 0.014, rng)[0] for R, t in ((Ri, ti), (Rj, tj))])
    P = dict(cam, hypotheses=256, min_pixels=W * H // 20)
    o = G.plane_extract_batch(depth, params=G.plane_extract_params(**P))
    want = [ref.extract_frame(f, **P) for f in depth]
    assert list(o["n_planes"]) == [w["n_planes"] for w in want] == [3, 3]
    # the pose of frame j in frame i: p_i = R p_j + t
    R = Ri.T @ Rj; t = Ri.T @ (tj - ti)
    pose = np.concatenate([t, ref.vro_quat(R)])
    cov = np.diag([1e-6] * 3 + [1e-6] * 3)
    a, b = o["ptr"][0], o["ptr"][1]
    got = G.plane_check_vro_batch(pose[None], [0, b - a], o["abcd"][a:b], o["cov16"][a:b], [0, o["ptr"][2] - b], o["abcd"][b:], o["cov16"][b:],
                                  cov=cov[None])
    w = pcr.check_record(pose, want[0]["abcd"][:3], want[0]["cov16"][:3].reshape(-1, 16), want[1]["abcd"][:3],
                         want[1]["cov16"][:3].reshape(-1, 16), cov=cov)
    assert got["status"][0] == G.FGO_PC_OK == w["status"]
    assert np.array_equal(got["match"], w["match"]) and got["n_matched"][0] == w["n_matched"] == 3, (got["match"], w["match"])
    assert sorted(got["match"]) == [0, 1, 2]
